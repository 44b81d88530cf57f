"""Wav2Vec2ForCTC.decode(num_beams=...) / evaluate(num_beams=...) on the GPU (tiny config, B = 3 clips of 0.3 to 0.6 s in
one padded batch): the beam result bit-equal to ops.ctc_beam on the model's own returned log-probs and inside the
invariants of tests/_ctc_beam_ref.py against float64, the greedy paths unchanged, timestamps equal to ``align`` on the best
sequences, evaluate's edit distances those of the best beam, and the job script's n-best output."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import _ctc_beam_ref as R
import _ctc_ref as C
from _margins import within
from oracle import wav2vec2_oracle as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_IN = 9600                                  # 0.6 s
SAMPLE_LENS = (9600, 7200, 4800)             # 0.6, 0.45 and 0.3 s
TINY = dict(hidden_size=64, num_hidden_layers=2, num_attention_heads=1, intermediate_size=128, conv_dim=(64, 64, 64),
            conv_stride=(5, 2, 2), conv_kernel=(10, 3, 2), num_conv_pos_embeddings=8, num_conv_pos_embedding_groups=4,
            num_codevectors_per_group=16, codevector_dim=32, proj_codevector_dim=64, num_negatives=10)
I32 = torch.int32


def W():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import wav2vec2
    return wav2vec2


@pytest.fixture(scope="module")
def setup(dev):
    """The model (the head scaled up so that the argmax moves between symbols), the padded batch, its mask and the model's
    own log-probs, once for the module."""
    m = W().create_full_model("asr", "base", device=dev, precision="bf16", seed=7, **TINY)
    g = torch.Generator().manual_seed(3)
    m.arena.param("lm_head.kernel").mul_(12.0)
    m.arena.param("lm_head.bias").copy_((torch.randn(m.config.vocab_size, generator=g) * 0.3).to(dev))
    m.refresh_shadows()
    x = torch.from_numpy(V.create_dummy_pool(seed=8, num_samples=3, length=T_IN)).clone()
    for b, n in enumerate(SAMPLE_LENS):
        x[b, n:] = 0
    x = x.to(dev)
    mask = W().frame_attention_mask(m.config, SAMPLE_LENS, T_IN)
    fl = [int(v) for v in mask.sum(dim=1).tolist()]
    out = m(x, attention_mask=mask)
    s = {"m": m, "x": x, "mask": mask, "fl": fl, "logp": out["log_probs"].contiguous(), "T": mask.shape[1]}
    yield s
    s.clear()
    import gc
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def beam_direct(s, K, dev):
    from tethys_speech_amd import ops
    B, T = 3, s["T"]
    tok = torch.full((B, K, T), -1, dtype=I32, device=dev)
    ln, sc = torch.zeros(B, K, dtype=I32, device=dev), torch.zeros(B, K, dtype=torch.float32, device=dev)
    nb = torch.zeros(B, dtype=I32, device=dev)
    ws = torch.empty(ops.ctc_beam_workspace_elems(B, K, T), dtype=I32, device=dev)
    ops.ctc_beam(s["logp"], torch.tensor(s["fl"], dtype=I32, device=dev), s["m"].config.ctc_blank_id, K, tok, ln, sc, nb, ws)
    torch.cuda.synchronize()
    return tok, ln, sc, nb


def test_decode_with_beams_equals_the_kernel_on_the_models_log_probs(dev, setup):
    s, m = setup, setup["m"]
    assert 14 <= min(s["fl"]) and max(s["fl"]) == s["T"] and len(set(s["fl"])) == 3
    K, Rn = 4, 2
    d = m.decode(s["x"], attention_mask=s["mask"], num_beams=K, num_return_sequences=Rn)
    tok, ln, sc, nb = beam_direct(s, K, dev)
    n = int(ln[:, :Rn].max())
    assert n >= 3 and d["sequences"].dtype == I32 and tuple(d["sequences"].shape) == (3, Rn, n)
    assert torch.equal(d["sequences"], tok[:, :Rn, :n]) and torch.equal(d["lengths"], ln[:, :Rn])
    assert torch.equal(d["sequences_scores"].view(I32), sc[:, :Rn].view(I32)) and torch.equal(d["n_beams"], nb)
    assert set(d) == {"sequences", "lengths", "sequences_scores", "n_beams"}
    d1 = m.decode(s["x"], attention_mask=s["mask"], num_beams=K)
    assert tuple(d1["sequences"].shape) == (3, int(ln[:, 0].max())) and tuple(d1["lengths"].shape) == (3,)
    assert torch.equal(d1["sequences"], tok[:, 0, :d1["sequences"].shape[1]]) and torch.equal(d1["sequences_scores"], sc[:, 0])
    # the invariants against float64, on the log-probs the model returned
    lp = s["logp"].double().cpu().numpy()
    seqs_h, len_h, sc_h = d["sequences"].cpu().numpy(), d["lengths"].cpu().numpy(), d["sequences_scores"].double().cpu().numpy()
    for b in range(3):
        assert int(nb[b]) == K and (np.diff(sc_h[b]) <= 0).all()
        rows = [tuple(seqs_h[b, r, :len_h[b, r]].tolist()) for r in range(Rn)]
        assert len(set(rows)) == Rn
        for r, seq in enumerate(rows):
            assert (seqs_h[b, r, len_h[b, r]:] == -1).all() and len(seq) <= s["fl"][b]
            assert all(0 <= t < m.config.vocab_size and t != m.config.ctc_blank_id for t in seq)
            full = -C.ctc_forward_ref(lp[b], np.array(seq, dtype=np.int64), s["fl"][b])["nll"]
            within("ctc beam model score above the log-likelihood", max(sc_h[b, r] - full, 0.0) / R.pruned_score_bound(lp[b], s["fl"][b]), 1.0)


def test_greedy_paths_are_unchanged(dev, setup):
    """decode() and evaluate() without num_beams (None or 1): the greedy kernels' own results, bit for bit."""
    from tethys_speech_amd import ops
    s, m = setup, setup["m"]
    B, T = 3, s["T"]
    logp = s["logp"]
    amax = torch.zeros(B * T, dtype=I32, device=dev)
    scratch = torch.empty(B * T, m.config.vocab_size, device=dev)
    ops.ctc_logsoftmax(m(s["x"], attention_mask=s["mask"])["logits"].view(B * T, -1).contiguous(), m.config.vocab_size, scratch, amax)
    assert torch.equal(scratch.view(B, T, -1), logp)
    fl = torch.tensor(s["fl"], dtype=I32, device=dev)
    tok, st, en = (torch.full((B, T), -1, dtype=I32, device=dev) for _ in range(3))
    ln, best = torch.zeros(B, dtype=I32, device=dev), torch.zeros(B, device=dev)
    ops.ctc_greedy(amax.view(B, T), logp, fl, m.config.ctc_blank_id, tok, ln, st, en, best)
    n = int(ln.max())
    for d in (m.decode(s["x"], attention_mask=s["mask"]), m.decode(s["x"], attention_mask=s["mask"], num_beams=1),
              m.decode(s["x"], s["mask"], None, 1, False)):
        assert set(d) == {"sequences", "lengths", "token_start_frames", "token_end_frames", "token_start_times",
                          "token_end_times", "best_path_logprob"}
        assert torch.equal(d["sequences"], tok[:, :n]) and torch.equal(d["lengths"], ln)
        assert torch.equal(d["token_start_frames"], st[:, :n]) and torch.equal(d["token_end_frames"], en[:, :n])
        assert torch.equal(d["best_path_logprob"].view(I32), best.view(I32))
    labels = torch.from_numpy(np.stack([C.labels_for("random", 9, m.config.vocab_size, seed=b) for b in range(B)]))
    e0 = m.evaluate(s["x"], labels, [9, 7, 5], attention_mask=s["mask"], return_items=True)
    e1 = m.evaluate(s["x"], labels, [9, 7, 5], attention_mask=s["mask"], return_items=True, num_beams=None)
    e2 = m.evaluate(s["x"], labels, [9, 7, 5], s["mask"], True, 1)
    hyp = tok.cpu().numpy()
    edits = sum(C.levenshtein(hyp[b, :int(ln[b])].tolist(), labels[b, :[9, 7, 5][b]].tolist()) for b in range(B))
    for e in (e0, e1, e2):
        assert set(e) == set(e0) and "beam_sequences" not in e and e["n_edits"] == float(edits)
        assert torch.equal(e["sequences"], tok[:, :n]) and torch.equal(e["nll"].view(I32), e0["nll"].view(I32))
        assert all(e[k] == e0[k] for k in ("nll_sum", "loss", "n_items", "n_infeasible", "n_ref_tokens", "token_error_rate"))


def test_timestamps_equal_align_on_the_best_sequences(dev, setup):
    s, m = setup, setup["m"]
    d = m.decode(s["x"], attention_mask=s["mask"], num_beams=4, num_return_sequences=2, return_timestamps=True)
    best, lens = d["sequences"][:, 0], d["lengths"][:, 0]
    nb = int(lens.max())
    labels = best[:, :nb].clamp_min(0).to(torch.int64).cpu()
    for b in range(3):
        labels[b, int(lens[b]):] = 1        # (past a length: any valid symbol)
    a = m.align(s["x"], labels, lens.cpu().tolist(), attention_mask=s["mask"])
    assert tuple(d["token_start_frames"].shape) == (3, nb) and int(a["infeasible"].sum()) == 0
    for k in ("token_start_frames", "token_end_frames", "token_start_times", "token_end_times"):
        assert torch.equal(d[k], a[k]), k
    for b in range(3):
        n = int(lens[b])
        st, en = d["token_start_frames"][b].cpu().numpy(), d["token_end_frames"][b].cpu().numpy()
        assert (st[:n] >= 0).all() and (en[:n] > st[:n]).all() and (en[:n] <= s["fl"][b]).all() and (st[n:] == -1).all()
        assert (st[1:n] >= en[:n - 1]).all()
    with pytest.raises(ValueError):
        m.decode(s["x"], attention_mask=s["mask"], num_beams=4, num_return_sequences=5)
    with pytest.raises(ValueError):
        m.decode(s["x"], attention_mask=s["mask"], num_beams=17)
    with pytest.raises(ValueError, match="4096 frames"):
        m.decode(torch.zeros(1, 4097 * 20 + 400, device=dev), num_beams=2)     # refused before the forward pass


def test_evaluate_with_beams_reports_the_best_beams_edits(dev, setup):
    s, m = setup, setup["m"]
    K = 4
    tok, ln, _, _ = beam_direct(s, K, dev)
    best = [tok[b, 0, :int(ln[b, 0])].cpu().tolist() for b in range(3)]
    labels = torch.zeros(3, max(len(best[0]), 9), dtype=torch.int64)
    lens = [len(best[0]), 9, 5]
    labels[0, :lens[0]] = torch.tensor(best[0])           # item 0 against its own best beam: no edit
    labels[1, :9] = torch.from_numpy(C.labels_for("random", 9, m.config.vocab_size, seed=1))
    labels[2, :5] = torch.from_numpy(C.labels_for("random", 5, m.config.vocab_size, seed=2))
    e = m.evaluate(s["x"], labels, lens, attention_mask=s["mask"], return_items=True, num_beams=K)
    g = m.evaluate(s["x"], labels, lens, attention_mask=s["mask"], return_items=True)
    edits = [C.levenshtein(best[b], labels[b, :lens[b]].tolist()) for b in range(3)]
    assert edits[0] == 0 and e["n_edits"] == float(sum(edits)) and e["token_error_rate"] == sum(edits) / sum(lens)
    for k in ("nll_sum", "loss", "n_items", "n_infeasible", "n_ref_tokens"):
        assert e[k] == g[k], k
    assert torch.equal(e["nll"].view(I32), g["nll"].view(I32)) and torch.equal(e["sequences"], g["sequences"])
    nb = max(len(x) for x in best)
    assert torch.equal(e["beam_sequences"], tok[:, 0, :nb]) and torch.equal(e["beam_lengths"], ln[:, 0])
    assert all(isinstance(v, float) for k, v in e.items() if not torch.is_tensor(v))


def test_job_script_prints_nbest(dev, capsys):
    spec = importlib.util.spec_from_file_location("wav2vec2_asr_job", os.path.join(ROOT, "speech_jobs", "wav2vec2_asr.py"))
    job = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(job)
    job.main(["--model_size", "tiny", "--batch_size", "2", "--seconds", "0.5", "--num_beams", "4", "--nbest", "2", "--timestamps"])
    lines = [json.loads(x) for x in capsys.readouterr().out.strip().splitlines()]
    assert len(lines) == 3 and lines[-1]["clips"] == 2
    for line in lines[:2]:
        assert 1 <= line["n_beams"] <= 4 and len(line["nbest"]) == min(2, line["n_beams"])
        assert line["nbest"][0]["tokens"] == line["tokens"] and line["nbest"][0]["score"] == line["sequence_score"]
        assert all(a["score"] >= b["score"] for a, b in zip(line["nbest"], line["nbest"][1:]))
        assert len(line["start"]) == len(line["end"]) == len(line["tokens"]) and "best_path_logprob" not in line
    job.main(["--model_size", "tiny", "--batch_size", "2", "--seconds", "0.5"])
    plain = [json.loads(x) for x in capsys.readouterr().out.strip().splitlines()]
    assert set(plain[0]) == {"clip", "frames", "tokens", "best_path_logprob"}      # the default output is as it was
    with pytest.raises(SystemExit):
        job.main(["--model_size", "tiny", "--nbest", "2"])
