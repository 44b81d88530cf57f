"""Wav2Vec2ForCTC.decode(num_beams=K, lm=...) / evaluate(..., lm=...) on the GPU (the tiny configuration and the padded
batch of tests/test_ctc_beam_gpu.py): the fused result bit-equal to ops.ctc_beam_lm on the model's own log-probs, ``lm=None``
bit-equal to the unfused kernel, timestamps equal to ``align`` on the fused best sequences, evaluate's edit distances
those of the fused best beam, a table that allows one token chain only forcing that chain, and the job script's n-best
output with the three scores."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import _ctc_lm_ref as L
import _ctc_ref as C
from oracle import wav2vec2_oracle as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_IN = 9600                                  # 0.6 s
SAMPLE_LENS = (9600, 7200, 4800)             # 0.6, 0.45 and 0.3 s
TINY = dict(hidden_size=64, num_hidden_layers=2, num_attention_heads=1, intermediate_size=128, conv_dim=(64, 64, 64),
            conv_stride=(5, 2, 2), conv_kernel=(10, 3, 2), num_conv_pos_embeddings=8, num_conv_pos_embedding_groups=4,
            num_codevectors_per_group=16, codevector_dim=32, proj_codevector_dim=64, num_negatives=10)
I32 = torch.int32
ALPHA, BETA = 0.75, 0.5


def W():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import wav2vec2
    return wav2vec2


@pytest.fixture(scope="module")
def setup(dev):
    """The model (the head scaled up so that the argmax moves between symbols), the padded batch, its mask, the model's own
    log-probs and an order-2 table, once for the module."""
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
    Vn = m.config.vocab_size
    lm = L.lm_table(Vn, 2, 5).astype(np.float32).reshape(Vn, Vn)
    s = {"m": m, "x": x, "mask": mask, "fl": fl, "logp": out["log_probs"].contiguous(), "T": mask.shape[1], "lm": lm}
    yield s
    s.clear()
    import gc
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def beam_direct(s, K, dev, lm=None, alpha=ALPHA, beta=BETA):
    from tethys_speech_amd import ops
    B, T = 3, s["T"]
    tok = torch.full((B, K, T), -1, dtype=I32, device=dev)
    ln, nb = torch.zeros(B, K, dtype=I32, device=dev), torch.zeros(B, dtype=I32, device=dev)
    sc, ctc, lms = (torch.zeros(B, K, dtype=torch.float32, device=dev) for _ in range(3))
    ws = torch.empty(ops.ctc_beam_workspace_elems(B, K, T), dtype=I32, device=dev)
    fl = torch.tensor(s["fl"], dtype=I32, device=dev)
    if lm is None:
        ops.ctc_beam(s["logp"], fl, s["m"].config.ctc_blank_id, K, tok, ln, sc, nb, ws)
    else:
        table = torch.from_numpy(np.ascontiguousarray(lm, dtype=np.float32).reshape(-1)).to(dev)
        ops.ctc_beam_lm(s["logp"], fl, s["m"].config.ctc_blank_id, K, table, lm.ndim, alpha, beta, tok, ln, sc, ctc, lms, nb, ws)
    torch.cuda.synchronize()
    return tok, ln, sc, ctc, lms, nb


def test_decode_with_lm_equals_the_kernel_on_the_models_log_probs(dev, setup):
    s, m = setup, setup["m"]
    K, Rn = 4, 2
    d = m.decode(s["x"], attention_mask=s["mask"], num_beams=K, num_return_sequences=Rn, lm=s["lm"], lm_alpha=ALPHA, lm_beta=BETA)
    tok, ln, sc, ctc, lms, nb = beam_direct(s, K, dev, s["lm"])
    n = int(ln[:, :Rn].max())
    assert set(d) == {"sequences", "lengths", "sequences_scores", "ctc_scores", "lm_scores", "n_beams"}
    assert n >= 3 and d["sequences"].dtype == I32 and tuple(d["sequences"].shape) == (3, Rn, n)
    assert torch.equal(d["sequences"], tok[:, :Rn, :n]) and torch.equal(d["lengths"], ln[:, :Rn]) and torch.equal(d["n_beams"], nb)
    for name, want in (("sequences_scores", sc), ("ctc_scores", ctc), ("lm_scores", lms)):
        assert tuple(d[name].shape) == (3, Rn) and torch.equal(d[name].view(I32), want[:, :Rn].view(I32)), name
    # the same table as a torch tensor, flat, in float64; R = 1 drops the rank dimension of all three scores
    d1 = m.decode(s["x"], attention_mask=s["mask"], num_beams=K, lm=torch.from_numpy(s["lm"]).double().reshape(-1),
                  lm_alpha=ALPHA, lm_beta=BETA)
    assert tuple(d1["lengths"].shape) == (3,) and torch.equal(d1["sequences"], tok[:, 0, :d1["sequences"].shape[1]])
    for name, want in (("sequences_scores", sc), ("ctc_scores", ctc), ("lm_scores", lms)):
        assert torch.equal(d1[name].view(I32), want[:, 0].view(I32)), name
    # against float64 on the returned log-probs: g along the tokens bit for bit, the fused score one fp32 add
    sc_h, ctc_h, lm_h = (d[k].cpu().numpy() for k in ("sequences_scores", "ctc_scores", "lm_scores"))
    seqs_h, len_h = d["sequences"].cpu().numpy(), d["lengths"].cpu().numpy()
    Vn, blank = m.config.vocab_size, m.config.ctc_blank_id
    for b in range(3):
        assert int(nb[b]) == K and (np.diff(sc_h[b]) <= 0).all() and (sc_h[b] == ctc_h[b] + lm_h[b]).all()
        for r in range(Rn):
            seq = tuple(seqs_h[b, r, :len_h[b, r]].tolist())
            g = L.g_along(seq, s["lm"].astype(np.float64), 2, ALPHA, BETA, Vn, blank)
            assert g.view(np.int32) == lm_h[b, r].view(np.int32), (b, r)
    # the model changes what is found: with these weights the fused best differs from the unfused best somewhere, or ranks differently
    plain = beam_direct(s, K, dev)
    assert not (torch.equal(plain[0], tok) and torch.equal(plain[1], ln))


def test_without_lm_the_result_is_todays(dev, setup):
    s, m = setup, setup["m"]
    K, Rn = 4, 3
    tok, ln, sc, _, _, nb = beam_direct(s, K, dev)
    n = int(ln[:, :Rn].max())
    for d in (m.decode(s["x"], attention_mask=s["mask"], num_beams=K, num_return_sequences=Rn),
              m.decode(s["x"], attention_mask=s["mask"], num_beams=K, num_return_sequences=Rn, lm=None, lm_alpha=2.0, lm_beta=1.0)):
        assert set(d) == {"sequences", "lengths", "sequences_scores", "n_beams"}
        assert torch.equal(d["sequences"], tok[:, :Rn, :n]) and torch.equal(d["lengths"], ln[:, :Rn])
        assert torch.equal(d["sequences_scores"].view(I32), sc[:, :Rn].view(I32)) and torch.equal(d["n_beams"], nb)
    # zero weights: the unfused search, its scores as numbers
    z = m.decode(s["x"], attention_mask=s["mask"], num_beams=K, num_return_sequences=Rn, lm=s["lm"], lm_alpha=0.0, lm_beta=0.0)
    assert torch.equal(z["sequences"], tok[:, :Rn, :n]) and bool((z["sequences_scores"] == sc[:, :Rn]).all())
    assert bool((z["ctc_scores"] == sc[:, :Rn]).all()) and bool((z["lm_scores"] == 0).all())
    for kw in (dict(lm=s["lm"]), dict(lm=s["lm"], num_beams=1), dict(lm=s["lm"][:, :-1], num_beams=4),
               dict(lm=s["lm"], num_beams=4, lm_alpha=-1.0), dict(lm=s["lm"], num_beams=4, lm_beta=float("nan"))):
        with pytest.raises(ValueError):
            m.decode(s["x"], attention_mask=s["mask"], **kw)
    with pytest.raises(ValueError):
        m.evaluate(s["x"], torch.ones(3, 2, dtype=torch.int64), attention_mask=s["mask"], lm=s["lm"])


def test_timestamps_equal_align_on_the_fused_best_sequences(dev, setup):
    s, m = setup, setup["m"]
    d = m.decode(s["x"], attention_mask=s["mask"], num_beams=4, num_return_sequences=2, return_timestamps=True, lm=s["lm"],
                 lm_alpha=ALPHA, lm_beta=BETA)
    tok, ln = beam_direct(s, 4, dev, s["lm"])[:2]
    best, lens = d["sequences"][:, 0], d["lengths"][:, 0]
    nb = int(lens.max())
    assert torch.equal(best[:, :nb], tok[:, 0, :nb]) and torch.equal(lens, ln[:, 0])
    labels = best[:, :nb].clamp_min(0).to(torch.int64).cpu()
    for b in range(3):
        labels[b, int(lens[b]):] = 1        # (past a length: any valid symbol)
    a = m.align(s["x"], labels, lens.cpu().tolist(), attention_mask=s["mask"])
    assert tuple(d["token_start_frames"].shape) == (3, nb) and int(a["infeasible"].sum()) == 0
    for k in ("token_start_frames", "token_end_frames", "token_start_times", "token_end_times"):
        assert torch.equal(d[k], a[k]), k


def test_evaluate_with_lm_reports_the_fused_best_beams_edits(dev, setup):
    s, m = setup, setup["m"]
    K = 4
    tok, ln = beam_direct(s, K, dev, s["lm"])[:2]
    best = [tok[b, 0, :int(ln[b, 0])].cpu().tolist() for b in range(3)]
    labels = torch.zeros(3, max(len(best[0]), 9), dtype=torch.int64)
    lens = [len(best[0]), 9, 5]
    labels[0, :lens[0]] = torch.tensor(best[0])           # item 0 against its own fused best beam: no edit
    labels[1, :9] = torch.from_numpy(C.labels_for("random", 9, m.config.vocab_size, seed=1))
    labels[2, :5] = torch.from_numpy(C.labels_for("random", 5, m.config.vocab_size, seed=2))
    e = m.evaluate(s["x"], labels, lens, attention_mask=s["mask"], return_items=True, num_beams=K, lm=s["lm"], lm_alpha=ALPHA,
                   lm_beta=BETA)
    g = m.evaluate(s["x"], labels, lens, attention_mask=s["mask"], return_items=True)
    edits = [C.levenshtein(best[b], labels[b, :lens[b]].tolist()) for b in range(3)]
    assert edits[0] == 0 and e["n_edits"] == float(sum(edits)) and e["token_error_rate"] == sum(edits) / sum(lens)
    for k in ("nll_sum", "loss", "n_items", "n_infeasible", "n_ref_tokens"):
        assert e[k] == g[k], k
    assert torch.equal(e["nll"].view(I32), g["nll"].view(I32)) and torch.equal(e["sequences"], g["sequences"])
    nb = max(len(x) for x in best)
    assert torch.equal(e["beam_sequences"], tok[:, 0, :nb]) and torch.equal(e["beam_lengths"], ln[:, 0])


def test_a_table_that_allows_one_chain_forces_it(dev, setup):
    """-inf everywhere except start -> 5 -> 9 -> 2 -> 5 -> ...: every beam is a prefix of that chain."""
    s, m = setup, setup["m"]
    Vn, blank = m.config.vocab_size, m.config.ctc_blank_id
    chain = [5, 9, 2]
    assert blank not in chain
    lm = np.full((Vn, Vn), -np.inf, dtype=np.float32)
    lm[blank, chain[0]] = -0.5
    for a, b in zip(chain, chain[1:] + chain[:1]):
        lm[a, b] = -0.5
    K = 4
    d = m.decode(s["x"], attention_mask=s["mask"], num_beams=K, num_return_sequences=K, lm=lm, lm_alpha=1.0, lm_beta=0.0)
    seqs, lens, nb = d["sequences"].cpu().numpy(), d["lengths"].cpu().numpy(), d["n_beams"].cpu().numpy()
    for b in range(3):
        assert 1 <= nb[b] <= K
        found = set()
        for r in range(int(nb[b])):
            seq = seqs[b, r, :lens[b, r]].tolist()
            assert seq == [chain[i % 3] for i in range(len(seq))], (b, r, seq)
            assert float(d["lm_scores"][b, r]) == -0.5 * len(seq)
            found.add(len(seq))
        assert len(found) == int(nb[b]) and max(found) >= 1           # distinct prefixes of the one chain, not only the empty one
        assert bool(torch.isneginf(d["sequences_scores"][b, int(nb[b]):]).all())


def test_job_script_prints_nbest_with_the_three_scores(dev, capsys, tmp_path):
    spec = importlib.util.spec_from_file_location("wav2vec2_asr_job_lm", os.path.join(ROOT, "speech_jobs", "wav2vec2_asr.py"))
    job = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(job)
    labels, table = tmp_path / "labels.txt", tmp_path / "lm.npy"
    labels.write_text("1 2 3 4\n5 6 5 6 7\n\n3 3 1\n")
    job.main(["--model_size", "tiny", "--build_lm", str(labels), "--lm_order", "2", "--lm_out", str(table)])
    built = json.loads(capsys.readouterr().out.strip())
    assert built["order"] == 2 and built["sequences"] == 4 and built["tokens"] == 12
    lm = np.load(table)
    assert lm.shape == (32, 32) and lm.dtype == np.float32 and np.array_equal(lm, W().ngram_lm_table(
        [[1, 2, 3, 4, 0], [5, 6, 5, 6, 7], [0] * 5, [3, 3, 1, 0, 0]], [4, 5, 0, 3], 2, 32, 0))
    job.main(["--model_size", "tiny", "--batch_size", "2", "--seconds", "0.5", "--num_beams", "4", "--nbest", "2", "--timestamps",
              "--lm", str(table), "--lm_alpha", "0.5", "--lm_beta", "0.25"])
    lines = [json.loads(x) for x in capsys.readouterr().out.strip().splitlines()]
    assert len(lines) == 3 and lines[-1]["clips"] == 2
    for line in lines[:2]:
        assert 1 <= line["n_beams"] <= 4 and len(line["nbest"]) == min(2, line["n_beams"])
        first = line["nbest"][0]
        assert first["tokens"] == line["tokens"] and first["score"] == line["sequence_score"]
        assert first["ctc_score"] == line["ctc_score"] and first["lm_score"] == line["lm_score"]
        for entry in line["nbest"]:
            assert entry["score"] == float(np.float32(entry["ctc_score"]) + np.float32(entry["lm_score"]))
        assert all(a["score"] >= b["score"] for a, b in zip(line["nbest"], line["nbest"][1:]))
        assert len(line["start"]) == len(line["end"]) == len(line["tokens"])
    job.main(["--model_size", "tiny", "--batch_size", "2", "--seconds", "0.5", "--num_beams", "4"])
    plain = [json.loads(x) for x in capsys.readouterr().out.strip().splitlines()]
    assert "ctc_score" not in plain[0] and "lm_score" not in plain[0]      # without a table the output is as it was
    with pytest.raises(SystemExit):
        job.main(["--model_size", "tiny", "--lm", str(table)])
    with pytest.raises(SystemExit):
        job.main(["--model_size", "tiny", "--build_lm", str(labels)])
