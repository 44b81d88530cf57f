"""Wav2Vec2ForCTC on the GPU (tiny config: 1 head of 64, 2 layers, 40 frames; bf16 and fp32): the head against a float64
head over the returned last hidden state with the bound of tests/_gemm_ref.py, and decode / evaluate / align against the
references of tests/_ctc_ref.py applied to the model's own returned log-probs - integer outputs exactly, nll within its
derived bound.  Also: a padded batch with a prefix mask, evaluate's sums over two half-batches, the training state and a
recorded plan of a pre-training model in the same process, load_pretrained_encoder, and the training calls that raise."""
import math

import numpy as np
import pytest
import torch

import _ctc_ref as C
import _gemm_ref as GR
from _margins import within
from oracle import wav2vec2_oracle as V

pytestmark = pytest.mark.gpu

T_IN, T = 800, 40
TINY = dict(hidden_size=64, num_hidden_layers=2, num_attention_heads=1, intermediate_size=128, conv_dim=(64, 64, 64),
            conv_stride=(5, 2, 2), conv_kernel=(10, 3, 2), num_conv_pos_embeddings=8, num_conv_pos_embedding_groups=4,
            num_codevectors_per_group=16, codevector_dim=32, proj_codevector_dim=64, num_negatives=10)


@pytest.fixture(scope="module")
def models():
    """The CTC models of this module, one per configuration, released when the module is done: a model owns a stream and
    its events, and the tests that follow measure run-to-run spreads of the training step."""
    cache = {}
    yield cache
    cache.clear()
    import gc
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def W():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import wav2vec2
    return wav2vec2


def model_for(models, precision, dev, **kw):
    """One CTC model per precision, shared by the tests: the head is scaled up so that the argmax moves between symbols."""
    key = (precision, tuple(sorted(kw.items())))
    if key not in models:
        m = W().create_full_model("asr", "base", device=dev, precision=precision, seed=7, **TINY, **kw)
        g = torch.Generator().manual_seed(3)
        m.arena.param("lm_head.kernel").mul_(12.0)
        m.arena.param("lm_head.bias").copy_((torch.randn(m.config.vocab_size, generator=g) * 0.3).to(dev))
        m.refresh_shadows()
        models[key] = m
    return models[key]


def clips(B, seed=5):
    return torch.from_numpy(V.create_dummy_pool(seed=seed, num_samples=B, length=T_IN))


def f64(t):
    return t.detach().double().cpu().numpy()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_head_matches_float64(dev, models, precision):
    m = model_for(models, precision, dev)
    cfg = m.config
    assert type(m).__name__ == "Wav2Vec2ForCTC"
    out = m(clips(3).to(dev))
    B, H, Vn = 3, cfg.hidden_size, cfg.vocab_size
    assert out["logits"].dtype == out["log_probs"].dtype == torch.float32
    assert tuple(out["logits"].shape) == tuple(out["log_probs"].shape) == (B, T, Vn)
    assert tuple(out["last_hidden_state"].shape) == (B, T, H) and "extract_features" in out
    x = f64(out["last_hidden_state"]).reshape(-1)
    w, _ = m.W("lm_head.kernel")   # what the GEMM read: the bf16 mirror on the bf16 model
    ref = GR.gemm_ref(x, f64(w).reshape(-1), np.zeros(B * T * Vn), B * T, Vn, H, H, 1, Vn, 1, Vn,
                      bias=f64(m.arena.param("lm_head.bias")), out_bf16=False, in_f32=precision == "fp32")
    r = GR.worst_ratio(f64(out["logits"]).reshape(1, 1, B * T, Vn), ref["ref"], ref["bound"])
    print(f"ctc head logits {precision}: {r:.3f} of the bound")
    within(f"ctc head logits {precision}", r, 1.0)
    logits = f64(out["logits"]).reshape(B * T, Vn)
    logp, amax, bound = C.logsoftmax_ref(logits)
    r = C.ratio(f64(out["log_probs"]).reshape(B * T, Vn), logp, bound)
    within(f"ctc head log_probs {precision}", r, 1.0)
    assert len(set(amax.tolist())) > 3, "the test's head does not move between symbols"


def batch_with_mask(m, dev):
    """B = 4 padded clips: 40, 33, 17 and 40 frames."""
    sample_lens = (T_IN, 33 * 20, 17 * 20, T_IN)
    mask = W().frame_attention_mask(m.config, sample_lens, T_IN)
    assert mask.sum(dim=1).tolist() == [40, 33, 17, 40]
    return clips(4, seed=8).to(dev), mask, [40, 33, 17, 40]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_decode_evaluate_align_equal_the_references(dev, models, precision):
    m = model_for(models, precision, dev)
    cfg = m.config
    x, mask, fl = batch_with_mask(m, dev)
    B = 4
    out = m(x, attention_mask=mask)
    lp, logits = f64(out["log_probs"]), f64(out["logits"])
    amax = np.argmax(logits, axis=2)

    # ---- decode
    d = m.decode(x, attention_mask=mask)
    refs = [C.greedy_ref(amax[b], lp[b], fl[b], cfg.ctc_blank_id) for b in range(B)]
    n = max(len(r["tokens"]) for r in refs)
    assert n >= 3 and tuple(d["sequences"].shape) == (B, n) and d["sequences"].dtype == torch.int32
    sec = W().frame_seconds(cfg)
    assert sec == 20 / 16000
    for b, r in enumerate(refs):
        k = len(r["tokens"])
        assert int(d["lengths"][b]) == k
        for name, key in (("sequences", "tokens"), ("token_start_frames", "start"), ("token_end_frames", "end")):
            row = d[name][b].cpu().numpy()
            assert np.array_equal(row[:k], r[key]) and (row[k:] == -1).all(), (b, name)
        for name, key in (("token_start_times", "start"), ("token_end_times", "end")):
            row = d[name][b].cpu().numpy()
            assert np.array_equal(row[:k], r[key] * sec) and (row[k:] == -1).all(), (b, name)
        assert (r["end"] <= fl[b]).all(), "a token past the clip's frames: the mask's frame_lens were not used"
        within(f"ctc model best_path_logprob {precision}", C.ratio([float(d["best_path_logprob"][b])], [r["best"]], [r["best_bound"]]), 1.0)

    # ---- evaluate: item 0 scored against its own transcript, 1 against random labels, 2 has too few frames, 3 has none
    L_max = max(len(refs[0]["tokens"]), 20)
    labels = np.zeros((B, L_max), dtype=np.int64)
    lens = [len(refs[0]["tokens"]), 9, 20, 0]
    labels[0, :lens[0]] = refs[0]["tokens"]
    labels[1, :9] = C.labels_for("random", 9, cfg.vocab_size, seed=1)
    labels[2, :20] = C.labels_for("equal", 20, cfg.vocab_size, seed=2)   # needs 39 frames, the clip has 17
    e = m.evaluate(x, torch.from_numpy(labels), lens, attention_mask=mask, return_items=True)
    fr = [C.ctc_forward_ref(lp[b], labels[b, :lens[b]], fl[b], cfg.ctc_blank_id) for b in range(B)]
    assert [r["infeasible"] for r in fr] == [0, 0, 1, 0] and e["infeasible"].tolist() == [0, 0, 1, 0]
    nll = f64(e["nll"])
    for b, r in enumerate(fr):
        if r["infeasible"]:
            assert nll[b] == math.inf
        else:
            ratio = C.ratio([nll[b]], [r["nll"]], [r["bound"]])
            print(f"ctc model nll {precision} item {b}: {ratio:.4f} of the bound {r['bound']:.3e}")
            within(f"ctc model nll {precision}", ratio, 1.0)
    assert all(isinstance(v, float) for k, v in e.items() if k not in ("nll", "infeasible", "sequences", "lengths"))
    assert e["n_items"] == 4.0 and e["n_infeasible"] == 1.0 and e["loss"] == math.inf
    assert e["nll_sum"] == float(nll[[0, 1, 3]].sum())
    edits = [C.levenshtein(refs[b]["tokens"].tolist(), labels[b, :lens[b]].tolist()) for b in range(B)]
    assert edits[0] == 0 and e["n_edits"] == float(sum(edits)) and e["n_ref_tokens"] == float(sum(lens))
    assert e["token_error_rate"] == sum(edits) / sum(lens)

    # ---- align: the same fp32 adds as the fp32 transcription, so the same path bit for bit; against float64 within e(P) + e(P*)
    a = m.align(x, torch.from_numpy(labels), lens, attention_mask=mask, return_states=True)
    assert a["infeasible"].tolist() == [0, 0, 1, 0] and tuple(a["token_start_frames"].shape) == (B, L_max)
    for b in range(B):
        lab = labels[b, :lens[b]]
        r32, r64 = C.viterbi_ref(lp[b], lab, fl[b], dtype=np.float32), C.viterbi_ref(lp[b], lab, fl[b])
        st, en = a["token_start_frames"][b].cpu().numpy(), a["token_end_frames"][b].cpu().numpy()
        states = a["states"][b].cpu().numpy()
        assert np.array_equal(st[:lens[b]], r32["start"]) and np.array_equal(en[:lens[b]], r32["end"]), b
        assert (st[lens[b]:] == -1).all() and (en[lens[b]:] == -1).all()
        assert np.array_equal(states[:fl[b]], r32["states"]) and (states[fl[b]:] == -1).all(), b
        assert float(a["path_logprob"][b]) == r32["total"]
        assert np.array_equal(a["token_start_times"][b].cpu().numpy(), np.where(st >= 0, st * sec, -1.0))
        if not r64["infeasible"]:
            assert C.path_problems(states[:fl[b]], lab, fl[b], st[:lens[b]], en[:lens[b]]) == []
            deficit = r64["total"] - C.path_score(lp[b], lab, states[:fl[b]])
            bound = C.path_bound(lp[b], lab, states[:fl[b]]) + C.path_bound(lp[b], lab, r64["states"])
            within(f"ctc model align deficit {precision}", max(deficit, 0.0) / bound, 1.0)


def test_loss_reductions(dev, models):
    """"sum" and "mean" as torch's ctc_loss; an infeasible item counts +inf, or 0 with ctc_zero_infinity."""
    x = clips(2, seed=8).to(dev)
    labels, lens = torch.tensor([[3, 4, 5], [6, 7, 0]]), [3, 2]
    m = model_for(models, "fp32", dev)
    e = m.evaluate(x, labels, lens, return_items=True)
    nll = f64(e["nll"])
    assert e["loss"] == float(nll.sum()) == e["nll_sum"]
    mm = model_for(models, "fp32", dev, ctc_loss_reduction="mean", ctc_zero_infinity=True)
    e2 = mm.evaluate(x, labels, lens, return_items=True)
    assert torch.equal(e2["nll"], e["nll"]) and e2["loss"] == float((nll / np.array([3, 2])).mean())
    long = torch.full((2, 45), 3)   # 45 equal labels need 89 frames
    e3 = mm.evaluate(x, long)
    assert e3["n_infeasible"] == 2.0 and e3["loss"] == 0.0 and e3["nll_sum"] == 0.0
    assert m.evaluate(x, long)["loss"] == math.inf


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_evaluate_sums_add_over_two_half_batches(dev, models, precision):
    m = model_for(models, precision, dev)
    x = clips(4, seed=11).to(dev)
    labels = torch.from_numpy(np.stack([C.labels_for("random", 6, m.config.vocab_size, seed=s) for s in range(4)]))
    lens = [6, 4, 5, 0]
    whole = m.evaluate(x, labels, lens, return_items=True)
    halves = [m.evaluate(x[i:i + 2], labels[i:i + 2], lens[i:i + 2], return_items=True) for i in (0, 2)]
    for k in ("n_items", "n_infeasible", "n_edits", "n_ref_tokens"):
        assert whole[k] == halves[0][k] + halves[1][k], k
    parts = torch.cat([halves[0]["nll"], halves[1]["nll"]])
    print(f"ctc evaluate halves {precision}: per-item nll differs by {float((parts - whole['nll']).abs().max()):.3e}")
    # every kernel of the pass works on a batch item (or a row) alone, in the same order whatever the batch: the same bits
    assert torch.equal(parts, whole["nll"])
    assert abs(whole["nll_sum"] - (halves[0]["nll_sum"] + halves[1]["nll_sum"])) <= 1e-12 * abs(whole["nll_sum"])


def test_training_state_is_untouched_and_training_calls_raise(dev, models):
    m = model_for(models, "bf16", dev)
    x, mask, _ = batch_with_mask(m, dev)
    labels = torch.full((4, 3), 5)
    m.decode(x, attention_mask=mask)
    m.evaluate(x, labels, attention_mask=mask)
    m.align(x, labels, attention_mask=mask)
    torch.cuda.synchronize()
    assert m._ws_sets == {} and m._ws_key is None and m._drop_step == 0 and m.ws == {}
    assert not bool(m.arena.g.any()) and not bool(m.arena.m.any())
    with pytest.raises(NotImplementedError, match="CTC fine-tuning is not built"):
        m.forward_backward(x, None)
    with pytest.raises(NotImplementedError, match="CTC fine-tuning is not built"):
        m(x, training=True)
    with pytest.raises(ValueError):
        m.evaluate(x, torch.zeros(4, 3, dtype=torch.int64))   # the blank as a label
    with pytest.raises(ValueError):
        m.decode(x, attention_mask=torch.ones(4, T + 1))


def test_recorded_plan_of_a_pretraining_model_replays_the_same_around_ctc_calls(dev, models):
    from tethys_speech_amd import ops, optim, train
    from tethys_speech_amd.dist import DataParallelStrategy
    from test_w2v_infer_gpu import _train_inputs
    from test_wav2vec2_gpu import build
    ctc = model_for(models, "bf16", dev)
    x, mask, _ = batch_with_mask(ctc, dev)

    def run(infer):
        model, _, _ = build("bf16", dev)
        opt = optim.Adam(3e-4, epsilon=1e-8)
        inputs = [_train_inputs(model, 3, 400, 60 + i, dev)[:2] for i in range(3)]
        old, train.USE_PLAN = train.USE_PLAN, True
        try:
            step = train.planned_step(DataParallelStrategy(0, 1, init=False), model, opt, "wav2vec2", pipelined=True)
            losses = []
            for i in range(8):
                if infer and i == 5:
                    assert step.planned is not None and step.planned.replays >= 1, "no plan was recorded before the calls"
                    state = (model._drop_step, model._ws_key, sorted(model._ws_sets))
                    ctc.decode(x, attention_mask=mask)
                    ctc.evaluate(x, torch.full((4, 3), 5), attention_mask=mask)
                    ctc.align(x, torch.full((4, 3), 5), attention_mask=mask)
                    assert state == (model._drop_step, model._ws_key, sorted(model._ws_sets))
                losses.append(step(*inputs[i % 3]))
            model.finish_late()
            torch.cuda.synchronize()
            assert step.planned is not None and step.planned.replays >= 4
            return [float(v.item()) for v in losses], model.arena.p.clone()
        finally:
            train.USE_PLAN = old

    was = ops.set_deterministic(True)
    try:
        la, pa = run(False)
        lb, pb = run(False)
        lc, pc = run(True)
    finally:
        ops.set_deterministic(was)
    spread = float((pa - pb).abs().max())   # (fp32 atomics of the Wav2Vec2 step: tests/test_w2v_infer_gpu.py)
    assert float((pa - pc).abs().max()) <= max(4.0 * spread, 1e-7), (float((pa - pc).abs().max()), spread)
    assert max(abs(a - b) for a, b in zip(la, lc)) <= max(4.0 * max(abs(a - b) for a, b in zip(la, lb)), 1e-6 * abs(la[0]))


def test_load_pretrained_encoder_round_trips_the_shared_tensors(dev, tmp_path):
    from tethys_speech_amd import train
    wav2vec2 = W()
    pre = wav2vec2.create_full_model("pretraining", "base", device=dev, precision="bf16", seed=21, **TINY)
    path = str(tmp_path / "pre.pt")
    train.save_weights(pre, path)
    m = wav2vec2.create_full_model("asr", "base", device=dev, precision="bf16", seed=22, **TINY)
    head = {k: m.arena.param(k).clone() for k in ("lm_head.kernel", "lm_head.bias")}
    copied = wav2vec2.load_pretrained_encoder(m, path)
    src, dst = pre.arena.ref_views(pre.arena.p), m.arena.ref_views(m.arena.p)
    assert set(copied) == {k for k in dst if not k.startswith("lm_head.")} and len(copied) > 20
    for k in copied:
        assert torch.equal(dst[k], src[k]), k
    for k, v in head.items():
        assert torch.equal(m.arena.param(k), v), k
    assert torch.equal(m.mirror.float(), m.arena.p.to(torch.bfloat16).float()), "the bf16 mirror was not refreshed"
    x = clips(2).to(dev)   # and the encoder computes what the pre-training model's does
    assert torch.equal(m(x)["last_hidden_state"], pre.forward_infer(x)["last_hidden_state"])
    other = wav2vec2.create_full_model("asr", "base", device=dev, precision="bf16", **dict(TINY, intermediate_size=256))
    with pytest.raises(ValueError, match="shape"):
        wav2vec2.load_pretrained_encoder(other, path)
