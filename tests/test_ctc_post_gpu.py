"""Wav2Vec2ForCTC.posteriors on the GPU (the tiny config of tests/test_ctc_gpu.py; fp32 and bf16; B = 3 with one padded
clip): against the float64 reference of tests/_ctc_post_ref.py fed the model's own returned log-probs (fp32, taken as exact
inputs) within its derived bounds, nll against evaluate's bit for bit, the padding conventions, two half batches (of a batch of 4)
against the whole, the training state, the training calls that still raise, and a recorded plan of a pre-training model in the
same process."""
import math

import numpy as np
import pytest
import torch

import _ctc_post_ref as P
import _ctc_ref as C
from _margins import within
from oracle import wav2vec2_oracle as V

pytestmark = pytest.mark.gpu

T_IN, T = 800, 40
TINY = dict(hidden_size=64, num_hidden_layers=2, num_attention_heads=1, intermediate_size=128, conv_dim=(64, 64, 64),
            conv_stride=(5, 2, 2), conv_kernel=(10, 3, 2), num_conv_pos_embeddings=8, num_conv_pos_embedding_groups=4,
            num_codevectors_per_group=16, codevector_dim=32, proj_codevector_dim=64, num_negatives=10)
FRAMES = [40, 33, 40]
L_MAX = 30


@pytest.fixture(scope="module")
def models():
    """One CTC model per precision, released when the module is done (a model owns a stream and its events)."""
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


def model_for(models, precision, dev):
    """The head is scaled up so that the posteriors are not near-uniform."""
    if precision not in models:
        m = W().create_full_model("asr", "base", device=dev, precision=precision, seed=7, **TINY)
        g = torch.Generator().manual_seed(3)
        m.arena.param("lm_head.kernel").mul_(12.0)
        m.arena.param("lm_head.bias").copy_((torch.randn(m.config.vocab_size, generator=g) * 0.3).to(dev))
        m.refresh_shadows()
        models[precision] = m
    return models[precision]


def f64(t):
    return t.detach().double().cpu().numpy()


def batch(m, dev, B=3):
    """B = 3 clips of 40, 33 (padded) and 40 frames; item 0 with 6 labels, item 1 with 9, item 2 with 30 equal labels, which
    need 59 frames: no path.  B = 4 adds a clip of 17 frames with 4 labels."""
    mask = W().frame_attention_mask(m.config, (T_IN, 33 * 20, T_IN, 17 * 20)[:B], T_IN)
    assert mask.sum(dim=1).tolist() == (FRAMES + [17])[:B]
    x = torch.from_numpy(V.create_dummy_pool(seed=8, num_samples=B, length=T_IN)).to(dev)
    Vn = m.config.vocab_size
    labels, lens = np.zeros((B, L_MAX), dtype=np.int64), [6, 9, 30, 4][:B]
    labels[0, :6] = C.labels_for("random", 6, Vn, seed=1)
    labels[1, :9] = C.labels_for("alt", 9, Vn, seed=2)
    labels[2, :30] = C.labels_for("equal", 30, Vn, seed=3)
    if B > 3:
        labels[3, :4] = C.labels_for("random", 4, Vn, seed=4)
    return x, mask, torch.from_numpy(labels), lens


KEYS = ("nll", "infeasible", "symbol_posteriors", "token_expected_frames", "token_center_frames", "token_center_times",
        "logit_grad", "state_posteriors")


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_posteriors_equal_the_reference_on_the_models_log_probs(dev, models, precision):
    m = model_for(models, precision, dev)
    cfg = m.config
    x, mask, labels, lens = batch(m, dev)
    B, Vn = 3, cfg.vocab_size
    lp = f64(m(x, attention_mask=mask)["log_probs"])
    out = m.posteriors(x, labels, lens, attention_mask=mask, return_logit_grad=True, return_states=True)
    assert sorted(out) == sorted(KEYS)
    plain = m.posteriors(x, labels, lens, attention_mask=mask)
    assert sorted(plain) == sorted(KEYS[:6]) and all(torch.equal(plain[k], out[k]) for k in plain)
    assert tuple(out["symbol_posteriors"].shape) == tuple(out["logit_grad"].shape) == (B, T, Vn)
    assert tuple(out["state_posteriors"].shape) == (B, T, 2 * L_MAX + 1)
    for k in ("token_expected_frames", "token_center_frames", "token_center_times"):
        assert tuple(out[k].shape) == (B, L_MAX)
    assert out["token_center_times"].dtype == torch.float64 and out["nll"].dtype == torch.float32
    assert out["infeasible"].dtype == torch.int32 and out["infeasible"].tolist() == [0, 0, 1]
    e = m.evaluate(x, labels, lens, attention_mask=mask, return_items=True)
    assert torch.equal(out["nll"].view(torch.int32), e["nll"].view(torch.int32)) and torch.equal(out["infeasible"], e["infeasible"])
    assert float(out["nll"][2]) == math.inf
    sec = W().frame_seconds(cfg)
    for b in range(B):
        L, Tb = lens[b], FRAMES[b]
        ref = P.post_ref(lp[b], labels[b, :L].numpy(), Tb, cfg.ctc_blank_id)
        got = {"gamma": f64(out["state_posteriors"][b, :Tb, :2 * L + 1]), "occ": f64(out["symbol_posteriors"][b, :Tb]),
               "grad": f64(out["logit_grad"][b, :Tb]), "tok_frames": f64(out["token_expected_frames"][b, :L]),
               "tok_center": f64(out["token_center_frames"][b, :L])}
        r = P.ratios(got, ref)
        print(f"ctc post model {precision} item {b}: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()) + " of the bound;  "
              + P.bound_report("", ref))
        for k, v in r.items():
            within(f"ctc post model {precision} {k}", v, 1.0)
        # the padding conventions
        assert not bool(out["symbol_posteriors"][b, Tb:].any()) and not bool(out["logit_grad"][b, Tb:].any())
        assert not bool(out["state_posteriors"][b, Tb:].any()) and not bool(out["state_posteriors"][b, :, 2 * L + 1:].any())
        for k in ("token_expected_frames", "token_center_frames", "token_center_times"):
            assert bool((out[k][b, L:] == -1).all()), (b, k)
        cen = out["token_center_frames"][b, :L]
        assert torch.equal(out["token_center_times"][b, :L], torch.where(cen >= 0, cen.double() * sec, -1.0))
        if ref["infeasible"]:
            assert not bool(out["symbol_posteriors"][b].any()) and not bool(out["logit_grad"][b].any())
            assert not bool(out["token_expected_frames"][b, :L].any()) and bool((cen == -1).all())
            assert bool((out["token_center_times"][b] == -1).all())
        else:
            assert bool((cen >= 0).all()) and bool((cen <= Tb - 1).all())


def test_no_labels_goes_through_the_unused_column(dev, models):
    m = model_for(models, "fp32", dev)
    x, mask, _, _ = batch(m, dev)
    out = m.posteriors(x, torch.zeros((3, 0), dtype=torch.int64), attention_mask=mask, return_states=True)
    assert tuple(out["token_expected_frames"].shape) == tuple(out["token_center_times"].shape) == (3, 0)
    assert tuple(out["state_posteriors"].shape) == (3, T, 1) and out["infeasible"].tolist() == [0, 0, 0]
    lp = f64(m(x, attention_mask=mask)["log_probs"])
    for b, Tb in enumerate(FRAMES):   # the one path: all blank
        ref = P.post_ref(lp[b], [], Tb, m.config.ctc_blank_id)
        got = {"gamma": f64(out["state_posteriors"][b, :Tb]), "occ": f64(out["symbol_posteriors"][b, :Tb]), "grad": ref["grad"],
               "tok_frames": np.zeros(0), "tok_center": np.zeros(0)}
        for k, v in P.ratios(got, ref).items():
            within(f"ctc post model no labels {k}", v, 1.0)
        assert not bool(out["symbol_posteriors"][b, Tb:].any()) and not bool(out["state_posteriors"][b, Tb:].any())


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_two_half_batches_equal_the_whole(dev, models, precision):
    m = model_for(models, precision, dev)
    x, mask, labels, lens = batch(m, dev, B=4)
    whole = m.posteriors(x, labels, lens, attention_mask=mask, return_logit_grad=True, return_states=True)
    parts = [m.posteriors(x[a:b], labels[a:b], lens[a:b], attention_mask=mask[a:b], return_logit_grad=True, return_states=True)
             for a, b in ((0, 2), (2, 4))]
    # every kernel of the pass works on a batch item (or a row) alone, in the same order whatever the batch: the same bits
    for k in KEYS:
        both = torch.cat([parts[0][k], parts[1][k]])
        assert torch.equal(both.view(torch.int64 if both.dtype == torch.float64 else torch.int32),
                           whole[k].view(torch.int64 if both.dtype == torch.float64 else torch.int32)), k


def test_training_state_is_untouched_and_training_calls_raise(dev, models):
    m = model_for(models, "bf16", dev)
    x, mask, labels, lens = batch(m, dev)
    m.posteriors(x, labels, lens, attention_mask=mask, return_logit_grad=True, return_states=True)
    torch.cuda.synchronize()
    assert m._ws_sets == {} and m._ws_key is None and m._drop_step == 0 and m.ws == {}
    assert not bool(m.arena.g.any()) and not bool(m.arena.m.any())
    with pytest.raises(NotImplementedError, match="CTC fine-tuning is not built"):
        m.forward_backward(x, None)
    with pytest.raises(NotImplementedError, match="CTC fine-tuning is not built"):
        m(x, training=True)
    with pytest.raises(ValueError):
        m.posteriors(x, torch.zeros(3, 3, dtype=torch.int64))   # the blank as a label
    with pytest.raises(ValueError):
        m.posteriors(x, labels, lens, attention_mask=torch.ones(3, T + 1))
    long = torch.zeros(1, (W().CTC_MAX_FRAMES + 2) * 20, device=dev)
    with pytest.raises(ValueError, match="at most 4096 frames"):
        m.posteriors(long, torch.full((1, 3), 5))


def test_recorded_plan_of_a_pretraining_model_replays_the_same_around_posteriors(dev, models):
    from tethys_speech_amd import ops, optim, train
    from tethys_speech_amd.dist import DataParallelStrategy
    from test_w2v_infer_gpu import _train_inputs
    from test_wav2vec2_gpu import build
    ctc = model_for(models, "bf16", dev)
    x, mask, labels, lens = batch(ctc, dev)

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
                    assert step.planned is not None and step.planned.replays >= 1, "no plan was recorded before the call"
                    state = (model._drop_step, model._ws_key, sorted(model._ws_sets))
                    ctc.posteriors(x, labels, lens, attention_mask=mask, return_logit_grad=True)
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
