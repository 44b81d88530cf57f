"""Wav2Vec2 inference on the GPU: attention with an additive key bias (tmi_attn_desc.mask_mode 2, tmi_softmax_bias_fwd),
the masked mean over time (tmi_masked_mean_pool), and ``Wav2Vec2ForPreTraining.forward_infer`` against the float64
restatement tests/_w2v_infer_ref.py of the reference's ``Wav2Vec2Model.call(..., training=False)`` (V:768-825)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _w2v_infer_ref as R  # noqa: E402
from _margins import within  # noqa: E402
from oracle import wav2vec2_oracle as V  # noqa: E402
from test_attention_forms_gpu import LAGS, bf  # noqa: E402
from test_wav2vec2_gpu import build, small_cfg  # noqa: E402

HD = 64
BF = torch.bfloat16
TMI_ERR_INVALID = -1


def _mods():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib, ops
    return ops, _lib


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float64) * scale


# ----------------------------------------------------------------------------- masks
def make_mask(kind, T, seed=0):
    m = torch.ones(T, dtype=torch.float64)
    if kind == "ones":
        pass
    elif kind == "prefix_mid":      # ends inside a 64-key tile
        n = max(1, (3 * T) // 5)
        assert n % 64 != 0 or T < 3
        m[n:] = 0
    elif kind == "prefix_edge":     # ends on a tile edge (the whole clip when it is no longer than one tile)
        n = (T - 1) // 64 * 64 if T > 64 else T
        m[n:] = 0
    elif kind == "holes":           # scattered zeros; from two tiles on, the whole first tile is masked as well
        g = torch.Generator().manual_seed(100 + seed)
        m = (torch.rand(T, generator=g) < 0.5).double()
        if T > 64:
            m[:64] = 0
        m[T - 1] = 1
    elif kind == "fraction":        # one value strictly between 0 and 1
        m[T // 2] = 0.5
        if T > 2:
            m[0] = 0
    elif kind == "zero":
        m[:] = 0
    else:
        raise KeyError(kind)
    return m


PAIRS = [("ones", "prefix_mid"), ("prefix_edge", "holes"), ("fraction", "zero")]
LENGTHS = [1, 63, 64, 65, 130, 200]  # on, next to and across the 64-key tile and the 128-query block


def run_attn(ops, q, k, v, mask, B, H, T, scale, dev, pad=3):
    """bf16 fused forward with mask_mode 2 on [B, T, H*64] inputs; o has ``pad`` guard rows behind every batch item."""
    qd, kd, vd = (t.to(BF).to(dev).contiguous() for t in (q, k, v))
    o = torch.full((B, T + pad, H * HD), 7.0, dtype=BF, device=dev)
    stats = torch.full((B, H, T, 2), float("nan"), dtype=torch.float32, device=dev)
    kb = ((1.0 - mask) * R.MASK_VALUE).to(torch.float32).to(dev)
    d = H * HD
    ops.attn_fwd((qd, 0, T * d, d), (kd, 0, T * d, d), (vd, 0, T * d, d), (o, 0, (T + pad) * d, d), stats, B, H, T, T, 2,
                 score_scale=scale, key_bias=kb)
    torch.cuda.synchronize()
    return o.cpu(), stats.cpu()


def heads(t, H):  # [B, T, H*64] -> [B, H, T, 64] float64
    return t.double().reshape(t.shape[0], t.shape[1], H, HD).permute(0, 2, 1, 3)


def restate_fwd(q, k, v, scale, mask, lag):
    """The forward with the kernel's bf16 rounding points (P before P.V, o on store), everything else in float64: the
    restatement of tests/test_attention_forms_gpu.py with the key term added to the scores."""
    s = (q @ k.transpose(-1, -2)) * scale + ((1.0 - mask) * R.MASK_VALUE)[:, None, None, :]
    e = torch.exp(s - s.amax(-1, keepdim=True) + lag * 0.6931471805599453)
    return bf((bf(e) @ v) / e.sum(-1, keepdim=True))


# One ulp of fp32 at 10000 * log2(e) = 14427 (log2 units, in [2^13, 2^14)) is 2^-10.  Where every key of a row carries the
# bias, each shifted score fl(s * c2 + bias2) is rounded to half such an ulp, and so is the row maximum it is subtracted
# from: the exponent of a probability is off by up to 2^-10 log2 units, the probability itself by a factor within
# 1 +- EPS_SHIFT, EPS_SHIFT = 2^(2^-10) - 1 = 6.8e-4, independently per key.  With p_j -> p_j (1 + e_j), |e_j| <= eps,
#   o' - o = sum_j p_j e_j (v_j - o) / sum_j p_j (1 + e_j),   so   |o' - o| <= eps / (1 - eps) * max_j |v_j - o|
# per output element.  That term, computed from the inputs and the float64 reference alone, is added to the bf16 rounding
# bound of such rows (twice the restatement's error); it is not fitted to what the kernel returns.
EPS_SHIFT = 2.0 ** (2.0 ** -10) - 1.0


@pytest.mark.parametrize("kinds", PAIRS, ids=["ones+prefix_mid", "prefix_edge+holes", "fraction+zero"])
@pytest.mark.parametrize("T", LENGTHS)
def test_attn_fwd_key_bias_matches_float64(dev, T, kinds):
    ops, _ = _mods()
    B, H = 2, 2
    scale = 1.0 / math.sqrt(HD)
    q, k, v = (bf(rnd((B, T, H * HD), 10 * T + i, s)) for i, s in enumerate((2.0, 2.0, 1.0)))
    mask = torch.stack([make_mask(kd, T, seed=T) for kd in kinds])
    o, stats = run_attn(ops, q, k, v, mask, B, H, T, scale, dev)
    assert bool(torch.isfinite(stats).all()), "stats must be finite for every row, the all-biased ones included"
    assert bool((o[:, T:].float() == 7.0).all()), "o rows at q >= Tq were written"
    qh, kh, vh = heads(q, H), heads(k, H), heads(v, H)
    ref, _ = R.masked_attention(qh, kh, vh, scale, mask)
    got = heads(o[:, :T], H)
    assert bool(torch.isfinite(got).all())
    rests = [restate_fwd(qh, kh, vh, scale, mask, lag) for lag in LAGS]
    for b, kind in enumerate(kinds):
        mag_row = ref[b].abs().amax(-1)                                   # [H, T]
        k_row = float(((got[b] - ref[b]).abs().amax(-1) / mag_row).max())
        r_row = max(float(((r[b] - ref[b]).abs().amax(-1) / mag_row).max()) for r in rests)
        k_all = float((got[b] - ref[b]).abs().max() / ref[b].abs().max())
        r_all = max(float((r[b] - ref[b]).abs().max() / ref[b].abs().max()) for r in rests)
        extra_row = extra_all = 0.0
        if kind == "zero":  # the fp32 precision of the shifted scores, derived above
            dev_v = (vh[b][:, None, :, :] - ref[b][:, :, None, :]).abs().amax(2)   # [H, T, 64]: max_j |v_j - o|
            term = EPS_SHIFT / (1.0 - EPS_SHIFT) * dev_v
            extra_row = float((term.amax(-1) / mag_row).max())
            extra_all = float(term.max() / ref[b].abs().max())
        print(f"attn key-bias T={T} {kind}: row {k_row:.3e} (restatement {r_row:.3e}, shift term {extra_row:.3e}); "
              f"whole {k_all:.3e} (restatement {r_all:.3e}, shift term {extra_all:.3e})")
        within(f"attn key-bias T={T} {kind} o row", k_row, 2.0 * r_row + extra_row)
        within(f"attn key-bias T={T} {kind} o whole", k_all, 2.0 * r_all + extra_all)


@pytest.mark.parametrize("T", [65, 200])
def test_attn_fwd_ignores_keys_whose_mask_is_zero_bit_for_bit(dev, T):
    """exp of anything near -10000 is 0 in fp32: k and v at keys with mask exactly 0 cannot reach o or the statistics of a
    row that keeps one unmasked key."""
    ops, _ = _mods()
    B, H = 2, 2
    scale = 1.0 / math.sqrt(HD)
    q, k, v = (bf(rnd((B, T, H * HD), 20 * T + i, s)) for i, s in enumerate((2.0, 2.0, 1.0)))
    mask = torch.stack([make_mask("prefix_mid", T), make_mask("holes", T, seed=T)])
    assert bool((mask.sum(1) >= 1).all()) and bool(((mask == 0) | (mask == 1)).all())
    o1, s1 = run_attn(ops, q, k, v, mask, B, H, T, scale, dev)
    dead = (mask == 0)[:, :, None]
    k2 = torch.where(dead, bf(rnd(k.shape, 77, 3.0)), k)
    v2 = torch.where(dead, bf(rnd(v.shape, 78, 3.0)), v)
    assert not torch.equal(k2, k)
    o2, s2 = run_attn(ops, q, k2, v2, mask, B, H, T, scale, dev)
    assert torch.equal(o1.view(torch.int16), o2.view(torch.int16))
    assert torch.equal(s1.view(torch.int32), s2.view(torch.int32))


def test_key_bias_rejections_by_return_code(dev):
    ops, _lib = _mods()
    lib = _lib.lib()
    B, H, T = 1, 2, 64
    d = H * HD
    x = torch.zeros(B, T, d, dtype=BF, device=dev)
    bufs = [torch.zeros_like(x) for _ in range(8)]
    stats = torch.zeros(B, H, T, 2, dtype=torch.float32, device=dev)
    delta = torch.zeros(B, H, T, dtype=torch.float32, device=dev)
    kb = torch.zeros(B, T, dtype=torch.float32, device=dev)
    m = lambda t: (t, 0, T * d, d)  # noqa: E731

    def desc(mask_mode, bias, dropout_p=0.0):
        dd = ops._attn_desc(m(bufs[0]), m(bufs[1]), m(bufs[2]), m(bufs[3]), stats, B, H, T, T, mask_mode)
        for name, field, t in (("d_o", "do", bufs[4]), ("dq", "dq", bufs[5]), ("dk", "dk", bufs[6]), ("dv", "dv", bufs[7])):
            setattr(dd, name, t.data_ptr())
            setattr(dd, f"{field}_sb", T * d)
            setattr(dd, f"{field}_st", d)
        dd.delta = delta.data_ptr()
        dd.dq_scale = 1.0
        if bias:
            dd.key_bias, dd.kb_sb = kb.data_ptr(), T
        if dropout_p:
            mask_buf = ops.attn_dropmask(dev, B, H, T, T)
            dd.dropout_p, dd.dropout_seed = dropout_p, 5
            dd.drop_mask, dd.drop_mask_bytes = mask_buf.data_ptr(), mask_buf.numel()
            dd._keep = mask_buf
        return dd

    s = ops.stream()
    ok = desc(2, True)
    assert lib.tmi_attn_fwd(C.byref(ok), s) == 0                                  # the accepted form, for contrast
    assert lib.tmi_attn_bwd(C.byref(desc(0, False)), s) == 0                      # the same descriptor is a valid backward ...
    assert lib.tmi_attn_bwd(C.byref(desc(2, True)), s) == TMI_ERR_INVALID         # ... until it asks for the key bias
    assert b"forward only" in lib.tmi_last_error()
    assert lib.tmi_attn_fwd(C.byref(desc(2, False)), s) == TMI_ERR_INVALID        # no bias pointer
    assert lib.tmi_attn_fwd(C.byref(desc(2, True, dropout_p=0.1)), s) == TMI_ERR_INVALID
    assert lib.tmi_attn_fwd(C.byref(desc(3, True)), s) == TMI_ERR_INVALID
    torch.cuda.synchronize()


def test_softmax_bias_fwd_matches_float64(dev):
    ops, _ = _mods()
    B, H, Tq, Tk = 2, 2, 65, 65
    worst = 0.0
    for kinds in PAIRS:
        mask = torch.stack([make_mask(kd, Tk, seed=Tk) for kd in kinds])
        s = rnd((B, H, Tq, Tk), 31, 3.0).float()
        kb = ((1.0 - mask) * R.MASK_VALUE).float()
        p = s.to(dev).contiguous()
        ops.softmax_bias_fwd(p, B * H * Tq, Tq, Tk, H, kb.to(dev))
        torch.cuda.synchronize()
        # (the term is added in fp32, as TensorFlow does and as test_kernels_gpu.test_softmax forms its masked reference:
        # what float64 checks is the softmax of those fp32 sums)
        ref = torch.softmax((s + kb[:, None, None, :]).double(), dim=-1)
        err = float((p.cpu().double() - ref).abs().max() / ref.abs().max())
        print(f"softmax bias {kinds}: {err:.3e}")
        worst = max(worst, err)
    within("softmax bias fwd fp32 vs float64 (2, 2, 65, 65)", worst, 2e-6)  # the fp32 bound of test_kernels_gpu.test_softmax


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,T,Cn", [(3, 1, 128), (2, 130, 128), (2, 37, 64)])
def test_masked_mean_pool(dev, dtype, B, T, Cn):
    ops, _ = _mods()
    x = rnd((B, T, Cn), 40 + T).to(dtype)
    xd = x.to(dev).contiguous()
    prefix = torch.stack([make_mask("prefix_mid", T), torch.ones(T, dtype=torch.float64)] + [make_mask("fraction", T)] * (B - 2))
    zero_row = prefix.clone()
    zero_row[B - 1] = 0
    for name, mask in (("none", None), ("prefix", prefix), ("zero row", zero_row)):
        md = None if mask is None else mask.float().to(dev).contiguous()
        out, out2 = (torch.full((B, Cn), float("nan"), dtype=torch.float32, device=dev) for _ in range(2))
        ops.masked_mean_pool(xd, md, out, B, T, Cn)
        ops.masked_mean_pool(xd, md, out2, B, T, Cn)
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), out2.view(torch.int32)), "two runs must be bit-identical"
        got = out.cpu().double()
        live = torch.ones(B, dtype=torch.bool) if mask is None else mask.sum(1) > 0
        ref = R.masked_mean(x.double()[live], None if mask is None else mask[live])
        assert bool((got[~live] == 0).all()), "a row whose mask sums to zero pools to exact zeros"
        err = float((got[live] - ref).abs().max() / ref.abs().max())
        within(f"masked mean pool {str(dtype).split('.')[-1]} ({B}, {T}, {Cn}) {name}", err, 2e-5)  # the project's fp32 kernel bound


# ----------------------------------------------------------------------------- the model
B_M, T_IN = 3, 2600            # 130 frames: two key tiles and a ragged third
SAMPLE_LENGTHS = (2600, 1700, 330)
# Bounds at about twice what the first GPU run measured (profiles/r08_test_margins.json; fp32: relative max, worst of the
# masked / unmasked calls 5.1e-7, 5.6e-7, 2.3e-7, 6.2e-7; bf16: relative L2 6.0e-3, 5.4e-3, 2.1e-3, 6.2e-3), under the caps
# of the classes stated at the top of tests/test_wav2vec2_gpu.py: fp32 1e-4 relative max, bf16 6e-2 relative L2 per tensor
BOUND = {"fp32": {"last_hidden_state": 1.2e-6, "extract_features": 1.2e-6, "pooled_output": 5e-7, "hidden_states": 1.3e-6},
         "bf16": {"last_hidden_state": 1.2e-2, "extract_features": 1.1e-2, "pooled_output": 4.5e-3, "hidden_states": 1.3e-2}}
CAP = {"fp32": 1e-4, "bf16": 6e-2}


def model_err(precision, got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double()
    if precision == "fp32":
        return float((got - ref).abs().max() / ref.abs().max())
    return float((got - ref).norm() / ref.norm())


def ref_params(model, precision):
    p = {k: v.detach().double().cpu().clone() for k, v in model.arena.ref_views(model.arena.p).items()}
    if precision == "bf16":
        for k in p:
            if k.endswith(".kernel"):
                p[k] = p[k].to(BF).double()
    return p


def check_outputs(tag, precision, out, ref, ocfg):
    names = ["last_hidden_state", "extract_features"] + (["pooled_output"] if "pooled_output" in out else [])
    worst = {}
    for n in names:
        worst[n] = model_err(precision, out[n], ref[n])
    if "hidden_states" in out:
        assert len(out["hidden_states"]) == ocfg.num_hidden_layers + 1
        worst["hidden_states"] = max(model_err(precision, g, r) for g, r in zip(out["hidden_states"], ref["hidden_states"]))
    for n, e in worst.items():
        print(f"w2v infer {tag} {precision} {n}: {e:.3e}")
        within(f"w2v infer {tag} {precision} {n}", e, min(BOUND[precision][n], CAP[precision]))


@pytest.fixture(scope="module")
def clips():
    return torch.from_numpy(V.create_dummy_pool(seed=21, num_samples=B_M, length=T_IN))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_masked_forward_matches_restatement(dev, precision, clips):
    from tethys_speech_amd import wav2vec2
    model, ocfg, _ = build(precision, dev)
    mask = wav2vec2.frame_attention_mask(model.config, SAMPLE_LENGTHS, T_IN)
    assert tuple(mask.shape) == (B_M, 130) and mask.sum(1).tolist() == [130.0, 85.0, 17.0]
    out = model(clips.to(dev), attention_mask=mask, output_hidden_states=True, pool="mean", training=False)
    torch.cuda.synchronize()
    assert out["last_hidden_state"].shape == (B_M, 130, 128) and out["extract_features"].shape == (B_M, 130, 64)
    assert out["pooled_output"].shape == (B_M, 128) and out["pooled_output"].dtype == torch.float32
    p = ref_params(model, precision)
    ref = R.forward(p, clips.double(), ocfg, mask.double())
    check_outputs("masked", precision, out, ref, ocfg)
    # without a mask: the unmasked kernels of the training step, the plain mean, no hidden_states unless asked for
    out0 = model.forward_infer(clips.to(dev), pool="mean")
    torch.cuda.synchronize()
    assert "hidden_states" not in out0
    check_outputs("unmasked", precision, out0, R.forward(p, clips.double(), ocfg, None), ocfg)
    # the mask matters: the short clip's frames differ between the two calls
    assert model_err(precision, out["last_hidden_state"][2], out0["last_hidden_state"][2].double().cpu()) > 1e-3


def _clips_and_negatives(model, T_in, dev):
    from tethys_speech_amd import wav2vec2
    cfg = model.config
    T = wav2vec2.frame_lengths(cfg, [T_in])[0]
    audio = torch.from_numpy(V.create_dummy_pool(seed=21, num_samples=B_M, length=T_in)).to(dev)
    neg = torch.from_numpy(wav2vec2.sample_negative_indices(np.random.default_rng(3), B_M, T, cfg.num_negatives)).to(dev)
    return audio, neg, T


@pytest.mark.parametrize("T_in", [T_IN, 1990])  # 130 frames; 100 frames behind an odd conv length (398 -> 199 -> 100)
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_forward_infer_is_the_training_forward_bit_for_bit(dev, precision, T_in):
    """The step and ``forward_infer`` run the same forward blocks on different buffers: without dropout the last hidden
    state and the extracted features of an inference call are the bits the training step left in ws["enc_x"] and
    ws["feats"] for the same clips and weights.  Neither T is a multiple of the 64-key attention tile, and the positional
    conv pads both (3 rows in front, 4 behind)."""
    from tethys_speech_amd import ops
    model, _, _ = build(precision, dev)
    cfg = model.config
    audio, neg, T = _clips_and_negatives(model, T_in, dev)
    assert T == {T_IN: 130, 1990: 100}[T_in] and T % 64 != 0
    was = ops.set_deterministic(True)
    try:
        model.forward_backward(audio, neg)
        assert model.T == T
        enc_x = model.ws["enc_x"].view(B_M, T, cfg.hidden_size).clone()
        feats = model.ws["feats"].view(B_M, T, cfg.conv_dim[-1]).clone()
        out = model.forward_infer(audio)
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(was)
    assert bool(torch.isfinite(enc_x.float()).all())
    assert torch.equal(out["extract_features"], feats)
    assert torch.equal(out["last_hidden_state"], enc_x)


def test_inference_after_a_dropout_step_passes_no_site(dev):
    """After ``enable_dropout`` and one training step, two inference calls agree bit for bit, and the step counter of the
    dropout masks has moved by the training step alone."""
    from tethys_speech_amd import ops
    model, _, _ = build("bf16", dev)
    c = model.config
    model.enable_dropout(c.hidden_dropout, c.attention_dropout, seed=11, act_p=c.activation_dropout)
    audio, neg, _ = _clips_and_negatives(model, T_IN, dev)
    was = ops.set_deterministic(True)
    try:
        assert model._drop_step == 0
        model.forward_backward(audio, neg)
        assert model._drop_step == 1
        first = model.forward_infer(audio)
        second = model.forward_infer(audio)
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(was)
    assert model._drop_step == 1
    for n in ("last_hidden_state", "extract_features"):
        assert torch.equal(first[n], second[n]), n


def _train_inputs(model, B, T_in, seed, dev):
    cfg = model.config
    from tethys_speech_amd import wav2vec2
    T = wav2vec2.frame_lengths(cfg, [T_in])[0]
    g = torch.Generator().manual_seed(seed)
    audio = torch.randn(B, T_in, generator=g).to(dev)
    neg = torch.from_numpy(wav2vec2.sample_negative_indices(np.random.default_rng(seed), B, T, cfg.num_negatives)).to(dev)
    codes = torch.randint(0, cfg.num_codevectors_per_group, (B, T, cfg.num_codevector_groups), generator=g, dtype=torch.int32).to(dev)
    return audio, neg, codes


def test_inference_between_training_steps_changes_nothing(dev):
    """Two teacher-forced training steps (bf16, dropout on); in the second run an inference call - another batch size,
    with a mask - sits between them.  The Wav2Vec2 step keeps fp32 atomics (GroupNorm statistics, codebook gradient:
    tests/test_plan_gpu.py), so two plain runs are compared first: where they agree bit for bit the run with the
    inference call must too; otherwise it must sit inside 4 x their spread, the form test_plan_gpu.py uses.  The training
    state the call could disturb (step counter of the dropout masks, workspace key, clean-gradient flag) is compared
    exactly either way."""
    from tethys_speech_amd import ops, wav2vec2

    def run(infer):
        model, _, _ = build("bf16", dev)
        c = model.config
        model.enable_dropout(c.hidden_dropout, c.attention_dropout, seed=11, act_p=c.activation_dropout)
        steps = [_train_inputs(model, 3, 400, 50 + i, dev) for i in range(2)]
        model.forward_backward(steps[0][0], steps[0][1], forced_codes=steps[0][2])
        if infer:
            clip = torch.from_numpy(V.create_dummy_pool(seed=5, num_samples=2, length=700)).to(dev)
            mask = wav2vec2.frame_attention_mask(c, (700, 250), 700)
            out = model(clip, attention_mask=mask, pool="mean", training=False)
            assert bool(torch.isfinite(out["last_hidden_state"].float()).all())
        state = (model._drop_step, model._ws_key, bool(getattr(model.arena, "g_clean", False)), sorted(model._ws_sets))
        loss = model.forward_backward(steps[1][0], steps[1][1], forced_codes=steps[1][2])
        torch.cuda.synchronize()
        return float(loss.item()), model.arena.g.clone(), state

    was = ops.set_deterministic(True)
    try:
        l0, g0, s0 = run(False)
        l1, g1, s1 = run(False)
        l2, g2, s2 = run(True)
    finally:
        ops.set_deterministic(was)
    assert s0 == s1 == s2, (s0, s2)
    spread_g, spread_l = float((g0 - g1).abs().max()), abs(l0 - l1)
    if spread_g == 0.0 and spread_l == 0.0:
        print("plain runs agree bit for bit: comparing the run with the inference call bit for bit")
        assert l2 == l0 and torch.equal(g2, g0)
    else:
        print(f"plain runs differ (loss {spread_l:.2e}, gradients {spread_g:.2e}): comparing within 4 x that spread")
        assert abs(l2 - l0) <= max(4.0 * spread_l, 1e-6 * abs(l0)), (l2, l0, spread_l)
        assert float((g2 - g0).abs().max()) <= max(4.0 * spread_g, 1e-7), (float((g2 - g0).abs().max()), spread_g)


def test_recorded_plan_replays_the_same_after_an_inference_call(dev):
    from tethys_speech_amd import ops, optim, train, wav2vec2
    from tethys_speech_amd.dist import DataParallelStrategy

    def run(infer):
        model, _, _ = build("bf16", dev)
        c = model.config
        model.enable_dropout(c.hidden_dropout, c.attention_dropout, seed=11, act_p=c.activation_dropout)
        opt = optim.Adam(3e-4, epsilon=1e-8)
        inputs = [_train_inputs(model, 3, 400, 60 + i, dev)[:2] for i in range(3)]
        old, train.USE_PLAN = train.USE_PLAN, True
        try:
            step = train.planned_step(DataParallelStrategy(0, 1, init=False), model, opt, "wav2vec2", pipelined=True)
            losses = []
            for i in range(8):
                if infer and i == 5:
                    assert step.planned is not None and step.planned.replays >= 1, "no plan was recorded before the call"
                    clip = torch.from_numpy(V.create_dummy_pool(seed=5, num_samples=2, length=700)).to(dev)
                    model(clip, attention_mask=wav2vec2.frame_attention_mask(c, (700, 250), 700), training=False)
                losses.append(step(*inputs[i % 3]))
            model.finish_late()
            torch.cuda.synchronize()
            assert step.planned is not None and step.planned.replays >= 4
            return [float(x.item()) for x in losses], model.arena.p.clone()
        finally:
            train.USE_PLAN = old

    was = ops.set_deterministic(True)
    try:
        la, pa = run(False)
        lb, pb = run(False)
        lc, pc = run(True)
    finally:
        ops.set_deterministic(was)
    spread = float((pa - pb).abs().max())  # (fp32 atomics of the Wav2Vec2 step: see the test above)
    print(f"planned runs: spread {spread:.2e}, with the inference call {float((pa - pc).abs().max()):.2e}")
    assert float((pa - pc).abs().max()) <= max(4.0 * spread, 1e-7), (float((pa - pc).abs().max()), spread)
    assert max(abs(a - b) for a, b in zip(la, lc)) <= max(4.0 * max(abs(a - b) for a, b in zip(la, lb)), 1e-6 * abs(la[0])), (la, lc)


def test_inference_after_an_optimizer_step_reads_the_updated_weights(dev, clips):
    from tethys_speech_amd import optim, train, wav2vec2
    from tethys_speech_amd.dist import DataParallelStrategy
    model, ocfg, _ = build("bf16", dev)
    mask = wav2vec2.frame_attention_mask(model.config, SAMPLE_LENGTHS, T_IN)
    before = model(clips.to(dev), attention_mask=mask, training=False)["last_hidden_state"].clone()
    opt = optim.Adam(1e-2, epsilon=1e-8)
    audio, neg, _ = _train_inputs(model, 2, 400, 70, dev)
    train.wav2vec2_train_step(DataParallelStrategy(0, 1, init=False), model, audio, neg, opt, pipelined=True)  # (leaves the late slice running)
    out = model(clips.to(dev), attention_mask=mask, pool="mean", training=False)
    model.finish_late()
    torch.cuda.synchronize()
    assert model_err("bf16", out["last_hidden_state"], before.double().cpu()) > 1e-2, "the update did not reach the output"
    ref = R.forward(ref_params(model, "bf16"), clips.double(), ocfg, mask.double())
    check_outputs("after update", "bf16", out, ref, ocfg)
