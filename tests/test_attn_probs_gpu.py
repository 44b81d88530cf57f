"""tmi_attn_probs (csrc/attention.hip) against the float64 softmax of tests/_attn_probs_ref.py on bf16-rounded q, k: the
attention weights of a call tmi_attn_fwd has made, recomputed from q, k and the forward's statistics.

B = 2 (3 with a key bias), H = 2, head_dim 64; q and k are column slices of one fused [B*T, 3*H*64] buffer where Tq == Tk,
buffers of their own otherwise.  The forward runs first (with the key-split workspace where ``ops.attn_fwd`` gives it one),
then tmi_attn_probs writes into a guard-filled buffer with p_sq = Tk + 5 and slack behind every (batch, head).

Checks per case and output dtype: every guard element intact bit for bit; exact zeros where the reference is exactly zero
(the masked keys of a partly masked row); two calls bit-identical; and, element by element,

    |P - Pref| <= Pref * rho + 2^-120            (bf16 output: + 2^-9, the rounding of a value <= 1 to 8 mantissa bits)

The derivation of rho, from the inputs alone (u = 2^-24, one fp32 rounding; x = the exponent in log2 units):

  The kernel evaluates p = exp2(x~ - m) * linv, or exp2(fma(s~, c2, nM)) with nM = log2(linv) - m on full unmasked tiles,
  where s~ is the MFMA's q.k, c2 = fl(score_scale * log2 e), and (m, linv = 1 / l) are the forward's statistics,
  l = sum_j exp2(x~'_j - m) with the forward's own x~'.  Write x~_ij = x_ij + d_ij.  Then p / p_true =
  2^(d_ij) / (sum_j p_j 2^(d'_ij)) times the roundings outside the exponent, so
      rho_ij = expm1(ln 2 * (E_ij + Ebar_i)) + C * u,      Ebar_i = max over the keys j with Pref_ij > 0 of E_ij
  (keys whose probability is exactly zero - in fp32 as in float64 - add nothing to l, whatever their rounding), with
    E_ij = 64 * 2u * c2 * sum_d |q_d| |k_d|          the fp32 accumulation of 64 exact bf16 products, 2u per add
         + 8u * (X_i + 8 + log2 Tk)                  eight roundings that act on the exponent, each on a value no larger
                                                     than X_i + 8 + log2 Tk, X_i = max over those keys of
                                                     |s_ij| c2 + |key_bias_j| log2 e: c2 (two: the constant log2 e, the
                                                     product), s~ * c2, key_bias * log2 e (two again), the add of the two,
                                                     the subtraction of m (|m| <= X_i + 8: the forward's lazy maximum lags
                                                     the true one by at most 2^8), and nM = log2(linv) - m (|log2 linv| <=
                                                     8 + log2 Tk; v_log_f32's 1 ulp is 2u of that).  The fma form has fewer.
    C = 4 + 1 + 1                                    two ulp (= 4u) of v_exp_f32, the product with linv, the store
      + 4 + Tk + 13 + 1                              the normaliser: v_exp_f32 again, Tk u for the fp32 sum inside l,
                                                     13u for the key-split fold (its exp2 4u, product, up to 8 adds) and
                                                     1u for 1 / l.
  mask_mode 1: a masked score is absorbed by the fp32 -1e9 (the test keeps |score| < 32, so also by -1e9 * log2 e, whose
  half ulp is 64 > 32 log2 e): x~ = x exactly there, so those keys carry E = 0 and no magnitude - in the fully masked last
  row x~ - m is exactly 0 for every key and only C u remains.

No constant here was fitted to what the kernel returns.  The measured worst |P - Pref| / bound per case goes through
``_margins.within(name, ratio, 1.0)`` (profiles/r11_attn_probs_margins.json)."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import _attn_probs_ref as A  # noqa: E402
from _margins import within  # noqa: E402

HD, H = 64, 2
D = H * HD
BF = torch.bfloat16
TMI_ERR_INVALID = -1
U = 2.0 ** -24
LOG2E = A.LOG2E
FLOOR = 2.0 ** -120
PATTERN = {torch.float32: (torch.int32, 0x5AA55AA5), BF: (torch.int16, 0x5AA5)}


def _mods():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib, ops
    return ops, _lib


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g, dtype=torch.float64) * scale).to(BF).double()


# name -> (mask_mode, Tq, Tk, score_scale, kind)
CASES = {}
for tq, tk in ((100, 100), (129, 65), (200, 200), (1, 1500), (5, 1500)):
    CASES[f"m0 {tq}x{tk}"] = (0, tq, tk, 1.0, "plain")
for t in (1, 3, 70, 130):
    CASES[f"m1 {t}x{t}"] = (1, t, t, 1.0, "plain")
for t in (100, 130):
    CASES[f"m2 {t}x{t}"] = (2, t, t, 1.0, "plain")
CASES["m0 200x200 scale"] = (0, 200, 200, 0.125, "unscaled")
CASES["m1 130x130 scale"] = (1, 130, 130, 0.125, "unscaled")
CASES["m2 130x130 scale"] = (2, 130, 130, 0.125, "unscaled")
CASES["m0 129x65 loud"] = (0, 129, 65, 1.0, "loud")
CASES["m0 5x1500 loud"] = (0, 5, 1500, 1.0, "loud")
CASES["m0 100x100 quiet"] = (0, 100, 100, 1.0, "quiet")
CASES["m0 1x1500 quiet"] = (0, 1, 1500, 1.0, "quiet")

_REF = {}


def case_inputs(name):
    """q [B, Tq, D], k [B, Tk, D] (bf16 values in float64), key_bias [B, Tk] or None, the float64 reference and rho: computed
    once per case and shared by the output dtypes."""
    if name in _REF:
        return _REF[name]
    mode, Tq, Tk, scale, kind = CASES[name]
    B = 3 if mode == 2 else 2
    seed = sum(ord(c) for c in name)
    qs, ks = {"plain": (0.5, 1.0), "unscaled": (2.0, 2.0), "loud": (0.5, 1.0), "quiet": (0.01, 1.0)}[kind]
    q, k = rnd((B, Tq, D), seed, qs), rnd((B, Tk, D), seed + 1, ks)
    if kind == "loud":  # one key of every (batch, head) 40 above the rest, for every query row
        for b in range(B):
            for h in range(H):
                q[b, :, h * HD] = 4.0
                k[b, :, h * HD] = 0.0
                k[b, (37 * b + 11 * h + 5) % Tk, h * HD] = 10.0
    kb = None
    if mode == 2:  # clip 0 unmasked, clip 1 with a tail of -10000, clip 2 with every key biased
        kb = torch.zeros(B, Tk, dtype=torch.float64)
        kb[1, (3 * Tk) // 5:] = -10000.0
        kb[2, :] = -10000.0

    def heads(t):
        return t.reshape(B, -1, H, HD).permute(0, 2, 1, 3)

    qh, kh = heads(q), heads(k)
    s = (qh @ kh.transpose(-1, -2)) * scale
    if mode == 1:
        assert float(s.abs().max()) < 32.0, "the -1e9 must absorb every masked score, in natural-log and in log2 units"
    ref = A.probs_ref(qh, kh, mode, scale, kb)
    # ---- rho (module docstring)
    c2 = scale * LOG2E
    acc = 128.0 * U * c2 * (qh.abs() @ kh.abs().transpose(-1, -2))
    mag = s.abs() * LOG2E
    if kb is not None:
        mag = mag + (kb.abs() * LOG2E)[:, None, None, :]
    if mode == 1:
        masked = torch.arange(Tk)[None, :] <= torch.arange(Tq)[:, None]
        acc = torch.where(masked, torch.zeros_like(acc), acc)
        mag = torch.where(masked, torch.zeros_like(mag), mag)
    live = ref > 0
    X = torch.where(live, mag, torch.zeros_like(mag)).amax(-1, keepdim=True)
    E = acc + 8.0 * U * (X + 8.0 + math.log2(Tk))
    if mode == 1:
        E = torch.where(masked, torch.zeros_like(E), E)
    Ebar = torch.where(live, E, torch.zeros_like(E)).amax(-1, keepdim=True)
    rho = torch.expm1(math.log(2.0) * (E + Ebar)) + (6.0 + 4.0 + Tk + 13.0 + 1.0) * U
    _REF[name] = (q, k, kb, ref, rho)
    return _REF[name]


class Run:
    """The forward of one case on the GPU, ready for tmi_attn_probs calls."""

    def __init__(self, dev, name):
        self.ops, self.lib_mod = _mods()
        self.lib = self.lib_mod.lib()
        self.mode, self.Tq, self.Tk, self.scale, _ = CASES[name]
        q, k, kb, self.ref, self.rho = case_inputs(name)
        self.B = B = q.shape[0]
        Tq, Tk = self.Tq, self.Tk
        self.dev = dev
        v = rnd((B, Tk, D), 99)
        if Tq == Tk:
            fused = torch.cat([q, k, v], dim=2).to(BF).reshape(B * Tq, 3 * D).contiguous().to(dev)
            self.q, self.k, vv = (fused, 0, Tq * 3 * D, 3 * D), (fused, D, Tk * 3 * D, 3 * D), (fused, 2 * D, Tk * 3 * D, 3 * D)
        else:
            qd = q.to(BF).reshape(B * Tq, D).contiguous().to(dev)
            kv = torch.cat([k, v], dim=2).to(BF).reshape(B * Tk, 2 * D).contiguous().to(dev)
            self.q, self.k, vv = (qd, 0, Tq * D, D), (kv, 0, Tk * 2 * D, 2 * D), (kv, D, Tk * 2 * D, 2 * D)
        o = torch.empty(B * Tq, D, dtype=BF, device=dev)
        self.stats = torch.full((B, H, Tq, 2), float("nan"), dtype=torch.float32, device=dev)
        self.kb = None if kb is None else kb.to(torch.float32).to(dev)
        self.ops.attn_fwd(self.q, self.k, vv, (o, 0, Tq * D, D), self.stats, B, H, Tq, Tk, self.mode, score_scale=self.scale,
                          key_bias=self.kb)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(self.stats).all())
        self.keep = (o, vv)

    def desc(self):
        d = self.ops._attn_desc(self.q, self.k, self.q, self.q, self.stats, self.B, H, self.Tq, self.Tk, self.mode, self.scale)
        d.workspace, d.workspace_bytes = None, 0
        if self.kb is not None:
            d.key_bias, d.kb_sb = self.kb.data_ptr(), self.kb.stride(0)
        return d

    def probs(self, dtype):
        """-> (P [B, H, Tq, Tk] on the CPU, True if every guard element is intact)."""
        it, pat = PATTERN[dtype]
        B, Tq, Tk = self.B, self.Tq, self.Tk
        p_sq = Tk + 5
        p_sbh = Tq * p_sq + 7
        front = 64
        flat = torch.full((front + B * H * p_sbh + 64,), pat, dtype=it, device=self.dev)
        body = flat[front:front + B * H * p_sbh].view(dtype)
        rc = self.lib.tmi_attn_probs(C.byref(self.desc()), body.data_ptr(), self.ops.dt(body), p_sbh, p_sq, self.ops.stream())
        self.lib_mod.check(rc, "tmi_attn_probs")
        torch.cuda.synchronize()
        bits = flat.cpu()
        owned = torch.zeros(flat.numel(), dtype=torch.bool)
        own = owned[front:front + B * H * p_sbh].view(B * H, p_sbh)[:, :Tq * p_sq].view(B * H, Tq, p_sq)
        own[:, :, :Tk] = True
        intact = bool((bits[~owned] == pat).all())
        vals = bits[front:front + B * H * p_sbh].view(dtype).view(B * H, p_sbh)[:, :Tq * p_sq].view(B, H, Tq, p_sq)[..., :Tk]
        return vals.clone(), intact


@pytest.mark.parametrize("name", list(CASES))
def test_probs_match_float64_softmax(dev, name):
    run = Run(dev, name)
    ref, rho = run.ref, run.rho
    for dtype, extra in ((torch.float32, 0.0), (BF, 2.0 ** -9)):
        tag = f"attn-probs {name} {'fp32' if dtype == torch.float32 else 'bf16'}"
        got, intact = run.probs(dtype)
        again, intact2 = run.probs(dtype)
        assert intact and intact2, (tag, "wrote outside q < Tq, key < Tk")
        it = PATTERN[dtype][0]
        assert torch.equal(got.contiguous().view(it), again.contiguous().view(it)), (tag, "two calls differ")
        g = got.double()
        assert bool(torch.isfinite(g).all()), tag
        assert int(g[ref == 0].count_nonzero()) == 0, (tag, "nonzero where the reference is exactly zero")
        ratio = float(((g - ref).abs() / (ref * rho + FLOOR + extra)).max())
        print(f"{tag}: worst |P - Pref| / bound = {ratio:.3f} (max rho {float(rho.max()):.2e}, max |P - Pref| {float((g - ref).abs().max()):.2e})")
        within(tag, ratio, 1.0)


def test_probs_rejections(dev):
    run = Run(dev, "m2 100x100")
    lib, ops = run.lib, run.ops
    B, Tq, Tk = run.B, run.Tq, run.Tk
    out = torch.zeros(B, H, Tq, Tk, dtype=torch.float32, device=dev)
    sbh, sq, st = Tq * Tk, Tk, ops.stream()

    def call(d, probs=out.data_ptr(), dtype=0, p_sbh=sbh, p_sq=sq):
        return lib.tmi_attn_probs(C.byref(d), probs, dtype, p_sbh, p_sq, st)

    assert call(run.desc()) == 0
    assert call(run.desc(), probs=None) == TMI_ERR_INVALID
    assert b"tmi_attn_probs" in lib.tmi_last_error()
    assert call(run.desc(), p_sq=Tk - 1) == TMI_ERR_INVALID
    assert call(run.desc(), p_sbh=Tq * Tk - 1) == TMI_ERR_INVALID
    assert call(run.desc(), dtype=2) == TMI_ERR_INVALID and call(run.desc(), dtype=-1) == TMI_ERR_INVALID
    d = run.desc()
    d.key_bias = None
    assert call(d) == TMI_ERR_INVALID          # mask_mode 2 without key_bias
    d = run.desc()
    d.mask_mode, d.dropout_p = 0, 0.1
    assert call(d) == TMI_ERR_INVALID          # inference-time weights: no dropout
    d = run.desc()
    d.stats = None
    assert call(d) == TMI_ERR_INVALID
    d = run.desc()
    d.mask_mode = 3
    assert call(d) == TMI_ERR_INVALID
    assert lib.tmi_attn_probs(None, out.data_ptr(), 0, sbh, sq, st) == TMI_ERR_INVALID
    torch.cuda.synchronize()


def test_ops_attn_probs_wrapper(dev):
    """``ops.attn_probs`` into a plain contiguous tensor equals the direct call bit for bit; a mis-shaped out is refused."""
    run = Run(dev, "m1 70x70")
    got, _ = run.probs(torch.float32)
    out = torch.empty(run.B, H, run.Tq, run.Tk, dtype=torch.float32, device=dev)
    run.ops.attn_probs(run.q, run.k, run.stats, out, run.B, H, run.Tq, run.Tk, mask_mode=1, score_scale=run.scale)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().view(torch.int32), got.contiguous().view(torch.int32))
    with pytest.raises(ValueError):
        run.ops.attn_probs(run.q, run.k, run.stats, out.transpose(2, 3), run.B, H, run.Tq, run.Tk, mask_mode=1)
