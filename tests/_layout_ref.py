"""References, seeded inputs and bounds for Dropout at every rate (the generator of csrc/tmi_common.h and its five consumers),
the cast / layout kernels (tmi_cast_bf16, tmi_transpose_cast_bf16, tmi_feat_to_channels_last) and tmi_logmel_from_spectrum
(csrc/adam_misc.hip).  CPU only: nothing here imports the GPU package, so tests/test_layout_ref_cpu.py checks the references,
the inputs and the bounds before tests/test_dropout_rates_gpu.py and tests/test_layout_kernels_gpu.py compare a kernel with
them.

The cast / layout kernels and tmi_dropout are bit-exact operations (one fp32 multiply, one add, one rounding; or a rounding
alone), so their references are bit patterns and index maps.  The log-mel bound is per element and analytic, in the style of
tests/_row_kernel_ref.py: a count of fp32 roundings times U = 2^-24, written next to it, fitted to nothing.
"""
import math

import numpy as np
import torch

import _row_kernel_ref as R

U, F32, BF16, F64 = R.U, R.F32, R.BF16, R.F64
gam = R.gam


# ================================================================================================= bf16 of fp32
def _f32_bits(words):
    return torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in words], dtype=torch.int32).view(F32)


# fp32 bit patterns a cast can get wrong.  bf16 keeps the upper 16 bits; 0x8000 in the lower half is a tie.
SPECIAL_WORDS = [
    0x3F808000, 0x3F818000,              # exact ties: to even (down, 0x3F80) and to odd's even neighbour (up, 0x3F82)
    0x3F807FFF, 0x3F808001,              # one fp32 ulp either side of the first tie
    0x3F817FFF, 0x3F818001,              # and of the second
    0xBF808000, 0xBF818000, 0xBF807FFF, 0xBF818001,   # the same with the sign set
    0x00000000, 0x80000000,              # +0, -0
    0x7F7F0000, 0x7F7F7FFF,              # the largest finite bf16; the last fp32 that still rounds to it
    0x7F7F8000, 0x7F7F8001,              # its rounding boundary (a tie: to even = inf) and the first fp32 above it
    0xFF7F0000, 0xFF7F8001,
    0x7F800000, 0xFF800000,              # +inf, -inf
    0x7FC00000, 0x7F800001, 0xFFFFFFFF,  # NaN: quiet, the signalling pattern a truncation turns into inf, all ones
    0x00000001, 0x007FFFFF, 0x80000001,  # fp32 denormals: the smallest (-> 0) and the largest (-> the smallest normal bf16)
    0x00008000, 0x00018000,              # denormal ties
]
SPECIAL = _f32_bits(SPECIAL_WORDS)
BF16_OVERFLOW = float(_f32_bits([0x7F7F8000])[0])   # |x| at or above this rounds to inf


def bf16_full(x32):
    """fp32 -> bf16, round to nearest even on the bit pattern (_row_kernel_ref.bf16_rne), NaN -> the quiet NaN 0x7FC0 (the
    comparison accepts any NaN there, see ``same_bits``).  |x| >= BF16_OVERFLOW comes out of the bit arithmetic as inf:
    0x7F7F8000 + 0x7FFF + 1 carries into the exponent."""
    x32 = x32.to(F32)
    nan = torch.isnan(x32)
    r = R.bf16_rne(torch.where(nan, torch.zeros_like(x32), x32)).clone()
    r.view(torch.int16)[nan] = 0x7FC0
    return r


def to_dtype(x32, dtype):
    return bf16_full(x32) if dtype == BF16 else x32.to(F32).clone()


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(got, want):
    """Bit for bit, except that where ``want`` is NaN ``got`` may be any NaN (sign and payload of a NaN are not contracted)."""
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if not want.dtype.is_floating_point:
        return torch.equal(got, want)
    gn, wn = torch.isnan(got), torch.isnan(want)
    return torch.equal(gn, wn) and torch.equal(bits(got)[~wn], bits(want)[~wn])


def special_input(shape, seed, scale=1.0):
    """fp32 Gaussian data with SPECIAL tiled through every third element: a period of 84 elements, which no row length of
    the GPU cases divides, so the values move through the lane positions from row to row."""
    x = R.randn(shape, seed, scale).float()
    flat = x.view(-1)
    n = flat[::3].numel()
    flat[::3] = SPECIAL.repeat(-(-n // SPECIAL.numel()))[:n]
    return x


# ================================================================================================= index maps
def cast_map(rows, cols, lds, ldd, src_off=0, dst_off=0):
    """tmi_cast_bf16 on flat buffers: dst[dst_off + r ldd + c] = bf16(src[src_off + r lds + c]) for c < cols and +0 for
    cols <= c < ldd.  -> (dst indices [rows, ldd], src indices [rows, cols])."""
    r = torch.arange(rows)[:, None]
    return dst_off + r * ldd + torch.arange(ldd)[None, :], src_off + r * lds + torch.arange(cols)[None, :]


def cast_ref(src_flat, rows, cols, lds, ldd, src_off=0, dst_off=0):
    """-> (flat dst indices the kernel owns, the bf16 values they must hold)."""
    di, si = cast_map(rows, cols, lds, ldd, src_off, dst_off)
    val = torch.zeros((rows, ldd), dtype=BF16)
    val[:, :cols] = bf16_full(src_flat[si])
    return di.reshape(-1), val.reshape(-1)


def transpose_ref(src_flat, rows, cols, lds, ldd, src_off=0, dst_off=0):
    """tmi_transpose_cast_bf16: dst[dst_off + c ldd + r] = bf16(src[src_off + r lds + c]); columns rows..ldd-1 of dst are not
    the kernel's."""
    r, c = torch.arange(rows)[:, None], torch.arange(cols)[None, :]
    di = dst_off + c * ldd + r
    return di.reshape(-1), bf16_full(src_flat[src_off + r * lds + c]).reshape(-1)


def feat_ref(feats, pad_left, pad_right, dtype):
    """tmi_feat_to_channels_last: feats [B, C, T] fp32 -> [B, pad_left + T + pad_right, C], out[b, pad_left + t, c] =
    feats[b, c, t], pad rows +0."""
    B, C, T = feats.shape
    out = torch.zeros((B, pad_left + T + pad_right, C), dtype=dtype)
    b, c, t = torch.arange(B)[:, None, None], torch.arange(C)[None, :, None], torch.arange(T)[None, None, :]
    out[b, pad_left + t, c] = to_dtype(feats, dtype)
    return out


# ================================================================================================= log-mel
LOGMEL_SHAPES = [(5, 33, 8),      # n_bins < 64: lanes idle in the power loop; frames % 4 = 1: three waves leave early
                 (7, 201, 80),    # Whisper's: the lane loop's second trip (16 lanes), frames % 4 = 3
                 (4, 64, 65),     # exactly one power trip; the second mel trip has ONE lane; a full workgroup
                 (1, 1, 1),
                 (6, 257, 130),   # five power trips with one lane in the last; three mel trips (2 lanes in the last)
                 (5, 4096, 3)]    # the largest n_bins: exactly 64 KiB of LDS
LOGMEL_KINDS = ["gauss", "zero", "spike", "empty-cols"]
LOGMEL_EPS = float(np.float32(1e-6))   # eps crosses the C ABI as fp32


def logmel_inputs(frames, n_bins, n_mels, kind, ld_spec):
    """-> spec [frames, ld_spec] fp32 (re | im | NaN pad columns), mel [n_bins, n_mels] fp32 >= 0."""
    spec = torch.full((frames, ld_spec), R.NAN, dtype=F32)
    body = R.randn((frames, 2 * n_bins), 71).float()
    if kind == "zero":
        body = torch.zeros_like(body)
    elif kind == "spike":   # one bin of 1e15 among bins of 1e-15: powers 1e30 and 1e-30, both normal fp32
        body = torch.full_like(body, 1e-15)
        body[torch.arange(frames), (torch.arange(frames) * 7) % n_bins] = 1e15
    spec[:, :2 * n_bins] = body
    mel = R.randn((n_bins, n_mels), 72).abs().float()
    if kind == "empty-cols":
        mel[:, ::3] = 0.0
    return spec, mel


def logmel_ref(spec32, mel32, eps32, channels_first):
    """log(sum_k (re_k^2 + im_k^2) mel[k, m] + float32(eps)) in float64 on the fp32 inputs.  spec32 [frames, >= 2 n_bins].
    -> (out [frames, n_mels] or [n_mels, frames], s = the sum + eps in the same layout)."""
    nb = mel32.shape[0]
    sp = spec32[:, :2 * nb].to(F64)
    power = sp[:, :nb] ** 2 + sp[:, nb:] ** 2
    s = power @ mel32.to(F64) + float(np.float32(eps32))
    if channels_first:
        s = s.t().contiguous()
    return torch.log(s), s


def logmel_bound(ref, s, n_bins):
    """Per element.  Every term of the sum is non-negative, so relative errors do not grow by cancellation.  Roundings on the
    way from one term to the sum: the power re^2 + im^2 (3: two squares and an addition; 2 when contracted to an fma), the
    n_bins fmas of the chain (1 each, a term passes through at most all of them), the eps addition (1): n_bins + 4.
        s' = s (1 + d), |d| <= g = gam(n_bins + 4)   ->   |log s' - log s| <= -log(1 - g)
    A product below the smallest normal fp32 (1e-30 * mel) rounds absolutely, by at most 2^-149 per operation:
    (n_bins + 2) 2^-149 / s on the logarithm.  logf itself: 3 U |ref| (OpenCL allows log 3 ulp; ROCm's device library is
    built to that)."""
    g = gam(n_bins + 4)
    return -math.log1p(-g) + (n_bins + 2) * 2.0 ** -149 / s + 3.0 * U * ref.abs()


def check_logmel(out, ref, bound):
    return R.ratio(out, ref, bound)


def logmel_fp32(spec32, mel32, eps32, channels_first, mutation=None):
    """The kernel's loop restated: fp32 power, then one fma per bin in bin order (the product of two fp32 is exact in
    float64, so float32(float64 product + acc) is the fma up to a double rounding), the eps addition, log in fp32.
    mutation: "layout" (the other layout's indexing into the same buffer shape), "no-eps", "re-for-im"."""
    nb, nm = mel32.shape
    sp = spec32[:, :2 * nb].numpy().astype(np.float32)
    re, im = sp[:, :nb], (sp[:, :nb] if mutation == "re-for-im" else sp[:, nb:])
    power = (re * re + im * im).astype(np.float32)
    mel = mel32.numpy().astype(np.float64)
    acc = np.zeros((sp.shape[0], nm), dtype=np.float32)
    for k in range(nb):
        acc = (power[:, k:k + 1].astype(np.float64) * mel[k][None, :] + acc.astype(np.float64)).astype(np.float32)
    e = np.float32(0.0 if mutation == "no-eps" else eps32)
    with np.errstate(divide="ignore"):
        out = np.log((acc + e).astype(np.float32)).astype(np.float32)
    out = torch.from_numpy(out)
    frames = out.shape[0]
    if mutation == "layout":    # written frame-major into a buffer that is read channels-first, or the other way round
        return out.reshape(-1).reshape(nm, frames) if channels_first else out.t().contiguous().reshape(frames, nm)
    return out.t().contiguous() if channels_first else out


# ================================================================================================= dropout
def dropout_expected(x, resid, keep, scale, dtype):
    """tmi_dropout's output: to_dtype(resid32 + where(keep, x32 * float32(scale), 0)) in fp32 - one multiply, one add, one
    rounding, each correctly rounded on both sides, so the comparison is on the bits."""
    v = torch.where(keep, x.float() * np.float32(scale), torch.zeros((), dtype=F32))
    if resid is not None:
        v = v + resid.float()
    return to_dtype(v, dtype)


# (threshold, rate): 1 - tm1 of the attention kernels is the most negative int16; 6554 - the baseline the first-generation
# tests use; 32767 / 32768 / 32769 - the sign boundary of the attention kernels' signed 16-bit draws and a step either side;
# 58982 - the positive half; 65535 - the last rate tmi_drop_ok accepts, keep scale 65536.
RATES = [(1, 2.0 ** -16), (6554, 0.1), (32767, 32767.0 / 65536.0), (32768, 0.5), (32769, 32769.0 / 65536.0), (58982, 0.9),
         (65535, 0.99999)]
RATE_IDS = [f"thr{t}" for t, _ in RATES]
P_OFF = 2.0 ** -18                       # p > 0 whose threshold is 0: must behave exactly like p = 0
P_REFUSED = [0.999995, 1.0, -0.1, R.NAN]   # threshold 65536; p = 1; p < 0; NaN


def drop_ok(p):
    """tmi_drop_ok of csrc/tmi_common.h together with the entry points' ``p >= 0``."""
    from oracle import dropout as DO
    return bool(p >= 0.0 and np.float32(p) < np.float32(1.0) and DO.drop_thr(p) <= 65535)


# seeds and shapes of the GPU files: tests/test_layout_ref_cpu.py checks at every rate that each mask has the expected keep
# fraction and holds at least one kept and one dropped element.  The small shapes' seeds were chosen for that: 19602
# attention scores expect 0.3 dropped elements at thr = 1, so most seeds give none.
FLAT_SEED = 0xFEEDFACE12345
FLAT_SHAPES = [(600, 1026), (600, 1024)]             # the pair kernel / the 16-byte kernel
LN_RATE_SHAPE = (130, 768)
LN_RATE_SEED_Y, LN_RATE_SEED_MASKED = 0xABCDEF12346, 0xABCDEF12349   # Dropout of the LayerNorm's output (and of dy) / of dx
ATTN_SEED = 0x5EED0001
# (B, H, Tq, Tk, mask_mode, seed): the one-launch backward; the dQ + dK/dV kernels, plain and causal; the key split + combine
ATTN_RATE_CASES = [(2, 2, 130, 200, 0, ATTN_SEED), (1, 2, 130, 300, 0, ATTN_SEED), (1, 2, 99, 99, 1, ATTN_SEED + 3),
                   (1, 2, 100, 520, 0, ATTN_SEED)]
# name -> (M, N, K, seed)
GEMM_RATE_CASES = {"small": (300, 96, 64, 0x1234ABCD567D), "generic": (300, 100, 64, 0x1234ABCD567D),
                   "resid": (600, 768, 3072, 0x1234ABCD5678), "narrow-tail": (200, 108, 576, 0x1234ABCD567D)}
LAYOUT_DROP_P = [0.1, 0.5]
LAYOUT_DROP_SHAPES = [(2100, 2048), (1030, 1026), (64, 1024), (1, 1024), (1, 1026), (600, 2), (3, 131072)]
LAYOUT_DROP_SEED = 0xC0FFEE123456789


def mask_conditions(keep, thr):
    """-> (kept, dropped, |keep fraction - expected| in binomial standard deviations)."""
    n = keep.size
    q = 1.0 - thr / 65536.0
    kept = int(keep.sum())
    return kept, n - kept, abs(kept - n * q) / math.sqrt(n * q * (1.0 - q))
