"""The kernels that write the model - the four Adam entry points, the gradient-exchange staging pair, the bias-gradient
column sum, the batched GELU backward (csrc/adam_misc.hip, the colsum / gelu_bwd part of csrc/layernorm.hip) - each against
a float64 reference (tests/_adam_ref.py, itself checked by tests/test_adam_ref_cpu.py) at the lengths where their loops change
path: tail only, vector only, both, a grid that wraps, a throttled grid, slices of an arena, unaligned pointers.

Every bound is analytic: a count of fp32 roundings times u = 2^-24 times the magnitudes of the REFERENCE's intermediates
(derivations: _adam_ref.adam_bounds and the comments above each test), or bit equality where the arithmetic leaves no
freedom.  Measured / bound goes through _margins.within under the names "optk ...".
"""
import math

import numpy as np
import pytest
import torch

import _adam_ref as R
from _margins import within

pytestmark = pytest.mark.gpu

from oracle import whisper_oracle as O  # noqa: E402  (checker only)

U = R.U
TMI_ERR_INVALID = -1  # include/tethys_mi.h
NAN = float("nan")


def _ops():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import ops
    return ops


def tol(dtype):   # tests/test_kernels_gpu.py: fp32 / bf16 kernels against float64, relative to the largest reference value
    return 1.5e-2 if dtype == torch.bfloat16 else 2e-5


def bits(t):
    """Bit pattern of a tensor on the CPU (NaN guards compare equal to themselves this way)."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def same(a, b):
    return torch.equal(bits(a), bits(b))


def guard_pattern(n, dtype):
    """7.0 / NaN alternating: a stray store of any finite value, or of NaN, shows."""
    t = torch.full((n,), 7.0, dtype=dtype)
    t[1::2] = NAN
    return t


class Arena:
    """p, g, m, v (fp32) and the mirror (bf16) as slices [s0, s0 + n) of larger buffers full of guard values."""

    def __init__(self, dev, n, s0=0, trail=64, data=None, grad=None):
        p, g, g2, m, v = R.adam_inputs(n) if data is None else data
        self.n, self.s0, self.s1, self.dev = n, s0, s0 + n, dev
        self.init = {"p": p, "g": g if grad is None else grad, "m": m, "v": v, "mirror": torch.full((n,), 3.0, dtype=torch.bfloat16)}
        self.g2 = g2
        self.buf = {}
        for k, t in self.init.items():
            full = guard_pattern(s0 + n + trail, t.dtype)
            full[s0:s0 + n] = t
            self.buf[k] = full.to(dev)
        self.guard0 = {k: b.cpu() for k, b in self.buf.items()}

    def __getitem__(self, k):
        return self.buf[k][self.s0:self.s1]

    def host(self, k):
        return self[k].cpu()

    def set_grad(self, g):
        self[("g")].copy_(g.to(self.dev))

    def guards_untouched(self):
        for k, b in self.buf.items():
            now, was = b.cpu(), self.guard0[k]
            if not (same(now[:self.s0], was[:self.s0]) and same(now[self.s1:], was[self.s1:])):
                return False
        return True


# ------------------------------------------------------------------------------------------- a. tmi_adam_step vs float64
# Bounds: _adam_ref.adam_bounds with kg = 1, i.e. k_m = 3, k_v = 5, k_p = 5 (eps_mode 0) / 6 (eps_mode 1) roundings; the
# derivation is in that function's docstring and tests/test_adam_ref_cpu.py holds a plain fp32 evaluation to the same bounds.
# Each step is compared from exactly shared inputs: the reference of step 2 starts from the p, m, v the kernel left.
@pytest.mark.parametrize("n,eps_mode,weight_decay,gscale,step,zero_grad", R.adam_cases())
def test_adam_step_against_float64(dev, n, eps_mode, weight_decay, gscale, step, zero_grad):
    ops = _ops()
    a = Arena(dev, n)
    kw = dict(eps_mode=eps_mode, weight_decay=weight_decay, gscale=gscale, **R.HYPER)
    cls = R.element_class(n)
    zero = (cls == R.ZERO_TIE_EVEN) | (cls == R.ZERO_TIE_ODD)
    tag = "wrapped" if n == R.WRAPPED_N else "small"
    for k, grad in enumerate((a.init["g"], a.g2)):
        a.set_grad(grad)
        p0, m0, v0 = a.host("p"), a.host("m"), a.host("v")
        t = R.adam_terms(p0, grad, m0, v0, step=step + k, **kw)
        b = R.adam_bounds(t)
        ops.adam_step(a["p"], a["g"], a["m"], a["v"], n, R.HYPER["lr"], R.HYPER["beta1"], R.HYPER["beta2"], R.HYPER["eps"],
                      step + k, eps_mode=eps_mode, weight_decay=weight_decay, gscale=gscale, mirror=a["mirror"],
                      zero_grad=zero_grad)
        p1, m1, v1, mir, g1 = (a.host(x) for x in ("p", "m", "v", "mirror", "g"))
        for name, got in (("p", p1), ("m", m1), ("v", v1)):
            frac = R.bound_fraction(got, t[name], b[name])
            print(f"adam_step n={n} mode={eps_mode} wd={weight_decay} step={step + k} {name}: {frac:.3f} of its bound")
            within(f"optk adam_step {name} / bound ({tag})", frac, 1.0, (n, eps_mode, weight_decay, step + k))
        # the mirror is bf16 round-to-nearest-even of the kernel's own fp32 p, bit for bit
        assert same(mir, p1.to(torch.bfloat16)) and torch.equal(R.bf16_bits(mir), R.bf16_rne_bits(p1))
        assert same(g1, torch.zeros_like(grad) if zero_grad else grad)
        if k == 0 and bool(zero.any()):
            # g = m = v = 0: no update at all, p only decays (one fp32 multiply), m and v stay exactly 0
            decay = torch.tensor(t["c"]["decay"], dtype=torch.float32)
            assert same(p1[zero], p0[zero] * decay)
            assert float(m1[zero].abs().max()) == 0.0 and float(v1[zero].abs().max()) == 0.0
            if weight_decay == 0.0:   # p is still the planted tie: the mirror went to the even upper half
                pb = bits(p0[zero]).to(torch.int64) & 0xFFFFFFFF
                assert torch.equal(R.bf16_bits(mir[zero]).to(torch.int64), (pb >> 16) + ((pb >> 16) & 1))
    assert a.guards_untouched()


# ------------------------------------------------------------------------------- b. launch geometry changes nothing
_GEOM = dict(eps_mode=1, weight_decay=0.1, gscale=0.125, step=2)


def _run_adam(ops, a, max_blocks=0, zero_grad=True, **over):
    kw = dict(_GEOM, **over)
    ops.adam_step(a["p"], a["g"], a["m"], a["v"], a.n, R.HYPER["lr"], R.HYPER["beta1"], R.HYPER["beta2"], R.HYPER["eps"], kw["step"],
                  eps_mode=kw["eps_mode"], weight_decay=kw["weight_decay"], gscale=kw["gscale"], mirror=a["mirror"],
                  zero_grad=zero_grad, max_blocks=max_blocks)
    return {k: a.host(k) for k in ("p", "m", "v", "mirror", "g")}


_BASE = {}


def _baseline(ops, dev, n):
    if n not in _BASE:
        _BASE[n] = _run_adam(ops, Arena(dev, n, s0=0, trail=0))
    return _BASE[n]


@pytest.mark.parametrize("s0", [4, 1028])
@pytest.mark.parametrize("max_blocks", [0, 1, 3, 48])
def test_adam_step_launch_geometry_is_bit_invariant(dev, max_blocks, s0):
    ops = _ops()
    n = R.WRAPPED_N
    base = _baseline(ops, dev, n)
    a = Arena(dev, n, s0=s0, trail=68)
    got = _run_adam(ops, a, max_blocks=max_blocks)
    for k in ("p", "m", "v", "mirror", "g"):
        assert same(got[k], base[k]), k
    assert float(got["g"].abs().max()) == 0.0
    assert a.guards_untouched()


# ------------------------------------------------------------------------- c. tmi_adam_scalars + tmi_adam_step_dev
def _scalars_py(lr, beta1, beta2, step, eps_mode, weight_decay):
    """The three fp32 values written independently: doubles on the fp32 arguments, rounded once; decay all in fp32."""
    lr32, b1, b2 = (float(np.float32(x)) for x in (lr, beta1, beta2))
    c1, c2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    if eps_mode == 0:
        s, vc = np.float32(lr32 * math.sqrt(c2) / c1), np.float32(1.0)
    else:
        s, vc = np.float32(lr32 / c1), np.float32(1.0 / math.sqrt(c2))
    return [float(s), float(vc), float(np.float32(1.0) - np.float32(lr) * np.float32(weight_decay))]


@pytest.mark.parametrize("step", [1, 2, 1000, 100000])
@pytest.mark.parametrize("weight_decay", [0.0, 0.1])
@pytest.mark.parametrize("eps_mode", [0, 1])
def test_adam_scalars(dev, eps_mode, weight_decay, step):
    ops = _ops()
    got = ops.adam_scalars(R.HYPER["lr"], R.HYPER["beta1"], R.HYPER["beta2"], step, eps_mode, weight_decay)
    assert got == _scalars_py(R.HYPER["lr"], R.HYPER["beta1"], R.HYPER["beta2"], step, eps_mode, weight_decay)
    c = R.adam_constants(step=step, eps_mode=eps_mode, weight_decay=weight_decay, **R.HYPER)
    assert got == [c["step_size"], c["vcorr"], c["decay"]]   # and the reference of (a) uses these very numbers


@pytest.mark.parametrize("eps_mode", [0, 1])
@pytest.mark.parametrize("n", [3, 1027, R.WRAPPED_N])
def test_adam_step_dev_is_adam_step(dev, n, eps_mode):
    """The captured-graph form (scalars read from device memory) is the same kernel instantiation as the direct call without
    zero_grad: bit-identical p, m, v, mirror; then the scalars are overwritten in place for the next step, as
    apply_gradients_dev does between replays, and both forms run again on the state they left."""
    ops = _ops()
    wd, gscale = 0.1, 0.125
    direct, viadev = Arena(dev, n), Arena(dev, n)
    scal = torch.zeros(3, dtype=torch.float32, device=dev)
    where = scal.data_ptr()
    for k, step in enumerate((1, 2)):
        if k == 1:
            direct.set_grad(direct.g2)
            viadev.set_grad(viadev.g2)
        scal.copy_(torch.tensor(ops.adam_scalars(R.HYPER["lr"], R.HYPER["beta1"], R.HYPER["beta2"], step, eps_mode, wd),
                                dtype=torch.float32))
        assert scal.data_ptr() == where
        want = _run_adam(ops, direct, zero_grad=False, eps_mode=eps_mode, weight_decay=wd, gscale=gscale, step=step)
        ops.adam_step_dev(viadev["p"], viadev["g"], viadev["m"], viadev["v"], n, R.HYPER["beta1"], R.HYPER["beta2"], R.HYPER["eps"],
                          scal, eps_mode=eps_mode, gscale=gscale, mirror=viadev["mirror"])
        for name in ("p", "m", "v", "mirror", "g"):
            assert same(viadev.host(name), want[name]), (name, step)
        assert not same(want["p"], direct.init["p"])
    assert viadev.guards_untouched()


# ------------------------------------------------------------------------------ d. tmi_adam_step_segments geometry
# Seven variables in an arena with gaps (elements no chunk covers).  A chunk whose first element is a multiple of 4 takes the
# 16-byte path with nv = length / 4 vectors; otherwise the scalar loop.
#   var 0  [0, 1)            length 1
#   var 1  [1, 4)            length 3
#   var 2  [5, 10)           length 5, start = 1 mod 4: scalar
#   var 3  [12, 1036)        length 1024, nv = 256: the two-loads loop (i + 256 < nv) must not run, its condition is strict
#   var 4  [1036, 2064)      length 1028, nv = 257: one two-loads trip, thread 0 only
#   var 5  [2064, 10256)     length 8192, nv = 2048: production's chunk
#   var 6  [10258, 18456)    length 8198 = chunks of 8192 + 6, start = 2 mod 4: scalar on a long chunk
SEG_CHUNKS = [(0, 1, 0), (1, 4, 1), (5, 10, 2), (12, 1036, 3), (1036, 2064, 4), (2064, 10256, 5), (10258, 18450, 6), (18450, 18456, 6)]
SEG_N = 18464
SEG_KW = dict(eps_mode=0, weight_decay=0.1, gscale=0.125, step=3)


def _seg_index():
    seg = torch.full((SEG_N,), -1, dtype=torch.int64)
    for lo, hi, s in SEG_CHUNKS:
        seg[lo:hi] = s
    return seg


def _seg_arena(dev, clipped):
    p, g, g2, m, v = R.adam_inputs(SEG_N)
    if clipped:   # (without the 1e4 plants: they would put every variable far above both clips)
        g = torch.where(g.abs() > 1.0, 0.03 * torch.sign(g), g)
    return Arena(dev, SEG_N, s0=0, trail=0, data=(p, g, g2, m, v))


def _seg_run(ops, a, chunks, ss, cg, ce, max_blocks=0):
    ops.adam_step_segments(a["p"], a["g"], a["m"], a["v"], a.n, chunks, ss, 7, cg, ce, R.HYPER["lr"], R.HYPER["beta1"], R.HYPER["beta2"],
                           R.HYPER["eps"], SEG_KW["step"], eps_mode=SEG_KW["eps_mode"], weight_decay=SEG_KW["weight_decay"],
                           gscale=SEG_KW["gscale"], mirror=a["mirror"], zero_grad=True, max_blocks=max_blocks)


def _sumsq32(g):
    seg = _seg_index()
    return torch.stack([(g[seg == s].double() ** 2).sum() for s in range(7)]).float()


def test_adam_segments_without_clipping_is_adam_step(dev):
    ops = _ops()
    chunks = torch.tensor(SEG_CHUNKS, dtype=torch.int64, device=dev)
    covered = _seg_index() >= 0
    a, flat = _seg_arena(dev, False), _seg_arena(dev, False)
    _seg_run(ops, a, chunks, None, 0.0, 0.0)
    want = _run_adam(ops, flat, **SEG_KW)
    for k in ("p", "m", "v", "mirror", "g"):
        got = a.host(k)
        assert same(got[covered], want[k][covered]), k
        assert same(got[~covered], a.init[k][~covered]), k   # the gaps belong to nobody
    assert float(a.host("g")[covered].abs().max()) == 0.0


# The clip factors add roundings to g' (block_sum_256: a 6-level butterfly and 3 cross-wave additions, depth 9, of
# non-negative terms):
#   c_g = clip_global / fmaxf(sqrtf(t), clip_global)     t: 9 -> 4.5 after the square root; sqrtf 1, divide 1: at most 7
#   c_s = clip_each / fmaxf(c_g * sqrtf(sumsq[s]), ..)   sqrtf 1, multiply 1, c_g's 7, divide 1: 10
#   scale = gscale * c_g * c_s                           two multiplies, then adam1's g * scale: 3
# so kg = 7 + 10 + 3 = 20 in place of 1 (fmaxf is exact and monotone: it never enlarges a relative error).  The kernel and
# the reference are given the same fp32 sums of squares, so these carry no error of their own.
SEG_KG = 20


@pytest.fixture(scope="module")
def seg_clipped(dev):
    """One launch over the whole table with both clips on: (arena, sumsq, outputs)."""
    ops = _ops()
    a = _seg_arena(dev, True)
    ss = _sumsq32(a.init["g"]).to(dev)
    chunks = torch.tensor(SEG_CHUNKS, dtype=torch.int64, device=dev)
    _seg_run(ops, a, chunks, ss, 1.0, 0.5)
    return a, ss, chunks, {k: a.host(k) for k in ("p", "m", "v", "mirror", "g")}


def test_adam_segments_with_clipping_against_float64(dev, seg_clipped):
    a, ss, chunks, got = seg_clipped
    seg = _seg_index()
    covered = seg >= 0
    cg, cs = R.clip_factors(ss.cpu().double(), seg.clamp(min=0), 1.0, 0.5)
    assert cg < 1.0 and bool((cs[covered] < 1.0).any()) and bool((cs[covered] == 1.0).any())   # both clips bite, not everywhere
    t = R.adam_terms(a.init["p"], a.init["g"], a.init["m"], a.init["v"], gfactor=cg * cs, **SEG_KW, **R.HYPER)
    b = R.adam_bounds(t, kg=SEG_KG)
    for name in ("p", "m", "v"):
        frac = R.bound_fraction(got[name][covered], t[name][covered], b[name][covered])
        print(f"adam_segments clipped {name}: {frac:.3f} of its bound")
        within(f"optk adam_segments clipped {name} / bound", frac, 1.0)
        assert same(got[name][~covered], a.init[name][~covered])
    assert same(got["mirror"][covered], got["p"][covered].to(torch.bfloat16))
    assert float(got["g"][covered].abs().max()) == 0.0 and same(got["g"][~covered], a.init["g"][~covered])


@pytest.mark.parametrize("k", [3, 5])
def test_adam_segments_in_two_launches(dev, seg_clipped, k):
    ops = _ops()
    _, ss, chunks, want = seg_clipped
    a = _seg_arena(dev, True)
    seg = _seg_index()
    late = torch.zeros(SEG_N, dtype=torch.bool)
    for lo, hi, _ in SEG_CHUNKS[k:]:
        late[lo:hi] = True
    _seg_run(ops, a, chunks[:k], ss, 1.0, 0.5)
    for name in ("p", "m", "v", "mirror", "g"):   # the first sub-table leaves the second one's elements, and the gaps, alone
        assert same(a.host(name)[late | (seg < 0)], a.init[name][late | (seg < 0)]), name
    _seg_run(ops, a, chunks[k:], ss, 1.0, 0.5, max_blocks=2)
    for name in ("p", "m", "v", "mirror", "g"):
        assert same(a.host(name), want[name]), name


def test_adam_segments_one_workgroup_walks_every_chunk(dev, seg_clipped):
    ops = _ops()
    _, ss, chunks, want = seg_clipped
    a = _seg_arena(dev, True)
    _seg_run(ops, a, chunks, ss, 1.0, 0.5, max_blocks=1)
    for name in ("p", "m", "v", "mirror", "g"):
        assert same(a.host(name), want[name]), name


# ------------------------------------------------------------------------------------------------- e. tmi_grad_pack
def _from_bits(words):
    return torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in words], dtype=torch.int64).to(torch.int32).view(torch.float32)


# +-0, fp32 subnormals, ties of both parities, the neighbourhood of bf16's largest finite value 0x7F7F0000 (0x7F7F7FFF is
# the last value that rounds down to it, 0x7F7F8000 is the tie that goes to the even side: infinity), fp32's largest, +-inf
_SPECIAL_BITS = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00012345, 0x807FFFFF, 0x00800000,
                 0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF,
                 0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7F8001, 0x7F7FFFFF, 0xFF7F7FFF, 0xFF7F8000, 0xFF7FFFFF,
                 0x7F800000, 0xFF800000, 0x7EFF8000, 0x7F000000]
PACK_NS = (1, 7, 8, 9, 8 * 256 * 2 + 5, 8 * 256 * 4096 + 8 * 100 + 3)   # the last wraps the 4096-workgroup grid once


def _pack_src(n):
    gen = torch.Generator().manual_seed(77 + n)
    x = torch.randn(n, generator=gen, dtype=torch.float32) * 0.05
    sp = _from_bits(_SPECIAL_BITS)
    i = torch.arange(n)
    planted = (i // len(sp)) % 3 == 0
    return torch.where(planted, sp[i % len(sp)], x)


_PACK_SRC = {}


@pytest.mark.parametrize("dst_off", [0, 1])
@pytest.mark.parametrize("src_off", [0, 1])
@pytest.mark.parametrize("n", PACK_NS)
def test_grad_pack_is_one_multiply_and_one_rounding(dev, n, src_off, dst_off):
    """dst = bf16(src * scale), bit for bit against the CPU: one fp32 multiply, one round-to-nearest-even.  An offset of one
    element on either pointer leaves the 16-byte path for the scalar one."""
    ops = _ops()
    if n not in _PACK_SRC:
        _PACK_SRC[n] = _pack_src(n)
    src = _PACK_SRC[n]
    sbuf = torch.zeros(n + 9, dtype=torch.float32)
    sbuf[src_off:src_off + n] = src
    sbuf = sbuf.to(dev)
    guard = guard_pattern(n + 24, torch.bfloat16)
    for scale in (1.0, 0.5, 1.0 / 3.0):
        dbuf = guard.to(dev)
        ops.grad_pack(sbuf[src_off:src_off + n], dbuf[dst_off:dst_off + n], n, scale)
        got = dbuf.cpu()
        want = (src * torch.tensor(float(np.float32(scale)), dtype=torch.float32)).to(torch.bfloat16)
        assert same(got[dst_off:dst_off + n], want), (scale, int((bits(got[dst_off:dst_off + n]) != bits(want)).sum()))
        assert same(got[:dst_off], guard[:dst_off]) and same(got[dst_off + n:], guard[dst_off + n:])
    prod = src * torch.tensor(float(np.float32(1.0 / 3.0)), dtype=torch.float32)   # torch's conversion is itself RNE
    assert torch.equal(R.bf16_bits(prod.to(torch.bfloat16)), R.bf16_rne_bits(prod))


# ----------------------------------------------------------------------------------------------- f. tmi_grad_unpack
# Against float64: nparts additions and one multiply, every partial sum at most sum|piece| -> (nparts + 1) u sum|piece| |scale|.
@pytest.mark.parametrize("n", [1, 9, 8 * 256 * 2 + 5])
@pytest.mark.parametrize("nparts", [1, 2, 8])
@pytest.mark.parametrize("wire", [torch.bfloat16, torch.float32])
def test_grad_unpack(dev, wire, nparts, n):
    ops = _ops()
    n8 = (n + 7) // 8 * 8
    gen = torch.Generator().manual_seed(n + nparts)
    for stride in (n8, n8 + 8, n8 + 3):   # the last: rows off the 16-byte grid, scalar path whenever nparts > 1
        src = torch.full((nparts * stride + 8,), NAN, dtype=torch.float32)
        pieces = torch.randn(nparts, n, generator=gen, dtype=torch.float32) * 0.05
        pieces[:, ::5] *= 1e3
        pieces = pieces.to(wire)
        for q in range(nparts):
            src[q * stride:q * stride + n] = pieces[q].float()
        src = src.to(wire)
        sdev = src.to(dev)
        for scale in (1.0, 0.125):
            for off in (0, 1):
                guard = guard_pattern(n + 16, torch.float32)
                dbuf = guard.to(dev)
                ops.grad_unpack(sdev, dbuf[off:off + n], n, nparts=nparts, part_stride=stride, scale=scale)
                got = dbuf.cpu()
                assert same(got[off:off + n], R.unpack_ref(src, nparts, stride, n, scale)), (stride, scale, off)
                assert same(got[:off], guard[:off]) and same(got[off + n:], guard[off + n:])
                exact = pieces.double().sum(0) * scale
                bound = (nparts + 1) * U * pieces.double().abs().sum(0) * scale
                within("optk grad_unpack / bound", R.bound_fraction(got[off:off + n], exact, bound), 1.0, (str(wire), nparts, n))


# ---------------------------------------------------------------------------------- g. tmi_colsum / tmi_colsum_batched
# Bound per column: rows * u * sum_rows|dy| for the additions (fewer than `rows` of them on any path: four loads per wave,
# eight waves, at most a few workgroups) plus one ulp of the pre-filled value the atomics add into.  The pre-fill is N(0, 1)
# and every multi-workgroup shape has sum|dy| in the tens, so the additions' allowance also covers a second atomic's rounding.
COLSUM_SHAPES = [(1, 8, 8), (31, 520, 520), (33, 776, 1024), (8 * 4 * 3 + 5, 2048 + 8, 2304)]


def _colsum_data(L, rows, N, ld, dy_sb, dtype, seed, exact=False):
    gen = torch.Generator().manual_seed(seed)
    flat = torch.full(((L - 1) * dy_sb + rows * ld + 8,), NAN, dtype=torch.float32)
    vals = torch.randn(L, rows, N, generator=gen, dtype=torch.float32)
    if exact:   # multiples of 1/8 below 16: every fp32 partial sum is exact, whatever the order
        vals = (vals * 16).round().clamp(-120, 120) / 8
    vals = vals.to(dtype)
    view = torch.as_strided(flat, (L, rows, N), (dy_sb, ld, 1))
    view.copy_(vals.float())
    return flat.to(dtype), vals


def _colsum_check(got, pre, vals, name, detail):
    ref = pre.double() + vals.double().sum(0)
    ulp = torch.from_numpy(np.spacing(np.abs(pre.numpy()))).double()
    bound = vals.shape[0] * U * vals.double().abs().sum(0) + ulp
    within(name, R.bound_fraction(got, ref, bound), 1.0, detail)


@pytest.mark.parametrize("rows,N,ld", COLSUM_SHAPES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_colsum_forms(dev, dtype, rows, N, ld):
    ops = _ops()
    gen = torch.Generator().manual_seed(rows)
    # one matrix with ld >= N through tmi_colsum, and the same through tmi_colsum_batched's L = 1, strides 0 form
    flat, vals = _colsum_data(1, rows, N, ld, 0, dtype, 300 + rows)
    fdev = flat.to(dev)
    for form in ("plain", "batched L=1"):
        pre = torch.randn(N + 8, generator=gen, dtype=torch.float32)
        out = pre.to(dev)
        if form == "plain":
            ops.bias_grad(torch.as_strided(fdev, (rows, N), (ld, 1)), out[:N])
        else:
            ops.bias_grad_batched(torch.as_strided(fdev, (1, rows, N), (0, ld, 1)), out, 0)
        got = out.cpu()
        _colsum_check(got[:N], pre[:N], vals[0], "optk colsum / bound", (form, str(dtype), rows, N, ld))
        assert same(got[N:], pre[N:])
    # three matrices, a NaN-filled gap between them, outputs N + 16 apart
    L, dy_sb, out_sb = 3, rows * ld + 8 * 5, N + 16
    flat, vals = _colsum_data(L, rows, N, ld, dy_sb, dtype, 400 + rows)
    fdev = flat.to(dev)
    pre = torch.randn(L * out_sb, generator=gen, dtype=torch.float32)
    out = pre.to(dev)
    ops.bias_grad_batched(torch.as_strided(fdev, (L, rows, N), (dy_sb, ld, 1)), out, out_sb)
    got = out.cpu().view(L, out_sb)
    for l in range(L):
        _colsum_check(got[l, :N], pre.view(L, out_sb)[l, :N], vals[l], "optk colsum batched / bound", (str(dtype), rows, N, ld, l))
    assert same(got[:, N:], pre.view(L, out_sb)[:, N:])


@pytest.mark.parametrize("rows,N,ld", COLSUM_SHAPES[1:])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_colsum_deterministic_mode(dev, dtype, rows, N, ld):
    """One workgroup per column group: no atomic order, so a run repeats bit for bit, for the rows in any order.  fp32 addition
    is not associative, so two ORDERS agree bit for bit only on data whose partial sums are all exact: on such data the result
    is also the exact sum, in either mode - every row counted once and once only."""
    ops = _ops()
    L, dy_sb, out_sb = 3, rows * ld + 8 * 5, N + 16
    perm = torch.randperm(rows, generator=torch.Generator().manual_seed(9))
    pre = torch.randn(L * out_sb, generator=torch.Generator().manual_seed(10), dtype=torch.float32).round()

    def run(vals):
        flat = torch.full(((L - 1) * dy_sb + rows * ld + 8,), NAN, dtype=torch.float32)
        torch.as_strided(flat, (L, rows, N), (dy_sb, ld, 1)).copy_(vals.float())
        out = pre.to(dev)
        ops.bias_grad_batched(torch.as_strided(flat.to(dtype).to(dev), (L, rows, N), (dy_sb, ld, 1)), out, out_sb)
        return out.cpu()

    _, vals = _colsum_data(L, rows, N, ld, dy_sb, dtype, 500 + rows)
    _, exact = _colsum_data(L, rows, N, ld, dy_sb, dtype, 600 + rows, exact=True)
    want = (pre.double().view(L, out_sb)[:, :N] + exact.double().sum(1)).float()
    assert same(run(exact).view(L, out_sb)[:, :N], want) and same(run(exact[:, perm]).view(L, out_sb)[:, :N], want)   # default mode
    was = ops.set_deterministic(True)
    try:
        first = run(vals)
        assert same(run(vals), first)
        permuted = run(vals[:, perm])
        assert same(run(vals[:, perm]), permuted)
        for l in range(L):
            _colsum_check(first.view(L, out_sb)[l, :N], pre.view(L, out_sb)[l, :N], vals[l], "optk colsum deterministic / bound",
                          (str(dtype), rows, N, ld, l))
        assert same(run(exact).view(L, out_sb)[:, :N], want) and same(run(exact[:, perm]).view(L, out_sb)[:, :N], want)
    finally:
        ops.set_deterministic(was)


# ------------------------------------------------------------------------------------------ h. tmi_gelu_bwd_batched
_GELU_PLANTED = [0.0, 0.5, -0.5, 3.0, -3.0, 6.0, -6.0, 12.0, -12.0]   # zero crossing, the derivative's extrema, both tails


@pytest.mark.parametrize("nlen", ["vec", "vec*257", "131072+vec*37"])
@pytest.mark.parametrize("nbatch", [1, 5, 64])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gelu_bwd_batched(dev, dtype, nbatch, nlen):
    """Three different batch strides (dx_sb != dy_sb is Whisper's FFN backward), dx's gaps are guards.  With nbatch = 64 the
    grid is capped at 64 workgroups per span, so the longest span wraps it."""
    ops = _ops()
    vec = 8 if dtype == torch.bfloat16 else 4
    n = {"vec": vec, "vec*257": vec * 257, "131072+vec*37": 131072 + vec * 37}[nlen]
    dy_sb, u_sb, dx_sb = n, n + vec, n + 2 * vec
    gen = torch.Generator().manual_seed(nbatch * 7 + vec)
    dy = torch.randn(nbatch, n, generator=gen, dtype=torch.float32).to(dtype)
    u = (torch.randn(nbatch, n, generator=gen, dtype=torch.float32) * 1.5)
    planted = torch.tensor(_GELU_PLANTED, dtype=torch.float32)
    k = min(n, len(planted))
    u[:, :k] = planted[:k]
    u[:, n - k:] = planted[:k].flip(0)
    u = u.to(dtype)
    ubuf = torch.full((nbatch, u_sb), NAN, dtype=dtype)
    ubuf[:, :n] = u
    guard = guard_pattern(nbatch * dx_sb, dtype).view(nbatch, dx_sb)
    dx = guard.to(dev)
    ops.gelu_bwd_batched(dy.to(dev), ubuf.to(dev), dx, n, nbatch, dy_sb, u_sb, dx_sb)
    got = dx.cpu()
    ur = u.double().requires_grad_(True)
    O.gelu_erf(ur).backward(dy.double())
    err = float((got[:, :n].double() - ur.grad).abs().max() / ur.grad.abs().max())
    within(f"optk gelu_bwd_batched {'bf16' if vec == 8 else 'fp32'} / tol", err / tol(dtype), 1.0, (nbatch, n))
    assert same(got[:, n:], guard[:, n:])
    if nbatch == 1:
        one = torch.empty(n, dtype=dtype, device=dev)
        ops.gelu_bwd(dy[0].to(dev), u[0].to(dev), one)
        assert same(one, got[0, :n])


# --------------------------------------------------------------------------------------------------- i. small ones
def test_sumsq_accumulate_and_overwrite(dev):
    ops = _ops()
    x = (torch.randn(5003, generator=torch.Generator().manual_seed(3), dtype=torch.float32))
    exact = float((x.double() ** 2).sum())
    out = torch.tensor([NAN, 7.0], dtype=torch.float32, device=dev)
    ops.sumsq(x.to(dev), out, x.numel(), accumulate=False)      # overwrites whatever was there
    got = out.cpu()
    # n additions of non-negative terms at most, on any path: n u relative (test_casts_and_feats allows 1e-4)
    within("optk sumsq / bound", abs(float(got[0]) - exact) / (x.numel() * U * exact), 1.0)
    assert float(got[1]) == 7.0
    out = torch.tensor([1000.0, 7.0], dtype=torch.float32, device=dev)
    ops.sumsq(x.to(dev), out, x.numel(), accumulate=True)       # adds to it
    got = out.cpu()
    within("optk sumsq accumulate / bound", abs(float(got[0]) - (1000.0 + exact)) / (x.numel() * U * (1000.0 + exact)), 1.0)
    assert float(got[1]) == 7.0


@pytest.mark.parametrize("a,b,w,scale", [(2.5, 0.75, 0.1, 0.125), (1e-3, 40.0, 3.0, 1.0 / 3.0), (NAN, 1.0, 0.1, 0.5), (1.0, NAN, 0.1, 0.5)])
def test_loss_combine(dev, a, b, w, scale):
    """out = (isnan(a + w b) ? 0 : a + w b) * scale: multiply, add, multiply = 3 roundings, held to 4 u."""
    ops = _ops()
    ta, tb = torch.tensor([a], dtype=torch.float32, device=dev), torch.tensor([b], dtype=torch.float32, device=dev)
    out = torch.tensor([NAN, 7.0], dtype=torch.float32, device=dev)
    ops.loss_combine(ta, tb, w, scale, out)
    got = out.cpu()
    a32, b32, w32, s32 = (float(np.float32(x)) for x in (a, b, w, scale))
    if math.isnan(a) or math.isnan(b):
        assert float(got[0]) == 0.0
    else:
        ref = (a32 + w32 * b32) * s32
        within("optk loss_combine / 4u", abs(float(got[0]) - ref) / (4 * U * (abs(a32) + abs(w32 * b32)) * abs(s32)), 1.0)
    assert float(got[1]) == 7.0


# ------------------------------------------------------------------------------------- j. rejections, by return code
def test_bad_arguments_are_refused_before_any_launch(dev):
    """Each call fails the host-side argument check; the buffers are large enough for every call as written all the same."""
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib
    L = _lib.lib()
    f = [torch.zeros(4096, dtype=torch.float32, device=dev) for _ in range(4)]
    h = torch.zeros(4096, dtype=torch.bfloat16, device=dev)
    act = torch.zeros(64, dtype=torch.uint8, device=dev)
    p, g, m, v = (t.data_ptr() for t in f)
    lr, b1, b2, eps = R.HYPER["lr"], R.HYPER["beta1"], R.HYPER["beta2"], R.HYPER["eps"]
    n = 64
    calls = {
        "adam_step, p off by one element": (b"tmi_adam_step:", lambda: L.tmi_adam_step(p + 4, g, m, v, n, lr, b1, b2, eps, 1, 0, 0.0, 1.0, None, 0, 0, None)),
        "adam_step, mirror off by two elements": (b"tmi_adam_step:", lambda: L.tmi_adam_step(p, g, m, v, n, lr, b1, b2, eps, 1, 0, 0.0, 1.0, h.data_ptr() + 4, 0, 0, None)),
        "adam_step, step 0": (b"tmi_adam_step:", lambda: L.tmi_adam_step(p, g, m, v, n, lr, b1, b2, eps, 0, 0, 0.0, 1.0, None, 0, 0, None)),
        "adam_step_rows, weight decay": (b"tmi_adam_step_rows:", lambda: L.tmi_adam_step_rows(p, g, m, v, 4, 16, act.data_ptr(), lr, b1, b2, eps, 1, 0, 0.1, 1.0, None, 0, None)),
        "grad_unpack, overlapping parts": (b"tmi_grad_unpack:", lambda: L.tmi_grad_unpack(p, _lib.TMI_F32, 2, n - 1, g, n, 1.0, None)),
        "colsum_batched, N = 4 in bf16": (b"tmi_colsum:", lambda: L.tmi_colsum_batched(h.data_ptr(), 8, 64, p, 8, 4, 4, 1, _lib.TMI_BF16, None)),
        "colsum_batched, dy_sb = 4 in bf16": (b"tmi_colsum:", lambda: L.tmi_colsum_batched(h.data_ptr(), 8, 4, p, 8, 4, 8, 2, _lib.TMI_BF16, None)),
        "gelu_bwd_batched, dx_sb = 2 (fp32)": (b"tmi_gelu_bwd:", lambda: L.tmi_gelu_bwd_batched(p, g, m, 8, 2, 8, 8, 2, _lib.TMI_F32, None)),
        "gelu_bwd_batched, dx_sb = 2 (bf16)": (b"tmi_gelu_bwd:", lambda: L.tmi_gelu_bwd_batched(h.data_ptr(), h.data_ptr() + 1024, h.data_ptr() + 2048, 8, 2, 8, 8, 2, _lib.TMI_BF16, None)),
    }
    for what, (who, call) in calls.items():
        rc = call()
        assert rc == TMI_ERR_INVALID, (what, rc)
        msg = L.tmi_last_error()
        assert msg and msg.startswith(who), (what, msg)
    torch.cuda.synchronize()
    assert all(float(t.abs().max()) == 0.0 for t in f) and float(h.float().abs().max()) == 0.0
