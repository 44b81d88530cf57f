"""tmi_dropout's shapes and fall-backs, tmi_cast_bf16, tmi_transpose_cast_bf16, tmi_feat_to_channels_last and
tmi_logmel_from_spectrum (csrc/adam_misc.hip) against tests/_layout_ref.py (itself checked by tests/test_layout_ref_cpu.py).

Every buffer lies inside 7.0 / NaN guards (_row_kernel_ref.guard_pattern), and so does every gap between rows that a kernel
does not own: after a call the owned elements are compared bit for bit with the reference (any NaN where it has a NaN), every
other element with what it held before.  The log-mel outputs go through _margins.within as measured / bound with the bound 1
under the names "logmel ..."; nothing here is fitted to what the kernels give.

Which branch a shape reaches, from the launch code:
  tmi_dropout     16-byte kernel when cols % 8 == 0 and every pointer and row stride is a multiple of 16 bytes, else the pair
                  kernel; both launch min(ceil(work / 256), 2048) workgroups and stride, so more than 524288 chunks of 8
                  (2100 x 2048) or pairs (1030 x 1026) make the second trip of the loop.
  tmi_cast_bf16   min(ceil(rows ldd / 256), 8192) workgroups: 2100003 elements are 8204.
  transpose       64 x 64 tiles: 1, 63, 64, 65, 130 are one lane, a ragged tile, a full one, a tile plus one, two plus two.
  feat            tiles of 64 padded time steps, 64 (C + 1) floats of LDS: C = 256 is 65792 bytes, above the 64 KiB default.
  log-mel         one wave per frame, four per workgroup; lanes stride n_bins and n_mels by 64; 4 n_bins floats of LDS.
"""
import pytest
import torch

import _layout_ref as L
import _row_kernel_ref as R
from _margins import within

pytestmark = pytest.mark.gpu

F32, BF16 = L.F32, L.BF16
DTYPES = [F32, BF16]
TMI_ERR_INVALID = -1  # include/tethys_mi.h
PAD = 64              # guard elements either side: a multiple of 16 bytes for both dtypes


def _mods():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib, ops
    return ops, _lib.lib(), _lib


def _DO():
    from oracle import dropout as DO
    return DO


def dt_code(dtype):
    import tethys_speech_amd._lib as LB
    return LB.TMI_BF16 if dtype == BF16 else LB.TMI_F32


class Buf:
    """``n`` elements inside guards; ``place(idx, values)`` writes inputs into the host image before it goes to the device."""

    def __init__(self, dev, dtype, n, idx=None, values=None):
        host = R.guard_pattern(n + 2 * PAD, dtype)
        if idx is not None:
            host[PAD + idx.reshape(-1)] = values.reshape(-1).to(dtype)
        self.host0, self.t, self.n, self.dtype = host.clone(), host.to(dev), n, dtype

    def ptr(self, off=0):
        return self.t.data_ptr() + (PAD + off) * self.t.element_size()

    def untouched(self):
        return torch.equal(L.bits(self.t), L.bits(self.host0))

    def check(self, idx, want, what):
        """The elements at ``idx`` (into the body) hold ``want``; everything else is what it was."""
        now = self.t.cpu()
        idx = idx.reshape(-1) + PAD
        assert L.same_bits(now[idx], want.reshape(-1)), what
        other = torch.ones(now.numel(), dtype=torch.bool)
        other[idx] = False
        assert torch.equal(L.bits(now)[other], L.bits(self.host0)[other]), f"{what}: a store outside the owned elements"


def rows_idx(rows, cols, ld, off=0):
    return off + torch.arange(rows)[:, None] * ld + torch.arange(cols)[None, :]


# =========================================================================================== tmi_dropout
_KEEP = {}


def _keep(rows, cols, p):
    if (rows, cols, p) not in _KEEP:
        _KEEP[(rows, cols, p)] = torch.from_numpy(_DO().keep_flat(L.LAYOUT_DROP_SEED, rows, cols, p))
    return _KEEP[(rows, cols, p)]


def _dropout(dev, dtype, rows, cols, p, *, ld_in=None, ld_res=None, ld_out=None, in_off=0, resid=True, in_place=False):
    """One C-level call on guarded buffers -> (rc, X, RS, OUT, the expected output [rows, cols])."""
    _, lib, _ = _mods()
    ld_in, ld_res, ld_out = ld_in or cols, ld_res or cols, ld_out or cols
    x = R.to_dtype(R.randn((rows, cols), 91), dtype)
    r = R.to_dtype(R.randn((rows, cols), 92), dtype) if resid else None
    X = Buf(dev, dtype, in_off + rows * ld_in, rows_idx(rows, cols, ld_in, in_off), x)
    RS = Buf(dev, dtype, rows * ld_res, rows_idx(rows, cols, ld_res), r) if resid else None
    OUT = X if in_place else Buf(dev, dtype, rows * ld_out)
    rc = lib.tmi_dropout(X.ptr(in_off), ld_in, RS.ptr() if resid else None, ld_res if resid else 0,
                         X.ptr(in_off) if in_place else OUT.ptr(), ld_in if in_place else ld_out, rows, cols, p,
                         L.LAYOUT_DROP_SEED, dt_code(dtype), _mods()[0].stream())
    torch.cuda.synchronize()
    return rc, X, RS, OUT, (x, r)


def _dropout_ok(dev, dtype, rows, cols, p, what, **kw):
    rc, X, RS, OUT, (x, r) = _dropout(dev, dtype, rows, cols, p, **kw)
    assert rc == 0, what
    want = L.dropout_expected(x, r, _keep(rows, cols, p), _DO().keep_scale(p), dtype)
    if kw.get("in_place"):
        OUT.check(rows_idx(rows, cols, kw.get("ld_in") or cols, kw.get("in_off", 0)), want, what)
    else:
        OUT.check(rows_idx(rows, cols, kw.get("ld_out") or cols), want, what)
        assert X.untouched(), what
    assert RS is None or RS.untouched(), what


@pytest.mark.parametrize("p", L.LAYOUT_DROP_P)
def test_dropout_16_byte_kernel_past_its_workgroup_cap(dev, p):
    assert 2100 * (2048 // 8) > 2048 * 256
    _dropout_ok(dev, BF16, 2100, 2048, p, "2100 x 2048 bf16")


@pytest.mark.parametrize("p", L.LAYOUT_DROP_P)
def test_dropout_pair_kernel_past_its_workgroup_cap(dev, p):
    assert 1026 % 8 != 0 and 1030 * (1026 // 2) > 2048 * 256
    _dropout_ok(dev, F32, 1030, 1026, p, "1030 x 1026 fp32")


@pytest.mark.parametrize("p", L.LAYOUT_DROP_P)
@pytest.mark.parametrize("dtype", DTYPES, ids=R.dname)
def test_dropout_falls_back_to_the_pair_kernel_on_misaligned_operands(dev, dtype, p):
    """cols % 8 == 0, so the 16-byte kernel would be chosen - were it not for an input pointer 4 bytes off, or a row stride
    of 1026 elements (not a multiple of 16 bytes in either dtype) on one operand.  The bits are those of the aligned call."""
    rows, cols = 64, 1024
    _dropout_ok(dev, dtype, rows, cols, p, "aligned")
    _dropout_ok(dev, dtype, rows, cols, p, "in + 4 bytes", in_off=4 // (2 if dtype == BF16 else 4))
    assert (1026 * 2) % 16 != 0 and (1026 * 4) % 16 != 0
    for which in ("ld_in", "ld_res", "ld_out"):
        _dropout_ok(dev, dtype, rows, cols, p, f"{which} = 1026", **{which: 1026})
    _dropout_ok(dev, dtype, rows, cols, p, "in place, ld 1026", ld_in=1026, in_place=True, resid=False)


@pytest.mark.parametrize("p", L.LAYOUT_DROP_P)
@pytest.mark.parametrize("dtype", DTYPES, ids=R.dname)
def test_dropout_one_row_two_columns_and_the_widest_row(dev, dtype, p):
    _dropout_ok(dev, dtype, 1, 1024, p, "rows = 1, 16-byte kernel")
    _dropout_ok(dev, dtype, 1, 1026, p, "rows = 1, pair kernel", resid=False)
    _dropout_ok(dev, dtype, 600, 2, p, "cols = 2")
    _dropout_ok(dev, dtype, 600, 2, p, "cols = 2, ld 5", ld_in=5, ld_res=3, ld_out=7)
    _dropout_ok(dev, dtype, 3, 131072, p, "cols = 2^17, the last accepted width")


@pytest.mark.parametrize("dtype", DTYPES, ids=R.dname)
def test_dropout_refuses_wide_odd_and_short_rows_and_writes_nothing(dev, dtype):
    ops, lib, _ = _mods()
    for what, rows, cols, ld in (("cols = 2^17 + 2", 1, 131074, {}), ("odd cols", 4, 7, {}), ("cols = 1", 4, 1, {}),
                                 ("ld_in < cols", 4, 8, dict(ld_in=6)), ("ld_out < cols", 4, 8, dict(ld_out=6)),
                                 ("ld_res < cols", 4, 8, dict(ld_res=6))):
        n = rows * cols   # the buffers hold whole rows of ``cols`` whatever the refused stride says
        X, RS = (Buf(dev, dtype, n, torch.arange(n), torch.ones(n)) for _ in range(2))
        OUT = Buf(dev, dtype, n)
        rc = lib.tmi_dropout(X.ptr(), ld.get("ld_in", cols), RS.ptr(), ld.get("ld_res", cols), OUT.ptr(), ld.get("ld_out", cols),
                             rows, cols, 0.1, 5, dt_code(dtype), ops.stream())
        torch.cuda.synchronize()
        assert rc == TMI_ERR_INVALID and OUT.untouched(), what


# =========================================================================================== tmi_cast_bf16
def _cast(dev, rows, cols, lds, ldd, src_off=0, dst_off=0, seed=93):
    ops, _, _ = _mods()
    n_src = src_off + (rows - 1) * lds + cols
    src = L.special_input((n_src,), seed)
    S = Buf(dev, F32, n_src, torch.arange(n_src), src)
    D = Buf(dev, BF16, dst_off + rows * ldd + 5)
    ops.cast_bf16(S.t, lds, D.t, ldd, rows, cols, src_off=PAD + src_off, dst_off=PAD + dst_off)
    torch.cuda.synchronize()
    idx, val = L.cast_ref(src, rows, cols, lds, ldd, src_off, dst_off)
    D.check(idx, val, ("cast", rows, cols, lds, ldd, src_off, dst_off))
    assert S.untouched()
    if ldd > cols:   # the pad columns are +0
        pad = D.t.cpu()[PAD + rows_idx(rows, ldd - cols, ldd, dst_off + cols)]
        assert not bool(L.bits(pad).count_nonzero())


def test_cast_bf16_arena_form_past_its_workgroup_cap(dev):
    n = 2_100_003
    assert -(-n // 256) > 8192
    _cast(dev, 1, n, n, n)


def test_cast_bf16_padded_rows_one_element_and_odd_offsets(dev):
    _cast(dev, 300, 205, 211, 208)
    _cast(dev, 1, 1, 1, 1)
    _cast(dev, 300, 205, 211, 208, src_off=3, dst_off=5)
    _cast(dev, 1, 4099, 4099, 4099, src_off=1, dst_off=7)


def test_cast_bf16_refusals_write_nothing(dev):
    _, lib, _ = _mods()
    st = _mods()[0].stream()
    S, D = Buf(dev, F32, 64, torch.arange(64), torch.ones(64)), Buf(dev, BF16, 64)
    for what, a in (("lds < cols", (S.ptr(), 7, D.ptr(), 8, 4, 8)), ("ldd < cols", (S.ptr(), 8, D.ptr(), 7, 4, 8)),
                    ("rows = 0", (S.ptr(), 8, D.ptr(), 8, 0, 8)), ("cols = 0", (S.ptr(), 8, D.ptr(), 8, 4, 0)),
                    ("src NULL", (None, 8, D.ptr(), 8, 4, 8)), ("dst NULL", (S.ptr(), 8, None, 8, 4, 8))):
        assert lib.tmi_cast_bf16(*a, st) == TMI_ERR_INVALID, what
        torch.cuda.synchronize()
        assert D.untouched(), what


# =========================================================================================== tmi_transpose_cast_bf16
TR_SHAPES = [(n, n) for n in (1, 63, 64, 65, 130)] + [(1, 130), (130, 1), (65, 63), (63, 65), (64, 130)]


@pytest.mark.parametrize("rows,cols", TR_SHAPES)
def test_transpose_cast_bf16_tile_edges_strides_and_offsets(dev, rows, cols):
    ops, _, _ = _mods()
    for lds, ldd, so, do in ((cols, rows, 0, 0), (cols + 3, rows + 5, 0, 0), (cols + 3, rows + 5, 3, 7)):
        n_src = so + (rows - 1) * lds + cols
        src = L.special_input((n_src,), 94)
        S = Buf(dev, F32, n_src, torch.arange(n_src), src)
        D = Buf(dev, BF16, do + cols * ldd)
        ops.transpose_cast_bf16(S.t, lds, D.t, ldd, rows, cols, src_off=PAD + so, dst_off=PAD + do)
        torch.cuda.synchronize()
        idx, val = L.transpose_ref(src, rows, cols, lds, ldd, so, do)
        D.check(idx, val, ("transpose", rows, cols, lds, ldd, so, do))   # columns rows..ldd-1 of dst keep their guards
        assert S.untouched()


def test_transpose_cast_bf16_refusals_write_nothing(dev):
    _, lib, _ = _mods()
    st = _mods()[0].stream()
    S, D = Buf(dev, F32, 64, torch.arange(64), torch.ones(64)), Buf(dev, BF16, 64)
    for what, a in (("lds < cols", (S.ptr(), 7, D.ptr(), 4, 4, 8)), ("ldd < rows", (S.ptr(), 8, D.ptr(), 3, 4, 8)),
                    ("rows = 0", (S.ptr(), 8, D.ptr(), 4, 0, 8)), ("src NULL", (None, 8, D.ptr(), 4, 4, 8))):
        assert lib.tmi_transpose_cast_bf16(*a, st) == TMI_ERR_INVALID, what
        torch.cuda.synchronize()
        assert D.untouched(), what


# =========================================================================================== tmi_feat_to_channels_last
FEAT_T = [1, 64, 300]
FEAT_PADS = [(0, 0), (1, 1), (70, 0), (0, 70)]   # 70: a whole 64-step tile of padding and six steps more


@pytest.mark.parametrize("dtype", DTYPES, ids=R.dname)
@pytest.mark.parametrize("Cn", [1, 80, 255, 256])
def test_feat_to_channels_last_every_width_length_and_padding(dev, Cn, dtype):
    """C = 256, the largest the entry point accepts, asks for 64 * 257 * 4 = 65792 bytes of dynamic LDS - more than the
    64 KiB a launch gets unless the kernel's limit is raised, which the entry point does for it."""
    _, lib, _ = _mods()
    B = 2
    for T in FEAT_T:
        f = L.special_input((B, Cn, T), 95 + T)
        Fb = Buf(dev, F32, f.numel(), torch.arange(f.numel()), f)
        for pl, pr in FEAT_PADS:
            n = B * (pl + T + pr) * Cn
            O = Buf(dev, dtype, n)
            rc = lib.tmi_feat_to_channels_last(Fb.ptr(), O.ptr(), B, Cn, T, pl, pr, dt_code(dtype), _mods()[0].stream())
            torch.cuda.synchronize()
            assert rc == 0, (Cn, T, pl, pr, lib.tmi_last_error())
            O.check(torch.arange(n), L.feat_ref(f, pl, pr, dtype), ("feat", Cn, T, pl, pr, R.dname(dtype)))
        assert Fb.untouched()


@pytest.mark.parametrize("dtype", DTYPES, ids=R.dname)
def test_feat_to_channels_last_refusals_write_nothing(dev, dtype):
    _, lib, _ = _mods()
    st = _mods()[0].stream()
    Fb, O = Buf(dev, F32, 1024, torch.arange(1024), torch.ones(1024)), Buf(dev, dtype, 1024)
    for what, a in (("C = 257", (Fb.ptr(), O.ptr(), 1, 257, 1, 0, 0)), ("B = 65536", (Fb.ptr(), O.ptr(), 65536, 1, 1, 0, 0)),
                    ("T = 0", (Fb.ptr(), O.ptr(), 1, 4, 0, 1, 1)), ("pad_left < 0", (Fb.ptr(), O.ptr(), 1, 4, 4, -1, 0)),
                    ("feats NULL", (None, O.ptr(), 1, 4, 4, 0, 0)), ("out NULL", (Fb.ptr(), None, 1, 4, 4, 0, 0))):
        assert lib.tmi_feat_to_channels_last(*a, dt_code(dtype), st) == TMI_ERR_INVALID, what
        torch.cuda.synchronize()
        assert O.untouched(), what


# =========================================================================================== tmi_logmel_from_spectrum
def _logmel_call(lib, S, M, O, ld_spec, frames, nb, nm, cf, ld_out, st):
    return lib.tmi_logmel_from_spectrum(None if S is None else S.ptr(), ld_spec, None if M is None else M.ptr(),
                                        None if O is None else O.ptr(), frames, nb, nm, L.LOGMEL_EPS, 1 if cf else 0, ld_out, st)


@pytest.mark.parametrize("kind", L.LOGMEL_KINDS)
@pytest.mark.parametrize("frames,nb,nm", L.LOGMEL_SHAPES)
def test_logmel_both_layouts_padded_strides_and_input_classes(dev, frames, nb, nm, kind):
    ops, lib, _ = _mods()
    st = ops.stream()
    for ld_spec in (2 * nb, 2 * nb + 3):
        spec, mel = L.logmel_inputs(frames, nb, nm, kind, ld_spec)
        S = Buf(dev, F32, spec.numel(), torch.arange(spec.numel()), spec)
        M = Buf(dev, F32, mel.numel(), torch.arange(mel.numel()), mel)
        for cf in (False, True):
            ref, s = L.logmel_ref(spec, mel, L.LOGMEL_EPS, cf)
            bound = L.logmel_bound(ref, s, nb)
            orow, ocol = ref.shape
            for ld_out in (ocol, ocol + 5):
                idx = rows_idx(orow, ocol, ld_out)
                runs = []
                for rep in range(2):
                    O = Buf(dev, F32, orow * ld_out)
                    assert _logmel_call(lib, S, M, O, ld_spec, frames, nb, nm, cf, ld_out, st) == 0
                    torch.cuda.synchronize()
                    got = O.t.cpu()[PAD + idx]
                    O.check(idx, got, ("logmel guards", frames, nb, nm, kind, cf, ld_spec, ld_out))
                    runs.append(got)
                assert torch.equal(L.bits(runs[0]), L.bits(runs[1])), "two calls on the same input differ"
                ratio = L.check_logmel(runs[0], ref, bound)
                detail = (frames, nb, nm, "channels-first" if cf else "frame-major", ld_spec, ld_out)
                print(f"logmel {kind}: {ratio:.3f} of its bound {detail}")
                within(f"logmel {kind} {'channels-first' if cf else 'frame-major'}", ratio, 1.0, detail)
        assert S.untouched() and M.untouched()


def test_logmel_refusals_write_nothing(dev):
    ops, lib, _ = _mods()
    st = ops.stream()
    frames, nb, nm = 5, 33, 8
    spec, mel = L.logmel_inputs(frames, nb, nm, "gauss", 2 * nb)
    S = Buf(dev, F32, spec.numel(), torch.arange(spec.numel()), spec)
    M = Buf(dev, F32, mel.numel(), torch.arange(mel.numel()), mel)
    O = Buf(dev, F32, 64 * 64)
    for what, a in (("n_bins = 4097", (S, M, O, 2 * 4097, frames, 4097, nm, False, nm)),
                    ("ld_spec < 2 n_bins", (S, M, O, 2 * nb - 1, frames, nb, nm, False, nm)),
                    ("frame-major ld_out < n_mels", (S, M, O, 2 * nb, frames, nb, nm, False, nm - 1)),
                    ("channels-first ld_out < frames", (S, M, O, 2 * nb, frames, nb, nm, True, frames - 1)),
                    ("spec NULL", (None, M, O, 2 * nb, frames, nb, nm, False, nm)),
                    ("mel NULL", (S, None, O, 2 * nb, frames, nb, nm, False, nm)),
                    ("out NULL", (S, M, None, 2 * nb, frames, nb, nm, False, nm)),
                    ("frames = 0", (S, M, O, 2 * nb, 0, nb, nm, False, nm))):
        assert _logmel_call(lib, *a, st) == TMI_ERR_INVALID, what
        torch.cuda.synchronize()
        assert O.untouched(), what
    assert _logmel_call(lib, S, M, O, 2 * nb, frames, nb, nm, False, nm, st) == 0   # the valid call is accepted
    torch.cuda.synchronize()
    assert not O.untouched()
