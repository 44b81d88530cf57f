"""tmi_layer_mix_fwd / tmi_layer_mix_bwd (csrc/layer_mix.hip) through the C ABI, against the float64 reference and the
derived bounds of tests/_layer_mix_ref.py (checked by tests/test_layer_mix_cpu.py), on its seeded cases: K 2 / 3 / 5 / 13 /
25 / 64, H 8 / 72 / 264 (an H-slice tail) / 1024, V 2 / 3 / 31 / 32 / 33 / 64 (both slice widths), bf16 and fp32 layers with
x_st = H, H + 8 (16-byte loads) and H + 1 / H + 3 (element loads), the layers as separate allocations, a permuted row_index
with one entry out of range, p 0 / 0.1 / 0.5, both reductions, ragged frame_lens with an item at 0 and one beyond T_max, an
infeasible item, and N * T_max at 350, at 513 (65 tiles: one lane of the fold adds two), at 8192 / 8193 (the last size with
tiles of 8 rows, the first with tiles of 16) and at 16500.

Every input and output lies inside a larger buffer of 7.0 / NaN guards (integers: 7 / a large negative) with padded
strides, compared bit for bit after the calls wherever the contract says nothing is written: the guard zones, the stride
padding, the frames past a clip, every input, and everything when a call is refused.  Measured / bound goes through
``_margins.within`` under the names "layer mix ..." with the bound 1; no bound is fitted to what the kernels give.  ``grad``
is seeded fp32 numbers, nonzero past the clips and on the infeasible item, where the call must not read them."""
import ctypes

import numpy as np
import pytest
import torch

import _ctc_head_ref as R
import _ctc_ref as C
import _layer_mix_ref as M
from _margins import within

pytestmark = pytest.mark.gpu

F32, I32, BF16 = torch.float32, torch.int32, torch.bfloat16
TMI_ERR_INVALID = -1
PAD = 64


def _L():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib as L
    return L


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


class G:
    """``n`` payload elements inside guards; ``v`` is the payload on the device."""

    def __init__(self, dev, dtype, n, fill=None):
        host = C.guard_pattern(n + 2 * PAD, F32 if dtype == BF16 else dtype).to(dtype)
        if fill is not None:
            fill(host[PAD:PAD + n])
        self.host0, self.t, self.n = host.clone(), host.to(dev), n
        self.v = self.t[PAD:PAD + n]

    def now(self):
        return self.t.cpu()[PAD:PAD + self.n]

    def same_where(self, keep=None):
        """The guard zones and every payload element with ``keep`` set (None: all) are bit for bit what they were."""
        full = torch.ones(self.n + 2 * PAD, dtype=torch.bool)
        if keep is not None:
            full[PAD:PAD + self.n] = torch.as_tensor(keep).reshape(-1)
        return torch.equal(bits(self.t)[full], bits(self.host0)[full])


def stream():
    return torch.cuda.current_stream().cuda_stream


def into(h, a, sn, st):
    a = torch.as_tensor(np.ascontiguousarray(a))
    n, T, c = a.shape
    torch.as_strided(h, (n, T, c), (sn, st, 1)).copy_(a.to(h.dtype))


def out_of(g, n, T, sn, st, cols):
    return torch.as_strided(g.now(), (n, T, cols), (sn, st, 1)).float().numpy().copy()


def unwritten(live, sn, st, cols):
    N, T = live.shape
    k = torch.ones(N * sn, dtype=torch.bool)
    torch.as_strided(k, (N, T, cols), (sn, st, 1)).copy_((~torch.from_numpy(live))[:, :, None].expand(N, T, cols))
    return k


class Call:
    """One case inside guard buffers; ``over`` replaces inputs of the case (a, p, reduction, frame_lens, infeasible) and the
    reference is then computed for them."""

    def __init__(self, dev, name, **over):
        if over:
            d = dict(M.case_inputs(name), **over)
            keep, _, scale = R.keep_masks(d["seed"], d["n_src"], d["row_index"], d["N"], d["T"], d["H"], d["p"])
            keep = None if d["p"] == 0.0 else keep
            x = M.gather_layers(d["layers"], d["row_index"], d["N"])
            f = M.forward(x, d["a"], d["frame_lens"])
            b = M.backward(x, d["a"], d["grad"], d["infeasible"], d["label_lens"], d["frame_lens"], d["reduction"], M.L_MAX, d["W"],
                           keep, scale)
        else:
            d, x, keep, _, scale, f, b = M.case_ref(name)
        self.dev, self.d, self.f, self.b, self.name = dev, d, f, b, name
        K, N, T, H, V = d["K"], d["N"], d["T"], d["H"], d["V"]
        self.dt = BF16 if d["dtype"] == "bf16" else F32
        self.x_st = d["x_st"]
        self.x_sn = T * self.x_st + (16 if d["x_st"] % 8 == 0 else 5)
        wide = d["x_st"] % 8 == 0                      # mixed: 16-byte stores, or element stores under odd strides
        self.m_st, self.gr_st = H + (4 if wide else 3), V + 2
        self.m_sn, self.gr_sn = T * self.m_st + (8 if wide else 5), T * self.gr_st + 5
        n_src = d["n_src"]
        # every layer is its own allocation, with guards of its own
        self.X = [G(dev, self.dt, n_src * self.x_sn, lambda h, k=k: into(h, d["layers"][k], self.x_sn, self.x_st)) for k in range(K)]
        self.table = (ctypes.c_void_p * K)(*[g.v.data_ptr() for g in self.X])
        cp = lambda a: (lambda h: h.copy_(torch.from_numpy(np.ascontiguousarray(a)).reshape(-1)))
        self.a, self.W = G(dev, F32, K, cp(d["a"])), G(dev, F32, H * V, cp(d["W"]))
        self.idx = None if d["row_index"] is None else G(dev, I32, N, cp(d["row_index"]))
        self.fl, self.ll = G(dev, I32, N, cp(d["frame_lens"])), G(dev, I32, N, cp(d["label_lens"]))
        self.grad = G(dev, F32, N * self.gr_sn, lambda h: into(h, d["grad"], self.gr_sn, self.gr_st))
        self.bad = G(dev, I32, N, cp(d["infeasible"]))
        self.inputs = self.X + [t for t in (self.a, self.W, self.idx, self.fl, self.ll, self.grad, self.bad) if t is not None]
        lib = _L().lib()
        nb = lib.tmi_layer_mix_workspace_bytes(N, T, H, V, K)
        assert nb == M.tiles(N * T) * K * 4
        self.mixed, self.w, self.g_a, self.dk, self.ws = (G(dev, F32, N * self.m_sn), G(dev, F32, K), G(dev, F32, K), G(dev, F32, K),
                                                          G(dev, F32, nb // 4))

    @staticmethod
    def _p(g):
        return None if g is None else g.v.data_ptr()

    def fwd_args(self, **over):
        d = self.d
        a = dict(layers=self.table, K=d["K"], x_dtype=1 if self.dt == BF16 else 0, x_sn=self.x_sn, x_st=self.x_st, n_src=d["n_src"],
                 row_index=self._p(self.idx), frame_lens=self.fl.v.data_ptr(), a=self.a.v.data_ptr(), w_out=self.w.v.data_ptr(),
                 mixed=self.mixed.v.data_ptr(), m_sn=self.m_sn, m_st=self.m_st, N=d["N"], T_max=d["T"], H=d["H"], stream=stream())
        a.update(over)
        return list(a.values())

    def bwd_args(self, **over):
        d = self.d
        a = dict(layers=self.table, K=d["K"], x_dtype=1 if self.dt == BF16 else 0, x_sn=self.x_sn, x_st=self.x_st, n_src=d["n_src"],
                 row_index=self._p(self.idx), frame_lens=self.fl.v.data_ptr(), label_lens=self.ll.v.data_ptr(), grad=self.grad.v.data_ptr(),
                 gr_sn=self.gr_sn, gr_st=self.gr_st, infeasible=self.bad.v.data_ptr(), p=d["p"], seed=d["seed"],
                 reduction=1 if d["reduction"] == "mean" else 0, W=self.W.v.data_ptr(), a=self.a.v.data_ptr(), g_a=self.g_a.v.data_ptr(),
                 d=self.dk.v.data_ptr(), workspace=self.ws.v.data_ptr(), workspace_bytes=self.ws.n * 4, N=d["N"], T_max=d["T"],
                 L_max=M.L_MAX, H=d["H"], V=d["V"], stream=stream())
        a.update(over)
        return list(a.values())

    def untouched(self, outputs=True):
        for t in self.inputs:
            assert t.same_where(), "an input was written"
        if outputs:
            for t in (self.mixed, self.w, self.g_a, self.dk, self.ws):
                assert t.same_where(), "a refused call wrote"

    def fwd(self, **over):
        lib = _L().lib()
        rc = lib.tmi_layer_mix_fwd(*self.fwd_args(**over))
        assert rc == 0, lib.tmi_last_error()
        torch.cuda.synchronize()
        d, live = self.d, self.f["live"]
        self.untouched(outputs=False)
        assert self.mixed.same_where(unwritten(live, self.m_sn, self.m_st, d["H"])), "mixed: a dead row or the padding was written"
        assert self.w.same_where(torch.zeros(d["K"], dtype=torch.bool))
        return {"mixed": out_of(self.mixed, d["N"], d["T"], self.m_sn, self.m_st, d["H"]), "w": self.w.now().numpy().copy(),
                "bits": torch.cat([bits(self.mixed.t), bits(self.w.t)]).clone()}

    def bwd(self, **over):
        lib = _L().lib()
        rc = lib.tmi_layer_mix_bwd(*self.bwd_args(**over))
        assert rc == 0, lib.tmi_last_error()
        torch.cuda.synchronize()
        self.untouched(outputs=False)
        for t in (self.g_a, self.dk, self.ws):   # (the whole workspace is the call's; its guards are not)
            assert t.same_where(torch.zeros(t.n, dtype=torch.bool))
        return {"g_a": self.g_a.now().numpy().copy(), "d": self.dk.now().numpy().copy(),
                "bits": torch.cat([bits(self.g_a.t), bits(self.dk.t)]).clone()}


def check(c, out, grads, tag):
    f, b, live = c.f, c.b, c.f["live"]
    assert np.isfinite(out["w"]).all() and np.isfinite(grads["g_a"]).all() and np.isfinite(grads["d"]).all()
    for key, got, ref, bound in (("w", out["w"], f["w"], f["b_w"]), ("mixed", out["mixed"][live], f["mixed"][live], f["b_mixed"][live]),
                                 ("d", grads["d"], b["d"], b["b_d"]), ("g_a", grads["g_a"], b["g_a"], b["b_g"])):
        q = C.ratio(got, ref, bound)
        print(f"layer mix {tag} {key}: {q:.4f} of its bound")
        within(f"layer mix {key} / bound", q, 1.0, tag)


@pytest.mark.parametrize("name", list(M.CASES))
def test_forward_and_backward_against_float64(dev, name):
    c = Call(dev, name)
    out, grads = c.fwd(), c.bwd()
    check(c, out, grads, name)
    # the same bits from a second pair of calls, into a workspace that now holds the first call's partial sums
    out2, grads2 = c.fwd(), c.bwd()
    assert torch.equal(out["bits"], out2["bits"]) and torch.equal(grads["bits"], grads2["bits"])


@pytest.mark.parametrize("reduction", ["sum", "mean"])
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_every_rate_and_both_reductions(dev, p, reduction):
    c = Call(dev, "R350 K5 bf16 perm", p=p, reduction=reduction)
    check(c, c.fwd(), c.bwd(), ("R350 K5 bf16 perm", p, reduction))


@pytest.mark.parametrize("a", [(80.0, -80.0, 0.0), (1e4, 1e4, 1e4)])
def test_extreme_logits_stay_finite_and_within_bounds(dev, a):
    c = Call(dev, "K3 tiny perm", a=np.asarray(a, dtype=np.float32))
    out, grads = c.fwd(), c.bwd()
    check(c, out, grads, ("K3 tiny perm", a))
    if a[0] == a[1]:
        assert out["w"].tolist() == [np.float32(1.0) / np.float32(3.0)] * 3


def test_optional_outputs_may_be_null_and_change_nothing(dev):
    full, bare = Call(dev, "K13 H72 V31 bf16 perm"), Call(dev, "K13 H72 V31 bf16 perm")
    a, ga = full.fwd(), full.bwd()
    lib = _L().lib()
    assert lib.tmi_layer_mix_fwd(*bare.fwd_args(w_out=None)) == 0 and lib.tmi_layer_mix_bwd(*bare.bwd_args(d=None)) == 0
    torch.cuda.synchronize()
    assert bare.w.same_where() and bare.dk.same_where()
    assert torch.equal(bits(bare.mixed.t), bits(full.mixed.t)) and torch.equal(bits(bare.g_a.t), bits(full.g_a.t))


def test_one_stacked_tensor_gives_the_bits_of_separate_layers(dev):
    """The host pointer table serves both callers: slices of one stacked [K, n_src, T, H] tensor, through ops."""
    from tethys_speech_amd import ops
    name = "K13 H72 V31 bf16 perm"
    c = Call(dev, name)
    d = c.d
    out, grads = c.fwd(), c.bwd()
    to = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a)).to(dev) if dt is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
    stacked = to(d["layers"], c.dt)
    N, T, H, V, K = d["N"], d["T"], d["H"], d["V"], d["K"]
    mixed, w, g_a, dk = torch.zeros((N, T, H), device=dev), torch.zeros(K, device=dev), torch.zeros(K, device=dev), torch.zeros(K, device=dev)
    fl, idx, a = to(d["frame_lens"]), to(d["row_index"]), to(d["a"])
    ops.layer_mix_fwd(stacked, a, fl, mixed, row_index=idx, w_out=w)
    ws = torch.empty(ops.layer_mix_workspace_elems(N, T, H, V, K), device=dev)
    ops.layer_mix_bwd(stacked, a, fl, to(d["label_lens"]), to(d["grad"]), to(d["infeasible"]), to(d["W"]), g_a, ws, M.L_MAX,
                      row_index=idx, p=d["p"], seed=d["seed"], reduction=d["reduction"], d=dk)
    torch.cuda.synchronize()
    live = c.f["live"]
    assert np.array_equal(mixed.cpu().numpy()[live].view(np.int32), out["mixed"][live].view(np.int32)) and not mixed.cpu().numpy()[~live].any()
    assert np.array_equal(w.cpu().numpy().view(np.int32), out["w"].view(np.int32))
    assert np.array_equal(g_a.cpu().numpy().view(np.int32), grads["g_a"].view(np.int32))
    assert np.array_equal(dk.cpu().numpy().view(np.int32), grads["d"].view(np.int32))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_one_layer_is_the_identity_exactly(dev, dtype):
    """K 1: w == 1, mixed is bit for bit (float) x gathered, g_a is exactly 0 (d is not)."""
    name = "K13 H72 V31 f32" if dtype == "fp32" else "K13 H72 V31 bf16 perm"
    c = Call(dev, name)
    d = c.d
    one = torch.tensor([0.37], dtype=F32, device=dev)
    out = c.fwd(K=1, a=one.data_ptr())
    grads = c.bwd(K=1, a=one.data_ptr())
    live = c.f["live"]
    x0 = R.gather(d["layers"][0], d["row_index"], d["N"]).astype(np.float32)
    assert out["w"][0] == 1.0 and np.array_equal(out["mixed"][live].view(np.int32), x0[live].view(np.int32))
    assert grads["g_a"][0] == 0.0 and grads["d"][0] != 0.0
    assert c.w.same_where(torch.arange(d["K"]) >= 1) and c.g_a.same_where(torch.arange(d["K"]) >= 1)


def test_no_live_row_gives_zeros(dev):
    c = Call(dev, "K13 H72 V31 bf16 perm")
    zero = torch.zeros(c.d["N"], dtype=I32, device=dev)
    lib = _L().lib()
    assert lib.tmi_layer_mix_fwd(*c.fwd_args(frame_lens=zero.data_ptr())) == 0
    assert lib.tmi_layer_mix_bwd(*c.bwd_args(frame_lens=zero.data_ptr())) == 0
    torch.cuda.synchronize()
    assert c.mixed.same_where() and not c.g_a.now().any() and not c.dk.now().any()
    assert abs(float(c.w.now().sum()) - 1.0) < 1e-6


def test_refused_calls_write_nothing_and_name_the_limit(dev):
    c = Call(dev, "K13 H72 V31 bf16 perm")
    lib = _L().lib()
    d = c.d
    big = 1 << 30
    K = d["K"]
    holed = (ctypes.c_void_p * K)(*[None if k == 5 else g.v.data_ptr() for k, g in enumerate(c.X)])
    odd = (ctypes.c_void_p * K)(*[g.v.data_ptr() + (2 if k == 7 else 0) for k, g in enumerate(c.X)])
    common = [dict(K=0), dict(K=65), dict(N=0), dict(N=65536), dict(T_max=0), dict(T_max=4097), dict(N=1025, T_max=4096), dict(H=12),
              dict(H=0), dict(H=4104), dict(x_dtype=2), dict(x_st=d["H"] - 1), dict(x_st=big + 8), dict(x_sn=d["T"] * c.x_st - 1),
              dict(n_src=0), dict(row_index=None, n_src=d["N"] - 1), dict(layers=None), dict(layers=holed), dict(layers=odd),
              dict(frame_lens=None), dict(a=None)]
    for over in common + [dict(mixed=None), dict(mixed=c.mixed.v.data_ptr() + 4), dict(m_st=d["H"] - 1), dict(m_sn=d["T"] * c.m_st - 1)]:
        assert lib.tmi_layer_mix_fwd(*c.fwd_args(**over)) == TMI_ERR_INVALID, over
        msg = lib.tmi_last_error().decode()
        assert msg.startswith("tmi_layer_mix_fwd:") and "1 <= K <= 64" in msg and "N*T_max <= 2^22" in msg, msg
    for over in common + [dict(V=1), dict(V=65), dict(p=1.0), dict(p=-0.1), dict(reduction=2), dict(L_max=0), dict(L_max=512),
                          dict(gr_st=d["V"] - 1), dict(gr_sn=d["T"] * c.gr_st - 1), dict(workspace_bytes=c.ws.n * 4 - 4),
                          dict(workspace=None), dict(workspace=c.ws.v.data_ptr() + 4), dict(grad=None), dict(infeasible=None),
                          dict(label_lens=None), dict(W=None), dict(W=c.W.v.data_ptr() + 4), dict(g_a=None)]:
        assert lib.tmi_layer_mix_bwd(*c.bwd_args(**over)) == TMI_ERR_INVALID, over
        msg = lib.tmi_last_error().decode()
        assert msg.startswith("tmi_layer_mix_bwd:") and "tmi_layer_mix_workspace_bytes" in msg, msg
    torch.cuda.synchronize()
    c.untouched()


def test_device_values_are_not_trusted(dev):
    """Frame lengths far outside [0, T_max], label lengths outside [0, L_max] and a negative row index: clamped or read as
    zeros, nothing outside the buffers is touched (the guards), and the result is that of the clamped values."""
    c = Call(dev, "R350 K5 bf16 perm")
    d = c.d
    base_out, base_g = c.fwd(), c.bwd()
    fl = d["frame_lens"].copy()
    fl[fl >= d["T"]] = 2 ** 31 - 1
    fl[fl == 0] = -(2 ** 31)
    ll = d["label_lens"].copy()
    ll[ll == 0] = -5
    ll[ll == M.L_MAX] = 10 ** 6
    idx = d["row_index"].copy()
    idx[idx >= d["n_src"]] = -(2 ** 31)
    c.fl.v.copy_(torch.from_numpy(fl).to(dev))
    c.ll.v.copy_(torch.from_numpy(ll).to(dev))
    c.idx.v.copy_(torch.from_numpy(idx).to(dev))
    for t in (c.fl, c.ll, c.idx):
        t.host0 = t.t.cpu().clone()
    out, g = c.fwd(), c.bwd()
    assert torch.equal(out["bits"], base_out["bits"]) and torch.equal(g["bits"], base_g["bits"])
