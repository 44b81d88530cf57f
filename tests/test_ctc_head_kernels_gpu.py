"""tmi_ctc_head_fwd / tmi_ctc_head_bwd (csrc/ctc_head.hip) through the C ABI, against the float64 reference and the derived
bounds of tests/_ctc_head_ref.py (checked by tests/test_ctc_head_cpu.py), on its seeded cases: H 8 / 64 / 768, V 2 / 31 /
32 / 33 / 64, N * T_max one below, at and one above the row chunk of 256 and at ten chunks, bf16 and fp32 features with
x_st = H, H + 8 (16-byte loads) and H + 1 / H + 3 (element loads), a permuted row_index with one entry out of range, p 0 /
0.1 / 0.9, both reductions, ragged frame_lens with an item at 0, one at T_max and one beyond it, an infeasible item and an
item without labels.

Every input and output lies inside a larger buffer of 7.0 / NaN guards (integers: 7 / a large negative) with padded
strides, compared bit for bit after the calls wherever the contract says nothing is written: the guard zones, the stride
padding, the frames past a clip, every input, and everything when a call is refused.  Measured / bound goes through
``_margins.within`` under the names "ctc head ..." with the bound 1; no bound is fitted to what the kernels give.  The
backward's grad / nll / infeasible are seeded fp32 numbers, nonzero past the clips and on the infeasible item, where the
call must not read them."""
import numpy as np
import pytest
import torch

import _ctc_head_ref as R
import _ctc_ref as C
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
    """a [n, T, c] into the flat payload h under the strides (sn, st)."""
    a = torch.as_tensor(np.ascontiguousarray(a))
    n, T, c = a.shape
    torch.as_strided(h, (n, T, c), (sn, st, 1)).copy_(a.to(h.dtype))


def out_of(g, n, T, sn, st, cols):
    return torch.as_strided(g.now(), (n, T, cols), (sn, st, 1)).float().numpy().copy()


def unwritten(live, sn, st, cols):
    """bool [N * sn]: True where a [N, T, cols] output under (sn, st) must hold its guard (dead rows, padding)."""
    N, T = live.shape
    k = torch.ones(N * sn, dtype=torch.bool)
    torch.as_strided(k, (N, T, cols), (sn, st, 1)).copy_((~torch.from_numpy(live))[:, :, None].expand(N, T, cols))
    return k


class Call:
    def __init__(self, dev, name, optional=True):
        d, x, keep, _, scale, f, g = R.case_ref(name)
        self.dev, self.d, self.f, self.g, self.name = dev, d, f, g, name
        N, T, H, V = d["N"], d["T"], d["H"], d["V"]
        self.dt = BF16 if d["dtype"] == "bf16" else F32
        self.x_st = d["x_st"]
        self.x_sn = T * self.x_st + (16 if d["x_st"] % 8 == 0 else 5)
        self.lp_st, self.lg_st, self.gr_st = V + 3, V + 1, V + 2
        self.lp_sn, self.lg_sn, self.gr_sn = T * self.lp_st + 7, T * self.lg_st + 2, T * self.gr_st + 5
        n_src = d["n_src"]
        self.X = G(dev, self.dt, n_src * self.x_sn, lambda h: into(h, d["hidden"], self.x_sn, self.x_st))
        self.W, self.b = G(dev, F32, H * V, lambda h: h.copy_(torch.from_numpy(d["W"]).reshape(-1))), G(dev, F32, V, lambda h: h.copy_(torch.from_numpy(d["b"])))
        self.idx = None if d["row_index"] is None else G(dev, I32, N, lambda h: h.copy_(torch.from_numpy(d["row_index"])))
        self.fl = G(dev, I32, N, lambda h: h.copy_(torch.from_numpy(d["frame_lens"])))
        self.ll = G(dev, I32, N, lambda h: h.copy_(torch.from_numpy(d["label_lens"])))
        self.grad = G(dev, F32, N * self.gr_sn, lambda h: into(h, d["grad"], self.gr_sn, self.gr_st))
        self.nll = G(dev, F32, N, lambda h: h.copy_(torch.from_numpy(d["nll"])))
        self.bad = G(dev, I32, N, lambda h: h.copy_(torch.from_numpy(d["infeasible"])))
        self.logp = G(dev, F32, N * self.lp_sn)
        self.logits = G(dev, F32, N * self.lg_sn) if optional else None
        self.amax = G(dev, I32, N * T) if optional else None
        self.inputs = [t for t in (self.X, self.W, self.b, self.idx, self.fl, self.ll, self.grad, self.nll, self.bad) if t is not None]
        lib = _L().lib()
        nb = lib.tmi_ctc_head_workspace_bytes(N, T, H, V)
        assert nb == -(-N * T // R.chunk_rows(N * T)) * (H * V + V) * 4
        self.gW, self.gb, self.loss, self.nbad, self.ws = G(dev, F32, H * V), G(dev, F32, V), G(dev, F32, 1), G(dev, I32, 1), G(dev, F32, nb // 4)

    @staticmethod
    def _p(g):
        return None if g is None else g.v.data_ptr()

    def fwd_args(self, **over):
        d = self.d
        a = dict(hidden=self.X.v.data_ptr(), x_dtype=1 if self.dt == BF16 else 0, x_sn=self.x_sn, x_st=self.x_st, n_src=d["n_src"],
                 row_index=self._p(self.idx), frame_lens=self.fl.v.data_ptr(), W=self.W.v.data_ptr(), b=self.b.v.data_ptr(), p=d["p"],
                 seed=d["seed"], logits=self._p(self.logits), lg_sn=self.lg_sn, lg_st=self.lg_st, logp=self.logp.v.data_ptr(),
                 lp_sn=self.lp_sn, lp_st=self.lp_st, argmax=self._p(self.amax), N=d["N"], T_max=d["T"], H=d["H"], V=d["V"], stream=stream())
        a.update(over)
        return list(a.values())

    def bwd_args(self, **over):
        d = self.d
        a = dict(hidden=self.X.v.data_ptr(), x_dtype=1 if self.dt == BF16 else 0, x_sn=self.x_sn, x_st=self.x_st, n_src=d["n_src"],
                 row_index=self._p(self.idx), frame_lens=self.fl.v.data_ptr(), label_lens=self.ll.v.data_ptr(), grad=self.grad.v.data_ptr(),
                 gr_sn=self.gr_sn, gr_st=self.gr_st, nll=self.nll.v.data_ptr(), infeasible=self.bad.v.data_ptr(), p=d["p"], seed=d["seed"],
                 reduction=1 if d["reduction"] == "mean" else 0, gW=self.gW.v.data_ptr(), gb=self.gb.v.data_ptr(),
                 loss=self.loss.v.data_ptr(), n_infeasible=self.nbad.v.data_ptr(), workspace=self.ws.v.data_ptr(),
                 workspace_bytes=self.ws.n * 4, N=d["N"], T_max=d["T"], L_max=R.L_MAX, H=d["H"], V=d["V"], stream=stream())
        a.update(over)
        return list(a.values())

    def untouched(self, outputs=True):
        for t in self.inputs:
            assert t.same_where(), "an input was written"
        if outputs:
            for t in (self.logp, self.logits, self.amax, self.gW, self.gb, self.loss, self.nbad, self.ws):
                assert t is None or t.same_where(), "a refused call wrote"

    def fwd(self):
        lib = _L().lib()
        rc = lib.tmi_ctc_head_fwd(*self.fwd_args())
        assert rc == 0, lib.tmi_last_error()
        torch.cuda.synchronize()
        d, live = self.d, self.f["live"]
        N, T, V = d["N"], d["T"], d["V"]
        self.untouched(outputs=False)
        assert self.logp.same_where(unwritten(live, self.lp_sn, self.lp_st, V)), "logp: a frame past a clip or the padding was written"
        out = {"logp": out_of(self.logp, N, T, self.lp_sn, self.lp_st, V), "logp_bits": bits(self.logp.t).clone()}
        if self.logits is not None:
            assert self.logits.same_where(unwritten(live, self.lg_sn, self.lg_st, V)) and self.amax.same_where(~torch.from_numpy(live).reshape(-1))
            out.update(logits=out_of(self.logits, N, T, self.lg_sn, self.lg_st, V), argmax=self.amax.now().view(N, T).numpy().copy(),
                       logits_bits=bits(self.logits.t).clone(), argmax_bits=bits(self.amax.t).clone())
        return out

    def bwd(self):
        lib = _L().lib()
        rc = lib.tmi_ctc_head_bwd(*self.bwd_args())
        assert rc == 0, lib.tmi_last_error()
        torch.cuda.synchronize()
        self.untouched(outputs=False)
        for t in (self.gW, self.gb, self.loss, self.nbad, self.ws):   # (the whole workspace is the call's; its guards are not)
            assert t.same_where(torch.zeros(t.n, dtype=torch.bool))
        d = self.d
        return {"gW": self.gW.now().view(d["H"], d["V"]).numpy().copy(), "gb": self.gb.now().numpy().copy(),
                "loss": float(self.loss.now()[0]), "n_infeasible": int(self.nbad.now()[0]),
                "bits": torch.cat([bits(self.gW.t), bits(self.gb.t), bits(self.loss.t), bits(self.nbad.t)]).clone()}


@pytest.mark.parametrize("name", list(R.CASES))
def test_forward_and_backward_against_float64(dev, name):
    c = Call(dev, name)
    d, f, g = c.d, c.f, c.g
    live = f["live"]
    out = c.fwd()
    for key in ("logits", "logp"):
        q = C.ratio(out[key][live], f[key][live], f["b_" + key][live])
        print(f"ctc head {name} {key}: {q:.4f} of its bound")
        within(f"ctc head {key} / bound", q, 1.0, name)
    dec = R.decided(f)
    assert int((live & ~dec).sum()) <= 0.01 * int(live.sum())
    assert np.array_equal(out["argmax"][dec], f["argmax"][dec])
    lg = out["logits"]
    first_max = np.argmax(lg, axis=2)   # (numpy's argmax is the first maximum: the rule on the device's own logits, every live row)
    assert np.array_equal(out["argmax"][live], first_max[live])
    # logp is logits - lse of the device's own logits: rows sum to one
    assert np.abs(np.exp(out["logp"][live].astype(np.float64)).sum(axis=1) - 1.0).max() < 1e-5
    grads = c.bwd()
    for key in ("gW", "gb", "loss"):
        q = C.ratio(grads[key], g[key], g["b_" + key])
        print(f"ctc head {name} {key}: {q:.4f} of its bound")
        within(f"ctc head {key} / bound", q, 1.0, name)
    assert grads["n_infeasible"] == g["n_infeasible"] == 1
    # the same bits from a second pair of calls, into a workspace that now holds the first call's partial sums
    out2, grads2 = c.fwd(), c.bwd()
    assert torch.equal(out["logp_bits"], out2["logp_bits"]) and torch.equal(out["logits_bits"], out2["logits_bits"])
    assert torch.equal(out["argmax_bits"], out2["argmax_bits"]) and torch.equal(grads["bits"], grads2["bits"])


@pytest.mark.parametrize("name", ["R256 H64 V31 bf16 perm", "R257 H64 V33 f32"])
def test_optional_outputs_may_be_null_and_change_nothing(dev, name):
    full, bare = Call(dev, name), Call(dev, name, optional=False)
    a, b = full.fwd(), bare.fwd()
    assert torch.equal(a["logp_bits"], b["logp_bits"])


def test_an_item_alone_gets_the_bits_it_gets_in_the_ragged_batch(dev):
    """p = 0: nothing of a row depends on its position.  Item 2 of the fp32 case, run as a batch of one through row_index."""
    name = "R255 H8 V2 f32"
    c = Call(dev, name)
    d = c.d
    out = c.fwd()
    lib = _L().lib()
    n, T, V = 2, d["T"], d["V"]
    idx, fl = torch.tensor([n], dtype=I32, device=dev), torch.tensor([int(d["frame_lens"][n])], dtype=I32, device=dev)
    lp = torch.full((1, T, V), 7.0, dtype=F32, device=dev)
    rc = lib.tmi_ctc_head_fwd(*c.fwd_args(row_index=idx.data_ptr(), frame_lens=fl.data_ptr(), logits=None, argmax=None,
                                           logp=lp.data_ptr(), lp_sn=T * V, lp_st=V, N=1))
    assert rc == 0, lib.tmi_last_error()
    torch.cuda.synchronize()
    Tn = int(np.clip(d["frame_lens"][n], 0, T))
    assert Tn > 1 and np.array_equal(lp.cpu().numpy()[0, :Tn].view(np.int32), out["logp"][n, :Tn].view(np.int32))
    assert bool((lp[0, Tn:] == 7.0).all())


def test_no_frames_at_all_gives_zero_gradients(dev):
    c = Call(dev, "H8 V32 bf16")
    zero = torch.zeros(c.d["N"], dtype=I32, device=dev)
    lib = _L().lib()
    assert lib.tmi_ctc_head_fwd(*c.fwd_args(frame_lens=zero.data_ptr())) == 0
    assert lib.tmi_ctc_head_bwd(*c.bwd_args(frame_lens=zero.data_ptr())) == 0
    torch.cuda.synchronize()
    assert c.logp.same_where() and c.logits.same_where() and c.amax.same_where()
    assert not c.gW.now().any() and not c.gb.now().any() and int(c.nbad.now()[0]) == 1


def test_refused_calls_write_nothing_and_name_the_limit(dev):
    c = Call(dev, "H8 V32 bf16")
    lib = _L().lib()
    d = c.d
    big = 1 << 30
    fwd_bad = [dict(N=0), dict(N=65536), dict(T_max=0), dict(T_max=4097), dict(N=1025, T_max=4096), dict(H=12), dict(H=0), dict(H=4104),
               dict(V=1), dict(V=65), dict(p=1.0), dict(p=-0.1), dict(x_dtype=2), dict(x_st=d["H"] - 1), dict(x_st=big + 8), dict(x_sn=d["T"] * c.x_st - 1),
               dict(lp_st=d["V"] - 1), dict(lp_sn=d["T"] * c.lp_st - 1), dict(lg_st=d["V"] - 1), dict(n_src=0), dict(n_src=d["N"] - 1),
               dict(hidden=None), dict(hidden=c.X.v.data_ptr() + 2), dict(W=None), dict(W=c.W.v.data_ptr() + 4), dict(b=None), dict(logp=None),
               dict(frame_lens=None), dict(logp=c.logp.v.data_ptr() + 2)]
    for over in fwd_bad:
        assert lib.tmi_ctc_head_fwd(*c.fwd_args(**over)) == TMI_ERR_INVALID, over
        msg = lib.tmi_last_error().decode()
        assert msg.startswith("tmi_ctc_head_fwd:") and "N*T_max <= 2^22" in msg and "multiple of 8" in msg, msg
    bwd_bad = [dict(N=0), dict(T_max=4097), dict(H=12), dict(V=65), dict(p=1.0), dict(reduction=2), dict(L_max=0), dict(L_max=512),
               dict(gr_st=d["V"] - 1), dict(gr_sn=d["T"] * c.gr_st - 1), dict(workspace_bytes=c.ws.n * 4 - 4), dict(workspace=None),
               dict(workspace=c.ws.v.data_ptr() + 4), dict(grad=None), dict(nll=None), dict(infeasible=None), dict(label_lens=None), dict(gW=None),
               dict(gb=None), dict(loss=None), dict(n_infeasible=None), dict(hidden=None), dict(frame_lens=None)]
    for over in bwd_bad:
        assert lib.tmi_ctc_head_bwd(*c.bwd_args(**over)) == TMI_ERR_INVALID, over
        msg = lib.tmi_last_error().decode()
        assert msg.startswith("tmi_ctc_head_bwd:") and "tmi_ctc_head_workspace_bytes" in msg, msg
    torch.cuda.synchronize()
    c.untouched()


def test_device_values_are_not_trusted(dev):
    """Frame lengths far outside [0, T_max], label lengths outside [0, L_max] and a negative row index: clamped or read as
    zeros, nothing outside the buffers is touched (the guards), and the result is that of the clamped values."""
    name = "R256 H64 V31 bf16 perm"
    c = Call(dev, name)
    d = c.d
    base_out, base_g = c.fwd(), c.bwd()
    fl = d["frame_lens"].copy()
    fl[fl >= d["T"]] = 2 ** 31 - 1
    fl[fl == 0] = -(2 ** 31)
    ll = d["label_lens"].copy()
    ll[ll == 0] = -5
    ll[ll == R.L_MAX] = 10 ** 6
    idx = d["row_index"].copy()
    idx[idx >= d["n_src"]] = -(2 ** 31)
    c.fl.v.copy_(torch.from_numpy(fl).to(dev))
    c.ll.v.copy_(torch.from_numpy(ll).to(dev))
    c.idx.v.copy_(torch.from_numpy(idx).to(dev))
    for t in (c.fl, c.ll, c.idx):
        t.host0 = t.t.cpu().clone()
    out, g = c.fwd(), c.bwd()
    assert torch.equal(out["logp_bits"], base_out["logp_bits"]) and torch.equal(g["bits"], base_g["bits"])
