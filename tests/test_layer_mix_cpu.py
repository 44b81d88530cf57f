"""The float64 reference of the layer-mix kernels (tests/_layer_mix_ref.py) checked without a GPU: against torch's float64
autograd and central differences, its bounds against an fp32 transcription and every listed mutation, the binding against
the header, the host refusals of the C ABI, the host validator, ``LayerMix`` and the planted problem's budget."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _ctc_head_ref as R
import _ctc_ref as C
import _layer_mix_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _W():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import wav2vec2 as W
    return W


def _small(p=0.3, seed=3):
    """K 4, N 4, T 12, H 8, V 5: item 1 infeasible (2 frames, 4 labels), item 2 without labels, ragged lengths."""
    g = np.random.default_rng(seed)
    K, N, T, H, V, L = 4, 4, 12, 8, 5, 4
    x = g.standard_normal((K, N, T, H)).astype(np.float32)
    a = (g.standard_normal(K) * 0.8).astype(np.float32)
    W = (g.standard_normal((H, V)) * 0.7).astype(np.float32)
    b = (g.standard_normal(V) * 0.3).astype(np.float32)
    frame_lens = np.array([12, 2, 9, 7], dtype=np.int32)
    label_lens = np.array([3, 4, 0, 2], dtype=np.int32)
    labels = g.integers(1, V, (N, L)).astype(np.int32)
    keep, _, scale = R.keep_masks(99, N, None, N, T, H, p)
    return dict(x=x, a=a, W=W, b=b, frame_lens=frame_lens, label_lens=label_lens, labels=labels, keep=None if p == 0.0 else keep,
                scale=scale, L=L)


def _torch_grads(d, reduction):
    x = torch.from_numpy(d["x"].astype(np.float64))
    a = torch.tensor(d["a"].astype(np.float64), requires_grad=True)
    w = torch.softmax(a, 0)
    w.retain_grad()
    mixed = (w[:, None, None, None] * x).sum(0)
    if d["keep"] is not None:
        mixed = torch.where(torch.from_numpy(d["keep"]), mixed * d["scale"], torch.zeros_like(mixed))
    Wt, b = torch.from_numpy(d["W"].astype(np.float64)), torch.from_numpy(d["b"].astype(np.float64))
    lp = torch.log_softmax(torch.nn.functional.linear(mixed, Wt.T, b), dim=2).transpose(0, 1)
    loss = torch.nn.functional.ctc_loss(lp, torch.from_numpy(d["labels"].astype(np.int64)), torch.from_numpy(d["frame_lens"].astype(np.int64)),
                                        torch.from_numpy(d["label_lens"].astype(np.int64)), blank=0, reduction=reduction,
                                        zero_infinity=True)
    loss.backward()
    return float(loss.detach()), w.grad.numpy(), a.grad.numpy()


@pytest.mark.parametrize("reduction", ["sum", "mean"])
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_reference_against_torch_float64_autograd(reduction, p):
    d = _small(p)
    mf, _, (grad, nll, bad), g, mb = M.step(d["x"], d["a"], d["W"], d["b"], d["frame_lens"], d["labels"], d["label_lens"], reduction,
                                            d["L"], d["keep"], d["scale"])
    assert bad.tolist() == [0, 1, 0, 0] and abs(mf["w"].sum() - 1.0) <= 1e-15
    loss, dw, ga = _torch_grads(d, reduction)
    assert abs(g["loss"] - loss) <= 1e-12 * max(1.0, abs(loss))
    assert np.abs(mb["d"] - dw).max() <= 1e-12 and np.abs(mb["g_a"] - ga).max() <= 1e-12
    assert np.abs(ga).max() > 1e-4 and abs(mb["g_a"].sum()) <= 1e-13


@pytest.mark.parametrize("reduction", ["sum", "mean"])
def test_reference_against_central_differences(reduction):
    d = _small(0.3, seed=8)
    args = (d["W"], d["b"], d["frame_lens"], d["labels"], d["label_lens"], reduction, d["L"], d["keep"], d["scale"])
    g_a = M.step(d["x"], d["a"], *args)[4]["g_a"]
    eps, base = 1e-6, R.f64(d["a"])
    for k in range(len(base)):
        hi, lo = base.copy(), base.copy()
        hi[k] += eps
        lo[k] -= eps
        num = (M.loss_of(d["x"], hi, *args) - M.loss_of(d["x"], lo, *args)) / (2 * eps)
        assert abs(num - g_a[k]) <= 1e-8, (k, num, g_a[k])


def test_no_live_row_gives_zeros_and_one_layer_gives_no_gradient():
    d = _small(0.0)
    mb = M.step(d["x"], d["a"], d["W"], d["b"], np.zeros(4, dtype=np.int32), d["labels"], d["label_lens"], "mean", d["L"])[4]
    assert not mb["d"].any() and not mb["g_a"].any()
    mf, _, _, _, mb = M.step(d["x"][:1], d["a"][:1], d["W"], d["b"], d["frame_lens"], d["labels"], d["label_lens"], "mean", d["L"])
    assert mf["w"].tolist() == [1.0] and mb["g_a"].tolist() == [0.0] and mb["d"][0] != 0.0
    live = mf["live"]
    assert np.array_equal(mf["mixed"][live], R.f64(d["x"][0])[live])


@pytest.mark.parametrize("name", [n for n in M.CASES if not n.startswith(("R16500", "R819", "K25"))])
def test_bounds_hold_an_fp32_transcription(name):
    d, x, keep, _, scale, f, b = M.case_ref(name)
    w, mixed = M.forward_f32(x, d["a"], d["frame_lens"])
    live = f["live"]
    assert C.ratio(w, f["w"], f["b_w"]) <= 1.0
    q = C.ratio(mixed[live], f["mixed"][live], f["b_mixed"][live])
    assert q <= 1.0 and (q > 0.0 or name in M.SPECIAL_A), (name, "mixed", q)   # (w = (1, 0, ~0): the sum is x_0 itself)
    dd, ga = M.backward_f32(x, d["a"], d["grad"], d["infeasible"], d["label_lens"], d["frame_lens"], d["reduction"], M.L_MAX, d["W"],
                            keep, scale)
    for got, key in ((dd, "d"), (ga, "g_a")):
        q = C.ratio(got, b[key], b["b_" + ("d" if key == "d" else "g")])
        assert 0.0 < q <= 1.0, (name, key, q)


@pytest.mark.parametrize("mutation", M.MUTATIONS)
def test_every_mutation_exceeds_the_bounds_on_its_cases(mutation):
    cases, keys = M.MUTATION_CASES[mutation]
    assert cases and set(M.MUTATION_CASES) == set(M.MUTATIONS)
    for name in cases:
        d, x, keep, _, scale, f, b = M.case_ref(name)
        m = M.mutated(name, mutation)
        for key in keys:
            if key == "mixed":
                q = C.ratio(m[key][f["live"]], f[key][f["live"]], f["b_mixed"][f["live"]])
            elif key == "w":
                q = C.ratio(m[key], f["w"], f["b_w"])
            else:
                q = C.ratio(m[key], b[key], b["b_" + ("d" if key == "d" else "g")])
            assert q > 1.0, (mutation, name, key, q)


def test_case_sizes_cover_the_partition():
    rows = {n: c[1] * c[2] for n, c in M.CASES.items()}
    assert {350, 16500, 8192, 8193, 513} <= set(rows.values())
    assert M.tile_rows(8192) == 8 and M.tiles(8192) == 1024 and M.tile_rows(8193) == 16 and M.tiles(8193) == 513
    assert M.tile_rows(16500) == 24 and M.tiles(16500) == 688 and M.tiles(513) == 65 and M.tiles(1992) == 249
    assert M.tile_rows(1 << 22) * M.MAX_TILES >= 1 << 22 and M.tiles(1 << 22) <= M.MAX_TILES
    assert any(c[3] % 256 and c[3] > 256 for c in M.CASES.values())            # an H-slice tail
    assert any(c[4] > 32 for c in M.CASES.values()) and any(c[4] % 2 for c in M.CASES.values())   # the 128-column slices, an odd V
    assert {c[0] for c in M.CASES.values()} >= {2, 3, 13, 25, 64}


def test_binding_header_and_host_refusals():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib
    header = open(os.path.join(ROOT, "include", "tethys_mi.h")).read()
    want = {"tmi_layer_mix_workspace_bytes": 5, "tmi_layer_mix_fwd": 17, "tmi_layer_mix_bwd": 28}
    for name, nargs in want.items():
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\);", header)
        assert m is not None, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == nargs, name
    assert _lib.ABI_VERSION == 31
    assert "tr = 8 * ceil(N*T_max / 8192)" in header and "g_a[k]    = w_k * (d_k - dot)" in header
    src = open(os.path.join(ROOT, "tethys-speech_amd", "csrc", "layer_mix.hip")).read()
    assert "atomic" not in src.replace("no atomic", "")
    assert "layer_mix.hip" in open(os.path.join(ROOT, "tethys-speech_amd", "csrc", "Makefile")).read()
    lib = _lib.lib()
    assert lib.tmi_abi_version() == 31
    wb = lib.tmi_layer_mix_workspace_bytes
    assert wb(8, 249, 768, 32, 13) == 249 * 13 * 4 and wb(2, 4096, 8, 2, 2) == 1024 * 2 * 4 and wb(3, 2731, 8, 2, 2) == 513 * 2 * 4
    assert wb(1024, 4096, 8, 2, 64) == 1024 * 64 * 4 and wb(1, 1, 8, 2, 1) == 4
    for bad in ((0, 1, 8, 2, 1), (65536, 1, 8, 2, 1), (1, 0, 8, 2, 1), (1, 4097, 8, 2, 1), (1025, 4096, 8, 2, 1), (1, 1, 0, 2, 1),
                (1, 1, 12, 2, 1), (1, 1, 4104, 2, 1), (1, 1, 8, 1, 1), (1, 1, 8, 65, 1), (1, 1, 8, 2, 0), (1, 1, 8, 2, 65)):
        assert wb(*bad) == -1, bad
    # a NULL or misaligned pointer is refused on the host before anything is launched (so this runs without a GPU)
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    p = p + (-p) % 16
    tab = lambda *ptrs: (ctypes.c_void_p * len(ptrs))(*ptrs)
    fwd = lambda layers, frame_lens, a, mixed, K=2: lib.tmi_layer_mix_fwd(layers, K, 0, 16, 8, 1, None, frame_lens, a, None, mixed, 16, 8,
                                                                         1, 2, 8, None)
    good = tab(p, p)
    for args in ((None, p, p, p), (tab(p, None), p, p, p), (tab(p, p + 4), p, p, p), (good, None, p, p), (good, p, None, p),
                 (good, p, p, None), (good, p, p, p + 4), (good, p, p, p, 0), (good, p, p, p, 65)):
        assert fwd(*args) == -1
        assert lib.tmi_last_error().decode().startswith("tmi_layer_mix_fwd:") and "1 <= K <= 64" in lib.tmi_last_error().decode()
    bwd = lambda layers, grad, Wp, a, g_a, ws, wsb=1 << 12, p_=0.0, red=1: lib.tmi_layer_mix_bwd(
        layers, 2, 0, 16, 8, 1, None, p, p, grad, 16, 8, p, p_, 0, red, Wp, a, g_a, None, ws, wsb, 1, 2, 3, 8, 2, None)
    for args in ((None, p, p, p, p, p), (tab(None, p), p, p, p, p, p), (good, None, p, p, p, p), (good, p, None, p, p, p),
                 (good, p, p + 4, p, p, p), (good, p, p, None, p, p), (good, p, p, p, None, p), (good, p, p, p, p, None),
                 (good, p, p, p, p, p, 4), (good, p, p, p, p, p, 1 << 12, 1.0), (good, p, p, p, p, p, 1 << 12, 0.0, 2)):
        assert bwd(*args) == -1
        assert lib.tmi_last_error().decode().startswith("tmi_layer_mix_bwd:") and "tmi_layer_mix_workspace_bytes" in lib.tmi_last_error().decode()


def test_check_layer_mix_args():
    W = _W()
    cfg = W.make_config("tiny", vocab_size=8)
    H = cfg.hidden_size
    mix = W.LayerMix(5, "cpu")
    assert W.check_layer_mix_args(cfg, (5, 3, 12, H), torch.bfloat16, mix) == (5, 3, 12)
    assert W.check_layer_mix_args(cfg, (5, 1, 4096, H), torch.float32, mix) == (5, 1, 4096)
    with pytest.raises(TypeError):
        W.check_layer_mix_args(cfg, (5, 3, 12, H), torch.bfloat16, None)
    for shape, dtype in (((3, 12, H), torch.float32), ((4, 3, 12, H), torch.float32), ((5, 3, 12, H - 8), torch.float32),
                         ((5, 0, 12, H), torch.float32), ((5, 3, 4097, H), torch.float32), ((5, 3, 12, H), torch.float16)):
        with pytest.raises(ValueError):
            W.check_layer_mix_args(cfg, shape, dtype, mix)
    for K in (0, 65):
        with pytest.raises(ValueError):
            W.LayerMix(K, "cpu")


def test_layer_mix_state_round_trip_and_the_arena():
    W = _W()
    cfg = W.make_config("tiny", vocab_size=8)
    before = W.W2VArena(cfg, "cpu", head="ctc")
    mix = W.LayerMix(cfg.num_hidden_layers + 1, "cpu")
    K = mix.num_layers
    assert K == 5 and mix.logits.dtype == torch.float32 and not mix.logits.any() and mix._p.numel() % 4 == 0 and mix._p.numel() >= K
    assert torch.equal(mix.weights(), torch.full((K,), 1.0 / K)) and all(getattr(mix, n).shape == (K,) for n in ("logits", "grad", "m", "v"))
    mix.logits.copy_(torch.arange(K, dtype=torch.float32))
    mix.m.fill_(0.25)
    mix.v.fill_(0.5)
    state = mix.state_dict()
    assert set(state) == {"logits", "m", "v"} and all(t.device.type == "cpu" and t.shape == (K,) for t in state.values())
    other = W.LayerMix(K, "cpu")
    other.load_state_dict(state)
    assert all(torch.equal(getattr(other, n), getattr(mix, n)) for n in ("logits", "m", "v")) and not other._p[K:].any()
    assert torch.allclose(other.weights().double(), torch.softmax(torch.arange(K, dtype=torch.float64), 0), atol=1e-7)
    other.load_state_dict({"logits": np.ones(K, dtype=np.float32)})   # the job's file: the logits alone
    assert not other.m.any() and not other.v.any() and other.logits.tolist() == [1.0] * K
    with pytest.raises(ValueError):
        other.load_state_dict({"logits": np.ones(K + 1, dtype=np.float32)})
    # the mix lives outside the arena: the layout is what it was and lm_head is still its tail
    after = W.W2VArena(cfg, "cpu", head="ctc")
    assert after.names == before.names and after.offsets == before.offsets and after.numel == before.numel
    assert after.names[-2:] == ["lm_head.kernel", "lm_head.bias"]
    src = open(os.path.join(ROOT, "tethys-speech_amd", "wav2vec2.py")).read()
    assert src.count('raise NotImplementedError("CTC fine-tuning is not built")') == 2
    assert all(hasattr(W.Wav2Vec2ForCTC, n) for n in ("set_layer_mix", "encode_features", "head_step", "evaluate_features"))


def test_planted_problem_is_solved_by_the_reference_inside_half_the_budget():
    pr = M.planted_problem()
    run = M.planted_run(M.PLANTED_STEPS, problem=pr)
    last = M.last_failing_step(run, pr["k_star"])
    print(f"planted layer-mix problem: token errors {run[0][0]} after step 1, the last failing step is {last}, budget {M.PLANTED_STEPS}")
    assert run[0][0] > 0 and 0 < last and 2 * last == M.PLANTED_STEPS and run[-1] == (0, pr["k_star"])
