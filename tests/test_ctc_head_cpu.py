"""The reference and bounds of tests/_ctc_head_ref.py, and the host side of the CTC probe, without a GPU: the float64
gradients against torch's float64 autograd through ctc_loss and against central finite differences, the bounds against an
honest fp32 transcription and every listed mutation, the cap on the rows whose argmax the bounds cannot decide,
check_ctc_head_args' refusals, the new symbols of the binding and the header with their NULL-pointer refusals, and the
planted problem solved by the reference alone inside half the step budget."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _ctc_head_ref as R
import _ctc_ref as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _W():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import wav2vec2 as W
    return W


def _small(p=0.3, seed=3):
    """N 4, T 12, H 8, V 5: item 1 infeasible (2 frames, 4 labels), item 2 without labels, ragged lengths."""
    g = np.random.default_rng(seed)
    N, T, H, V, L = 4, 12, 8, 5, 4
    x = g.standard_normal((N, T, H)).astype(np.float32)
    W = (g.standard_normal((H, V)) * 0.7).astype(np.float32)
    b = (g.standard_normal(V) * 0.3).astype(np.float32)
    frame_lens = np.array([12, 2, 9, 7], dtype=np.int32)
    label_lens = np.array([3, 4, 0, 2], dtype=np.int32)
    labels = g.integers(1, V, (N, L)).astype(np.int32)
    keep, _, scale = R.keep_masks(99, N, None, N, T, H, p)
    return dict(x=x, W=W, b=b, frame_lens=frame_lens, label_lens=label_lens, labels=labels, keep=None if p == 0.0 else keep,
                scale=scale, L=L)


def _torch_grads(d, reduction):
    x = torch.from_numpy(d["x"].astype(np.float64))
    if d["keep"] is not None:
        x = torch.where(torch.from_numpy(d["keep"]), x * d["scale"], torch.zeros_like(x))
    W = torch.tensor(d["W"].astype(np.float64), requires_grad=True)
    b = torch.tensor(d["b"].astype(np.float64), requires_grad=True)
    lp = torch.log_softmax(x @ W + b, dim=2).transpose(0, 1)   # [T, N, V]
    loss = torch.nn.functional.ctc_loss(lp, torch.from_numpy(d["labels"].astype(np.int64)), torch.from_numpy(d["frame_lens"].astype(np.int64)),
                                        torch.from_numpy(d["label_lens"].astype(np.int64)), blank=0, reduction=reduction,
                                        zero_infinity=True)
    loss.backward()
    return float(loss.detach()), W.grad.numpy(), b.grad.numpy()


@pytest.mark.parametrize("reduction", ["sum", "mean"])
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_reference_against_torch_float64_autograd(reduction, p):
    d = _small(p)
    _, (grad, nll, bad), g = R.step(d["x"], d["W"], d["b"], d["frame_lens"], d["labels"], d["label_lens"], reduction, d["L"],
                                    d["keep"], d["scale"])
    assert bad.tolist() == [0, 1, 0, 0] and g["n_infeasible"] == 1 and nll[1] == 0.0 and not grad[1].any()
    loss, gW, gb = _torch_grads(d, reduction)
    assert abs(g["loss"] - loss) <= 1e-12 * max(1.0, abs(loss))
    assert np.abs(g["gW"] - gW).max() <= 1e-12 and np.abs(g["gb"] - gb).max() <= 1e-12
    assert np.abs(gW).max() > 1e-3 and not grad[0, 12:].any() and not grad[3, 7:].any()


@pytest.mark.parametrize("reduction", ["sum", "mean"])
def test_reference_against_central_differences(reduction):
    d = _small(0.3, seed=8)
    args = (d["frame_lens"], d["labels"], d["label_lens"], reduction, d["L"], d["keep"], d["scale"])
    g = R.step(d["x"], d["W"], d["b"], *args)[2]
    eps = 1e-6
    for name, key in (("W", "gW"), ("b", "gb")):
        base = R.f64(d[name])
        num = np.zeros_like(base)
        for idx in np.ndindex(base.shape):
            hi, lo = base.copy(), base.copy()
            hi[idx] += eps
            lo[idx] -= eps
            kw_hi, kw_lo = dict(d, **{name: hi}), dict(d, **{name: lo})
            num[idx] = (R.loss_of(d["x"], kw_hi["W"], kw_hi["b"], *args) - R.loss_of(d["x"], kw_lo["W"], kw_lo["b"], *args)) / (2 * eps)
        assert np.abs(num - g[key]).max() <= 1e-8, (name, np.abs(num - g[key]).max())


def test_no_frames_at_all_gives_zero_gradients_and_zero_loss():
    d = _small(0.0)
    fl = np.zeros(4, dtype=np.int32)
    f, (grad, nll, bad), g = R.step(d["x"], d["W"], d["b"], fl, d["labels"], d["label_lens"], "mean", d["L"])
    assert bad.tolist() == [1, 1, 1, 1] and g["loss"] == 0.0 and not g["gW"].any() and not g["gb"].any() and not f["live"].any()


@pytest.mark.parametrize("name", [n for n in R.CASES if not n.startswith("R2400")])
def test_bounds_hold_an_fp32_transcription(name):
    d, x, keep, _, scale, f, g = R.case_ref(name)
    k = None if d["p"] == 0.0 else keep
    lg, lp = R.forward_f32(x, d["W"], d["b"], d["frame_lens"], k, scale)
    live = f["live"]
    for got, key in ((lg, "logits"), (lp, "logp")):
        q = C.ratio(got[live], f[key][live], f["b_" + key][live])
        assert 0.0 < q <= 1.0, (name, key, q)
    xd32 = f["xd"].astype(np.float32)   # (x * scale rounded once, as the kernel forms it)
    gW, gb, loss = R.backward_f32(xd32, d["grad"], d["nll"], d["infeasible"], d["label_lens"], d["frame_lens"], d["reduction"], R.L_MAX)
    for got, key in ((gW, "gW"), (gb, "gb"), (loss, "loss")):
        q = C.ratio(got, g[key], g["b_" + key])
        assert 0.0 < q <= 1.0, (name, key, q)


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_mutation_exceeds_the_bounds_on_its_cases(mutation):
    cases, keys = R.MUTATION_CASES[mutation]
    assert cases and set(R.MUTATION_CASES) == set(R.MUTATIONS)
    for name in cases:
        d, x, keep, _, scale, f, g = R.case_ref(name)
        m = R.mutated(name, mutation)
        for key in keys:
            if key in ("logits", "logp"):
                live = f["live"]
                q = C.ratio(m[key][live], f[key][live], f["b_" + key][live])
            else:
                q = C.ratio(m[key], g[key], g["b_" + key])
            assert q > 1.0, (mutation, name, key, q)


@pytest.mark.parametrize("name", list(R.CASES))
def test_the_reference_decides_the_argmax_of_99_percent_of_the_rows(name):
    d, x, keep, _, scale, f, g = R.case_ref(name)
    live, dec = f["live"], R.decided(f)
    assert int(live.sum()) > 0 and int((live & ~dec).sum()) <= 0.01 * int(live.sum()), (name, int((live & ~dec).sum()), int(live.sum()))
    # the cases hold what the kernels' tests lean on
    fl = d["frame_lens"]
    assert (fl == 0).any() and (fl >= d["T"]).any() and (d["label_lens"] == 0).any() and d["infeasible"].sum() == 1
    assert R.chunk_rows(d["N"] * d["T"]) == 256 and R.chunk_rows(16384) == 256 and R.chunk_rows(16385) == 512 and R.chunk_rows(1 << 22) == 65536


def test_case_sizes_cover_the_row_chunk_and_the_shapes():
    rows = {c[0] * c[1] for c in R.CASES.values()}
    assert {255, 256, 257, 2400} <= rows
    assert {c[2] for c in R.CASES.values()} == {8, 64, 768} and {c[3] for c in R.CASES.values()} == {2, 31, 32, 33, 64}
    assert {c[4] for c in R.CASES.values()} == {"fp32", "bf16"} and {c[5] for c in R.CASES.values()} == {0.0, 0.1, 0.9}
    assert {c[6] for c in R.CASES.values()} == {"sum", "mean"} and any(c[7] % 8 for c in R.CASES.values())
    assert max(c[0] * c[1] * c[2] * c[3] for c in R.CASES.values()) == 8 * 300 * 768 * 32


def test_bf16_round_is_torchs():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(4096, generator=g) * 3.0
    assert np.array_equal(R.bf16_round(x.numpy()), x.to(torch.bfloat16).float().numpy())


def test_check_ctc_head_args():
    W = _W()
    cfg = W.make_config("tiny", vocab_size=8)
    H = cfg.hidden_size
    lab = np.array([[1, 2, 3], [4, 5, 0], [7, 0, 0]])
    N, T, fl, l32, lens = W.check_ctc_head_args(cfg, (3, 20, H), torch.bfloat16, [20, 7, 1], lab, [3, 2, 1])
    assert (N, T) == (3, 20) and fl.dtype == np.int32 and fl.tolist() == [20, 7, 1] and l32.dtype == np.int32 and lens.tolist() == [3, 2, 1]
    full = W.check_ctc_head_args(cfg, (3, 20, H), torch.float32, torch.tensor([20, 7, 1]), torch.from_numpy(lab[:, :1]))
    assert full[4].tolist() == [1, 1, 1]   # (without label_lengths every row is full; lab's padding zeros would be blanks: refused below)
    ok = dict(hidden_shape=(3, 20, H), hidden_dtype=torch.bfloat16, frame_lengths=[20, 7, 1], labels=lab, label_lengths=[3, 2, 1])
    for kw in (dict(frame_lengths=[20, 7, 0]), dict(frame_lengths=[21, 7, 1]), dict(frame_lengths=[20, 7]), dict(frame_lengths=[20.0, 7.0, 1.0]),
               dict(labels=None), dict(label_lengths=None), dict(label_lengths=[3, 3, 1]), dict(label_lengths=[4, 2, 1]),
               dict(labels=np.array([[1, 2, 8], [4, 5, 0], [7, 0, 0]])), dict(labels=lab[:2]), dict(labels=lab.astype(np.float32)),
               dict(hidden_dtype=torch.float16), dict(hidden_shape=(3, 20, H + 8)), dict(hidden_shape=(3, 20)), dict(hidden_shape=(3, 0, H)),
               dict(hidden_shape=(3, 4097, H))):
        with pytest.raises(ValueError):
            W.check_ctc_head_args(cfg, **dict(ok, **kw))
    with pytest.raises(ValueError):
        W.check_ctc_head_args(W.make_config("tiny", vocab_size=65), **ok)
    with pytest.raises(ValueError):
        W.check_ctc_head_args(W.make_config("tiny", vocab_size=8, hidden_size=260, num_attention_heads=4), **dict(ok, hidden_shape=(3, 20, 260)))
    assert W.check_ctc_head_args(cfg, (70000, 1, H), torch.float32, np.ones(70000, dtype=np.int64), np.ones((70000, 1), dtype=np.int64))[0] == 70000
    assert W.ctc_head_batch_limit(1) == 65535 and W.ctc_head_batch_limit(4096) == 1024 and W.ctc_head_batch_limit(300) == (1 << 22) // 300
    # the label rules are check_ctc_args' own
    T_in = 4000
    assert W.check_ctc_args(cfg, (3, T_in), lab, [3, 2, 1])[4].tolist() == l32.tolist()
    assert W.SITE_CTC == 6 == R.SITE_CTC and len({W.SITE_FE, W.SITE_FP, W.SITE_PH, W.SITE_PQ, W.SITE_CLS, W.SITE_CTC}) == 6


def test_arena_the_ctc_head_is_the_contiguous_tail():
    W = _W()
    cfg = W.make_config("tiny", vocab_size=8)
    a = W.W2VArena(cfg, "cpu", head="ctc")
    assert a.names[-2:] == ["lm_head.kernel", "lm_head.bias"]
    lo = a.offsets["lm_head.kernel"]
    assert a.offsets["lm_head.bias"] == lo + (cfg.hidden_size * 8 + 7) // 8 * 8 and a.numel == a.offsets["lm_head.bias"] + 8
    assert max(a.offsets[n] + int(np.prod(a.shapes[n])) for n in a.names[:-2]) <= lo


def test_binding_header_and_null_refusals():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib
    header = open(os.path.join(ROOT, "include", "tethys_mi.h")).read()
    want = {"tmi_ctc_head_workspace_bytes": 4, "tmi_ctc_head_fwd": 23, "tmi_ctc_head_bwd": 28}
    for name, nargs in want.items():
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\);", header)
        assert m is not None, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == nargs, name
    assert _lib.ABI_VERSION == 31
    assert "rc = 256 * ceil(N*T_max / 16384)" in header and "w_n" in header
    src = open(os.path.join(ROOT, "tethys-speech_amd", "csrc", "ctc_head.hip")).read()
    assert "atomic" not in src.replace("no atomic", "").replace("floating-point atomic", "")
    assert "ctc_head.hip" in open(os.path.join(ROOT, "tethys-speech_amd", "csrc", "Makefile")).read()
    lib = _lib.lib()
    assert lib.tmi_abi_version() == 31
    wb = lib.tmi_ctc_head_workspace_bytes
    assert wb(8, 300, 768, 32) == 10 * (768 * 32 + 32) * 4 and wb(4, 64, 64, 31) == (64 * 31 + 31) * 4 and wb(257, 1, 64, 33) == 2 * (64 * 33 + 33) * 4
    assert wb(1024, 4096, 8, 2) == 64 * (8 * 2 + 2) * 4
    for bad in ((0, 1, 8, 2), (65536, 1, 8, 2), (1, 0, 8, 2), (1, 4097, 8, 2), (1025, 4096, 8, 2), (1, 1, 0, 2), (1, 1, 12, 2), (1, 1, 4104, 2),
                (1, 1, 8, 1), (1, 1, 8, 65)):
        assert wb(*bad) == -1, bad
    # a NULL pointer is refused on the host before anything is launched (so this runs without a GPU): -1, the function named
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    p = p + (-p) % 16
    fwd = lambda hidden, frame_lens, Wp, b, logp: lib.tmi_ctc_head_fwd(hidden, 0, 16, 8, 1, None, frame_lens, Wp, b, 0.0, 0, None, 0, 0,
                                                                       logp, 16, 8, None, 1, 2, 8, 2, None)
    for args in ((None, p, p, p, p), (p, None, p, p, p), (p, p, None, p, p), (p, p, p, None, p), (p, p, p, p, None), (p + 4, p, p, p, p)):
        assert fwd(*args) == -1
        assert lib.tmi_last_error().decode().startswith("tmi_ctc_head_fwd:") and "2 <= V <= 64" in lib.tmi_last_error().decode()
    bwd = lambda hidden, grad, gW, ws, wsb=1 << 12, p_=0.0, red=1: lib.tmi_ctc_head_bwd(
        hidden, 0, 16, 8, 1, None, p, p, grad, 16, 8, p, p, p_, 0, red, gW, p, p, p, ws, wsb, 1, 2, 3, 8, 2, None)
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None), (p, p, p, p, 8), (p, p, p, p, 1 << 12, 1.0),
                 (p, p, p, p, 1 << 12, 0.0, 2)):
        assert bwd(*args) == -1
        assert lib.tmi_last_error().decode().startswith("tmi_ctc_head_bwd:") and "tmi_ctc_head_workspace_bytes" in lib.tmi_last_error().decode()


def test_training_calls_keep_their_message():
    W = _W()
    src = open(os.path.join(ROOT, "tethys-speech_amd", "wav2vec2.py")).read()
    assert src.count('raise NotImplementedError("CTC fine-tuning is not built")') == 2
    assert callable(W.fit_ctc_head) and all(hasattr(W.Wav2Vec2ForCTC, n) for n in ("encode_features", "head_step", "evaluate_features"))


def test_planted_problem_is_solved_by_the_reference_inside_half_the_budget():
    errs = R.planted_run(R.PLANTED_STEPS)
    failing = [i + 1 for i, e in enumerate(errs) if e]
    last = failing[-1] if failing else 0
    print(f"planted problem: token errors {errs[0]} after step 1, the last failing step is {last}, budget {R.PLANTED_STEPS}")
    assert errs[0] > 0 and 0 < last and 2 * last <= R.PLANTED_STEPS and errs[-1] == 0
