"""The CTC probe of Wav2Vec2ForCTC on the GPU (the "tiny" size with vocab_size 8: hidden 256, 4 heads of 64, 4 layers;
clips of 4000 samples; fp32 and bf16): ``encode_features`` bit for bit ``forward_infer``'s last hidden state, five
``head_step``s held to float64 one stage at a time, the arena outside the head's slice, ``evaluate_features`` against
``evaluate``, ``fit_ctc_head`` twice with one seed, the training calls that still raise, the job in a child process, and
the planted problem of tests/_ctc_head_ref.py learnt to a token error rate of 0 inside the step budget.

Each stage of a step is compared with the float64 reference fed what the DEVICE held going into that stage, so no stage
is charged another's error and every bound is the derived one: log_probs from (hidden, W, b) under ``_ctc_head_ref``;
logit_grad from the device's log_probs under ``_ctc_post_ref``; gW / gb / loss from the device's logit_grad under
``_ctc_head_ref`` (the nll enters the loss with ``_ctc_post_ref``'s own nll bound added, weighted by w_n); the Adam update
from the device's gradient and moments under ``_adam_ref``."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _adam_ref as A
import _ctc_head_ref as R
import _ctc_post_ref as P
import _ctc_ref as C
from _margins import within
from oracle import wav2vec2_oracle as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_IN, VOCAB = 4000, 8
HEAD = ("lm_head.kernel", "lm_head.bias")


def W():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import wav2vec2
    return wav2vec2


@pytest.fixture(scope="module")
def models():
    cache = {}
    yield cache
    cache.clear()
    import gc
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def model_for(models, precision, dev, reduction="mean"):
    """One model per (precision, reduction); the head is scaled up and given a bias so that the posteriors are not uniform."""
    key = (precision, reduction)
    if key not in models:
        m = W().create_full_model("asr", "tiny", device=dev, precision=precision, seed=7, vocab_size=VOCAB,
                                  ctc_loss_reduction=reduction, ctc_zero_infinity=True)
        g = torch.Generator().manual_seed(3)
        m.arena.param("lm_head.kernel").mul_(6.0)
        m.arena.param("lm_head.bias").copy_((torch.randn(VOCAB, generator=g) * 0.3).to(dev))
        m.refresh_shadows()
        models[key] = m
    return models[key]


def clips(B, seed=5):
    return torch.from_numpy(V.create_dummy_pool(seed=seed, num_samples=B, length=T_IN))


def f64(t):
    return t.detach().double().cpu().numpy()


def snapshot(m):
    out = {n: getattr(m.arena, n).clone() for n in ("p", "m", "v")}
    if m.mirror is not None:
        out["mirror"] = m.mirror.clone()
    return out


def restore(m, snap):
    for name, was in snap.items():
        (m.mirror if name == "mirror" else getattr(m.arena, name)).copy_(was)


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_encode_features_is_forward_infers_last_hidden_state(dev, models, precision, ragged):
    m = model_for(models, precision, dev)
    x = clips(4).to(dev)
    mask = W().frame_attention_mask(m.config, (T_IN, 3300, 1700, 900), T_IN) if ragged else None
    want = m.forward_infer(x, attention_mask=mask)["last_hidden_state"]
    got = m.encode_features(x, attention_mask=mask)
    T = W().frame_lengths(m.config, [T_IN])[0]
    assert got["hidden"].dtype == m.dtype and tuple(got["hidden"].shape) == (4, T, m.config.hidden_size)
    assert torch.equal(got["hidden"].view(torch.int16 if precision == "bf16" else torch.int32),
                       want.view(torch.int16 if precision == "bf16" else torch.int32))
    assert got["frame_lengths"].dtype == torch.int32 and got["frame_lengths"].is_cuda
    assert got["frame_lengths"].tolist() == (mask.sum(1).int().tolist() if ragged else [T] * 4)
    assert m.head_lo == m.arena.offsets["lm_head.kernel"] and m.head_hi == m.arena.numel


def step_batch(T, n_src):
    """Five items drawn from ``n_src`` cached clips: ragged lengths with one at T, an item without labels (2), an item
    with 4 labels on 2 frames (3: infeasible)."""
    rng = np.random.default_rng(31)
    N, L = 5, 4
    idx = rng.integers(0, n_src, N).astype(np.int32)
    fl = np.array([T, T - 13, T // 2, 2, T - 1], dtype=np.int32)
    lens = np.array([4, 3, 0, 4, 2], dtype=np.int32)
    labels = np.zeros((N, L), dtype=np.int32)
    for n in range(N):
        labels[n, :lens[n]] = C.labels_for("distinct", int(lens[n]), VOCAB, seed=40 + n)
    return N, L, idx, fl, labels, lens


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_five_head_steps_stage_by_stage_against_float64(dev, models, precision, reduction):
    from tethys_speech_amd import optim
    m = model_for(models, precision, dev, reduction)
    lo, hi = m.head_lo, m.head_hi
    keep0 = snapshot(m)
    try:
        enc = m.encode_features(clips(4, seed=13).to(dev))
        hidden = enc["hidden"]
        n_src, T, H = hidden.shape
        N, L, idx, fl, labels, lens = step_batch(T, n_src)
        to = lambda a: torch.from_numpy(a).to(dev)
        idx_d, fl_d, lab_d, lens_d = to(idx), to(fl), to(labels), to(lens)
        W().check_ctc_head_args(m.config, (N, T, H), hidden.dtype, fl, labels, lens)
        opt = optim.Adam(1e-3)
        m.arena.m.zero_()
        m.arena.v.zero_()
        start = snapshot(m)
        hyper = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7, eps_mode=0)
        x = R.gather(hidden.float().cpu().numpy(), idx)
        a = m.arena
        for t in range(5):
            before = snapshot(m)
            r = m.head_step(hidden, fl_d, lab_d, lens_d, opt, row_index=idx_d, dropout=0.1, seed=77, step=t, return_intermediates=True)
            assert tuple(r["loss"].shape) == (1,) and r["loss"].is_cuda and r["n_infeasible"].dtype == torch.int32
            assert int(r["n_infeasible"]) == 1
            tag = (precision, reduction, t)
            params = {k: before["p"][a.offsets[k]:a.offsets[k] + int(np.prod(a.shapes[k]))].view(*a.shapes[k]).cpu().numpy() for k in HEAD}
            keep, _, scale = R.keep_masks(R.step_seed(77, t), N, None, N, T, H, 0.1)
            # stage 1: the log-probs from (hidden, W, b)
            f = R.forward(x, params[HEAD[0]], params[HEAD[1]], fl, keep, scale)
            live = f["live"]
            lp_dev = f64(r["log_probs"])
            q = C.ratio(lp_dev[live], f["logp"][live], f["b_logp"][live])
            print(f"ctc head step {tag} log_probs: {q:.4f} of its bound")
            within("ctc head step log_probs / bound", q, 1.0, tag)
            assert not lp_dev[~live].any()
            # stage 2: the logit gradient from the device's log-probs
            grad_dev = f64(r["logit_grad"])
            nll_ref, e_nll, bad = np.zeros(N), np.zeros(N), np.zeros(N, dtype=np.int64)
            for n in range(N):
                Tn = int(fl[n])
                ref = P.post_ref(lp_dev[n], labels[n, :lens[n]], Tn)
                bad[n] = ref["infeasible"]
                if ref["infeasible"]:
                    assert not grad_dev[n].any()
                    continue
                nll_ref[n], e_nll[n] = ref["nll"], ref["bound_nll"]
                within("ctc head step logit_grad / bound", C.ratio(grad_dev[n, :Tn], ref["grad"], ref["b_grad"]), 1.0, tag + (n,))
                assert not grad_dev[n, Tn:].any()
            assert bad.tolist() == [0, 0, 0, 1, 0]
            # stage 3: gW, gb and the loss from the device's logit gradient
            g = R.backward(f["xd"], grad_dev, nll_ref, bad, lens, fl, reduction, L)
            for name, key in zip(HEAD, ("gW", "gb")):
                q = C.ratio(f64(a.grad(name)), g[key], g["b_" + key])
                print(f"ctc head step {tag} {key}: {q:.4f} of its bound")
                within(f"ctc head step {key} / bound", q, 1.0, tag)
            b_loss = g["b_loss"] + float((g["w"] * e_nll).sum()) * (1 + R.SLACK)
            within("ctc head step loss / bound", C.ratio(float(r["loss"]), g["loss"], b_loss), 1.0, tag)
            assert float(r["loss"]) > 0.0
            # stage 4: Keras Adam in float64 on the step's own gradients, from the state the device held
            sl = slice(lo, hi)
            tr = A.adam_terms(before["p"][sl], a.g[sl], before["m"][sl], before["v"][sl], step=t + 1, **hyper)
            ab = A.adam_bounds(tr)
            for name in ("p", "m", "v"):
                within(f"ctc head step adam {name} / bound", A.bound_fraction(getattr(a, name)[sl], tr[name], ab[name]), 1.0, tag)
            assert float((a.p[sl] - before["p"][sl]).abs().max()) > 0.0
            if m.mirror is not None:
                assert torch.equal(m.mirror[sl], a.p[sl].to(torch.bfloat16))
        assert opt.iterations == 5
        # every parameter, moment and mirror element outside the head's slice is bit for bit what it was
        for name, was in start.items():
            now = m.mirror if name == "mirror" else getattr(a, name)
            it = torch.int16 if name == "mirror" else torch.int32
            assert torch.equal(now[:lo].view(it), was[:lo].view(it)), name
            assert now.numel() == hi
    finally:
        restore(m, keep0)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_evaluate_features_against_evaluate(dev, models, precision):
    m = model_for(models, precision, dev)
    wav2vec2 = W()
    x = clips(4, seed=9).to(dev)
    mask = wav2vec2.frame_attention_mask(m.config, (T_IN, 3300, 1700, 900), T_IN)
    labels = np.zeros((4, 5), dtype=np.int64)
    lens = [5, 3, 0, 4]
    for n in range(4):
        labels[n, :lens[n]] = C.labels_for("random", lens[n], VOCAB, seed=60 + n)
    enc = m.encode_features(x, attention_mask=mask)
    e = m.evaluate_features(enc["hidden"], enc["frame_lengths"], labels, lens)
    keys = {"nll_sum", "n_items", "n_infeasible", "loss", "n_edits", "n_sub", "n_del", "n_ins", "n_ref_tokens", "n_hyp_tokens",
            "token_error_rate"}
    assert set(e) == keys and all(isinstance(v, float) for v in e.values())
    assert e["n_items"] == 4.0 and e["n_ref_tokens"] == 12.0 and e["n_edits"] == e["n_sub"] + e["n_del"] + e["n_ins"]
    # against the float64 head on the same features: the nll sum within the forward-recursion bounds on the device's inputs
    p = {k: m.arena.param(k).detach().cpu().numpy() for k in HEAD}
    fl = enc["frame_lengths"].cpu().numpy()
    f = R.forward(enc["hidden"].float().cpu().numpy(), p[HEAD[0]], p[HEAD[1]], fl)
    total, bound = 0.0, 0.0
    for n in range(4):
        ref = C.ctc_forward_ref(f["logp"][n], labels[n, :lens[n]], int(fl[n]))
        total += ref["nll"]
        bound += ref["bound"] + f["b_logp"][n][f["live"][n]].max() * int(fl[n])   # (every frame's log-prob enters a path once)
    assert abs(e["nll_sum"] - total) <= bound, (e["nll_sum"], total, bound)
    hyp = R.greedy_transcripts(f["logp"], fl)
    dec = R.decided(f)
    if all(dec[n, :int(fl[n])].all() for n in range(4)):
        assert e["n_edits"] == float(sum(C.levenshtein(h, list(labels[n, :lens[n]])) for n, h in enumerate(hyp)))
    # against evaluate on the audio.  fp32: the same head in another summation order, so both lie within the bound of the
    # float64 value; bf16: evaluate's GEMM reads the bf16 mirror of lm_head, so only the counts are compared
    ev = m.evaluate(x, labels, lens, attention_mask=mask, edit_ops=True)
    assert ev["n_items"] == e["n_items"] and ev["n_ref_tokens"] == e["n_ref_tokens"] and ev["n_infeasible"] == e["n_infeasible"]
    if precision == "fp32":
        assert abs(ev["nll_sum"] - e["nll_sum"]) <= 2.0 * bound, (ev["nll_sum"], e["nll_sum"], bound)


def test_fit_ctc_head_is_reproducible(dev, models):
    m = model_for(models, "bf16", dev)
    keep0 = snapshot(m)
    try:
        enc = m.encode_features(clips(6, seed=21).to(dev), attention_mask=W().frame_attention_mask(
            m.config, (T_IN, 3300, 1700, T_IN, 900, 2000), T_IN))
        labels = np.zeros((6, 4), dtype=np.int64)
        lens = [4, 3, 2, 0, 1, 4]
        for n in range(6):
            labels[n, :lens[n]] = C.labels_for("random", lens[n], VOCAB, seed=80 + n)
        eval_set = (enc["hidden"][:3], enc["frame_lengths"][:3], labels[:3], lens[:3])
        runs = []
        for _ in range(2):
            restore(m, keep0)
            m.arena.m.zero_()
            m.arena.v.zero_()
            hist = W().fit_ctc_head(m, enc["hidden"], enc["frame_lengths"], labels, lens, epochs=2, batch_size=4, learning_rate=1e-2,
                                    seed=3, eval_set=eval_set)
            runs.append((hist, m.arena.p[m.head_lo:].clone(), m.arena.m[m.head_lo:].clone()))
        (h0, p0, m0), (h1, p1, m1) = runs
        assert h0 == h1 and len(h0) == 2
        assert set(h0[0]) == {"epoch", "loss", "n_infeasible", "eval_loss", "eval_token_error_rate"}
        assert torch.equal(p0.view(torch.int32), p1.view(torch.int32)) and torch.equal(m0.view(torch.int32), m1.view(torch.int32))
        assert not torch.equal(p0, keep0["p"][m.head_lo:]) and all(np.isfinite(h["loss"]) for h in h0)
        assert torch.equal(m.arena.p[:m.head_lo], keep0["p"][:m.head_lo])
        assert torch.equal(m.mirror[m.head_lo:], m.arena.p[m.head_lo:].to(torch.bfloat16))
    finally:
        restore(m, keep0)


def test_the_pinned_training_calls_still_raise(dev, models):
    m = model_for(models, "bf16", dev)
    x = clips(2).to(dev)
    with pytest.raises(NotImplementedError, match="CTC fine-tuning is not built"):
        m.forward_backward(x, None)
    with pytest.raises(NotImplementedError, match="CTC fine-tuning is not built"):
        m(x, training=True)


def test_head_step_refuses_host_side_mistakes(dev, models):
    from tethys_speech_amd import optim
    m = model_for(models, "bf16", dev)
    H = m.config.hidden_size
    hid = torch.zeros((2, 10, H), dtype=torch.bfloat16, device=dev)
    i32 = lambda *a: torch.tensor(a, dtype=torch.int32, device=dev)
    fl, ll, lab = i32(10, 5), i32(1, 1), torch.ones((2, 1), dtype=torch.int32, device=dev)
    opt = optim.Adam(1e-3)
    for bad in (dict(hidden=hid.float()), dict(hidden=hid[:, :, :H - 8]), dict(fl=fl.long()), dict(fl=i32(10)), dict(lab=lab.long()),
                dict(lab=lab[:1]), dict(ll=ll.cpu()), dict(row_index=torch.zeros(2, dtype=torch.int64, device=dev))):
        kw = dict(hidden=hid, fl=fl, lab=lab, ll=ll, row_index=None)
        kw.update(bad)
        with pytest.raises((TypeError, ValueError)):
            m.head_step(kw["hidden"], kw["fl"], kw["lab"], kw["ll"], opt, row_index=kw["row_index"])
    with pytest.raises(ValueError):
        m.head_step(hid, fl, lab, ll, opt, dropout=1.0)
    assert opt.iterations == 0


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_planted_problem_is_learnt_exactly(dev, models, precision):
    """hidden[n, t] = E[path(n, t)] + 0.5 noise in the first 32 of the model's 256 columns, zeros in the rest: a zero feature
    adds exact zeros to the logits, its weights get exact zero gradients and stay 0 under Adam, so this is the H = 32
    problem of ``_ctc_head_ref.planted_run`` with the same initial head, the same dropout masks (columns below 32 of the
    same rows) and the same Adam - up to fp32 (and, on the bf16 model, the rounding of the features).  The budget
    ``PLANTED_STEPS`` is at least twice the float64 reference's own last failing step (asserted in test_ctc_head_cpu.py)."""
    from tethys_speech_amd import optim
    m = model_for(models, precision, dev)
    keep0 = snapshot(m)
    c, pr = R.PLANTED, R.planted_problem()
    try:
        assert m.config.ctc_loss_reduction == "mean"
        Hm = m.config.hidden_size
        hidden = torch.zeros((c["N"], c["T"], Hm), dtype=torch.float32)
        hidden[:, :, :c["H"]] = torch.from_numpy(pr["hidden"])
        hidden = hidden.to(dev, m.dtype)
        W0, b0 = R.glorot(c["H"], c["V"], 5)
        a = m.arena
        a.param("lm_head.kernel").zero_()
        a.param("lm_head.kernel")[:c["H"]].copy_(torch.from_numpy(W0).to(dev))
        a.param("lm_head.bias").copy_(torch.from_numpy(b0).to(dev))
        a.m.zero_()
        a.v.zero_()
        m.refresh_shadows()
        to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        fl_d, lab_d, lens_d = to(pr["frame_lens"]), to(pr["labels"]), to(pr["label_lens"])
        first = m.evaluate_features(hidden, pr["frame_lens"], pr["labels"], pr["label_lens"])
        opt = optim.Adam(c["lr"])
        for t in range(R.PLANTED_STEPS):
            m.head_step(hidden, fl_d, lab_d, lens_d, opt, dropout=c["dropout"], seed=0, step=t)
        last = m.evaluate_features(hidden, pr["frame_lens"], pr["labels"], pr["label_lens"])
        print(f"planted problem {precision}: token error rate {first['token_error_rate']:.3f} -> {last['token_error_rate']:.3f}, "
              f"loss {first['loss']:.4f} -> {last['loss']:.4f} after {R.PLANTED_STEPS} steps")
        assert first["token_error_rate"] > 0.0 and last["n_ref_tokens"] == float(pr["label_lens"].sum())
        assert last["token_error_rate"] == 0.0 and last["n_edits"] == 0.0 and last["n_infeasible"] == 0.0
        assert not a.param("lm_head.kernel")[c["H"]:].any()
        # decode / evaluate see the trained head at once: the mirror inside the slice is the parameters cast to bf16
        if m.mirror is not None:
            assert torch.equal(m.mirror[m.head_lo:], a.p[m.head_lo:].to(torch.bfloat16))
    finally:
        restore(m, keep0)


def test_asr_job_fit_head(dev, tmp_path):
    """The CLI end to end in ONE child process on the smallest built-in size: --fit_head --epochs 2 --save."""
    lab, save = tmp_path / "labels.txt", str(tmp_path / "head.pt")
    lab.write_text("1 2 3\n4 5\n\n6 7 1 2\n")
    args = [sys.executable, os.path.join(ROOT, "speech_jobs", "wav2vec2_asr.py"), "--model_size", "tiny", "--vocab_size", str(VOCAB),
            "--batch_size", "4", "--seconds", "0.25", "--labels", str(lab), "--edit_ops", "--fit_head", "--epochs", "2",
            "--train_batch_size", "3", "--learning_rate", "0.01", "--save", save]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run(args, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [json.loads(s) for s in p.stdout.splitlines() if s.startswith("{")]
    epochs = [r for r in lines if "fit_head_epoch" in r]
    assert [r["fit_head_epoch"] for r in epochs] == [1, 2] and all(np.isfinite(r["loss"]) for r in epochs)
    fit = [r for r in lines if "fit_head" in r]
    assert len(fit) == 1 and fit[0]["epochs"] == 2 and fit[0]["fit_head"]["n_ref_tokens"] == 9.0
    summary = lines[-1]
    assert summary["clips"] == 4 and summary["n_ref_tokens"] == 9.0 and len(lines) == 2 + 1 + 4 + 1
    ck = torch.load(save, map_location="cpu")
    head = [v for k, v in ck.items() if "lm_head" in k and tuple(v.shape) == (256, VOCAB)]
    assert len(head) == 1 and bool(head[0].abs().max() > 0)
