"""The CTC probe behind a learned weighted sum over layers, on the GPU (the "tiny" size with vocab_size 8: hidden 256, 4
layers, so K = 5; clips of 4000 samples; fp32 and bf16): ``encode_features(layers="all")`` bit for bit ``forward_infer``'s
hidden states, a one-layer mix bit for bit the plain ``head_step``, five mixed head steps held to float64 one stage at a
time, the arena outside the head's slice, the attached mix in ``model(inputs)`` / ``evaluate`` / ``decode`` / ``align`` /
``posteriors``, ``fit_ctc_head`` twice with one seed, the job in a child process, and the planted problem of
tests/_layer_mix_ref.py (the signal in one middle layer of five) learnt inside the step budget.

As in tests/test_ctc_head_gpu.py each stage of a step is compared with the float64 reference fed what the DEVICE held going
into that stage, so no stage is charged another's error and every bound is the derived one: ``mixed`` and the weights from
(layers, logits) under ``_layer_mix_ref``; log_probs from the device's ``mixed`` under ``_ctc_head_ref``; logit_grad from
the device's log_probs under ``_ctc_post_ref``; gW / gb / loss and the logits' gradient from the device's logit_grad; the
two Adam updates from the device's gradients and moments under ``_adam_ref``."""
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
import _layer_mix_ref as M
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


def ibits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def snapshot(m):
    out = {n: getattr(m.arena, n).clone() for n in ("p", "m", "v")}
    if m.mirror is not None:
        out["mirror"] = m.mirror.clone()
    return out


def restore(m, snap):
    for name, was in snap.items():
        (m.mirror if name == "mirror" else getattr(m.arena, name)).copy_(was)


def some_mix(m, dev, seed=17):
    mix = W().LayerMix(m.config.num_hidden_layers + 1, dev)
    mix.logits.copy_((torch.randn(mix.num_layers, generator=torch.Generator().manual_seed(seed)) * 0.8).to(dev))
    return mix


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_encode_features_all_layers_is_forward_infers_hidden_states(dev, models, precision, ragged):
    m = model_for(models, precision, dev)
    x = clips(3).to(dev)
    mask = W().frame_attention_mask(m.config, (T_IN, 3300, 1700), T_IN) if ragged else None
    want = m.forward_infer(x, attention_mask=mask, output_hidden_states=True)
    plain = m.encode_features(x, attention_mask=mask)
    got = m.encode_features(x, attention_mask=mask, layers="all")
    K = m.config.num_hidden_layers + 1
    assert set(plain) == {"hidden", "frame_lengths"} and set(got) == {"hidden", "frame_lengths", "hidden_layers"}
    assert got["hidden_layers"].dtype == m.dtype and tuple(got["hidden_layers"].shape) == (K,) + tuple(want["last_hidden_state"].shape)
    assert len(want["hidden_states"]) == K
    for k in range(K):
        assert torch.equal(ibits(got["hidden_layers"][k]), ibits(want["hidden_states"][k])), k
    assert torch.equal(ibits(got["hidden"]), ibits(plain["hidden"])) and torch.equal(ibits(got["hidden_layers"][-1]), ibits(got["hidden"]))
    assert torch.equal(got["frame_lengths"], plain["frame_lengths"])
    with pytest.raises(ValueError):
        m.encode_features(x, layers="last")


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


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_a_mix_of_one_layer_is_the_plain_head_step_bit_for_bit(dev, models, precision):
    from tethys_speech_amd import optim
    m = model_for(models, precision, dev)
    keep0 = snapshot(m)
    try:
        hidden = m.encode_features(clips(4, seed=13).to(dev))["hidden"]
        n_src, T, H = hidden.shape
        N, L, idx, fl, labels, lens = step_batch(T, n_src)
        to = lambda a: torch.from_numpy(a).to(dev)
        idx_d, fl_d, lab_d, lens_d = to(idx), to(fl), to(labels), to(lens)
        runs = []
        for mix in (None, W().LayerMix(1, dev)):
            restore(m, keep0)
            m.arena.m.zero_()
            m.arena.v.zero_()
            opt = optim.Adam(1e-3)
            feats = hidden if mix is None else hidden.unsqueeze(0)
            losses = [m.head_step(feats, fl_d, lab_d, lens_d, opt, row_index=idx_d, dropout=0.1, seed=5, step=t, layer_mix=mix)["loss"]
                      for t in range(3)]
            runs.append((torch.cat(losses), *(getattr(m.arena, n)[m.head_lo:].clone() for n in ("p", "m", "v"))))
            if mix is not None:
                assert not mix.logits.any() and not mix.grad.any() and opt.iterations == 3   # (one layer: no gradient, exactly)
        for a, b in zip(*runs):
            assert torch.equal(ibits(a), ibits(b))
        assert not torch.equal(runs[0][1], keep0["p"][m.head_lo:])
    finally:
        restore(m, keep0)


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_five_mixed_head_steps_stage_by_stage_against_float64(dev, models, precision, reduction):
    from tethys_speech_amd import optim
    m = model_for(models, precision, dev, reduction)
    lo, hi = m.head_lo, m.head_hi
    keep0 = snapshot(m)
    try:
        enc = m.encode_features(clips(4, seed=13).to(dev), layers="all")
        layers = enc["hidden_layers"]
        K, n_src, T, H = layers.shape
        N, L, idx, fl, labels, lens = step_batch(T, n_src)
        to = lambda a: torch.from_numpy(a).to(dev)
        idx_d, fl_d, lab_d, lens_d = to(idx), to(fl), to(labels), to(lens)
        mix = some_mix(m, dev)
        assert W().check_layer_mix_args(m.config, tuple(layers.shape), layers.dtype, mix) == (K, n_src, T)
        opt = optim.Adam(1e-3)
        m.arena.m.zero_()
        m.arena.v.zero_()
        start = snapshot(m)
        hyper = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7, eps_mode=0)
        x = M.gather_layers(layers.float().cpu().numpy(), idx)
        a = m.arena
        for t in range(5):
            before = snapshot(m)
            mix0 = {n: getattr(mix, "_" + n).clone() for n in ("p", "m", "v")}
            r = m.head_step(layers, fl_d, lab_d, lens_d, opt, row_index=idx_d, dropout=0.1, seed=77, step=t, return_intermediates=True,
                            layer_mix=mix)
            assert int(r["n_infeasible"]) == 1 and tuple(r["loss"].shape) == (1,)
            tag = (precision, reduction, t)
            params = {k: before["p"][a.offsets[k]:a.offsets[k] + int(np.prod(a.shapes[k]))].view(*a.shapes[k]).cpu().numpy() for k in HEAD}
            logits0 = mix0["p"][:K].cpu().numpy()
            keep, _, scale = R.keep_masks(R.step_seed(77, t), N, None, N, T, H, 0.1)
            # stage 0: the weights and the mixed features from (layers, logits)
            mf = M.forward(x, logits0, fl)
            live = mf["live"]
            within("mixed head step layer_weights / bound", C.ratio(f64(r["layer_weights"]), mf["w"], mf["b_w"]), 1.0, tag)
            mixed_dev = f64(r["mixed"])
            q = C.ratio(mixed_dev[live], mf["mixed"][live], mf["b_mixed"][live])
            print(f"mixed head step {tag} mixed: {q:.4f} of its bound")
            within("mixed head step mixed / bound", q, 1.0, tag)
            assert not mixed_dev[~live].any()
            # stage 1: the log-probs from the device's mixed features
            f = R.forward(mixed_dev, params[HEAD[0]], params[HEAD[1]], fl, keep, scale)
            lp_dev = f64(r["log_probs"])
            within("mixed head step log_probs / bound", C.ratio(lp_dev[live], f["logp"][live], f["b_logp"][live]), 1.0, tag)
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
                within("mixed head step logit_grad / bound", C.ratio(grad_dev[n, :Tn], ref["grad"], ref["b_grad"]), 1.0, tag + (n,))
            assert bad.tolist() == [0, 0, 0, 1, 0]
            # stage 3: gW, gb and the loss from the device's logit gradient
            g = R.backward(f["xd"], grad_dev, nll_ref, bad, lens, fl, reduction, L)
            for name, key in zip(HEAD, ("gW", "gb")):
                within(f"mixed head step {key} / bound", C.ratio(f64(a.grad(name)), g[key], g["b_" + key]), 1.0, tag)
            b_loss = g["b_loss"] + float((g["w"] * e_nll).sum()) * (1 + R.SLACK)
            within("mixed head step loss / bound", C.ratio(float(r["loss"]), g["loss"], b_loss), 1.0, tag)
            # stage 4: the gradient of the logits from the device's logit gradient, the layers and the head's W
            mb = M.backward(x, logits0, grad_dev, bad, lens, fl, reduction, L, params[HEAD[0]], keep, scale)
            q = C.ratio(f64(r["layer_logit_grad"]), mb["g_a"], mb["b_g"])
            print(f"mixed head step {tag} g_a: {q:.4f} of its bound")
            within("mixed head step g_a / bound", q, 1.0, tag)
            assert np.abs(mb["g_a"]).max() > 0.0 and torch.equal(r["layer_logit_grad"], mix.grad)
            # stage 5: Keras Adam in float64 on the step's own gradients, from the state the device held: the head, the mix
            sl = slice(lo, hi)
            tr = A.adam_terms(before["p"][sl], a.g[sl], before["m"][sl], before["v"][sl], step=t + 1, **hyper)
            ab = A.adam_bounds(tr)
            for name in ("p", "m", "v"):
                within(f"mixed head step adam {name} / bound", A.bound_fraction(getattr(a, name)[sl], tr[name], ab[name]), 1.0, tag)
            tr = A.adam_terms(mix0["p"], mix._g, mix0["m"], mix0["v"], step=t + 1, **hyper)
            ab = A.adam_bounds(tr)
            for name in ("p", "m", "v"):
                within(f"mixed head step mix adam {name} / bound", A.bound_fraction(getattr(mix, "_" + name), tr[name], ab[name]), 1.0, tag)
            assert float((mix.logits - mix0["p"][:K]).abs().max()) > 0.0 and not mix._p[K:].any()
            if m.mirror is not None:
                assert torch.equal(m.mirror[sl], a.p[sl].to(torch.bfloat16))
        assert opt.iterations == 5
        for name, was in start.items():   # outside the head's slice the arena is bit for bit what it was
            now = m.mirror if name == "mirror" else getattr(a, name)
            assert torch.equal(ibits(now[:lo]), ibits(was[:lo])), name
            assert now.numel() == hi
    finally:
        restore(m, keep0)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_an_attached_mix_is_what_inference_reads(dev, models, precision):
    from tethys_speech_amd import ops
    m = model_for(models, precision, dev)
    wav2vec2 = W()
    x = clips(4, seed=9).to(dev)
    mask = wav2vec2.frame_attention_mask(m.config, (T_IN, 3300, 1700, 900), T_IN)
    labels = np.zeros((4, 5), dtype=np.int64)
    lens = [5, 3, 0, 4]
    for n in range(4):
        labels[n, :lens[n]] = C.labels_for("random", lens[n], VOCAB, seed=60 + n)
    base = m(x, attention_mask=mask)
    base_eval = m.evaluate(x, labels, lens, attention_mask=mask, edit_ops=True)
    mix = some_mix(m, dev)
    with pytest.raises(ValueError):
        m.set_layer_mix(wav2vec2.LayerMix(3, dev))
    with pytest.raises(TypeError):
        m.set_layer_mix("uniform")
    m.set_layer_mix(mix)
    try:
        got = m(x, attention_mask=mask)
        enc = m.encode_features(x, attention_mask=mask, layers="all")
        assert torch.equal(ibits(got["last_hidden_state"]), ibits(base["last_hidden_state"]))
        B, T, H = enc["hidden"].shape
        full = torch.full((B,), T, dtype=torch.int32, device=dev)
        mixed = torch.zeros((B, T, H), dtype=torch.float32, device=dev)
        logp, logits = torch.zeros((B, T, VOCAB), device=dev), torch.zeros((B, T, VOCAB), device=dev)
        ops.layer_mix_fwd(enc["hidden_layers"], mix.logits, full, mixed)
        ops.ctc_head_fwd(mixed, m.arena.param(HEAD[0]), m.arena.param(HEAD[1]), full, logp, logits=logits)
        assert torch.equal(ibits(got["log_probs"]), ibits(logp)) and torch.equal(ibits(got["logits"]), ibits(logits))
        assert not torch.equal(got["log_probs"], base["log_probs"])
        ev = m.evaluate(x, labels, lens, attention_mask=mask, edit_ops=True)
        ef = m.evaluate_features(enc["hidden_layers"], enc["frame_lengths"], labels, lens, layer_mix=mix)
        for k in ("n_items", "n_infeasible", "n_edits", "n_sub", "n_del", "n_ins", "n_ref_tokens", "n_hyp_tokens", "token_error_rate"):
            assert ev[k] == ef[k], k
        # the same fp32 nll per item on both paths, added on the host in float64 in the items' order, in one or two pieces
        assert abs(ev["nll_sum"] - ef["nll_sum"]) <= 4 * 2.0 ** -52 * abs(ef["nll_sum"]), (ev["nll_sum"], ef["nll_sum"])
        dec = m.decode(x, attention_mask=mask)
        beam = m.decode(x, attention_mask=mask, num_beams=4)
        assert dec["sequences"].shape[0] == 4 and beam["sequences"].shape[0] == 4 and dec["lengths"].shape[0] == 4
        al = m.align(x, labels, lens, attention_mask=mask)
        po = m.posteriors(x, labels, lens, attention_mask=mask)
        assert al is not None and bool(torch.isfinite(po["nll"]).all())
    finally:
        m.set_layer_mix(None)
    again = m(x, attention_mask=mask)
    assert torch.equal(ibits(again["log_probs"]), ibits(base["log_probs"])) and torch.equal(ibits(again["logits"]), ibits(base["logits"]))
    assert m.evaluate(x, labels, lens, attention_mask=mask, edit_ops=True) == base_eval


def test_fit_ctc_head_with_a_mix_is_reproducible(dev, models):
    m = model_for(models, "bf16", dev)
    keep0 = snapshot(m)
    try:
        enc = m.encode_features(clips(6, seed=21).to(dev), attention_mask=W().frame_attention_mask(
            m.config, (T_IN, 3300, 1700, T_IN, 900, 2000), T_IN), layers="all")
        labels = np.zeros((6, 4), dtype=np.int64)
        lens = [4, 3, 2, 0, 1, 4]
        for n in range(6):
            labels[n, :lens[n]] = C.labels_for("random", lens[n], VOCAB, seed=80 + n)
        eval_set = (enc["hidden_layers"][:, :3], enc["frame_lengths"][:3], labels[:3], lens[:3])
        runs = []
        for _ in range(2):
            restore(m, keep0)
            m.arena.m.zero_()
            m.arena.v.zero_()
            mix = W().LayerMix(5, dev)
            hist = W().fit_ctc_head(m, enc["hidden_layers"], enc["frame_lengths"], labels, lens, epochs=2, batch_size=4,
                                    learning_rate=1e-2, seed=3, eval_set=eval_set, layer_mix=mix, mix_learning_rate=5e-2)
            runs.append((hist, m.arena.p[m.head_lo:].clone(), mix.logits.clone(), mix.m.clone()))
        (h0, p0, l0, m0), (h1, p1, l1, m1) = runs
        assert h0 == h1 and len(h0) == 2
        assert set(h0[0]) == {"epoch", "loss", "n_infeasible", "eval_loss", "eval_token_error_rate", "layer_weights"}
        assert len(h0[1]["layer_weights"]) == 5 and abs(sum(h0[1]["layer_weights"]) - 1.0) < 1e-12
        assert np.allclose(h0[1]["layer_weights"], mix.weights().cpu().numpy(), atol=1e-6)
        for a, b in ((p0, p1), (l0, l1), (m0, m1)):
            assert torch.equal(ibits(a), ibits(b))
        assert bool(l0.any()) and float(l0.abs().max()) > 0.05   # (four steps at the mix's own rate, 5e-2)
        assert torch.equal(m.arena.p[:m.head_lo], keep0["p"][:m.head_lo])
    finally:
        restore(m, keep0)


def test_mixed_calls_refuse_host_side_mistakes(dev, models):
    from tethys_speech_amd import optim
    m = model_for(models, "bf16", dev)
    H = m.config.hidden_size
    lay = torch.zeros((5, 2, 10, H), dtype=torch.bfloat16, device=dev)
    i32 = lambda *a: torch.tensor(a, dtype=torch.int32, device=dev)
    fl, ll, lab = i32(10, 5), i32(1, 1), torch.ones((2, 1), dtype=torch.int32, device=dev)
    opt, mix = optim.Adam(1e-3), W().LayerMix(5, dev)
    for bad in (dict(hidden=lay[0]), dict(hidden=lay[:4]), dict(hidden=lay.float()), dict(mix=W().LayerMix(4, dev)), dict(mix="mix"),
                dict(mix=W().LayerMix(5, "cpu"))):
        kw = dict(hidden=lay, mix=mix)
        kw.update(bad)
        with pytest.raises((TypeError, ValueError)):
            m.head_step(kw["hidden"], fl, lab, ll, opt, layer_mix=kw["mix"])
    assert opt.iterations == 0 and not mix.logits.any()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_planted_problem_finds_the_layer_and_is_learnt_exactly(dev, models, precision):
    """The planted problem of ``_layer_mix_ref``: the features of ``_ctc_head_ref``'s problem in layer k* = 2 of K = 5, noise
    of the same scale in the other four, in the first 32 of the model's 256 columns (zeros in the rest, as
    tests/test_ctc_head_gpu.py places them).  From uniform weights, inside ``PLANTED_STEPS`` = twice the float64 reference's
    own last failing step (asserted in test_layer_mix_cpu.py): a token error rate of exactly 0, and the largest weight on
    k*."""
    from tethys_speech_amd import optim
    m = model_for(models, precision, dev)
    keep0 = snapshot(m)
    c, pr = M.PLANTED, M.planted_problem()
    try:
        assert m.config.ctc_loss_reduction == "mean"
        Hm, K = m.config.hidden_size, c["K"]
        layers = torch.zeros((K, c["N"], c["T"], Hm), dtype=torch.float32)
        layers[:, :, :, :c["H"]] = torch.from_numpy(pr["layers"])
        layers = layers.to(dev, m.dtype)
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
        mix = W().LayerMix(K, dev, learning_rate=c["mix_lr"])
        first = m.evaluate_features(layers, pr["frame_lens"], pr["labels"], pr["label_lens"], layer_mix=mix)
        opt = optim.Adam(c["lr"])
        for t in range(M.PLANTED_STEPS):
            m.head_step(layers, fl_d, lab_d, lens_d, opt, dropout=c["dropout"], seed=0, step=t, layer_mix=mix)
        last = m.evaluate_features(layers, pr["frame_lens"], pr["labels"], pr["label_lens"], layer_mix=mix)
        w = mix.weights().cpu().numpy()
        print(f"planted layer-mix problem {precision}: token error rate {first['token_error_rate']:.3f} -> {last['token_error_rate']:.3f}, "
              f"weights {np.round(w.astype(np.float64), 3).tolist()} after {M.PLANTED_STEPS} steps")
        assert first["token_error_rate"] > 0.0 and last["n_ref_tokens"] == float(pr["label_lens"].sum())
        assert last["token_error_rate"] == 0.0 and last["n_edits"] == 0.0 and last["n_infeasible"] == 0.0
        assert int(np.argmax(w)) == pr["k_star"]
    finally:
        restore(m, keep0)


def test_asr_job_fit_head_with_a_layer_mix(dev, tmp_path):
    """The CLI end to end in ONE child process on the smallest built-in size: --fit_head --layer_mix --layer_mix_file (the
    logits the fit starts from) --save; the rest of the job decodes through the attached mix."""
    lab, save, init = tmp_path / "labels.txt", str(tmp_path / "head.pt"), str(tmp_path / "init.npy")
    lab.write_text("1 2 3\n4 5\n\n6 7 1 2\n")
    np.save(init, np.array([0.0, 0.5, 1.0, 0.5, 0.0], dtype=np.float32))
    args = [sys.executable, os.path.join(ROOT, "speech_jobs", "wav2vec2_asr.py"), "--model_size", "tiny", "--vocab_size", str(VOCAB),
            "--batch_size", "4", "--seconds", "0.25", "--labels", str(lab), "--edit_ops", "--fit_head", "--epochs", "2",
            "--train_batch_size", "3", "--learning_rate", "0.01", "--save", save, "--layer_mix", "--layer_mix_file", init]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run(args, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [json.loads(s) for s in p.stdout.splitlines() if s.startswith("{")]
    epochs = [r for r in lines if "fit_head_epoch" in r]
    assert [r["fit_head_epoch"] for r in epochs] == [1, 2] and all(np.isfinite(r["loss"]) for r in epochs)
    assert all(len(r["layer_weights"]) == 5 and abs(sum(r["layer_weights"]) - 1.0) < 1e-9 for r in epochs)
    fit = [r for r in lines if "fit_head" in r]
    assert len(fit) == 1 and fit[0]["epochs"] == 2 and fit[0]["fit_head"]["n_ref_tokens"] == 9.0 and len(fit[0]["layer_weights"]) == 5
    summary = lines[-1]
    assert summary["clips"] == 4 and summary["n_ref_tokens"] == 9.0 and len(lines) == 2 + 1 + 4 + 1
    logits = np.load(save + ".layermix.npy")
    assert logits.shape == (5,) and logits.dtype == np.float32 and np.isfinite(logits).all()
    assert not np.array_equal(logits, np.load(init)) and np.argmax(logits) == 2
    ck = torch.load(save, map_location="cpu")
    head = [v for k, v in ck.items() if "lm_head" in k and tuple(v.shape) == (256, VOCAB)]
    assert len(head) == 1 and bool(head[0].abs().max() > 0)
