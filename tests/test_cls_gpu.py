"""Wav2Vec2ForSequenceClassification on the GPU (the "tiny" size: hidden 256, 4 heads of 64, 4 layers; clips of 4000
samples = 100 frames; fp32 and bf16): the pooled output bit for bit ``forward_infer(pool="mean")``'s, the head against the
float64 reference of tests/_cls_ref.py fed the model's OWN pooled output (so the encoder's error is not charged to the
head), evaluate's sums, the training calls that raise, a pre-training ``save_weights`` file loaded into the model, five
``head_step``s and ``fit_head``, and the job in a child process.

The head steps are held to the float64 reference one step at a time, from exactly shared inputs, as
tests/test_optimizer_kernels_gpu.py does for Adam: the reference of step t starts from the head parameters and moments
the device holds before the step.  The gradients the step leaves in the arena are compared with the float64 gradients at
those parameters under the same mask (bounds of _cls_ref), and the update with float64 Keras Adam applied to the step's own
gradients (bounds of _adam_ref).  A free-running float64 trajectory has no derived bound: near a zero gradient Adam's
update m / (sqrt(v) + eps) turns a rounding error of the gradient into a step of either sign."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _adam_ref as A
import _cls_ref as R
from _margins import within
from oracle import wav2vec2_oracle as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_IN, C = 4000, 5
HEAD = ("classifier_proj.kernel", "classifier_proj.bias", "classifier.kernel", "classifier.bias")


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


def model_for(models, precision, dev):
    """One model per precision; the classifier is scaled up and given a bias so that the predictions move between classes."""
    if precision not in models:
        m = W().create_classification_model("tiny", num_labels=C, device=dev, precision=precision, seed=7)
        g = torch.Generator().manual_seed(3)
        m.arena.param("classifier.kernel").mul_(6.0)
        m.arena.param("classifier_proj.kernel").mul_(4.0)
        m.arena.param("classifier.bias").copy_((torch.randn(C, generator=g) * 0.2).to(dev))
        m.arena.param("classifier_proj.bias").copy_((torch.randn(m.config.classifier_proj_size, generator=g) * 0.2).to(dev))
        m.refresh_shadows()
        models[precision] = m
    return models[precision]


def clips(B, seed=5):
    return torch.from_numpy(V.create_dummy_pool(seed=seed, num_samples=B, length=T_IN))


def f64(t):
    return t.detach().double().cpu().numpy()


def head_params(m):
    return {k: m.arena.param(k).detach().cpu().numpy().copy() for k in HEAD}


def reference(m, pooled, labels, keep=None, scale=1.0, params=None):
    p = params or head_params(m)
    x = pooled.detach().cpu().numpy()
    f = R.forward(x, p[HEAD[0]], p[HEAD[1]], p[HEAD[2]], p[HEAD[3]], labels, keep, scale)
    fb = R.forward_bounds(x, p[HEAD[0]], p[HEAD[1]], p[HEAD[2]], p[HEAD[3]], f, keep, scale)
    return x, p, f, fb


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_pooled_output_is_forward_infers_and_the_head_matches_float64(dev, models, precision, ragged):
    m = model_for(models, precision, dev)
    wav2vec2 = W()
    B = 6
    x = clips(B).to(dev)
    mask = wav2vec2.frame_attention_mask(m.config, (T_IN, 3300, 1700, T_IN, 900, 2000), T_IN) if ragged else None
    labels = np.array([0, 4, -1, 2, 1, 3])
    out = m(x, attention_mask=mask, labels=labels)
    base = wav2vec2.Wav2Vec2ForPreTraining.forward_infer(m, x, attention_mask=mask, pool="mean")
    assert "logits" not in base
    assert torch.equal(out["pooled_output"], base["pooled_output"]) and out["pooled_output"].dtype == torch.float32
    assert torch.equal(out["last_hidden_state"], base["last_hidden_state"])
    assert torch.equal(m.pool_features(x, attention_mask=mask), base["pooled_output"])
    assert tuple(out["logits"].shape) == tuple(out["log_probs"].shape) == (B, C) and out["predictions"].dtype == torch.int32
    _, _, f, fb = reference(m, out["pooled_output"], labels)
    tag = f"{precision} ragged={ragged}"
    for k, name in (("logits", "logits"), ("log_probs", "log_probs"), ("nll", "nll")):
        q = R.ratio(f64(out[name]), f[k], fb[k])
        print(f"cls model {tag} {k}: {q:.4f} of its bound")
        within(f"cls model {k} / bound", q, 1.0, tag)
    pd, rd = R.decided(f, fb)
    pred, rank = out["predictions"].cpu().numpy(), out["label_rank"].cpu().numpy()
    assert np.array_equal(pred[pd], f["pred"][pd]) and np.array_equal(rank[rd], f["label_rank"][rd])
    assert np.array_equal(rank, R.label_rank(f64(out["logits"]), labels)) and rank[2] == -1 and float(out["nll"][2]) == 0.0
    n = int((labels >= 0).sum())
    loss_bound = fb["nll"].sum() / n + R.gam(B + 2) * abs(f["nll"].sum() / n) + 2.0 ** -126
    within("cls model loss / bound", abs(float(out["loss"]) - f["nll"].sum() / n) / loss_bound, 1.0, tag)
    assert tuple(out["loss"].shape) == (1,)
    # without labels: the same logits, no loss
    plain = m(x, attention_mask=mask)
    assert torch.equal(plain["logits"], out["logits"]) and "loss" not in plain and "nll" not in plain
    hs = m(x, attention_mask=mask, output_hidden_states=True, output_attentions=True)
    assert len(hs["hidden_states"]) == m.config.num_hidden_layers + 1 and len(hs["attentions"]) == m.config.num_hidden_layers


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_evaluate_sums_equal_the_items(dev, models, precision):
    m = model_for(models, precision, dev)
    B = 8
    x = clips(B, seed=9).to(dev)
    labels = torch.tensor([0, 1, 2, 3, 4, -1, 2, 0])
    ks = (1, 2, 3, C)
    r = m.evaluate(x, labels, top_k=ks, return_items=True, confusion=True)
    rank, nll, pred = r["label_rank"].cpu().numpy(), f64(r["nll"]), r["predictions"].cpu().numpy()
    valid = labels.numpy() >= 0
    assert r["n_items"] == 7 and rank[5] == -1 and nll[5] == 0.0
    assert r["nll_sum"] == float(nll.sum()) and r["loss"] == r["nll_sum"] / 7
    assert r["n_correct"] == int((rank == 0).sum()) == int(((pred == labels.numpy()) & valid).sum())
    assert r["accuracy"] == r["n_correct"] / 7
    for k in ks:
        assert r["topk_correct"][k] == int(((rank >= 0) & (rank < k)).sum())
    got = [r["topk_accuracy"][k] for k in ks]
    assert got == sorted(got) and got[0] == r["accuracy"] and got[-1] == 1.0
    want = np.zeros((C, C), dtype=np.int64)
    for lab, p_ in zip(labels.numpy()[valid], pred[valid]):
        want[lab, p_] += 1
    table = r["confusion"]
    assert table.dtype == torch.int64 and table.is_cuda and np.array_equal(table.cpu().numpy(), want)
    r2 = m.evaluate(x, labels, confusion=table)   # the previous table passed in: accumulated on the device
    assert r2["confusion"] is table and np.array_equal(table.cpu().numpy(), 2 * want)
    assert r2["nll_sum"] == r["nll_sum"] and "nll" not in r2
    # the same numbers from cached features
    e = m.evaluate_features(m.pool_features(x), labels, top_k=ks)
    assert (e["n_items"], e["nll_sum"], e["n_correct"], e["topk_correct"]) == (7, r["nll_sum"], r["n_correct"], r["topk_correct"])
    with pytest.raises(ValueError):
        m.evaluate(x, torch.tensor([0, 1, 2, 3, 4, 5, 2, 0]))
    with pytest.raises(ValueError):
        m.evaluate(x, labels, top_k=(C + 1,))


def test_training_calls_raise(dev, models):
    m = model_for(models, "bf16", dev)
    x = clips(2).to(dev)
    with pytest.raises(NotImplementedError, match="encoder fine-tuning is not built"):
        m.forward_backward(x, None)
    with pytest.raises(NotImplementedError, match="encoder fine-tuning is not built"):
        m(x, training=True)
    with pytest.raises(NotImplementedError):
        W().create_full_model("classification", "tiny", device=dev)


def test_a_pretraining_weights_file_loads(dev, tmp_path):
    from tethys_speech_amd import train
    wav2vec2 = W()
    pre = wav2vec2.create_full_model("pretraining", "tiny", device=dev, precision="bf16", seed=21)
    path = str(tmp_path / "pre.pt")
    train.save_weights(pre, path)
    m = wav2vec2.create_classification_model("tiny", num_labels=C, device=dev, precision="bf16", seed=22)
    head = {k: m.arena.param(k).clone() for k in HEAD}
    copied = wav2vec2.load_pretrained_encoder(m, path)
    dst = m.arena.ref_views(m.arena.p)
    assert set(copied) == {k for k in dst if not k.startswith(("classifier_proj.", "classifier."))} and len(copied) > 20
    for k, v in head.items():
        assert torch.equal(m.arena.param(k), v), k
    assert torch.equal(m.mirror.float(), m.arena.p.to(torch.bfloat16).float()), "the bf16 mirror was not refreshed"
    x = clips(2).to(dev)
    want = pre.forward_infer(x, pool="mean")
    got = m(x)
    assert torch.equal(got["last_hidden_state"], want["last_hidden_state"])
    assert torch.equal(got["pooled_output"], want["pooled_output"])


def snapshot(m):
    out = {n: getattr(m.arena, n).clone() for n in ("p", "m", "v")}
    if m.mirror is not None:
        out["mirror"] = m.mirror.clone()
    return out


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_five_head_steps_against_float64(dev, models, precision):
    from tethys_speech_amd import optim
    m = model_for(models, precision, dev)
    lo, hi = m.head_lo, m.head_hi
    keep0 = snapshot(m)
    try:
        rng = np.random.default_rng(31)
        feats = m.pool_features(clips(6, seed=13).to(dev))
        n_src, N, P = 6, 9, m.config.classifier_proj_size
        idx = rng.integers(0, n_src, N).astype(np.int32)
        labels = rng.integers(0, C, N).astype(np.int32)
        labels[4] = -1
        idx_d, lab_d = torch.from_numpy(idx).to(dev), torch.from_numpy(labels).to(dev)
        opt = optim.Adam(1e-3)
        m.arena.m.zero_()
        m.arena.v.zero_()
        start = snapshot(m)
        hyper = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7, eps_mode=0)
        for t in range(5):
            before = snapshot(m)
            loss = m.head_step(feats, lab_d, opt, row_index=idx_d, dropout=0.1, seed=77, step=t)
            assert tuple(loss.shape) == (1,) and loss.is_cuda
            keep, scale = R.keep_mask(77, t, N, P, 0.1)
            a = m.arena
            params = {k: before["p"][a.offsets[k]:a.offsets[k] + int(np.prod(a.shapes[k]))].view(*a.shapes[k]).cpu().numpy()
                      for k in HEAD}
            x, _, f, fb = reference(m, feats[idx_d.long()], labels, keep, scale, params)
            rg = R.backward(x, params[HEAD[2]], f, keep, scale)
            gb = R.backward_bounds(x, params[HEAD[2]], f, rg, fb, keep, scale)
            q = R.ratio(float(loss), rg["loss"], gb["loss"])
            print(f"cls step {precision} {t}: loss {float(loss):.6f}, {q:.4f} of its bound")
            within("cls step loss / bound", q, 1.0, (precision, t))
            for name, key in zip(HEAD, ("gWp", "gbp", "gWc", "gbc")):
                q = R.ratio(f64(m.arena.grad(name)), rg[key], gb[key])
                within(f"cls step {key} / bound", q, 1.0, (precision, t))
            # Keras Adam in float64 on the step's own gradients, from the state the device held
            sl = slice(lo, hi)
            tr = A.adam_terms(before["p"][sl], m.arena.g[sl], before["m"][sl], before["v"][sl], step=t + 1, **hyper)
            ab = A.adam_bounds(tr)
            for name in ("p", "m", "v"):
                q = A.bound_fraction(getattr(m.arena, name)[sl], tr[name], ab[name])
                within(f"cls step adam {name} / bound", q, 1.0, (precision, t))
            assert float((m.arena.p[sl] - before["p"][sl]).abs().max()) > 0.0
            if m.mirror is not None:
                assert torch.equal(m.mirror[sl], m.arena.p[sl].to(torch.bfloat16))
        assert opt.iterations == 5
        # every non-head parameter, moment and mirror element is bit for bit what it was
        for name, was in start.items():
            now = m.mirror if name == "mirror" else getattr(m.arena, name)
            assert torch.equal(now[:lo].view(torch.int16 if name == "mirror" else torch.int32),
                               was[:lo].view(torch.int16 if name == "mirror" else torch.int32)), name
            assert now.numel() == hi
    finally:
        for name, was in keep0.items():
            (m.mirror if name == "mirror" else getattr(m.arena, name)).copy_(was)


def test_fit_head_is_reproducible(dev, models):
    m = model_for(models, "bf16", dev)
    keep0 = snapshot(m)
    try:
        g = torch.Generator().manual_seed(5)
        feats = (torch.randn(64, m.config.hidden_size, generator=g) * 0.5).to(dev)
        labels = torch.randint(0, C, (64,), generator=g)
        runs = []
        for _ in range(2):
            for name, was in keep0.items():
                (m.mirror if name == "mirror" else getattr(m.arena, name)).copy_(was)
            m.arena.m.zero_()
            m.arena.v.zero_()
            hist = W().fit_head(m, feats, labels, epochs=2, batch_size=24, learning_rate=1e-2, seed=3,
                                eval_features=feats[:16], eval_labels=labels[:16])
            runs.append((hist, m.arena.p[m.head_lo:].clone(), m.arena.m[m.head_lo:].clone()))
        (h0, p0, m0), (h1, p1, m1) = runs
        assert h0 == h1 and len(h0) == 2 and set(h0[0]) == {"epoch", "loss", "eval_loss", "eval_accuracy"}
        assert torch.equal(p0.view(torch.int32), p1.view(torch.int32)) and torch.equal(m0.view(torch.int32), m1.view(torch.int32))
        assert not torch.equal(p0, keep0["p"][m.head_lo:]) and all(np.isfinite(h["loss"]) for h in h0)
        assert torch.equal(m.arena.p[:m.head_lo], keep0["p"][:m.head_lo])
    finally:
        for name, was in keep0.items():
            (m.mirror if name == "mirror" else getattr(m.arena, name)).copy_(was)


def test_classify_job(dev, tmp_path):
    """The CLI end to end in ONE child process on the smallest built-in size: --eval and --fit_head --epochs 1."""
    out, conf = str(tmp_path / "cls.json"), str(tmp_path / "conf.npy")
    args = [sys.executable, os.path.join(ROOT, "speech_jobs", "wav2vec2_classify.py"), "--model_size", "tiny", "--num_labels", "3",
            "--num_clips", "6", "--batch_size", "4", "--clip_samples", "4000", "--ragged", "--eval", "--top_k", "2", "--confusion",
            conf, "--fit_head", "--epochs", "1", "--out", out]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run(args, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.load(open(out))
    assert res["ragged"] is True and res["model_size"] == "tiny" and res["num_labels"] == 3
    ev = res["eval"]
    assert f"Loss: {ev['loss']:.4f}, Accuracy: {ev['accuracy']:.4f}, Top-2 accuracy: {ev['topk_accuracy']['2']:.4f}" in p.stdout
    assert ev["n_items"] == 6 and 0.0 <= ev["accuracy"] <= ev["topk_accuracy"]["2"] <= 1.0
    table = np.load(conf)
    assert table.shape == (3, 3) and int(table.sum()) == 6 and table.sum(axis=1).tolist() == [2, 2, 2]
    fit = res["fit_head"]
    assert f"Epoch 1: loss {fit['history'][0]['loss']:.4f}" in p.stdout
    assert f"Fit: loss {fit['loss']:.4f}, accuracy {fit['accuracy']:.4f}" in p.stdout and len(fit["history"]) == 1
