"""The reference and bounds of tests/_cls_ref.py, and the host side of Wav2Vec2ForSequenceClassification, without a GPU:
the float64 gradients against central finite differences, closed forms (one class, uniform logits, hand-made ties), the
bounds against an honest fp32 transcription, check_classification_args' refusals, the config per size, the arena layout
and the new symbols of the binding and the header."""
import math
import os
import re

import numpy as np
import pytest
import torch

import _cls_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _W():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import wav2vec2 as W
    return W


def _case(N=5, H=8, P=6, C=4, seed=3, p=0.0, all_labelled=False):
    d = R.head_inputs(N, H, P, C, seed)
    if all_labelled:
        d["labels"] = np.where(d["labels"] < 0, 0, d["labels"])
    keep, scale = (None, 1.0) if p == 0.0 else R.keep_mask_seed(1234, N, P, p)
    return d, keep, scale


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_reference_gradients_against_central_differences(p):
    d, keep, scale = _case(p=p)
    f = R.forward(d["x"], d["Wp"], d["bp"], d["Wc"], d["bc"], d["labels"], keep, scale)
    g = R.backward(d["x"], d["Wc"], f, keep, scale)
    assert g["n_valid"] == int((d["labels"] >= 0).sum()) and 0 < g["n_valid"] < len(d["labels"])
    assert abs(g["loss"] - R.loss_of(d["x"], d["Wp"], d["bp"], d["Wc"], d["bc"], d["labels"], keep, scale)) < 1e-15
    eps = 1e-6
    for name, key in (("Wp", "gWp"), ("bp", "gbp"), ("Wc", "gWc"), ("bc", "gbc")):
        base = R.f64(d[name])
        num = np.zeros_like(base)
        for idx in np.ndindex(base.shape):
            hi, lo = base.copy(), base.copy()
            hi[idx] += eps
            lo[idx] -= eps
            kw_hi, kw_lo = dict(d, **{name: hi}), dict(d, **{name: lo})
            num[idx] = (R.loss_of(kw_hi["x"], kw_hi["Wp"], kw_hi["bp"], kw_hi["Wc"], kw_hi["bc"], d["labels"], keep, scale) -
                        R.loss_of(kw_lo["x"], kw_lo["Wp"], kw_lo["bp"], kw_lo["Wc"], kw_lo["bc"], d["labels"], keep, scale)) / (2 * eps)
        assert np.abs(num - g[key]).max() <= 1e-9, (name, np.abs(num - g[key]).max())


def test_one_class_has_zero_loss_and_zero_gradients():
    d, _, _ = _case(C=1, all_labelled=True)
    f = R.forward(d["x"], d["Wp"], d["bp"], d["Wc"], d["bc"], d["labels"])
    g = R.backward(d["x"], d["Wc"], f)
    assert np.all(f["nll"] == 0.0) and np.all(f["pred"] == 0) and np.all(f["label_rank"] == 0)
    for k in ("gWp", "gbp", "gWc", "gbc"):
        assert np.all(g[k] == 0.0)


def test_uniform_logits_give_log_c():
    d, _, _ = _case(C=7, all_labelled=True)
    d["Wc"][:] = 0.0
    d["bc"][:] = 0.25
    f = R.forward(d["x"], d["Wp"], d["bp"], d["Wc"], d["bc"], d["labels"])
    assert np.abs(f["nll"] - math.log(7)).max() < 1e-15
    assert np.all(f["pred"] == 0) and np.array_equal(f["label_rank"], d["labels"])   # every class ties: the rank is the index


def test_label_rank_on_hand_made_ties():
    lg = np.array([[1.0, 3.0, 3.0, 2.0, 3.0],
                   [0.0, -0.0, 0.0, 0.0, 0.0],
                   [5.0, 4.0, 3.0, 2.0, 1.0]])
    assert R.label_rank(lg, [1, 0, 0]).tolist() == [0, 0, 0]
    assert R.label_rank(lg, [2, 1, 4]).tolist() == [1, 1, 4]     # (-0 ties with +0)
    assert R.label_rank(lg, [4, 4, 2]).tolist() == [2, 4, 2]
    assert R.label_rank(lg, [0, -1, 5]).tolist() == [4, -1, -1]  # unlabelled: outside [0, C)
    r = R.label_rank(lg, [3, 2, 1])
    assert r.tolist() == [3, 2, 1] and all((r == 0) == (np.argmax(lg, axis=1) == np.array([3, 2, 1])))


def test_unlabelled_rows_score_zero_and_all_unlabelled_has_no_gradient():
    d, _, _ = _case()
    lab = np.full_like(d["labels"], -1)
    f = R.forward(d["x"], d["Wp"], d["bp"], d["Wc"], d["bc"], lab)
    g = R.backward(d["x"], d["Wc"], f)
    assert np.all(f["nll"] == 0.0) and np.all(f["label_rank"] == -1) and g["n_valid"] == 0 and g["loss"] == 0.0
    assert all(np.all(g[k] == 0.0) for k in ("gWp", "gbp", "gWc", "gbc", "dpre"))


def _fp32_transcription(d, keep, scale):
    """The kernel's operations in numpy float32, one rounding per operation (no fused multiply-add: more roundings than the
    kernel makes, so it must still be inside the bounds)."""
    f32 = np.float32
    x, Wp, bp, Wc, bc = (np.asarray(d[k], dtype=f32) for k in ("x", "Wp", "bp", "Wc", "bc"))
    N, H = x.shape
    P, C = Wc.shape
    pre = np.zeros((N, P), dtype=f32)
    for h in range(H):
        pre = pre + x[:, h:h + 1] * Wp[h][None, :]
    z = np.tanh(pre + bp).astype(f32)
    y = z if keep is None else np.where(keep, z * f32(scale), f32(0))
    lg = np.zeros((N, C), dtype=f32)
    for c in range(P):
        lg = lg + y[:, c:c + 1] * Wc[c][None, :]
    lg = lg + bc
    m = lg.max(axis=1, keepdims=True)
    s = np.zeros((N, 1), dtype=f32)
    for k in range(C):
        s = s + np.exp(lg[:, k:k + 1] - m).astype(f32)
    lse = m + np.log(s).astype(f32)
    return dict(z=z, logits=lg, log_probs=lg - lse)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_forward_bounds_hold_an_fp32_transcription_and_see_an_off_by_a_few_ulp_error(p):
    d, keep, scale = _case(N=9, H=100, P=62, C=7, seed=11, p=p)
    f = R.forward(d["x"], d["Wp"], d["bp"], d["Wc"], d["bc"], d["labels"], keep, scale)
    fb = R.forward_bounds(d["x"], d["Wp"], d["bp"], d["Wc"], d["bc"], f, keep, scale)
    got = _fp32_transcription(d, keep, scale)
    for k in ("z", "logits", "log_probs"):
        q = R.ratio(got[k], f[k], fb[k])
        assert 0.0 < q <= 1.0, (k, q)
    # worst-case bounds of dot products of length 100 and 62 are loose, but they still see a bf16 rounding of the logits
    # (2^-9 relative) and a dropped bias
    assert R.ratio(f["logits"] * (1 + 2.0 ** -9), f["logits"], fb["logits"]) > 1.0
    assert R.ratio(f["logits"] - R.f64(d["bc"]), f["logits"], fb["logits"]) > 1.0


def test_check_classification_args_refusals():
    W = _W()
    cfg = W.make_config("tiny", num_labels=5)
    T = W.frame_lengths(cfg, [4000])[0]
    B, T2, lab, ks = W.check_classification_args(cfg, (3, 4000), [0, 4, -1], torch.ones(3, T), top_k=(1, 5))
    assert (B, T2, ks) == (3, T, (1, 5)) and lab.dtype == torch.int32 and lab.tolist() == [0, 4, -1]
    assert W.check_classification_args(cfg, (3, 4000))[2] is None
    for kw in (dict(labels=[0, 5, 1]), dict(labels=[0, -2, 1]), dict(labels=[0, 1]), dict(labels=torch.ones(3)),
               dict(labels=torch.zeros(3, 1, dtype=torch.int64)), dict(top_k=(0,)), dict(top_k=(6,)), dict(top_k=()),
               dict(top_k=(1, 1)), dict(top_k=(1.0,)), dict(attention_mask=torch.ones(3, T + 1)),
               dict(attention_mask=torch.ones(2, T))):
        with pytest.raises(ValueError):
            W.check_classification_args(cfg, (3, 4000), **kw)
    for shape in ((0, 4000), (3, 0), (3,), (65536, 4000)):
        with pytest.raises(ValueError):
            W.check_classification_args(cfg, shape)
    for over in (dict(num_labels=0), dict(num_labels=1025), dict(classifier_proj_size=63), dict(classifier_proj_size=1026),
                 dict(hidden_size=4100, num_attention_heads=4), dict(hidden_size=258, num_attention_heads=2)):
        with pytest.raises(ValueError):
            W.check_classification_args(W.make_config("tiny", **over), (3, 4000))
    assert W.check_classification_args(W.make_config("tiny", num_labels=1024, classifier_proj_size=1024), (65535, 1))[0] == 65535


def test_config_values_per_size():
    W = _W()
    assert (W.Wav2Vec2Config().classifier_proj_size, W.Wav2Vec2Config().num_labels) == (256, 2)
    assert W.make_config("base").classifier_proj_size == 256
    assert W.make_config("small").classifier_proj_size == 128
    assert W.make_config("tiny").classifier_proj_size == 64
    assert W.make_config("tiny", num_labels=7).num_labels == 7 and W.make_config("small").num_labels == 2
    assert W.SITE_CLS == 5 == R.SITE_CLS
    assert len({W.SITE_FE, W.SITE_FP, W.SITE_PH, W.SITE_PQ, W.SITE_CLS}) == 5


def test_arena_layout_the_head_is_the_contiguous_tail():
    W = _W()
    cfg = W.make_config("tiny", num_labels=7)
    H, P = cfg.hidden_size, cfg.classifier_proj_size
    pre, ctc, cls = W.W2VArena(cfg, "cpu"), W.W2VArena(cfg, "cpu", head="ctc"), W.W2VArena(cfg, "cpu", head="classification")
    head = ["classifier_proj.kernel", "classifier_proj.bias", "classifier.kernel", "classifier.bias"]
    base = ctc.names[:-2]
    assert cls.names == base + head
    assert all(cls.shapes[n] == ctc.shapes[n] and cls.offsets[n] == ctc.offsets[n] for n in base)
    assert [cls.shapes[n] for n in head] == [(H, P), (P,), (P, 7), (7,)]
    lo = cls.offsets[head[0]]
    assert lo == ctc.offsets["lm_head.kernel"] and all(cls.offsets[n] >= lo for n in head)
    assert max(cls.offsets[n] + int(np.prod(cls.shapes[n])) for n in base) <= lo
    pos = lo
    for n in head:   # nothing but alignment padding between the head's tensors, and the arena ends with them
        assert cls.offsets[n] == pos
        pos += (int(np.prod(cls.shapes[n])) + 7) // 8 * 8
    assert pos == cls.numel
    # the two existing arenas are what they were (the sizes of the parent commit, tiny config)
    other = W.make_config("tiny")
    assert W.W2VArena(other, "cpu").numel == W.W2VArena(cfg, "cpu").numel == pre.numel
    assert W.W2VArena(other, "cpu", head="ctc").numel == ctc.numel
    assert "classifier.kernel" not in pre.names and "classifier.kernel" not in ctc.names
    # Keras defaults: glorot kernels inside their limit, zero biases; the base model's draws do not depend on the head
    cls.init_keras_defaults(7)
    ctc.init_keras_defaults(7)
    assert torch.equal(cls.p[:lo], ctc.p[:lo])
    for n, lim in ((head[0], math.sqrt(6.0 / (H + P))), (head[2], math.sqrt(6.0 / (P + 7)))):
        w = cls.param(n)
        assert float(w.abs().max()) <= lim and float(w.abs().max()) > 0.5 * lim
    assert float(cls.param(head[1]).abs().max()) == 0.0 and float(cls.param(head[3]).abs().max()) == 0.0


def test_binding_and_header_have_the_new_symbols():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib
    header = open(os.path.join(ROOT, "include", "tethys_mi.h")).read()
    want = {"tmi_cls_head_workspace_bytes": 4, "tmi_cls_head_fwd": 27, "tmi_cls_head_bwd": 24}
    for name, nargs in want.items():
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\);", header)
        assert m is not None, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == nargs, name
    assert _lib.ABI_VERSION == 31
    assert "label_rank" in header and "n_valid" in header


def test_factories():
    W = _W()
    with pytest.raises(NotImplementedError):
        W.create_full_model("classification", "tiny", device="cpu")   # the pinned refusal stays
    assert callable(W.create_classification_model) and issubclass(W.Wav2Vec2ForSequenceClassification, W.Wav2Vec2ForPreTraining)
    assert W.Wav2Vec2ForSequenceClassification._arena_head == "classification"
