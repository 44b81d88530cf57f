"""The weighted training loss (decoder_attention_mask, W:596-598) without a GPU: the fp64 reference of the GPU tests against
autograd and against the oracle's unweighted loss, the masked dummy dataset, the host-side argument checks and the new C
entry points in the built library."""
import inspect

import numpy as np
import pytest
import torch

import _masked_loss_ref as M
from oracle import whisper_oracle as O

KW = dict(d_model=32, encoder_attention_heads=2, decoder_attention_heads=2, d_ff=64, vocab_size=120, encoder_layers=1,
          decoder_layers=1, n_mels=8, n_ctx=16, decoder_start_token_id=110, max_target_positions=16)


def _mask(B, S, seed=3):
    """0/1 entries, the fractional weights 0.5 and 2.0, a zero at t = 0, one all-zero sample, a nonzero last column."""
    rng = np.random.default_rng(seed)
    m = (rng.random((B, S)) < 0.6).astype(np.float64)
    m[0, 0], m[0, 1], m[0, 2], m[0, 3] = 0.0, 0.5, 2.0, 1.0
    m[1] = 0.0
    m[:, -1] = 1.0
    return m


def test_closed_form_gradient_equals_autograd():
    B, S, V = 3, 7, 19
    g = torch.Generator().manual_seed(1)
    z = torch.randn(B, S, V, generator=g, dtype=torch.float64) * 2.0
    labels = torch.randint(0, V, (B, S), generator=g, dtype=torch.int32)
    mask = _mask(B, S)
    for scale in (1.0, 0.37):
        loss, d = M.weighted_xent(z, labels, mask, scale)
        leaf = z.clone().requires_grad_(True)
        w = torch.from_numpy(mask)[:, :-1]
        nll = torch.nn.functional.cross_entropy(leaf[:, :-1].reshape(-1, V), labels[:, 1:].long().reshape(-1),
                                                reduction="none").reshape(B, S - 1)
        ref = (nll * w).sum() / w.sum()
        (ref * scale).backward()
        assert abs(loss - float(ref.detach())) <= 1e-12
        assert float((d - leaf.grad).abs().max()) <= 1e-12
        assert float(d[:, -1].abs().max()) == 0.0 and float(d[1].abs().max()) == 0.0


def test_unscored_rows_may_hold_anything_and_the_last_mask_column_is_ignored():
    B, S, V = 3, 6, 11
    g = torch.Generator().manual_seed(2)
    z = torch.randn(B, S, V, generator=g, dtype=torch.float64)
    labels = torch.randint(0, V, (B, S), generator=g, dtype=torch.int32)
    mask = _mask(B, S)
    loss, d = M.weighted_xent(z, labels, mask)
    other = mask.copy()
    other[:, -1] = 0.0
    loss2, d2 = M.weighted_xent(z, labels, other)
    assert loss2 == loss and torch.equal(d, d2)
    bad = z.clone()
    bad[torch.from_numpy(M.weights_of(mask).numpy() == 0)] = float("nan")
    bad[1, 0] = float("inf")
    loss3, d3 = M.weighted_xent(bad, labels, mask)
    assert loss3 == loss and torch.equal(d, d3)


def test_zero_sum_convention():
    B, S, V = 2, 5, 7
    z = torch.randn(B, S, V, dtype=torch.float64)
    labels = torch.zeros(B, S, dtype=torch.int32)
    mask = np.zeros((B, S))
    mask[:, -1] = 1.0  # (only the ignored column)
    loss, d = M.weighted_xent(z, labels, mask)
    assert loss == 0.0 and float(d.abs().max()) == 0.0
    cfg = O.make_config("small", dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, **KW)
    p = O.init_params(cfg, seed=1, dtype=torch.float64)
    feats, lab = O.create_dummy_pool(seed=1, n_mels=8, seq_len=16, max_target_length=5, num_samples=2)
    l0, g0 = M.loss_and_grads(p, torch.from_numpy(feats), torch.from_numpy(lab), mask, cfg)
    assert float(l0) == 0.0 and all(float(v.abs().max()) == 0.0 for v in g0.values())


def test_all_ones_mask_is_the_oracles_plain_mean():
    cfg = O.make_config("small", dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, **KW)
    p = O.init_params(cfg, seed=2, dtype=torch.float64)
    feats, lab = O.create_dummy_pool(seed=2, n_mels=8, seq_len=16, max_target_length=6, num_samples=3)
    f, l = torch.from_numpy(feats), torch.from_numpy(lab)
    l_ref, g_ref = O.loss_and_grads(p, f, l, cfg)
    l_got, g_got = M.loss_and_grads(p, f, l, np.ones(lab.shape), cfg)
    assert abs(float(l_got) - float(l_ref)) <= 1e-12
    assert max(float((g_got[k] - g_ref[k]).abs().max()) for k in g_ref) <= 1e-12
    # and the closed form on the oracle's logits is what autograd sends into them
    _, logits = O.forward_loss(p, f, l, cfg)
    mask = _mask(3, 6)
    loss_c, _ = M.weighted_xent(logits.detach(), lab, mask)
    loss_a, _ = M.forward_loss(p, f, l, mask, cfg)
    assert abs(loss_c - float(loss_a)) <= 1e-12
    # train_steps with all-ones masks is O.train_steps
    import copy
    a, _ = O.train_steps(cfg, copy.deepcopy(p), feats, lab, 2, 3, lr=1e-3)
    b, _ = M.train_steps(cfg, copy.deepcopy(p), feats, lab, np.ones(lab.shape), 2, 3, lr=1e-3)
    assert max(abs(x - y) for x, y in zip(a, b)) <= 1e-12


def _data():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import data
    return data


@pytest.mark.parametrize("world", [1, 2])
def test_masked_dummy_dataset(world):
    data = _data()
    kw = dict(n_mels=4, seq_len=8, max_target_length=60, device="cpu", seed=5, num_samples=8)
    _, pool_labels = data.make_pool(5, 4, 8, 60, 8)
    assert (pool_labels == 0).any()
    seen = []
    for rank in range(world):
        ds = data.create_dummy_dataset(3, rank=rank, world=world, with_mask=True, **kw)
        plain = data.create_dummy_dataset(3, rank=rank, world=world, **kw)
        sizes = []
        for _ in range(5):
            f, l, m = next(ds)
            pf, pl = next(plain)  # with_mask=False: the tuples of today
            assert torch.equal(f, pf) and torch.equal(l, pl)
            assert m.dtype == torch.float32 and m.shape == l.shape and m.device == l.device
            assert torch.equal(m, (l != 0).to(torch.float32))
            sizes.append(int(l.shape[0]))
        seen.append(sizes)
    # pool of 8: world 1 sees 3, 3, 2 (the short final batch); world 2 (global batch 6) sees 3+3, then 2+0
    assert seen == ([[3, 3, 2, 3, 3]] if world == 1 else [[3, 2, 3, 2, 3], [3, 0, 3, 0, 3]])
    assert len(next(data.create_dummy_dataset(3, **kw))) == 2
    assert len(next(data.DummyDataset(3, **kw, with_mask=False))) == 2


def test_host_side_argument_errors():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import train, whisper
    cfg = whisper.make_config("small", **KW)
    ok = whisper.prepare_loss_mask(cfg, (2, 5), np.array([[1, 1, 0, 0, 1]] * 2, dtype=bool), "cpu")
    assert ok.dtype == torch.float32 and ok.tolist() == [[1.0, 1.0, 0.0, 0.0, 1.0]] * 2
    assert whisper.prepare_loss_mask(cfg, (2, 5), torch.tensor([[0.5, 2.0, 0, 0, 0]] * 2), "cpu").dtype == torch.float32
    assert float(whisper.prepare_loss_mask(cfg, (2, 5), np.zeros((2, 5)), "cpu").sum()) == 0.0  # all-zero: defined, no error
    with pytest.raises(ValueError):
        whisper.prepare_loss_mask(cfg, (2, 5), np.ones((2, 4)), "cpu")
    with pytest.raises(ValueError):
        whisper.prepare_loss_mask(cfg, (2, 5), np.ones((5,)), "cpu")
    with pytest.raises(ValueError):
        whisper.prepare_loss_mask(cfg, (2, 5), -np.ones((2, 5)), "cpu")
    with pytest.raises(ValueError):
        whisper.prepare_loss_mask(cfg, (2, 1), np.ones((2, 1)), "cpu")  # S = 1 leaves no scored row
    with pytest.raises(TypeError):
        whisper.prepare_loss_mask(cfg, (2, 5), np.ones((2, 5), dtype=np.complex64), "cpu")
    with pytest.raises(TypeError):
        whisper.prepare_loss_mask(cfg, (2, 5), np.array([["a"] * 5] * 2), "cpu")
    with pytest.raises(ValueError):
        train.distributed_train_step(None, None, (1, 2, 3, 4), None)
    with pytest.raises(ValueError):
        train.distributed_train_step(None, None, (1,), None)

    class OneReplica:
        world = 1
    with pytest.raises(ValueError, match="decoder_attention_mask"):
        train.GraphedTrainStep(OneReplica(), None, None, (1, 2, 3))
    sig = inspect.signature(whisper.WhisperForConditionalGeneration.forward_backward).parameters
    assert list(sig)[1:] == ["features", "labels", "loss_scale", "grad_ready", "early_update", "decoder_attention_mask"]
    assert sig["decoder_attention_mask"].default is None
    assert inspect.signature(train.train_whisper).parameters["mask_padding"].default is False
    assert "decoder_attention_mask" in inspect.signature(whisper.WhisperForConditionalGeneration.__call__).parameters


def test_library_has_the_weighted_entry_points():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib
    h = _lib.lib()
    for name in ("tmi_xent_weights", "tmi_xent_weighted", "tmi_linear_xent_weighted", "tmi_sum_scale_dev"):
        assert name in _lib.SIGNATURES and hasattr(h, name)
    # null arguments are rejected before any launch
    assert h.tmi_xent_weights(None, 0, 0, 0, None, None, None) == -1 and b"tmi_xent_weights" in h.tmi_last_error()
    assert h.tmi_xent_weighted(None, 0, None, None, None, None, 0, 0, 0, 1.0, 0, None) == -1
    assert h.tmi_linear_xent_weighted(None, 0, None, 0, 0, 0, None, 0, None, None, None, None, 0, 0, 0, 1.0, 0, None) == -1
    assert h.tmi_sum_scale_dev(None, None, 0, None, None) == -1 and b"tmi_sum_scale_dev" in h.tmi_last_error()
