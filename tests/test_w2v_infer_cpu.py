"""Host-side checks of the Wav2Vec2 inference surface: the float64 restatement tests/_w2v_infer_ref.py itself, the frame
arithmetic of the "same"-padded stem, argument validation, and the library's new entry points.  No GPU."""
import math

import pytest
import torch

import _w2v_infer_ref as R
from oracle import wav2vec2_oracle as V


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float64) * scale


SMALL = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
             conv_dim=(64, 64, 64), conv_stride=(5, 2, 2), conv_kernel=(10, 3, 2), num_conv_pos_embeddings=8,
             num_conv_pos_embedding_groups=4, num_codevectors_per_group=16, codevector_dim=32,
             proj_codevector_dim=64, num_negatives=10)  # the small model of tests/test_wav2vec2_gpu.py


def _qkv(B=2, H=2, Tq=5, Tk=7, hd=4, seed=1):
    return rnd((B, H, Tq, hd), seed), rnd((B, H, Tk, hd), seed + 1), rnd((B, H, Tk, hd), seed + 2)


def test_masked_attention_equals_a_naive_row_loop():
    q, k, v = _qkv()
    mask = torch.tensor([[1, 1, 0.5, 0, 1, 0, 0], [0, 0, 0, 0, 0, 0, 0]], dtype=torch.float64)
    for m in (None, mask):
        got, _ = R.masked_attention(q, k, v, 0.5, m)
        assert float((got - R.masked_attention_naive(q, k, v, 0.5, m)).abs().max()) <= 1e-13


def test_prefix_mask_equals_attention_over_the_valid_keys_alone():
    q, k, v = _qkv(Tk=9)
    lens = [6, 1]
    mask = (torch.arange(9)[None, :] < torch.tensor(lens)[:, None]).double()
    got, p = R.masked_attention(q, k, v, 0.5, mask)
    for b, n in enumerate(lens):
        alone, _ = R.masked_attention(q[b:b + 1], k[b:b + 1, :, :n], v[b:b + 1, :, :n], 0.5, None)
        assert float((got[b] - alone[0]).abs().max()) <= 1e-14   # exp(-10000 + O(10)) underflows to 0 in float64 too
        assert float(p[b, :, :, n:].abs().max()) == 0.0


def test_all_zero_mask_equals_the_unmasked_softmax():
    q, k, v = _qkv()
    got, _ = R.masked_attention(q, k, v, 0.5, torch.zeros(2, 7, dtype=torch.float64))
    plain, _ = R.masked_attention(q, k, v, 0.5, None)
    # every score is shifted by the same -10000: the shift cancels up to the rounding of s - 10000 in float64 (ulp 1.8e-12)
    assert float((got - plain).abs().max()) <= 1e-10


def test_masked_mean():
    x = rnd((2, 5, 3), 9)
    mask = torch.tensor([[1, 1, 1, 0, 0], [1, 0.5, 0, 0, 0]], dtype=torch.float64)
    got = R.masked_mean(x, mask)
    assert torch.allclose(got[0], x[0, :3].mean(0), atol=1e-15)
    assert torch.allclose(got[1], (x[1, 0] + 0.5 * x[1, 1]) / 1.5, atol=1e-15)
    assert torch.allclose(R.masked_mean(x, None), x.mean(1), atol=1e-15)


def _lengths_around_stride_multiples(cfg, upto):
    total = math.prod(cfg.conv_stride)
    out = set(range(1, 40))
    for s in {cfg.conv_stride[0], cfg.conv_stride[0] * cfg.conv_stride[1], total}:
        for mult in range(1, upto // s + 1):
            out.update((mult * s - 1, mult * s, mult * s + 1))
    return sorted(n for n in out if 1 <= n <= upto)


@pytest.mark.parametrize("name,over,upto", [("base", {}, 3 * 320 + 5), ("small-test", SMALL, 20 * 20 + 5)])
def test_frame_lengths_equal_the_oracle(name, over, upto):
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import wav2vec2
    cfg, ocfg = wav2vec2.make_config("base", **over), V.make_config("base", **over)
    lengths = _lengths_around_stride_multiples(cfg, upto) + [32000, 2600, 1700, 330]
    assert wav2vec2.frame_lengths(cfg, lengths) == [V.feature_lengths(ocfg, n)[-1] for n in lengths]
    assert wav2vec2.frame_lengths(cfg, [0]) == [0]


def test_frame_attention_mask_shapes_and_values():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import wav2vec2
    cfg = wav2vec2.make_config("base", **SMALL)
    m = wav2vec2.frame_attention_mask(cfg, (2600, 1700, 330, 0), 2600)
    assert m.dtype == torch.float32 and tuple(m.shape) == (4, 130)
    assert m.sum(1).tolist() == [130.0, 85.0, 17.0, 0.0]
    for row, n in zip(m, (130, 85, 17, 0)):
        assert bool((row[:n] == 1).all()) and bool((row[n:] == 0).all())
    with pytest.raises(ValueError):
        wav2vec2.frame_attention_mask(cfg, (2601,), 2600)


def test_argument_validation():
    """Everything that is refused is refused before the model's parameters or workspaces are looked at, so an object with
    a configuration and a device alone is enough (constructing a model needs a GPU: it packs weights with a kernel)."""
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import wav2vec2
    model = object.__new__(wav2vec2.Wav2Vec2ForPreTraining)
    model.config, model.device = wav2vec2.make_config("base", **SMALL), torch.device("cpu")
    x = torch.zeros(2, 2600)
    with pytest.raises(ValueError, match="attention_mask must be"):
        model(x, attention_mask=torch.ones(2, 129), training=False)
    with pytest.raises(ValueError, match="attention_mask must be"):
        model(x, attention_mask=torch.ones(130), training=False)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        model(x, attention_mask=torch.full((2, 130), 2.0), training=False)
    with pytest.raises(ValueError, match="pool"):
        model(x, pool="max", training=False)
    with pytest.raises(ValueError, match="inference call"):
        model(x, neg_indices=torch.zeros(2, 10, dtype=torch.int32), attention_mask=torch.ones(2, 130), training=True)
    with pytest.raises(ValueError, match="neg_indices"):
        model(x, training=True)
    with pytest.raises(TypeError):
        model(x.double(), training=False)


def test_library_exports_the_new_entry_points():
    import ctypes
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib
    h = _lib.lib()
    for name in ("tmi_softmax_bias_fwd", "tmi_masked_mean_pool"):
        assert name in _lib.SIGNATURES and hasattr(h, name)
    assert _lib.ABI_VERSION == 31 and h.tmi_abi_version() == 31
    fields = [n for n, _ in _lib.AttnDesc._fields_]
    assert fields[-2:] == ["key_bias", "kb_sb"] and _lib.AttnDesc.key_bias.offset == ctypes.sizeof(_lib.AttnDesc) - 16
    # refused without a launch: no pointers at all
    assert h.tmi_softmax_bias_fwd(None, 4, 2, 2, 1, None, 0, None) == -1
    assert h.tmi_masked_mean_pool(None, 0, None, None, 1, 1, 4, None) == -1
