"""Host-side checks of the attention-weight outputs: the new entry point in the header, the binding and the library, the
argument validator of ``output_attentions``, and the float64 helper tests/_attn_probs_ref.py against the oracle's own
forwards.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import _attn_probs_ref as A
import _w2v_infer_ref as R
from oracle import wav2vec2_oracle as V
from oracle import whisper_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TINY = dict(d_model=128, encoder_attention_heads=2, decoder_attention_heads=2, d_ff=256, vocab_size=131, encoder_layers=2,
            decoder_layers=2, n_mels=8, n_ctx=96, decoder_start_token_id=130, max_target_positions=16)
SMALL_W2V = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                 conv_dim=(64, 64, 64), conv_stride=(5, 2, 2), conv_kernel=(10, 3, 2), num_conv_pos_embeddings=8,
                 num_conv_pos_embedding_groups=4, num_codevectors_per_group=16, codevector_dim=32,
                 proj_codevector_dim=64, num_negatives=10)  # the small model of tests/test_wav2vec2_gpu.py


def _lib():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib
    return _lib


# ----------------------------------------------------------------------------- the entry point
def test_entry_point_is_declared_and_bound():
    _lib_mod = _lib()
    header = open(os.path.join(ROOT, "include", "tethys_mi.h")).read()
    m = re.search(r"int\s+tmi_attn_probs\s*\(([^)]*)\)\s*;", header)
    assert m, "tmi_attn_probs is not declared in include/tethys_mi.h"
    assert [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")] == ["d", "probs", "probs_dtype", "p_sbh", "p_sq", "stream"]
    assert "tmi_attn_probs" in _lib_mod.SIGNATURES
    res, args = _lib_mod.SIGNATURES["tmi_attn_probs"]
    assert res is _lib_mod.c_i32 and len(args) == 6


def test_null_arguments_are_rejected_without_a_gpu():
    _lib_mod = _lib()
    h = _lib_mod.lib()
    assert h.tmi_attn_probs(None, None, 0, 0, 0, None) == -1
    assert b"tmi_attn_probs" in h.tmi_last_error()


def test_abi_version_is_unchanged():
    _lib_mod = _lib()
    assert _lib_mod.ABI_VERSION == 31 and _lib_mod.lib().tmi_abi_version() == 31


# ----------------------------------------------------------------------------- check_output_attentions
def test_check_output_attentions():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import whisper
    cfg = whisper.make_config("small", **TINY)
    chk = whisper.check_output_attentions
    assert chk(cfg, False) == () and chk(cfg, None) == ()
    assert chk(cfg, True) == ("encoder", "decoder", "cross")
    assert chk(cfg, ("cross",)) == ("cross",) and chk(cfg, ["cross", "encoder"]) == ("encoder", "cross")
    assert chk(cfg, {"decoder"}) == ("decoder",) and chk(cfg, ()) == ()
    for bad in (("crosss",), ("encoder", "self"), "cross", 3, 1.5, object()):
        with pytest.raises(ValueError):
            chk(cfg, bad)


def test_transcribe_cli_has_the_flag():
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "speech_jobs", "whisper_transcribe.py"), "--help"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--save_cross_attentions" in r.stdout


# ----------------------------------------------------------------------------- the helper against the oracle
def _whisper_case():
    cfg = O.make_config("small", dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, **TINY)
    p = O.init_params(cfg, seed=3, dtype=torch.float64)
    feats = torch.from_numpy(np.random.default_rng(7).standard_normal((2, 8, 140))).double()
    ids = torch.from_numpy(np.random.default_rng(8).integers(0, 130, (2, 5)))
    ids[:, 0] = cfg.decoder_start_token_id
    return cfg, p, feats, ids


def test_whisper_helper_equals_the_oracle_forward():
    cfg, p, feats, ids = _whisper_case()
    got = A.whisper_forward(p, feats, ids, cfg)
    enc = O.encoder(p, feats, cfg, training=False)
    h = O.decoder(p, ids, enc, cfg, training=False)
    assert float((got["encoder_last_hidden_state"] - enc).abs().max()) <= 1e-12
    assert float((got["last_hidden_state"] - h).abs().max()) <= 1e-12
    assert float((got["logits"] - h @ p["lm_head.kernel"]).abs().max()) <= 1e-12
    T, S = enc.shape[1], ids.shape[1]
    assert T == 70
    shapes = {"encoder_attentions": (2, 2, T, T), "decoder_attentions": (2, 2, S, S), "cross_attentions": (2, 2, S, T),
              "encoder_hidden_states": (2, T, 128), "decoder_hidden_states": (2, S, 128)}
    for k, shp in shapes.items():
        assert len(got[k]) == 2 and all(tuple(t.shape) == shp for t in got[k]), k
    for k in ("encoder_attentions", "decoder_attentions", "cross_attentions"):
        for t in got[k]:
            assert float((t.sum(-1) - 1.0).abs().max()) <= 1e-12 and float(t.min()) >= 0.0
    # layer inputs: the first is the stem / embedding output, the second what layer 0 returns
    x1 = O.encoder_layer(p, "encoder.layers.0", got["encoder_hidden_states"][0], cfg, False)
    assert float((got["encoder_hidden_states"][1] - x1).abs().max()) <= 1e-12
    y1 = O.decoder_layer(p, "decoder.layers.0", got["decoder_hidden_states"][0], enc, torch.from_numpy(O.decoder_mask(S))[None],
                         cfg, False)
    assert float((got["decoder_hidden_states"][1] - y1).abs().max()) <= 1e-12


def test_whisper_decoder_mask_rows():
    """W:416-418 inverted: row i sees keys j > i only - exact zeros at j <= i wherever a later key exists - and the last
    row, fully masked, is exactly uniform (every score is absorbed by the fp32 -1e9)."""
    cfg, p, feats, ids = _whisper_case()
    S = ids.shape[1]
    for t in A.whisper_forward(p, feats, ids, cfg)["decoder_attentions"]:
        for i in range(S - 1):
            assert float(t[:, :, i, :i + 1].abs().max()) == 0.0
            assert float((t[:, :, i, i + 1:].sum(-1) - 1.0).abs().max()) <= 1e-12
        assert bool((t[:, :, S - 1, :] == 1.0 / S).all())


def test_probs_ref_mask_modes():
    g = torch.Generator().manual_seed(4)
    q, k = (torch.randn(2, 2, 6, 64, generator=g, dtype=torch.float64).to(torch.bfloat16).double() * 0.5 for _ in range(2))
    p0 = A.probs_ref(q, k, 0, 1.0)
    p1 = A.probs_ref(q, k, 1, 1.0)
    kb = torch.tensor([[0.0] * 6, [0, 0, 0, -10000.0, -10000.0, -10000.0]], dtype=torch.float64)
    p2 = A.probs_ref(q, k, 2, 1.0, kb)
    for p in (p0, p1, p2):
        assert float((p.sum(-1) - 1.0).abs().max()) <= 1e-12
    for i in range(5):
        assert float(p1[:, :, i, :i + 1].abs().max()) == 0.0
    assert bool((p1[:, :, 5] == 1.0 / 6).all())
    assert float((p2[0] - p0[0]).abs().max()) == 0.0
    assert float(p2[1, :, :, 3:].abs().max()) == 0.0
    assert float((p2[1, :, :, :3] - torch.softmax((q[1] @ k[1, :, :3].transpose(-1, -2)), -1)).abs().max()) <= 1e-15
    # every key biased: an ordinary softmax of shifted scores
    pz = A.probs_ref(q, k, 2, 1.0, torch.full((2, 6), -10000.0, dtype=torch.float64))
    assert float((pz - p0).abs().max()) <= 1e-10


def test_w2v_helper_equals_the_restated_forward():
    cfg = V.make_config("base", **SMALL_W2V)
    p = V.init_params(cfg, seed=5, dtype=torch.float64)
    audio = torch.from_numpy(V.create_dummy_pool(seed=21, num_samples=3, length=2600)).double()
    T = 130
    lens = torch.tensor([130, 85, 17])
    mask = (torch.arange(T)[None, :] < lens[:, None]).double()
    for m in (None, mask):
        got, ref = A.w2v_forward(p, audio, cfg, m), R.forward(p, audio, cfg, m)
        assert float((got["last_hidden_state"] - ref["last_hidden_state"]).abs().max()) <= 1e-12
        assert float((got["extract_features"] - ref["extract_features"]).abs().max()) <= 1e-12
        for a, b in zip(got["hidden_states"], ref["hidden_states"]):
            assert float((a - b).abs().max()) <= 1e-12
        assert len(got["attentions"]) == cfg.num_hidden_layers
        for t in got["attentions"]:
            assert tuple(t.shape) == (3, 2, T, T) and float((t.sum(-1) - 1.0).abs().max()) <= 1e-12
            if m is not None:
                for b, n in ((1, 85), (2, 17)):  # the clips with masked keys
                    assert float(t[b, :, :, n:].abs().max()) == 0.0
