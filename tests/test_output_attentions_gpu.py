"""``output_attentions`` / ``output_hidden_states`` of the two inference calls against the float64 forwards of
tests/_attn_probs_ref.py.  These tests check wiring - which layer, which buffer, which mask, which scale - where a mistake
is of order 1, so the tensors are held to the caps the project states for these classes at the top of
tests/test_wav2vec2_gpu.py as they stand: fp32 1e-4 relative max, bf16 6e-2 relative L2, per tensor.  The measured values
go through ``_margins.within``; the kernel's own precision is the business of tests/test_attn_probs_gpu.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _attn_probs_ref as A  # noqa: E402
from _margins import within  # noqa: E402
from oracle import wav2vec2_oracle as V  # noqa: E402
from oracle import whisper_oracle as O  # noqa: E402
from test_w2v_infer_gpu import B_M, CAP, SAMPLE_LENGTHS, T_IN, model_err, ref_params  # noqa: E402
from test_wav2vec2_gpu import build  # noqa: E402

BF = torch.bfloat16
TINY = dict(d_model=128, encoder_attention_heads=2, decoder_attention_heads=2, d_ff=256, vocab_size=131, encoder_layers=2,
            decoder_layers=2, n_mels=8, n_ctx=96, decoder_start_token_id=130, max_target_positions=16)
W_B, W_TIN, W_T, W_S = 2, 140, 70, 5
_CACHE = {}


def _whisper_setup():
    if "w" not in _CACHE:
        ocfg = O.make_config("small", dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, **TINY)
        params = O.init_params(ocfg, seed=3, dtype=torch.float64)
        feats = torch.from_numpy(np.random.default_rng(7).standard_normal((W_B, 8, W_TIN)).astype(np.float32))
        ids = torch.from_numpy(np.random.default_rng(8).integers(0, 130, (W_B, W_S)).astype(np.int32))
        ids[:, 0] = ocfg.decoder_start_token_id
        _CACHE["w"] = (ocfg, params, feats, ids)
    return _CACHE["w"]


def _whisper_ref(precision):
    """The float64 forward on the values the kernels read (bf16: the kernels rounded to bf16), once per precision."""
    key = ("wref", precision)
    if key not in _CACHE:
        ocfg, params, feats, ids = _whisper_setup()
        p = dict(params)
        if precision == "bf16":
            p = {k: (v.to(BF).double() if k.endswith(".kernel") else v) for k, v in p.items()}
        _CACHE[key] = A.whisper_forward(p, feats.double(), ids, ocfg)
    return _CACHE[key]


def _whisper_model(dev, precision):
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import whisper
    _, params, _, _ = _whisper_setup()
    m = whisper.create_whisper_model("small", device=dev, precision=precision, seed=1234, **TINY)
    m.arena.load_ref({k: v.float() for k, v in params.items()})
    m.refresh_shadows()
    return m


WHISPER_SHAPES = {"encoder_attentions": (W_B, 2, W_T, W_T), "decoder_attentions": (W_B, 2, W_S, W_S),
                  "cross_attentions": (W_B, 2, W_S, W_T), "encoder_hidden_states": (W_B, W_T, 128),
                  "decoder_hidden_states": (W_B, W_S, 128)}
NEW_KEYS = set(WHISPER_SHAPES)


def _compare(tag, precision, got, ref):
    for i, (g, r) in enumerate(zip(got, ref)):
        assert tuple(g.shape) == tuple(r.shape), (tag, i, tuple(g.shape))
        assert bool(torch.isfinite(g.float()).all()), (tag, i)
        e = model_err(precision, g, r)
        print(f"{tag} {precision} layer {i}: {e:.3e}")
        within(f"{tag} {precision}", e, CAP[precision])


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_whisper_outputs_match_float64(dev, precision):
    _, _, feats, ids = _whisper_setup()
    ref = _whisper_ref(precision)
    model = _whisper_model(dev, precision)
    f, dec = feats.to(dev), ids.to(dev)
    plain = model(f, decoder_input_ids=dec, training=False)
    assert not (NEW_KEYS & set(plain))
    out = model(f, decoder_input_ids=dec, training=False, output_attentions=True, output_hidden_states=True)
    torch.cuda.synchronize()
    assert set(out) == set(plain) | NEW_KEYS
    for k in ("logits", "last_hidden_state", "encoder_last_hidden_state"):  # the call's other outputs: bit for bit
        assert torch.equal(out[k], plain[k]), k
        within(f"output_attentions whisper {k} {precision}", model_err(precision, out[k], ref[k]), CAP[precision])
    for k, shp in WHISPER_SHAPES.items():
        assert isinstance(out[k], tuple) and len(out[k]) == 2, k
        assert all(tuple(t.shape) == shp and t.dtype == model.dtype for t in out[k]), k
        _compare(f"output_attentions whisper {k}", precision, out[k], ref[k])
    for t in out["decoder_attentions"]:  # the inverted mask: exact zeros at keys j <= i of every row that has a later key
        for i in range(W_S - 1):
            assert int(t[:, :, i, :i + 1].count_nonzero()) == 0, i
        assert float((t[:, :, W_S - 1].float() - 1.0 / W_S).abs().max()) <= 1e-2 / W_S
    # the layer inputs are copies, not views of the shared workspace: layer 0's differs from layer 1's
    assert not torch.equal(out["encoder_hidden_states"][0], out["encoder_hidden_states"][1])
    # selections: only the keys asked for, the same tensors
    for sel, keys in ((("cross",), {"cross_attentions"}), (["decoder", "encoder"], {"encoder_attentions", "decoder_attentions"}),
                      (False, set())):
        o2 = model.forward_infer(f, decoder_input_ids=dec, output_attentions=sel)
        assert set(o2) == set(plain) | keys, sel
        for k in keys:
            assert all(torch.equal(a, b) for a, b in zip(o2[k], out[k])), k
        assert torch.equal(o2["logits"], plain["logits"])
    o3 = model.forward_infer(f, decoder_input_ids=dec, output_hidden_states=True)
    assert set(o3) == set(plain) | {"encoder_hidden_states", "decoder_hidden_states"}
    # fp32 weights from the bf16 model; the compute dtype otherwise
    o4 = model.forward_infer(f, decoder_input_ids=dec, output_attentions=("cross", "decoder"), attentions_dtype=torch.float32)
    assert all(t.dtype == torch.float32 for k in ("cross_attentions", "decoder_attentions") for t in o4[k])
    _compare("output_attentions whisper cross_attentions as fp32", precision, o4["cross_attentions"], ref["cross_attentions"])
    if precision == "bf16":
        for a, b in zip(o4["cross_attentions"], out["cross_attentions"]):
            assert torch.equal(a.to(BF), b), "the bf16 weights are the fp32 ones rounded once"
    torch.cuda.synchronize()


def test_whisper_argument_checks(dev):
    _, _, feats, ids = _whisper_setup()
    model = _whisper_model(dev, "bf16")
    f = feats.to(dev)
    labels = torch.randint(0, 130, (W_B, 6), dtype=torch.int32, device=dev)
    for kw in (dict(output_attentions=True), dict(output_hidden_states=True), dict(attentions_dtype=torch.float32)):
        with pytest.raises(ValueError):
            model(f, labels=labels, training=True, **kw)
    with pytest.raises(ValueError):
        model.forward_infer(f, decoder_input_ids=ids.to(dev), output_attentions=("self",))
    with pytest.raises(ValueError):
        model.forward_infer(f, decoder_input_ids=ids.to(dev), output_attentions=True, attentions_dtype=torch.float16)


def test_output_attentions_between_training_steps_changes_nothing(dev):
    """Two training steps with Adam (bf16, dropout on, deterministic); in the second run an ``output_attentions`` call -
    another batch size - sits between them: losses, parameters and Adam moments bit for bit the same."""
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import ops, optim, train, whisper
    from tethys_speech_amd.data import create_dummy_dataset
    from tethys_speech_amd.dist import DataParallelStrategy
    tiny = dict(TINY, vocab_size=160, n_mels=16, decoder_start_token_id=150, max_target_positions=32)

    def run(infer):
        model = whisper.create_whisper_model("small", device=dev, precision="bf16", seed=5, **tiny)
        model.enable_dropout(0.1, 0.1, seed=77)
        opt = optim.Adam(1e-3)
        it = iter(create_dummy_dataset(3, n_mels=16, seq_len=96, max_target_length=12, device=dev, seed=9, num_samples=8))
        step = train.planned_step(DataParallelStrategy(0, 1, init=False), model, opt, "whisper", pipelined=True)
        gfeats = torch.from_numpy(np.random.default_rng(1).standard_normal((2, 16, 80)).astype(np.float32)).to(dev)
        dec = torch.tensor([[150, 3, 4, 5], [150, 7, 8, 9]], dtype=torch.int32, device=dev)
        losses = []
        for i in range(3):
            losses.append(step(*next(it)))
            if infer:
                before = (model._drop_step, model._ws_key)
                out = model(gfeats, decoder_input_ids=dec, training=False, output_attentions=True, output_hidden_states=True)
                assert len(out["cross_attentions"]) == 2 and (model._drop_step, model._ws_key) == before
        model.finish_late()
        torch.cuda.synchronize()
        return [float(x.item()) for x in losses], model.arena.p.clone(), model.arena.m.clone()

    was, old = ops.set_deterministic(True), train.USE_PLAN
    train.USE_PLAN = False
    try:
        l0, p0, m0 = run(False)
        l1, p1, m1 = run(True)
    finally:
        train.USE_PLAN = old
        ops.set_deterministic(was)
    assert l0 == l1, (l0, l1)
    assert torch.equal(p0, p1) and torch.equal(m0, m1)


# ----------------------------------------------------------------------------- Wav2Vec2
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_wav2vec2_attentions_match_float64(dev, precision):
    from tethys_speech_amd import wav2vec2
    model, ocfg, _ = build(precision, dev)
    clips = torch.from_numpy(V.create_dummy_pool(seed=21, num_samples=B_M, length=T_IN))
    mask = wav2vec2.frame_attention_mask(model.config, SAMPLE_LENGTHS, T_IN)
    assert mask.sum(1).tolist() == [130.0, 85.0, 17.0]
    p = ref_params(model, precision)
    for tag, m in (("masked", mask), ("unmasked", None)):
        ref = A.w2v_forward(p, clips.double(), ocfg, None if m is None else m.double())
        plain = model(clips.to(dev), attention_mask=m, training=False)
        assert "attentions" not in plain
        out = model(clips.to(dev), attention_mask=m, training=False, output_attentions=True, output_hidden_states=True)
        torch.cuda.synchronize()
        assert set(out) == set(plain) | {"attentions", "hidden_states"}
        for k in ("last_hidden_state", "extract_features"):
            assert torch.equal(out[k], plain[k]), k
        att = out["attentions"]
        assert isinstance(att, tuple) and len(att) == ocfg.num_hidden_layers
        assert all(tuple(t.shape) == (B_M, 2, 130, 130) and t.dtype == model.dtype for t in att)
        _compare(f"output_attentions w2v {tag} attentions", precision, att, ref["attentions"])
        _compare(f"output_attentions w2v {tag} hidden_states", precision, out["hidden_states"], ref["hidden_states"])
        if m is not None:  # the columns of masked keys, for the clips that also have unmasked ones
            for t in att:
                assert float(t[1, :, :, 85:].float().abs().max()) < 1e-30 and float(t[2, :, :, 17:].float().abs().max()) < 1e-30
                assert float((t[1, :, :, :85].float().sum(-1) - 1.0).abs().max()) < 2e-2
        o32 = model.forward_infer(clips.to(dev), attention_mask=m, output_attentions=True, attentions_dtype=torch.float32)
        assert all(t.dtype == torch.float32 for t in o32["attentions"]) and "hidden_states" not in o32
        _compare(f"output_attentions w2v {tag} attentions as fp32", precision, o32["attentions"], ref["attentions"])
    with pytest.raises(ValueError):
        model(clips.to(dev), neg_indices=torch.zeros(B_M, 130, 10, dtype=torch.int32), output_attentions=True)


# ----------------------------------------------------------------------------- the CLI
def test_transcribe_saves_cross_attentions(dev, tmp_path, capsys):
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("whisper_transcribe", os.path.join(root, "speech_jobs", "whisper_transcribe.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    path = str(tmp_path / "cross.npz")
    mod.main(["--model_type", "tiny", "--max_length", "3", "--save_cross_attentions", path])
    capsys.readouterr()
    z = np.load(path)
    assert list(z["clips"]) == ["dummy0"]
    ids, att = z["ids_0"], z["attn_0"]
    S = ids.shape[0]
    assert ids.dtype == np.int32 and 2 <= S <= 4 and ids[0] == 50257
    assert att.dtype == np.float32 and att.shape == (4, S, 1499)  # tiny: 4 decoder layers; the dummy clip has 2998 frames
    assert np.all(np.isfinite(att)) and np.abs(att.sum(-1) - 1.0).max() < 1e-2  # a mean of rows that each sum to 1
