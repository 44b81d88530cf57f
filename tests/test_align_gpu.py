"""``model.align`` and the timestamp switches of ``generate`` / ``transcribe_audio`` on the tiny model of
tests/test_attn_probs_cpu.py (2 + 2 layers, 2 heads, n_ctx 96, at most 16 positions), fp32 and bf16.

The reference is the GPU's own fp32 ``cross_attentions`` (``forward_infer`` on each row alone, over [start, tokens])
pushed through tests/_align_ref.py: the cost must lie within ``cost_ref``'s per-element bound, the path must be valid and
its float64 cost within e(P) + e(P*) + the cells' bounds of the float64 optimum (``dtw_bounds``).  A row of one token has
the cost 0 exactly (and no finite bound: its variance is 0), so its path is the tie rule's: along the row."""
import numpy as np
import pytest
import torch

import _align_ref as A
from _margins import within
from oracle import whisper_oracle as O

pytestmark = pytest.mark.gpu

TINY = dict(d_model=128, encoder_attention_heads=2, decoder_attention_heads=2, d_ff=256, vocab_size=131, encoder_layers=2,
            decoder_layers=2, n_mels=8, n_ctx=96, decoder_start_token_id=130, max_target_positions=16)
N, T_IN, T, NTOK = 4, 140, 70, 9
LENGTHS = [3, 9, 9, 1]
_CACHE = {}


def _setup():
    if "s" not in _CACHE:
        ocfg = O.make_config("small", dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, **TINY)
        params = O.init_params(ocfg, seed=3, dtype=torch.float64)
        feats = torch.from_numpy(np.random.default_rng(7).standard_normal((N, 8, T_IN)).astype(np.float32))
        seq = torch.from_numpy(np.random.default_rng(8).integers(0, 130, (N, 1 + NTOK)).astype(np.int32))
        seq[:, 0] = ocfg.decoder_start_token_id
        _CACHE["s"] = (params, feats, seq)
    return _CACHE["s"]


def _model(dev, precision, **over):
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import whisper
    key = ("m", precision, tuple(sorted(over.items())))
    if key not in _CACHE:
        kw = dict(TINY)
        kw.update(over)
        m = whisper.create_whisper_model("small", device=dev, precision=precision, seed=1234, **kw)
        if not over:
            m.arena.load_ref({k: v.float() for k, v in _setup()[0].items()})
            m.refresh_shadows()
        _CACHE[key] = m
    return _CACHE[key]


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))


def _check_row(tag, model, f, seq, i, L, cols, heads, out, width=7):
    """Row i of ``out`` (an ``align`` result with paths) against the row's own weights through the reference."""
    o = model.forward_infer(f[i:i + 1], decoder_input_ids=seq[i:i + 1, :1 + L], output_attentions=("cross",),
                            attentions_dtype=torch.float32)
    layers = sorted({l for l, _ in heads})
    ref, bound = None, None
    for l in layers:
        hw = np.zeros(2, dtype=np.float32)
        for ll, h in heads:
            if ll == l:
                hw[h] = np.float32(1.0 / len(heads))
        p = o["cross_attentions"][l][:, :, 1:, :].double().cpu().numpy()
        r, b = A.cost_ref(p, [L], [cols], hw, width, True, base=None if ref is None else ref)
        # (a later layer's own bound counts the base's magnitude; the base's error passes through its one rounding)
        bound = b if bound is None else b + bound * (1 + A.gam(2))
        ref = r
    ref, bound = ref[0, :L, :cols], bound[0, :L, :cols]
    got = out["cost"][i, :L, :cols].double().cpu()
    path = out["paths"][i].cpu().numpy().astype(np.int64)
    st, en = out["token_start_frames"][i].cpu().numpy(), out["token_end_frames"][i].cpu().numpy()
    assert A.path_problems(path, L, cols, st[:L], en[:L]) == [], tag
    assert np.all(st[L:] == -1) and np.all(en[L:] == -1)
    if L == 1:
        assert bool((got == 0).all()), "one token: the cost is exactly 0"
        assert [tuple(x) for x in path] == [(0, j) for j in range(cols)]
        assert float(out["path_cost"][i]) == 0.0
        return
    ratio = A.ratio(got, torch.from_numpy(ref), torch.from_numpy(bound))
    print(f"align {tag} row {i} ({L} x {cols}): cost at {ratio:.3f} of its bound")
    within(f"align model cost {tag}", ratio, 1.0)
    best = A.dtw_ref(ref)
    excess_bound, total_bound = A.dtw_bounds(ref, best, path, cell_bound=bound)
    excess = A.path_cost(ref, path) - best["total"]
    within(f"align model path excess {tag}", max(excess, 0.0) / excess_bound, 1.0)
    within(f"align model path_cost {tag}", abs(float(out["path_cost"][i]) - best["total"]) / total_bound, 1.0)
    # monotone: starts do not decrease, a token ends where the next begins or one frame later
    assert np.all(np.diff(st[:L]) >= 0)
    assert all(en[k] in (st[k + 1], st[k + 1] + 1) for k in range(L - 1))
    assert st[0] == 0 and en[L - 1] == cols


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_align_matches_its_own_attentions(dev, precision):
    from tethys_speech_amd import whisper
    _, feats, seq = _setup()
    model = _model(dev, precision)
    f, s = feats.to(dev), seq.to(dev)
    out = model.align(f, s, LENGTHS, return_path=True)
    torch.cuda.synchronize()
    assert tuple(out["token_start_frames"].shape) == (N, NTOK) and out["token_start_frames"].dtype == torch.int32
    assert tuple(out["cost"].shape) == (N, NTOK, T) and len(out["paths"]) == N and tuple(out["path_cost"].shape) == (N,)
    for i, L in enumerate(LENGTHS):
        _check_row(f"default {precision}", model, f, s, i, L, T, [(1, 0), (1, 1)], out)
    for k in ("start", "end"):
        fr, tm = out[f"token_{k}_frames"], out[f"token_{k}_times"]
        assert tm.dtype == torch.float32
        assert torch.equal(tm, torch.where(fr >= 0, fr.float() * whisper.FRAME_SECONDS, -1.0))
    # heads of two layers (the cost accumulates in layer order), a narrower filter, fewer frames
    heads, nf = [(1, 0), (0, 1), (0, 0)], [70, 40, 33, 10]
    out2 = model.align(f, s, LENGTHS, num_frames=nf, alignment_heads=heads, medfilt_width=3, return_path=True)
    for i, L in enumerate(LENGTHS):
        _check_row(f"two layers {precision}", model, f, s, i, L, nf[i], heads, out2, width=3)
        assert int(out2["token_end_frames"][i, :L].max()) == nf[i] and int(out2["token_start_frames"][i, :L].max()) < nf[i]
        assert bool((out2["cost"][i, :, nf[i]:] == 0).all())
    # without the paths: the same compact outputs
    out3 = model.align(f, s, LENGTHS)
    assert set(out3) == {"token_start_frames", "token_end_frames", "token_start_times", "token_end_times", "path_cost"}
    for k in out3:
        assert _same(out3[k], out[k]), k


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_ragged_batch_equals_each_row_alone(dev, precision):
    _, feats, seq = _setup()
    model = _model(dev, precision)
    f, s = feats.to(dev), seq.to(dev)
    batch = model.align(f, s, LENGTHS)
    for i, L in enumerate(LENGTHS):
        alone = model.align(f[i:i + 1], s[i:i + 1], [L])
        for k in batch:
            assert _same(alone[k][0], batch[k][i]), (k, i)
    # lengths None: every token; N = B * R rows over B clips: row i belongs to clip i // R
    full = model.align(f, s)
    assert bool((full["token_start_frames"] >= 0).all())
    pairs = model.align(f[:2], s)
    rep = model.align(f[[0, 0, 1, 1]], s)
    for k in pairs:
        assert _same(pairs[k], rep[k]), k
    short = model.align(f[:2], s, num_frames=[50, 30])
    assert [int(short["token_end_frames"][i].max()) for i in range(4)] == [50, 50, 30, 30]
    for bad in (dict(num_frames=[71] * 4), dict(num_frames=[70] * 3), dict(lengths=[10, 1, 1, 1])):
        with pytest.raises(ValueError):
            model.align(f, s, **bad)
    with pytest.raises(ValueError):
        model.align(f[:3], s)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_generate_with_token_timestamps(dev, precision):
    _, feats, _ = _setup()
    model = _model(dev, precision)
    f = feats.to(dev)
    modes = {"greedy": dict(), "beam": dict(num_beams=3, num_return_sequences=2),
             "sample": dict(do_sample=True, top_k=8, temperature=1.3, seed=5)}
    for name, kw in modes.items():
        out = model.generate(f, max_length=8, eos_token_id=-1 if name == "greedy" else None, return_token_timestamps=True, **kw)
        plain = model.generate(f, max_length=8, eos_token_id=-1 if name == "greedy" else None, return_dict_in_generate=True, **kw)
        if not isinstance(plain, dict):
            plain = {"sequences": plain}
        assert set(out) == set(plain) | {"token_start_frames", "token_end_frames", "token_start_times", "token_end_times",
                                         "path_cost"}, name
        for k in plain:  # with the flag off nothing changes: the same ids, scores and lengths
            assert torch.equal(out[k], plain[k]), (name, k)
        al = model.align(f, out["sequences"], out.get("lengths"))
        for k in al:
            assert _same(al[k], out[k]), (name, k)
        rows, n = out["sequences"].shape[0], out["sequences"].shape[1] - 1
        assert rows == (8 if name == "beam" else 4) and tuple(out["token_start_frames"].shape) == (rows, n)
        lens = out["lengths"].cpu().tolist() if "lengths" in out else [n] * rows
        for r in range(rows):
            st, en = out["token_start_frames"][r].cpu().numpy(), out["token_end_frames"][r].cpu().numpy()
            assert np.all(st[:lens[r]] >= 0) and np.all(en[:lens[r]] <= T) and np.all(st[lens[r]:] == -1)
    with pytest.raises(ValueError):
        model.generate(f, max_length=16, return_token_timestamps=True)  # no decoder position for token 16


def test_transcribe_audio_with_timestamps(dev):
    from tethys_speech_amd import whisper
    model = _model(dev, "bf16", n_mels=80, n_ctx=1500)
    plain = whisper.transcribe_audio(model, None, max_length=6)
    got = whisper.transcribe_audio(model, None, max_length=6, return_timestamps=True)
    assert set(got) == {"ids", "token_start_times", "token_end_times"}
    assert np.array_equal(got["ids"], plain)
    n = len(got["ids"]) - 1
    t0, t1 = got["token_start_times"], got["token_end_times"]
    assert t0.shape == (n,) and t1.shape == (n,) and t0.dtype == np.float32
    assert np.all(t0 >= 0) and np.all(t1 <= 30.0) and np.all(t0 < t1) and np.all(np.diff(t0) >= 0)
    assert t0[0] == 0 and abs(float(t1[-1]) - 1499 * 0.02) < 1e-4  # the clip's 2998 log-mel frames: 1499 encoder frames

    class Tok:
        def decode(self, ids):
            return " ".join(str(int(i)) for i in ids)
    txt = whisper.transcribe_audio(model, None, tokenizer=Tok(), max_length=6, return_timestamps=True)
    assert txt["text"] == " ".join(str(int(i)) for i in plain) and np.array_equal(txt["token_start_times"], t0)
