"""Whisper inference on the GPU: tmi_lm_head_argmax against an fp64 torch restatement, the forward-only pass
(W:547-616, training=False) and greedy ``generate`` (W:636-709) against the oracle, the EOS stop, non-interference with
training (eager and launch plans, dropout on), checkpoint restore, ``transcribe_audio`` (W:962-986) and the full-size
decode.  The reduced model: head_dim 64 (two heads of d 128), 2 + 2 layers, the real 80 mels / 1500 frames / 51865
tokens, so the start token 50257 and the padded LM head [d, 51904] are the real ones."""
import numpy as np
import pytest
import torch

from _margins import within

pytestmark = pytest.mark.gpu

V, VP = 51865, 51904
_RED = dict(d_model=128, encoder_attention_heads=2, decoder_attention_heads=2, d_ff=256, encoder_layers=2,
            decoder_layers=2)


def _mods():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import ops, whisper
    from oracle import whisper_oracle as O
    return ops, whisper, O


# ----------------------------------------------------------------------------- 1. the kernel
def _ref_logits(x, gamma, beta, eps, w):
    """fp64: LayerNorm (or none) then x . w over the first V columns; also sum_k |y_k w_kn| (the rounding scale)."""
    y = x.double()
    if gamma is not None:
        mu = y.mean(1, keepdim=True)
        var = ((y - mu) ** 2).mean(1, keepdim=True)
        y = (y - mu) / torch.sqrt(var + eps) * gamma.double() + beta.double()
    wd = w[:, :V].double()
    return y @ wd, (y.abs() @ wd.abs()).max(1).values


def _check_ids(ids, z, scale, rel, name):
    """The id equals the fp64 argmax where the top-2 margin exceeds the bound, else its logit is within the bound."""
    ids = ids.long()
    top2 = z.topk(2, dim=1)
    bound = rel * scale
    zmax = top2.values[:, 0]
    chosen = z.gather(1, ids[:, None])[:, 0]
    assert bool(((ids >= 0) & (ids < V)).all()), ids
    clear = (top2.values[:, 0] - top2.values[:, 1]) > bound
    assert torch.equal(ids[clear], top2.indices[clear, 0]), (name, ids[clear], top2.indices[clear, 0])
    within(f"lm_head_argmax {name} (max - chosen) / scale", float(((zmax - chosen) / scale).max()), rel)


def _run_kernel(ops, x, x_ld, w, M, d, gamma, beta, eos_id=-1, ws=None, eps=1e-5):
    dev = w.device
    ids = torch.full((M, 3), -7, dtype=torch.int32, device=dev)  # column 1 of a [M, 3] matrix: ids_ld = 3
    cnt = torch.full((1,), -1, dtype=torch.int32, device=dev)
    ws = torch.zeros(M + 1, dtype=torch.int64, device=dev) if ws is None else ws
    ops.lm_head_argmax(x, x_ld, w, VP, M, d, V, ids[:, 1:], 3, ws, gamma=gamma, beta=beta, eps=eps, eos_id=eos_id,
                       eos_count=cnt)
    torch.cuda.synchronize()
    assert bool((ids[:, 0] == -7).all()) and bool((ids[:, 2] == -7).all()), "wrote outside its column"
    assert int(ws.abs().sum()) == 0, "the workspace is not left zero"
    return ids[:, 1].clone(), int(cnt.item())


@pytest.mark.parametrize("wdt", ["bf16", "fp32"])
def test_lm_head_argmax_matches_fp64(dev, wdt):
    ops, _, _ = _mods()
    g = torch.Generator(device=dev).manual_seed(1)
    for d in (384, 768, 1280):
        w = torch.zeros(d, VP, device=dev)
        w[:, :V] = torch.randn(d, V, device=dev, generator=g) * d ** -0.5
        w = w.to(torch.bfloat16) if wdt == "bf16" else w
        xdt = torch.bfloat16 if wdt == "bf16" else torch.float32
        gamma = 1 + 0.1 * torch.randn(d, device=dev, generator=g)
        beta = 0.1 * torch.randn(d, device=dev, generator=g)
        for M in (1, 3, 8, 16, 40):
            # rows at a stride (the last position of each of M samples of 5 positions), LayerNorm in the prologue
            full = (torch.randn(M * 5, d, device=dev, generator=g) * 2 + 0.5).to(xdt)
            x = full[4:]
            eos = int(torch.randint(0, V, (1,), device=dev, generator=g))
            ids, cnt = _run_kernel(ops, x, 5 * d, w, M, d, gamma, beta, eos_id=eos)
            z, scale = _ref_logits(full[4::5], gamma, beta, 1e-5, w)
            _check_ids(ids, z, scale, 1e-5, f"{wdt} d{d} M{M} LN")
            assert cnt == int((ids == eos).sum())
            # without the LayerNorm; the EOS count with an id that some rows chose
            ids2, cnt2 = _run_kernel(ops, x, 5 * d, w, M, d, None, None, eos_id=int(ids[0]))
            z2, scale2 = _ref_logits(full[4::5], None, None, 0.0, w)
            _check_ids(ids2, z2, scale2, 1e-5, f"{wdt} d{d} M{M} plain")
            assert cnt2 == int((ids2 == int(ids[0])).sum())


def test_lm_head_argmax_ties_pads_reset_and_load(dev):
    ops, _, _ = _mods()
    g = torch.Generator(device=dev).manual_seed(2)
    d, M = 768, 8
    w32 = torch.zeros(d, VP, device=dev)
    w32[:, :V] = torch.randn(d, V, device=dev, generator=g) * d ** -0.5
    x = torch.randn(M, d, device=dev, generator=g)
    # duplicated columns tie to the smaller index: copy each row's winner to a smaller column (same group of 8, and another
    # workgroup), the copies compute bit-identical logits
    for wdt in (torch.float32, torch.bfloat16):
        w = w32.clone()
        ids0, _ = _run_kernel(ops, x.to(wdt), d, w.to(wdt), M, d, None, None)
        a = int(ids0[0])
        for b in sorted({max(a - 1, 0), 5, a - (a % 8)} - {a}):
            w2 = w.clone()
            w2[:, b] = w2[:, a]
            ids, _ = _run_kernel(ops, x.to(wdt), d, w2.to(wdt), M, d, None, None)
            assert int(ids[0]) == min(a, b), (a, b, int(ids[0]))
        # a whole row of equal logits (x = 0): column 0
        xz = x.clone()
        xz[3] = 0
        ids, _ = _run_kernel(ops, xz.to(wdt), d, w.to(wdt), M, d, None, None)
        assert int(ids[3]) == 0
    # all real logits negative: the zero pad columns [V, VP) must never win
    wneg = torch.zeros(d, VP, device=dev)
    wneg[:, :V] = -(torch.rand(d, V, device=dev, generator=g) + 0.1)
    xp = torch.rand(M, d, device=dev, generator=g) + 0.1
    for wdt in (torch.float32, torch.bfloat16):
        ids, _ = _run_kernel(ops, xp.to(wdt), d, wneg.to(wdt), M, d, None, None)
        z, scale = _ref_logits(xp.to(wdt), None, None, 0.0, wneg.to(wdt))
        assert bool((ids < V).all())
        _check_ids(ids, z, scale, 1e-5, "all-negative")
    # three back-to-back calls on one workspace with different inputs, no synchronisation between them
    wb = w32.to(torch.bfloat16)
    ws = torch.zeros(M + 1, dtype=torch.int64, device=dev)
    xs = [torch.randn(M, d, device=dev, generator=g).to(torch.bfloat16) for _ in range(3)]
    outs = [torch.empty(M, dtype=torch.int32, device=dev) for _ in range(3)]
    cnts = [torch.empty(1, dtype=torch.int32, device=dev) for _ in range(3)]
    for xi, o, c in zip(xs, outs, cnts):
        ops.lm_head_argmax(xi, d, wb, VP, M, d, V, o, 1, ws, eos_id=7, eos_count=c)
    torch.cuda.synchronize()
    assert int(ws.abs().sum()) == 0
    for xi, o, c in zip(xs, outs, cnts):
        z, scale = _ref_logits(xi, None, None, 0.0, wb)
        _check_ids(o, z, scale, 1e-5, "back-to-back")
        assert int(c) == int((o == 7).sum())
    # bit-identical beside a busy second stream
    quiet = [_run_kernel(ops, xi, d, wb, M, d, None, None)[0] for xi in xs]
    side = torch.cuda.Stream(device=dev)
    big = torch.randn(4096, 4096, device=dev, generator=g)
    with torch.cuda.stream(side):
        for _ in range(20):
            big = torch.tanh(big @ big)
    busy = [_run_kernel(ops, xi, d, wb, M, d, None, None)[0] for xi in xs]
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(quiet, busy))


def test_lm_head_argmax_rejects_bad_arguments(dev):
    ops, _, _ = _mods()
    from tethys_speech_amd._lib import TmiError
    d, M = 128, 2
    x = torch.randn(M, d, device=dev)
    w = torch.zeros(d, VP, device=dev)
    ids = torch.empty(M, dtype=torch.int32, device=dev)
    ws = torch.zeros(M + 1, dtype=torch.int64, device=dev)
    for kw in (dict(w_ld=V), dict(V=VP + 8), dict(ws=torch.zeros(M, dtype=torch.int64, device=dev))):
        args = dict(w_ld=VP, V=V, ws=ws)
        args.update(kw)
        with pytest.raises(TmiError):
            ops.lm_head_argmax(x, d, w, args["w_ld"], M, d, args["V"], ids, 1, args["ws"])
    with pytest.raises(TmiError):
        ops.lm_head_argmax(x, d, w, VP, M, d, V, ids, 1, ws, gamma=torch.ones(d, device=dev))  # gamma without beta


# ----------------------------------------------------------------------------- model fixtures
_CACHE = {}


def _setup(T_in=3000, B=2):
    """Reduced config, oracle parameters (fp64), features, oracle encoder output (fp64)."""
    key = (T_in, B)
    if key not in _CACHE:
        _, whisper, O = _mods()
        ocfg = O.make_config("small", dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, **_RED)
        params = O.init_params(ocfg, seed=3, dtype=torch.float64)
        feats = torch.from_numpy(np.random.default_rng(T_in).standard_normal((B, 80, T_in)).astype(np.float32))
        enc = O.encoder(params, feats.double(), ocfg, training=False)
        _CACHE[key] = (ocfg, params, feats, enc)
    return _CACHE[key]


def _model(dev, precision, params, seed=1234):
    _, whisper, _ = _mods()
    m = whisper.create_whisper_model("small", device=dev, precision=precision, seed=seed, **_RED)
    m.arena.load_ref({k: v.float() for k, v in params.items()})
    m.refresh_shadows()
    return m


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


# ----------------------------------------------------------------------------- 2. forward-only pass
@pytest.mark.parametrize("T_in", [3000, 2998])
def test_forward_only_logits_match_oracle(dev, T_in):
    _, whisper, O = _mods()
    ocfg, params, feats, enc = _setup(T_in)
    B = feats.shape[0]
    assert enc.shape[1] == (1500 if T_in == 3000 else 1499)
    rng = np.random.default_rng(T_in + 1)
    for precision, bound in (("fp32", 1e-5), ("bf16", 3e-2)):
        model = _model(dev, precision, params)
        for S in (1, 7, 100):
            labels = torch.from_numpy(rng.integers(3, V, (B, S)).astype(np.int32))
            dec_in = O.decoder_input_ids(labels, ocfg.decoder_start_token_id)
            h = O.decoder(params, dec_in, enc, ocfg, training=False)
            ref = h @ params["lm_head.kernel"]
            out = model(feats.to(dev), labels=labels.to(dev), training=False)
            assert out["loss"] is None and tuple(out["logits"].shape) == (B, S, V)
            within(f"forward logits {precision}", _rel(out["logits"], ref), bound, (S, T_in))
            within(f"forward dec hidden {precision}", _rel(out["last_hidden_state"], h), bound, (S, T_in))
            within(f"forward enc hidden {precision}", _rel(out["encoder_last_hidden_state"], enc), bound, (S, T_in))
            # the same sequence given as decoder_input_ids
            out2 = model(feats.to(dev), decoder_input_ids=dec_in.to(dev), training=False)
            assert torch.equal(out2["logits"], out["logits"])
        with pytest.raises(ValueError):
            model(feats.to(dev), decoder_input_ids=torch.full((B, 2), 7, dtype=torch.int32), training=False)


# ----------------------------------------------------------------------------- 3. generate against the oracle
def _oracle_prefix_logits(O, params, ocfg, enc, ids, t):
    """Logits of the last position when the decoder sees ids[:, :t] (the whole prefix: the inverted mask makes every
    position depend on the later ones)."""
    h = O.decoder(params, ids[:, :t].long(), enc, ocfg, training=False)
    return h[:, -1] @ params["lm_head.kernel"]


def _oracle_greedy(O, params, ocfg, enc, B, max_length):
    ids = torch.full((B, 1), ocfg.decoder_start_token_id, dtype=torch.int64)
    for _ in range(max_length):
        z = _oracle_prefix_logits(O, params, ocfg, enc, ids, ids.shape[1])
        nxt = z.argmax(1)
        ids = torch.cat([ids, nxt[:, None]], 1)
        if bool((nxt == ocfg.eos_token_id).all()):
            break
    return ids


def test_generate_matches_oracle_greedy_loop(dev):
    _, whisper, O = _mods()
    ocfg, params, feats, enc = _setup(3000)
    B, L = feats.shape[0], 24
    ref_ids = _oracle_greedy(O, params, ocfg, enc, B, L)
    for precision, rel in (("fp32", 1e-4), ("bf16", 5e-2)):
        model = _model(dev, precision, params)
        ids = model.generate(feats.to(dev), max_length=L).cpu().long()
        assert ids.shape[0] == B and 2 <= ids.shape[1] <= 1 + L and bool((ids[:, 0] == 50257).all())
        all_clear = True
        for t in range(1, ids.shape[1]):
            z = _oracle_prefix_logits(O, params, ocfg, enc, ids, t)  # teacher-forced on the model's own prefix
            scale = z.abs().max(1).values + 1e-6
            top2 = z.topk(2, dim=1)
            clear = (top2.values[:, 0] - top2.values[:, 1]) > rel * scale
            all_clear &= bool(clear.all())
            if precision == "fp32":
                assert torch.equal(ids[clear, t], top2.indices[clear, 0]), (t, ids[:, t], top2.indices[:, 0])
            chosen = z.gather(1, ids[:, t:t + 1])[:, 0]
            within(f"generate {precision} (max - chosen) / max|z|", float(((top2.values[:, 0] - chosen) / scale).max()), rel)
        if precision == "fp32" and all_clear:
            assert torch.equal(ids, ref_ids), (ids, ref_ids)
        # two calls give identical ids
        assert torch.equal(model.generate(feats.to(dev), max_length=L).cpu().long(), ids)


# ----------------------------------------------------------------------------- 4. EOS
def test_generate_eos_stop_rules(dev):
    _, whisper, O = _mods()
    ocfg, params, _, _ = _setup(3000)
    B = 3
    feats = torch.from_numpy(np.random.default_rng(5).standard_normal((B, 80, 400)).astype(np.float32)).to(dev)
    model = _model(dev, "fp32", params)
    # an EOS column that dominates every row: one step, [B, 2], ending in EOS
    p2 = dict(params)
    p2["decoder.layer_norm.beta"] = torch.full_like(params["decoder.layer_norm.beta"], 10.0)
    lm = params["lm_head.kernel"].clone()
    lm[:, 2] = 1.0
    p2["lm_head.kernel"] = lm
    m2 = _model(dev, "fp32", p2)
    ids = m2.generate(feats, max_length=20).cpu()
    assert tuple(ids.shape) == (B, 2) and bool((ids[:, 1] == 2).all())
    # only some rows emit the stop token: decoding runs on to max_length (or to a step where every row emits it)
    L = 16
    free = model.generate(feats, max_length=L, eos_token_id=-1).cpu()
    assert tuple(free.shape) == (B, 1 + L)
    cands = []
    for tok in torch.unique(free[:, 1:]).tolist():
        hit = (free[:, 1:] == tok)
        partial = bool((hit.any(0) & ~hit.all(0)).any())
        full = [t + 1 for t in range(L) if bool(hit[:, t].all())]
        if partial:
            cands.append((tok, full[0] if full else L))
    assert cands, "no token is emitted by some rows only (degenerate decode)"
    for tok, n in cands[:3]:
        got = model.generate(feats, max_length=L, eos_token_id=tok).cpu()
        assert torch.equal(got, free[:, :1 + n]), (tok, n)


# ----------------------------------------------------------------------------- 5. non-interference with training
def _train_run(dev, planned, with_generate, steps=9):
    _, whisper, _ = _mods()
    from tethys_speech_amd import ops, optim, train
    from tethys_speech_amd.data import create_dummy_dataset
    from tethys_speech_amd.dist import DataParallelStrategy
    tiny = dict(d_model=128, encoder_attention_heads=2, decoder_attention_heads=2, d_ff=256, vocab_size=160,
                encoder_layers=2, decoder_layers=2, n_mels=16, n_ctx=64, decoder_start_token_id=150, max_target_positions=32)
    was = ops.set_deterministic(True)
    old = train.USE_PLAN
    try:
        strategy = DataParallelStrategy(0, 1, init=False)
        model = whisper.create_whisper_model("small", device=dev, precision="bf16", seed=5, **tiny)
        model.enable_dropout(0.1, 0.1, seed=77)
        opt = optim.Adam(1e-3)
        it = iter(create_dummy_dataset(3, n_mels=16, seq_len=96, max_target_length=12, device=dev, seed=9, num_samples=8))
        gfeats = torch.from_numpy(np.random.default_rng(1).standard_normal((2, 16, 80)).astype(np.float32)).to(dev)
        train.USE_PLAN = planned
        step = train.planned_step(strategy, model, opt, "whisper", pipelined=True)
        losses, gens = [], []
        drop_step = model._drop_step
        for _ in range(steps):
            losses.append(step(*next(it)))
            if with_generate:
                before = model._drop_step
                gens.append(model.generate(gfeats, max_length=5).cpu())
                assert model._drop_step == before
        model.finish_late()
        torch.cuda.synchronize()
        assert model._drop_step == drop_step + steps
        if planned:
            assert step.planned is not None and step.planned.replays >= 2
        return [float(x.item()) for x in losses], model.arena.p.clone(), model.arena.m.clone(), gens
    finally:
        train.USE_PLAN = old
        ops.set_deterministic(was)


@pytest.mark.parametrize("planned", [False, True])
def test_generate_between_training_steps_changes_nothing(dev, planned):
    l0, p0, m0, _ = _train_run(dev, planned, False)
    l1, p1, m1, gens = _train_run(dev, planned, True)
    assert l0 == l1, (l0, l1)
    assert torch.equal(p0, p1) and torch.equal(m0, m1)
    assert len(gens) == 9 and all(g.shape[0] == 2 for g in gens)


# ----------------------------------------------------------------------------- 6. checkpoint
def test_checkpoint_load_weights_then_generate(dev, tmp_path):
    _, whisper, _ = _mods()
    from tethys_speech_amd import optim, train
    ocfg, params, feats, _ = _setup(3000)
    f = feats[:, :, :600].contiguous().to(dev)
    for precision in ("fp32", "bf16"):
        m1 = _model(dev, precision, params)
        ref = m1.generate(f, max_length=10)
        path = str(tmp_path / f"ck_{precision}.pt")
        train.save_checkpoint(m1, optim.Adam(1e-3), path)
        m2 = whisper.create_whisper_model("small", device=dev, precision=precision, seed=99, **_RED)
        assert not torch.equal(m2.arena.p, m1.arena.p)
        train.load_weights(m2, path)
        assert torch.equal(m2.generate(f, max_length=10), ref)
        wpath = str(tmp_path / f"w_{precision}.pt")
        train.save_weights(m1, wpath)
        m3 = whisper.create_whisper_model("small", device=dev, precision=precision, seed=98, **_RED)
        train.load_weights(m3, wpath)
        assert torch.equal(m3.generate(f, max_length=10), ref)


# ----------------------------------------------------------------------------- 7. transcribe_audio
def test_transcribe_audio(dev, tmp_path):
    import wave
    _, whisper, _ = _mods()
    from tethys_speech_amd.frontend import LogMelFrontend
    _, params, _, _ = _setup(3000)
    model = _model(dev, "bf16", params)
    fe = LogMelFrontend(device=dev)
    got = whisper.transcribe_audio(model, None, max_length=8)
    wav = torch.from_numpy(whisper.dummy_waveform()).to(dev)
    feats = fe(wav)
    assert tuple(feats.shape) == (1, 80, 2998)
    ref = model.generate(feats, max_length=8)[0].cpu().numpy()
    assert isinstance(got, np.ndarray) and np.array_equal(got, ref) and got[0] == 50257
    # a .wav file (2 s of noise, 16-bit PCM mono 16 kHz) written here
    pcm = (np.random.default_rng(4).standard_normal(32000) * 3000).clip(-32768, 32767).astype("<i2")
    p = tmp_path / "clip.wav"
    with wave.open(str(p), "wb") as fw:
        fw.setnchannels(1)
        fw.setsampwidth(2)
        fw.setframerate(16000)
        fw.writeframes(pcm.tobytes())
    got = whisper.transcribe_audio(model, str(p), max_length=8)
    ref = model.generate(fe(torch.from_numpy(pcm.astype(np.float32) / 32768.0).to(dev)), max_length=8)[0].cpu().numpy()
    assert np.array_equal(got, ref) and got[0] == 50257

    class Tok:
        def decode(self, ids):
            return " ".join(str(int(i)) for i in ids)
    assert whisper.transcribe_audio(model, str(p), tokenizer=Tok(), max_length=8) == " ".join(str(int(i)) for i in ref)


# ----------------------------------------------------------------------------- 8. full size
def test_full_size_generate_448_steps(dev):
    _, whisper, _ = _mods()
    model = whisper.create_whisper_model("small", device=dev, precision="bf16")
    feats = torch.randn(8, 80, 3000, generator=torch.Generator().manual_seed(0)).to(dev)
    ids = model.generate(feats, max_length=448, eos_token_id=-1)
    assert tuple(ids.shape) == (8, 449) and ids.dtype == torch.int32
    assert bool((ids[:, 0] == 50257).all()) and bool(((ids >= 0) & (ids < V)).all())
