"""Sampled decoding on the GPU: tmi_lm_head_sample against the fp64 restatement of its rule (tests/_sample_ref.py) - token
for token on inputs whose scores are exact, on random inputs wherever the draw is decided - its semantics, rejections
and record / replay, ``generate(do_sample=True)`` on the reduced model, non-interference with training,
``transcribe_audio(do_sample=True)`` and one full-size call."""
import numpy as np
import pytest
import torch

import _sample_ref as R
from _margins import within

pytestmark = pytest.mark.gpu

V, VP = 51865, 51904
_RED = dict(d_model=128, encoder_attention_heads=2, decoder_attention_heads=2, d_ff=256, encoder_layers=2,
            decoder_layers=2)
REL = R.REL


def _mods():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import ops, whisper
    from oracle import whisper_oracle as O
    return ops, whisper, O


def _sample(ops, x, x_ld, w, w_ld, M, d, Vr, top_k, top_p=1.0, temperature=1.0, seed=0, gamma=None, beta=None, ws=None,
            finished=None, suppress_id=-1, eos_id=-1, pad_id=0, ids=None, ids_ld=1, expect_error=False):
    dev = w.device
    ids = torch.full((M,), -7, dtype=torch.int32, device=dev) if ids is None else ids
    lp = torch.full((M,), float("nan"), device=dev)
    fin = torch.zeros(M, dtype=torch.int32, device=dev) if finished is None else finished
    cnt = torch.full((1,), -7, dtype=torch.int32, device=dev)
    ws = torch.zeros(ops.lm_head_sample_workspace_elems(M, Vr, top_k), dtype=torch.int64, device=dev) if ws is None else ws
    call = lambda: ops.lm_head_sample(x, x_ld, w, w_ld, M, d, Vr, ids, ids_ld, fin, cnt, ws, temperature=temperature,  # noqa: E731
                                      top_k=top_k, top_p=top_p, seed=seed, suppress_id=suppress_id, eos_id=eos_id,
                                      pad_id=pad_id, logprob=lp, gamma=gamma, beta=beta)
    if expect_error:
        from tethys_speech_amd._lib import TmiError
        with pytest.raises(TmiError):
            call()
        torch.cuda.synchronize()
        assert bool((ids == -7).all()) and int(cnt) == -7 and bool(torch.isnan(lp).all()), "a rejected call wrote its outputs"
        return None
    call()
    torch.cuda.synchronize()
    assert int(ws.abs().sum()) == 0, "the workspace is not left zero"
    return ids.cpu().long().numpy(), lp.cpu().double().numpy(), fin.cpu().numpy(), int(cnt)


# ----------------------------------------------------------------------------- 1. exact scores, token for token
@pytest.mark.parametrize("M", R.EXACT_MS)
def test_exact_scores_token_for_token(dev, M):
    """Inputs, seeds and the reference's choices are tests/_sample_ref.py's (built on the host; test_sample_cpu.py holds
    every configuration to the 1 % cap from the reference alone, and so does this test before it launches anything).
    At b = 0 equal scores are no doubt - their column order is the rule's own, and the scores are exact - so a row is
    undecided only when the draw or the nucleus test is within P_TOL of an edge of the running sums, or two perturbed
    scores of the Gumbel rule within 2 G_TOL.  Measured: |logprob - fp64| in the top-k test's bound form, and as it
    is (the relative error of p_i that P_TOL has to cover, next to the running sums' own, measured on the host): at
    most 5.6e-8 of (scale + |lse|) and 1.4e-6 absolute on an MI355X."""
    ops, _, _ = _mods()
    x, w, z, scale = R.exact_inputs(M)
    refs = {(T, k, p): R.exact_choice(M, T, k, p) for T in R.EXACT_TS for k, p in R.EXACT_KP}
    for cfg, ref in refs.items():
        assert R.cap_ok(ref[2], R.EXACT_CAP), (M, cfg, int((~ref[2]).sum()))
    worst = worst_abs = 0.0
    for wdt in (torch.bfloat16, torch.float32):
        xd, wd = torch.from_numpy(x).to(dev).to(wdt), torch.from_numpy(w).to(dev).to(wdt)
        for (T, top_k, top_p), (tok, _, dec, allowed) in refs.items():
            s, lse, _ = R.exact_ranked(M, T)
            ids, lp, _, _ = _sample(ops, xd, 128, wd, VP, M, 128, V, top_k, top_p, T, R.exact_seed(M, T, top_k, top_p))
            name = f"exact M{M} T{T} k{top_k} p{top_p}"
            assert np.array_equal(ids[dec], tok[dec]), (name, ids, tok)
            for r in np.nonzero(~dec)[0]:
                assert ids[r] in allowed[r], (name, r)
            err = np.abs(lp - (s[np.arange(M), ids] - lse))
            worst = max(worst, float((err / (scale / T + np.abs(lse))).max()))
            worst_abs = max(worst_abs, float(err.max()))
            if top_k == 1:
                assert np.array_equal(ids, np.argsort(-z, axis=1, kind="stable")[:, 0])
    within(f"lm_head_sample exact M{M} |lp - lp64| / (scale + |lse|)", worst, REL)
    within("lm_head_sample exact |lp - lp64| (the relative error of p_i)", worst_abs, R.P_LP_TOL)


# ----------------------------------------------------------------------------- 2. random inputs with LayerNorm
@pytest.mark.parametrize("wdt", ["bf16", "fp32"])
def test_random_inputs_with_layernorm_match_on_decided_rows(dev, wdt):
    """b = REL * (scale + |lse|) per row, the top-k test's bound on the scores.  Inputs, seeds and the reference are
    tests/_sample_ref.py's, built on the host: every configuration is held to the 10 % cap from the reference alone
    before anything is launched (and in test_sample_cpu.py)."""
    ops, _, _ = _mods()
    T = R.RANDOM_T
    for d in R.RANDOM_DS:
        w, gamma, beta, xs, refs = R.random_inputs(wdt, d)
        choices = {(M, k, p): R.random_choice(refs[M], wdt, d, M, k, p) for M in R.RANDOM_MS for k, p in R.RANDOM_KP}
        for cfg, ch in choices.items():
            assert R.cap_ok(ch[2], R.RANDOM_CAP), (wdt, d, cfg, int((~ch[2]).sum()))
        w, gamma, beta = w.to(dev), gamma.to(dev), beta.to(dev)
        for M in R.RANDOM_MS:
            x = xs[M].to(dev)[2:]  # the last of every 3 positions, read in place
            s, lse, _, b = refs[M]
            worst = 0.0
            for top_k, top_p in R.RANDOM_KP:
                tok, _, dec, allowed = choices[(M, top_k, top_p)]
                ids, lp, _, _ = _sample(ops, x, 3 * d, w, VP, M, d, V, top_k, top_p, T, R.random_seed(wdt, d, M, top_k, top_p),
                                        gamma=gamma, beta=beta)
                name = f"{wdt} d{d} M{M} k{top_k} p{top_p}"
                assert np.array_equal(ids[dec], tok[dec]), (name, ids, tok, dec)
                for r in np.nonzero(~dec)[0]:
                    assert ids[r] in allowed[r], (name, r)
                worst = max(worst, float((np.abs(lp - (s[np.arange(M), ids] - lse)) / b * REL).max()))
            within(f"lm_head_sample {wdt} d{d} M{M} |lp - lp64| / (scale + |lse|)", worst, REL)


# ----------------------------------------------------------------------------- 3. semantics
def _small(dev, M=6, d=128, Vr=1000, seed=5, dtype=torch.float32):
    g = torch.Generator(device=dev).manual_seed(seed)
    ld = (Vr + 7) // 8 * 8
    w = torch.zeros(d, ld, device=dev)
    w[:, :Vr] = torch.randn(d, Vr, device=dev, generator=g) * 0.2
    x = torch.randn(M, d, device=dev, generator=g)
    return x.to(dtype), w.to(dtype), ld


def test_seeds_repeat_and_differ_and_workspace_is_reused(dev):
    ops, _, _ = _mods()
    M, d, Vr = 40, 128, 1000
    x, w, ld = _small(dev, M, d, Vr)
    for top_k in (0, 50):
        ws = torch.zeros(ops.lm_head_sample_workspace_elems(M, Vr, top_k), dtype=torch.int64, device=dev)
        a = _sample(ops, x, d, w, ld, M, d, Vr, top_k, seed=3, ws=ws)
        b = _sample(ops, x, d, w, ld, M, d, Vr, top_k, seed=3, ws=ws)  # (the workspace the first call left behind)
        c = _sample(ops, x, d, w, ld, M, d, Vr, top_k, seed=4, ws=ws)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert not np.array_equal(a[0], c[0])


def test_finished_rows_eos_suppression_ties_and_padded_tail(dev):
    ops, _, _ = _mods()
    M, d, Vr = 6, 128, 1000
    x, w, ld = _small(dev, M, d, Vr)
    # a finished row gives pad and logprob 0, and stays finished
    fin = torch.tensor([0, 1, 0, 0, 5, 0], dtype=torch.int32, device=dev)
    ids, lp, f, n = _sample(ops, x, d, w, ld, M, d, Vr, 20, seed=1, finished=fin, pad_id=777, eos_id=Vr + 5)
    assert ids[1] == 777 and ids[4] == 777 and lp[1] == 0 and lp[4] == 0 and n == 2 and f.tolist() == [0, 1, 0, 0, 5, 0]
    assert all(0 <= ids[r] < Vr and lp[r] < 0 for r in (0, 2, 3, 5))
    # a dominant EOS column: every live row draws it and is finished afterwards, in both modes
    w2 = w.clone()
    x2 = x.clone()
    x2[:, 0] = 30.0
    w2[0, :] = -1.0
    w2[0, 9] = 1.0
    for top_k in (0, 50):
        fin = torch.tensor([0, 0, 1, 0, 0, 0], dtype=torch.int32, device=dev)
        ids, lp, f, n = _sample(ops, x2, d, w2, ld, M, d, Vr, top_k, seed=2, finished=fin, eos_id=9, pad_id=0)
        assert ids.tolist() == [9, 9, 0, 9, 9, 9] and f.tolist() == [1] * 6 and n == 6
        # ... and suppressed, it is never drawn although it is the largest score
        for seed in range(4):
            ids, _, f, n = _sample(ops, x2, d, w2, ld, M, d, Vr, top_k, seed=seed, suppress_id=9, eos_id=9)
            assert 9 not in ids and n == 0 and not f.any()
    # equal scores resolve to the smaller column at top_k = 1 (columns 700 and 300 hold the same, largest, weights)
    w3 = w.clone()
    w3[:, 700] = 0.0
    w3[:, 300] = 0.0
    x3 = x.clone()
    x3[:, 1] = 40.0
    w3[1, 700] = 1.0
    w3[1, 300] = 1.0
    ids, _, _, _ = _sample(ops, x3, d, w3, ld, M, d, Vr, 1, seed=0)
    assert ids.tolist() == [300] * M
    # V not a multiple of 128 (nor of 8): the padded tail holds the largest weights and is never chosen
    Vr2 = 1003
    x4, w4, ld4 = _small(dev, M, d, Vr2)
    w4[:, Vr2:] = 5.0 * x4[0].sign()[:, None]
    for top_k in (0, 1, 64):
        for seed in range(3):
            ids, _, _, _ = _sample(ops, x4, d, w4, ld4, M, d, Vr2, top_k, seed=seed)
            assert bool((ids < Vr2).all()) and bool((ids >= 0).all())
    # no column can be drawn (one column, suppressed): pad and logprob 0 in both modes
    x5, w5, ld5 = _small(dev, 2, d, 1)
    for top_k in (0, 3):
        ids, lp, f, n = _sample(ops, x5, d, w5, ld5, 2, d, 1, top_k, seed=1, suppress_id=0, pad_id=777)
        assert ids.tolist() == [777, 777] and lp.tolist() == [0.0, 0.0] and n == 0
    # strided ids
    out = torch.full((M, 4), -1, dtype=torch.int32, device=dev)
    _sample(ops, x, d, w, ld, M, d, Vr, 5, seed=1, ids=out[:, 2:], ids_ld=4)
    assert bool((out[:, 2] >= 0).all()) and bool((out[:, [0, 1, 3]] == -1).all())


# ----------------------------------------------------------------------------- 4. rejections
def test_lm_head_sample_rejects_bad_arguments(dev):
    ops, _, _ = _mods()
    M, d, Vr = 4, 128, 1000
    x, w, ld = _small(dev, M, d, Vr)
    good = dict(top_k=50, top_p=0.9, temperature=1.0)
    big = torch.zeros(ops.lm_head_sample_workspace_elems(M, Vr, 64) * 2, dtype=torch.int64, device=dev)
    for bad in (dict(top_k=65), dict(top_p=0.0), dict(top_p=1.5), dict(top_k=0, top_p=0.9), dict(temperature=0.0),
                dict(temperature=-1.0)):
        a = {**good, **bad}
        _sample(ops, x, d, w, ld, M, d, Vr, a["top_k"], a["top_p"], a["temperature"], ws=big, expect_error=True)
    short = torch.zeros(ops.lm_head_sample_workspace_elems(M, Vr, 50) - 1, dtype=torch.int64, device=dev)
    _sample(ops, x, d, w, ld, M, d, Vr, 50, ws=short, expect_error=True)
    _sample(ops, x, d, w, ld - 8, M, d, Vr, 50, ws=big, expect_error=True)  # w_ld < V
    _sample(ops, x, d, w, ld + 4, M, d, Vr, 50, ws=big, expect_error=True)  # w_ld not a multiple of 8
    _sample(ops, x, d, w.view(-1)[1:], ld, M, d, Vr, 50, ws=big, expect_error=True)  # w not 16-byte aligned
    with pytest.raises(ValueError):
        ops.lm_head_sample_workspace_elems(M, Vr, 65)


# ----------------------------------------------------------------------------- 5. record / replay
def test_recorded_sample_call_replays_the_call_that_was_made(dev):
    ops, _, _ = _mods()
    from tethys_speech_amd import plan
    M, d, Vr = 2, 128, 160
    x, w, ld = _small(dev, M, d, Vr, dtype=torch.bfloat16)
    ids, lp = torch.empty(M, dtype=torch.int32, device=dev), torch.empty(M, device=dev)
    fin, cnt = torch.zeros(M, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    ws = torch.zeros(ops.lm_head_sample_workspace_elems(M, Vr, 8), dtype=torch.int64, device=dev)
    outs = [ids, lp, cnt]

    def run():
        ops.lm_head_sample(x, d, w, ld, M, d, Vr, ids, 1, fin, cnt, ws, temperature=0.7, top_k=8, top_p=0.8, seed=11, logprob=lp)

    def reset():
        for t in outs:
            t.fill_(-3)
        fin.zero_()

    def snap():
        torch.cuda.synchronize()
        return [t.clone() for t in outs + [fin, ws]]

    same = lambda a, b: all(torch.equal(p, q) for p, q in zip(a, b))  # noqa: E731
    reset()
    run()
    eager = snap()
    assert bool((eager[0] >= 0).all())
    p = plan.LaunchPlan()
    reset()
    with p.recording():
        before = p.launches
        run()
        assert p.launches == before + 1
    assert same(snap(), eager)
    reset()
    p.replay(0, 0)
    assert same(snap(), eager)


# ----------------------------------------------------------------------------- 6. generate on the reduced model
_CACHE = {}


def _setup():
    if not _CACHE:
        _, whisper, O = _mods()
        ocfg = O.make_config("small", dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, **_RED)
        params = O.init_params(ocfg, seed=3, dtype=torch.float64)
        feats = torch.from_numpy(np.random.default_rng(800).standard_normal((3, 80, 800)).astype(np.float32))
        _CACHE["v"] = (params, feats)
    return _CACHE["v"]


def _model(dev, precision, params):
    _, whisper, _ = _mods()
    m = whisper.create_whisper_model("small", device=dev, precision=precision, seed=1234, **_RED)
    m.arena.load_ref({k: v.float() for k, v in params.items()})
    m.refresh_shadows()
    return m


def test_generate_top_k_one_is_greedy_and_seeds_repeat(dev):
    params, feats = _setup()
    f = feats.to(dev)
    model = _model(dev, "fp32", params)
    L = 10
    greedy = model.generate(f, max_length=L).cpu()
    eos, pad = model.config.eos_token_id, model.config.pad_token_id
    got = model.generate(f, max_length=L, do_sample=True, top_k=1, temperature=0.6, seed=9).cpu()
    assert got.dtype == torch.int32 and int(got[0, 0]) == model.config.decoder_start_token_id
    for b in range(3):
        row, ref = got[b].tolist(), greedy[b].tolist()
        n = ref.index(eos) + 1 if eos in ref[1:] else len(ref)
        n = min(n, len(row))
        assert row[:n] == ref[:n] and all(t == pad for t in row[n:] if eos in row[:n])
    kw = dict(max_length=L, do_sample=True, temperature=1.3, top_k=50, top_p=0.95, eos_token_id=-1)
    a, b2, c = model.generate(f, seed=1, **kw), model.generate(f, seed=1, **kw), model.generate(f, seed=2, **kw)
    assert torch.equal(a, b2) and not torch.equal(a, c) and tuple(a.shape) == (3, L + 1)
    g0, g1 = (model.generate(f, seed=s, **{**kw, "top_k": 0, "top_p": None}) for s in (1, 2))
    assert not torch.equal(g0, g1) and bool(((g0 >= 0) & (g0 < V)).all())
    # the not-sampled paths ignore the sampling arguments as before
    assert torch.equal(model.generate(f, max_length=L, temperature=0.5, top_k=3, top_p=0.2, min_length=4), greedy.to(dev))


def test_generate_follows_the_rule_on_the_models_own_logits(dev):
    """Every step's token is the restated rule's on the model's logits / T (fp64, from forward_infer's normalised hidden
    state through the LM head) with that step's seed, on decided rows (b: the top-k test's bound); token_logprobs are
    the log-softmax at the token within that bound;
    sequences_scores and lengths are consistent; min_length keeps an EOS the model does emit out of the first columns."""
    params, feats = _setup()
    f = feats.to(dev)
    p2 = dict(params)
    lm = params["lm_head.kernel"].clone().double()
    eos = 2
    lm[:, eos] = lm[:, eos] * 0 + params["lm_head.kernel"].abs().mean() * 3  # an EOS the model emits often, not always
    p2["lm_head.kernel"] = lm
    p2["decoder.layer_norm.beta"] = params["decoder.layer_norm.beta"] + 0.05
    model = _model(dev, "fp32", p2)
    T, L, seed = 0.9, 8, 77
    pad = model.config.pad_token_id
    for top_k, top_p, min_length in ((50, 0.9, 0), (0, None, 0), (50, 1.0, 5)):
        out = model.generate(f, max_length=L, do_sample=True, temperature=T, top_k=top_k, top_p=top_p, seed=seed,
                             min_length=min_length, return_dict_in_generate=True)
        seq, tlp = out["sequences"].cpu().long(), out["token_logprobs"].cpu().double()
        n = seq.shape[1] - 1
        assert tuple(tlp.shape) == (3, n)
        assert not bool((seq[:, 1:1 + min_length] == eos).any())
        done = np.zeros(3, bool)
        lens = np.full(3, n)
        for t in range(1, n + 1):
            y = model.forward_infer(f, decoder_input_ids=seq[:, :t].to(dev))["last_hidden_state"][:, -1].double().cpu()
            # fp64 from the normalised hidden state through the LM head, as the kernel tests' reference; the top-k test's bound
            logits = (y @ lm).numpy()
            scale = (y.abs() @ lm.abs()).max(1).values.numpy() / T
            s, lse, top = R.rank(logits / T, suppress_id=eos if t <= min_length else -1)
            b = REL * (scale + np.abs(lse))
            st = R.step_seed(seed, t)
            tok, _, dec, _ = R.choose_topk(s, lse, top, st, top_k, 1.0 if top_p is None else top_p, b=b) if top_k else \
                R.choose_gumbel(s, lse, st, b=b)
            for r in range(3):
                if done[r]:
                    assert int(seq[r, t]) == pad and float(tlp[r, t - 1]) == 0.0
                    continue
                if dec[r]:
                    assert int(seq[r, t]) == int(tok[r]), (top_k, t, r)
                want = s[r, int(seq[r, t])] - lse[r]
                within("generate(do_sample) |token_logprob - log_softmax| / (scale + |lse|)",
                       abs(float(tlp[r, t - 1]) - want) / (scale[r] + abs(lse[r])), REL)
                if int(seq[r, t]) == eos:
                    done[r], lens[r] = True, t
        assert out["lengths"].cpu().tolist() == lens.tolist()
        assert torch.allclose(out["sequences_scores"].cpu().double(), tlp.sum(1), atol=1e-5)


def test_generate_min_length_and_the_stop(dev):
    """An EOS column that dominates every row: without min_length every row ends at once; with it EOS stays out of the
    first min_length columns and comes right after; a finished row's later columns are pad."""
    params, feats = _setup()
    f = feats.to(dev)
    p2 = dict(params)
    p2["decoder.layer_norm.beta"] = torch.full_like(params["decoder.layer_norm.beta"], 10.0)
    lm = params["lm_head.kernel"].clone()
    lm[:, 2] = 1.0
    p2["lm_head.kernel"] = lm
    m2 = _model(dev, "fp32", p2)
    for top_k in (0, 50):
        out = m2.generate(f, max_length=9, do_sample=True, top_k=top_k, seed=1, return_dict_in_generate=True)
        assert out["sequences"][:, 1].tolist() == [2, 2, 2] and out["lengths"].tolist() == [1, 1, 1]
        assert out["sequences"].shape[1] == 2
        out = m2.generate(f, max_length=9, do_sample=True, top_k=top_k, seed=1, min_length=5, return_dict_in_generate=True)
        seq = out["sequences"]
        assert tuple(seq.shape) == (3, 7) and not bool((seq[:, 1:6] == 2).any()) and seq[:, 6].tolist() == [2, 2, 2]
        assert out["lengths"].tolist() == [6, 6, 6]
        assert torch.allclose(out["sequences_scores"], out["token_logprobs"].sum(1))


def test_a_row_that_finishes_early_pads_while_the_others_go_on(dev):
    """The end-of-text id is set to the token one row drew at its third step (EOS disabled) of a seeded run: rows are
    independent and the draws do not depend on the id, so the same seed repeats every row up to its first such token;
    from there on that row is pad with log-probability 0 while the other rows continue unchanged."""
    params, feats = _setup()
    f = feats.to(dev)
    model = _model(dev, "fp32", params)
    pad, L = model.config.pad_token_id, 8
    kw = dict(max_length=L, do_sample=True, temperature=1.5, top_k=0, seed=21, return_dict_in_generate=True)
    free = model.generate(f, eos_token_id=-1, **kw)
    a, alp = free["sequences"].cpu(), free["token_logprobs"].cpu()
    e = int(a[0, 3])
    assert e != pad and not bool((a[1:, 1:] == e).any()) and not bool((a[0, 1:3] == e).any()), "pick another seed"
    out = model.generate(f, eos_token_id=e, **kw)
    seq, tlp = out["sequences"].cpu(), out["token_logprobs"].cpu()
    assert tuple(seq.shape) == (3, L + 1) and torch.equal(seq[1:], a[1:]) and torch.equal(tlp[1:], alp[1:])
    assert torch.equal(seq[0, :4], a[0, :4]) and bool((seq[0, 4:] == pad).all())
    assert torch.equal(tlp[0, :3], alp[0, :3]) and bool((tlp[0, 3:] == 0).all())
    assert out["lengths"].tolist() == [3, L, L]
    assert torch.allclose(out["sequences_scores"].cpu(), tlp.sum(1))


# ----------------------------------------------------------------------------- 7. around it
def _train_run(dev, planned, with_generate, steps=4):
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
        for i in range(steps):
            losses.append(step(*next(it)))
            if with_generate:
                before = model._drop_step
                gens.append(model.generate(gfeats, max_length=5, do_sample=True, top_k=(0, 20)[i & 1], seed=i).cpu())
                assert model._drop_step == before
        model.finish_late()
        torch.cuda.synchronize()
        return [float(x.item()) for x in losses], model.arena.p.clone(), model.arena.m.clone(), gens
    finally:
        train.USE_PLAN = old
        ops.set_deterministic(was)


@pytest.mark.parametrize("planned", [False, True])
def test_sampled_generate_between_training_steps_changes_nothing(dev, planned):
    l0, p0, m0, _ = _train_run(dev, planned, False)
    l1, p1, m1, gens = _train_run(dev, planned, True)
    assert l0 == l1, (l0, l1)
    assert torch.equal(p0, p1) and torch.equal(m0, m1)
    assert len(gens) == 4 and all(g.shape[0] == 2 and bool(((g >= 0) & (g < 160)).all()) for g in gens)


def test_transcribe_audio_with_sampling(dev):
    _, whisper, _ = _mods()
    from tethys_speech_amd.frontend import LogMelFrontend
    params, _ = _setup()
    model = _model(dev, "bf16", params)
    kw = dict(do_sample=True, temperature=0.8, top_k=20, top_p=0.9, seed=4)
    got = whisper.transcribe_audio(model, None, max_length=6, **kw)
    feats = LogMelFrontend(device=dev)(torch.from_numpy(whisper.dummy_waveform()).to(dev))
    ref = model.generate(feats, max_length=6, **kw)[0].cpu().numpy()
    assert isinstance(got, np.ndarray) and np.array_equal(got, ref) and got[0] == 50257


def test_full_size_sampled_generate(dev):
    """small-ref, bf16, B = 8, 16 steps.  (d = 768 at 8 rows takes 24 KiB of LDS; the opt-in above 64 KiB is reached by the
    random-input test's d = 1280, M = 17.)"""
    _, whisper, _ = _mods()
    model = whisper.create_whisper_model("small", device=dev, precision="bf16")
    feats = torch.randn(8, 80, 3000, generator=torch.Generator().manual_seed(0)).to(dev)
    out = model.generate(feats, max_length=16, do_sample=True, top_k=50, top_p=0.9, seed=3, eos_token_id=-1,
                         return_dict_in_generate=True)
    seq = out["sequences"]
    assert tuple(seq.shape) == (8, 17) and seq.dtype == torch.int32
    assert bool((seq[:, 0] == 50257).all()) and bool(((seq >= 0) & (seq < V)).all())
    assert bool((out["lengths"] == 16).all()) and bool(torch.isfinite(out["token_logprobs"]).all())
    assert bool((out["token_logprobs"] <= 0).all())
