"""``WhisperForConditionalGeneration.evaluate`` / ``.score`` on the GPU, on the reduced model of the decoding tests (d_model
128, 2 + 2 layers, 2 heads, d_ff 256, the real vocabulary): against the fp64 oracle and tests/_eval_ref.py, against the
training step's own loss, against beam search's scores, mask cases, non-interference with training, peak memory, and one
full-size call.

The LM head of the oracle-parity tests is the initialiser's plus six columns g * u (gains 4, 2, 1, -1, -2, -4 along one
unit direction u, at columns on both sides of the chunk boundaries), and the decoder's final LayerNorm gets the bias
0.3 * sqrt(d) * u: with the initialiser alone the largest of 51865 near-equal logits is closer to the runner-up than bf16
can tell, and the accuracy comparison would decide nothing.  With them x = h . u is 3.4 +- 1 in every row, the top two
logits are 4 x (column 30000, in the fourth chunk) and 2 x, far enough apart for bf16, and the top logit is of the size of
the other 51859 columns' log-sum-exp (10.9), so the softmax is not degenerate.  Labels equal to the top column are planted
at a third of the positions, so the accuracy compared is not 0 == 0.

``scale`` is the rounding scale of a row's logits, max_n sum_k |h_k w_kn| (tests/_sample_ref.py's), from the oracle's
decoder output h and LM head w."""
import numpy as np
import pytest
import torch

import _eval_ref as E
from _margins import within

pytestmark = pytest.mark.gpu

V, VP = 51865, 51904
T_IN = 300
_RED = dict(d_model=128, encoder_attention_heads=2, decoder_attention_heads=2, d_ff=256, encoder_layers=2, decoder_layers=2)
PEAK_COLS, PEAK_GAINS, PEAK_BIAS = (30000, 8191, 8192, 11, 49152, 51864), (4.0, 2.0, 1.0, -1.0, -2.0, -4.0), 0.3
PARAM_SEED, DATA_SEED = 3, 21

# Bounds, each about twice the largest value measured on an MI355X (profiles/r09_eval_margins.json, the
# record the test session writes of every figure that goes through ``within``):
# |logit - oracle| / scale: fp32 2.0e-7, bf16 2.3e-3 (bf16 activations through 2 + 2 layers)
LOGIT_REL = {"fp32": 4e-7, "bf16": 4.6e-3}
# |token_logprob - fp64| / (scale + |lse|), the largest over the rows: fp32 1.3e-7, bf16 1.3e-3
LP_REL = {"fp32": 2.7e-7, "bf16": 2.5e-3}
# |loss - fp64| / mean(scale + |lse|), plain and masked, a comparison of its own: fp32 2.3e-8, bf16 3.2e-4.  The rows' errors
# largely cancel in the mean, so a bias common to the rows (a weight normalisation, a drifting fold) shows here long before
# it reaches the per-row bound.  evaluate's sums are fp64 on the host, so the fp32 figure has no floor of its own to respect.
LOSS_REL = {"fp32": 4.7e-8, "bf16": 6.4e-4}
# |evaluate loss - forward_backward loss| / max(1, loss), the training path as the yardstick: fp32 1.7e-8, bf16 5.4e-8 at a
# loss of 9.3.  The yardstick is an fp32 number: one ulp of it is 1.0e-7 of its value, and the bound is not put below that.
TRAIN_REL = {"fp32": 1.1e-7, "bf16": 1.1e-7}
# |sequences_logprob / len - beam score| / max(1, |score|), beam search's own scores as the yardstick: fp32 1.7e-7, bf16 3.9e-3
# (bf16: tmi_lm_head_topk normalises the hidden state in fp32 and never rounds a logit; here both pass through bf16)
BEAM_REL = {"fp32": 3.4e-7, "bf16": 8e-3}

_CACHE = {}


def _mods():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import ops, whisper
    from oracle import whisper_oracle as O
    return ops, whisper, O


def _setup():
    if "setup" not in _CACHE:
        _, _, O = _mods()
        ocfg = O.make_config("small", dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, **_RED)
        params = O.init_params(ocfg, seed=PARAM_SEED, dtype=torch.float64)
        u = torch.randn(ocfg.d_model, generator=torch.Generator().manual_seed(PARAM_SEED), dtype=torch.float64)
        u /= u.norm()
        lm = params["lm_head.kernel"].clone()
        for c, g in zip(PEAK_COLS, PEAK_GAINS):
            lm[:, c] = g * u
        params["lm_head.kernel"] = lm
        params["decoder.layer_norm.beta"] = params["decoder.layer_norm.beta"] + PEAK_BIAS * ocfg.d_model ** 0.5 * u
        feats = torch.from_numpy(np.random.default_rng(DATA_SEED).standard_normal((3, 80, T_IN)).astype(np.float32))
        _CACHE["setup"] = (ocfg, params, feats)
    return _CACHE["setup"]


def _oracle_params(precision):
    """The oracle's parameters: for bf16 with the kernels rounded to bf16, the values the kernels read."""
    key = ("params", precision)
    if key not in _CACHE:
        _, params, _ = _setup()
        p = dict(params)
        if precision == "bf16":
            for k in p:
                if k.endswith(".kernel"):
                    p[k] = p[k].to(torch.bfloat16).double()
        _CACHE[key] = p
    return _CACHE[key]


def _case(precision, B, S):
    """Batch, oracle logits and fp64 references of one (precision, B, S), computed once on the host."""
    key = (precision, B, S)
    if key in _CACHE:
        return _CACHE[key]
    _, _, O = _mods()
    ocfg, _, feats = _setup()
    p = _oracle_params(precision)
    f = feats[:B]
    rng = np.random.default_rng(100 * B + S)
    labels = rng.integers(0, V, (B, S)).astype(np.int32)
    labels[:, 1:][rng.random((B, S - 1)) < 0.34] = PEAK_COLS[0]  # planted hits (row t is scored against labels[:, t + 1])
    labels[0, S - 1] = PEAK_COLS[0]
    labels = torch.from_numpy(labels)
    loss_ref, _ = O.forward_loss(p, f, labels, ocfg, training=False)
    # the same forward, with the decoder output kept: the logits and their rounding scale
    enc = O.encoder(p, f.double(), ocfg, training=False)
    h = O.decoder(p, O.decoder_input_ids(labels, ocfg.decoder_start_token_id), enc, ocfg, training=False).reshape(B * S, -1)
    lm = p["lm_head.kernel"][:, :V]
    z = (h @ lm).numpy()
    scale = (h.abs() @ lm.abs()).max(dim=1).values.numpy()
    mask = (rng.random((B, S)) < 0.7).astype(np.int32)
    mask[0, 0] = 1
    out = dict(feats=f, labels=labels, z=z, loss=float(loss_ref), mask=mask, scale=scale, gap=E.top2_gap(z, V))
    for name, m in (("plain", None), ("masked", mask)):
        t, w = E.shift_targets(labels.numpy(), m)
        lse, arg, lp = E.fold(z, V, t.reshape(-1))
        out[name] = dict(t=t, w=w, lse=lse.reshape(B, S), arg=arg.reshape(B, S), lp=lp.reshape(B, S))
    _CACHE[key] = out
    return out


def _model(dev, precision):
    _, whisper, _ = _mods()
    _, params, _ = _setup()
    m = whisper.create_whisper_model("small", device=dev, precision=precision, **_RED)
    m.arena.load_ref({k: v.float() for k, v in params.items()})
    m.refresh_shadows()
    return m


def _check_sums(tag, got, ref, c, precision, undecided, checks):
    """loss and accuracy of ``got`` (evaluate's dict) against the fp64 reference ``ref`` of case ``c``; the loss figure is
    appended to ``checks`` (name, measured, bound) for the caller to assert once every figure is printed."""
    B, S = ref["t"].shape
    unit = (c["scale"] + np.abs(ref["lse"].reshape(-1))).reshape(B, S)[:, :-1]
    w = ref["w"]
    loss, acc, loss_sum, n_correct, n_tokens = E.weighted(ref["lp"], ref["arg"], ref["t"], w)
    assert got["n_tokens"] == n_tokens and abs(got["loss"] - got["loss_sum"] / got["n_tokens"]) < 1e-15
    mean_unit = float((w * unit).sum() / w.sum())
    e = abs(got["loss"] - loss) / mean_unit
    print(f"evaluate {tag}: |loss - fp64| / mean(scale + |lse|) = {e:.3e} (loss {got['loss']:.6f}, fp64 {loss:.6f})")
    checks.append((f"evaluate {precision} |loss - fp64| / mean(scale + |lse|)", e, LOSS_REL[precision]))
    # accuracy: the undecided rows are left out - they may go either way
    und = undecided.reshape(B, S)[:, :-1]
    hit = (ref["arg"][:, :-1] == ref["t"][:, :-1]).astype(np.float64)
    lo = float((w * hit * ~und).sum())
    hi = lo + float((w * und).sum())
    assert lo <= got["n_correct"] <= hi, (tag, got["n_correct"], lo, hi)
    assert abs(got["accuracy"] - got["n_correct"] / got["n_tokens"]) < 1e-15
    return loss


@pytest.mark.parametrize("S", [2, 9])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_evaluate_matches_oracle(dev, precision, B, S):
    """loss against oracle.forward_loss(training=False); token log-probabilities, the masked loss and the accuracy against
    tests/_eval_ref.py fed the oracle's logits (bf16: the oracle on the bf16-rounded kernels)."""
    c = _case(precision, B, S)
    # from the oracle alone, before anything is launched: at most 1 % of the rows may be undecided
    undecided = c["gap"] <= 2 * LOGIT_REL[precision] * c["scale"]
    assert undecided.sum() <= 0.01 * undecided.size, (undecided.sum(), undecided.size, "pick other seeds")
    model = _model(dev, precision)
    feats, labels = c["feats"].to(dev), c["labels"].to(dev)
    got = model.evaluate(feats, labels, return_token_logprobs=True)
    ref = c["plain"]
    assert abs(E.weighted(ref["lp"], ref["arg"], ref["t"], ref["w"])[0] - c["loss"]) < 1e-9  # the restatement is the oracle's loss
    # the logit error the undecided rule assumes, checked on the materialised route
    z = model(feats, labels=labels, training=False)["logits"].double().cpu().reshape(B * S, V).numpy()
    e = float((np.abs(z - c["z"]).max(axis=1) / c["scale"]).max())
    print(f"evaluate {precision} B{B} S{S}: |logit - oracle| / scale = {e:.3e}")
    checks = [(f"evaluate {precision} |logit - oracle| / scale", e, LOGIT_REL[precision])]
    lp = got["token_logprobs"]
    assert lp.shape == (B, S - 1) and lp.dtype == torch.float32
    unit = (c["scale"] + np.abs(ref["lse"].reshape(-1))).reshape(B, S)[:, :-1]
    e = float((np.abs(lp.double().cpu().numpy() - ref["lp"][:, :-1]) / unit).max())
    print(f"evaluate {precision} B{B} S{S}: |token_logprob - fp64| / (scale + |lse|) = {e:.3e}")
    checks.append((f"evaluate {precision} |token_logprob - fp64| / (scale + |lse|)", e, LP_REL[precision]))
    _check_sums(f"{precision} B{B} S{S}", got, ref, c, precision, undecided, checks)
    assert isinstance(got["loss"], float) and isinstance(got["accuracy"], float)
    assert got["n_correct"] >= 1.0  # (the planted hits: the accuracy comparison is not 0 == 0)
    gm = model.evaluate(feats, labels, decoder_attention_mask=torch.from_numpy(c["mask"]).to(dev), return_token_logprobs=True)
    _check_sums(f"{precision} B{B} S{S} masked", gm, c["masked"], c, precision, undecided, checks)
    for name, measured, bound in checks:
        within(name, measured, bound)
    w = torch.from_numpy(c["masked"]["w"])
    assert bool((gm["token_logprobs"].cpu()[w == 0] == 0).all())
    assert torch.equal(gm["token_logprobs"].cpu()[w > 0], lp.cpu()[w > 0])  # a row's score does not depend on the others' weights


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_evaluate_agrees_with_the_training_loss(dev, precision):
    """Dropout off, same weights, same batch: the loss ``forward_backward`` reports (one fused row pass over materialised
    logits) and ``evaluate``'s (chunks folded online) differ in the order of the log-sum-exp only."""
    c = _case(precision, 3, 9)
    model = _model(dev, precision)
    feats, labels = c["feats"].to(dev), c["labels"].to(dev)
    train_loss = float(model.forward_backward(feats, labels).item())
    got = model.evaluate(feats, labels)["loss"]
    e = abs(got - train_loss) / max(1.0, abs(train_loss))
    print(f"evaluate {precision}: |loss - training loss| / max(1, loss) = {e:.3e} ({got:.7f} vs {train_loss:.7f})")
    within(f"evaluate {precision} |loss - forward_backward loss| / max(1, loss)", e, TRAIN_REL[precision])


def test_mask_cases(dev):
    c = _case("fp32", 3, 9)
    model = _model(dev, "fp32")
    feats, labels = c["feats"].to(dev), c["labels"].to(dev)
    plain = model.evaluate(feats, labels, return_token_logprobs=True)
    ones = model.evaluate(feats, labels, decoder_attention_mask=torch.ones(3, 9, dtype=torch.int32, device=dev),
                          return_token_logprobs=True)
    assert torch.equal(plain["token_logprobs"], ones["token_logprobs"])
    assert all(plain[k] == ones[k] for k in ("loss", "accuracy", "loss_sum", "n_correct", "n_tokens"))
    # one item masked except for a single token; the mask's last column is not a weight (W:597)
    mask = torch.ones(3, 9, dtype=torch.int32)
    mask[1] = 0
    mask[1, 4] = 1
    mask[2, 8] = 0
    got = model.evaluate(feats, labels, decoder_attention_mask=mask, return_token_logprobs=True)
    w = mask[:, :-1].double()
    lp = got["token_logprobs"].double().cpu()
    assert got["n_tokens"] == 17.0 and bool((lp[1, [0, 1, 2, 3, 5, 6, 7]] == 0).all())
    assert torch.equal(got["token_logprobs"][w.to(dev) > 0], plain["token_logprobs"][w.to(dev) > 0])
    assert got["loss_sum"] == float(-(w * lp).sum()) and got["loss"] == got["loss_sum"] / 17.0
    # float weights are the reference's tf.cast(mask): a weight of 0.5 counts half
    half = model.evaluate(feats, labels, decoder_attention_mask=mask.float() * 0.5)
    assert half["n_tokens"] == 8.5 and abs(half["loss"] - got["loss"]) <= 1e-12 * abs(got["loss"])
    whisper = _mods()[1]
    for bad in (torch.zeros(3, 9, dtype=torch.int32), torch.cat([torch.zeros(3, 8), torch.ones(3, 1)], dim=1)):
        with pytest.raises(ValueError):
            model.evaluate(feats, labels, decoder_attention_mask=bad)
    with pytest.raises(ValueError):
        whisper.check_evaluate_args(model.config, (3, 9), (3, 9), mask_sum=0.0)
    with pytest.raises(ValueError):
        model.evaluate(feats, labels[:, :1])
    with pytest.raises(ValueError):
        model.evaluate(feats, torch.full((3, 9), V, dtype=torch.int32, device=dev))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_score_reproduces_beam_search_scores(dev, precision):
    """Two independent kernels against each other: tmi_lm_head_topk's log-probabilities summed by tmi_beam_step, and
    tmi_logprob_fold over the chunked LM head of the same prefixes."""
    model = _model(dev, precision)
    _, _, feats = _setup()
    f = feats[:2].to(dev)
    K, R, L, lpen = 3, 2, 6, 1.0
    out = model.generate(f, max_length=L, num_beams=K, num_return_sequences=R, length_penalty=lpen, return_dict_in_generate=True)
    seq, scores, lens = out["sequences"], out["sequences_scores"].double().cpu(), out["lengths"]
    got = model.score(f, seq, lens)
    n = seq.shape[1] - 1
    assert got["token_logprobs"].shape == (2 * R, n) and got["sequences_logprob"].shape == (2 * R,)
    tl = got["token_logprobs"].double().cpu()
    ln = lens.cpu().long()
    assert bool((tl[torch.arange(n)[None, :] >= ln[:, None]] == 0).all()) and bool((tl[torch.arange(n)[None, :] < ln[:, None]] < 0).all())
    assert np.allclose(E.score_sums(tl.numpy(), ln.numpy()), got["sequences_logprob"].double().cpu().numpy(), rtol=1e-6, atol=0)
    mine = got["sequences_logprob"].double().cpu() / ln.double() ** lpen
    e = float(((mine - scores).abs() / scores.abs().clamp(min=1.0)).max())
    print(f"score {precision}: |sequences_logprob / len - beam score| / max(1, |score|) = {e:.3e}")
    within(f"score {precision} |sequences_logprob / len - beam score| / max(1, |score|)", e, BEAM_REL[precision])
    # features given per sequence instead of per item: the same scores (the encoder then runs N times)
    again = model.score(f.repeat_interleave(R, 0), seq, lens)["sequences_logprob"].double().cpu() / ln.double() ** lpen
    within(f"score {precision} |sequences_logprob / len - beam score| / max(1, |score|)",
           float(((again - scores).abs() / scores.abs().clamp(min=1.0)).max()), BEAM_REL[precision])
    # a shorter length scores a prefix: the first token's decoder run is the same in both calls, the LayerNorm works row by
    # row, and the LM head's rows do not mix - measured on an MI355X the first token's score is the same to the bit (0.0 in
    # both precisions), and that is what is asserted
    short = model.score(f, seq, torch.ones_like(lens))
    assert torch.equal(short["token_logprobs"][:, 0], got["token_logprobs"][:, 0])
    assert bool((short["token_logprobs"][:, 1:] == 0).all())
    with pytest.raises(ValueError):  # sequences must start with the start token
        model.score(f, seq[:, 1:], None)


def _train_run(dev, planned, with_eval, steps=6):
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
        ef, el = next(iter(create_dummy_dataset(2, n_mels=16, seq_len=80, max_target_length=10, device=dev, seed=4, num_samples=2)))
        train.USE_PLAN = planned
        step = train.planned_step(strategy, model, opt, "whisper", pipelined=True)
        losses, evals = [], []
        for _ in range(steps):
            losses.append(step(*next(it)))
            if with_eval:
                before = model._drop_step
                evals.append(model.evaluate(ef, el)["loss"])
                assert model._drop_step == before
        model.finish_late()
        torch.cuda.synchronize()
        extra = None
        if with_eval:  # dropout is off inside evaluate even after enable_dropout: two calls agree to the bit; generate is unchanged by it
            g0 = model.generate(ef, max_length=5)
            a, b = model.evaluate(ef, el)["loss"], model.evaluate(ef, el)["loss"]
            extra = (a == b, torch.equal(g0, model.generate(ef, max_length=5)))
        return [float(x.item()) for x in losses], model.arena.p.clone(), model.arena.m.clone(), evals, extra
    finally:
        train.USE_PLAN = old
        ops.set_deterministic(was)


@pytest.mark.parametrize("planned", [False, True])
def test_evaluate_between_training_steps_changes_nothing(dev, planned):
    """step, evaluate, step == step, step to the bit (losses, parameters, Adam moments), on plain launches and on a recorded
    plan, with dropout enabled for training."""
    l0, p0, m0, _, _ = _train_run(dev, planned, False)
    l1, p1, m1, evals, extra = _train_run(dev, planned, True)
    assert l0 == l1, (l0, l1)
    assert torch.equal(p0, p1) and torch.equal(m0, m1)
    assert len(evals) == 6 and all(np.isfinite(evals)) and len(set(evals)) == 6  # (the weights moved between them)
    assert extra == (True, True)


def test_peak_memory_stays_below_half_the_logits(dev):
    """B = 2, S = 448: with the workspace warm, evaluate's peak above the level before the call stays under half of
    B * S * Vp * elt - the chunk scratch is [B*S, 8192] of the 51904 columns; the materialised route cannot meet it."""
    model = _model(dev, "bf16")
    _, _, feats = _setup()
    B, S = 2, 448
    f = feats[:B].to(dev)
    labels = torch.from_numpy(np.random.default_rng(1).integers(0, V, (B, S)).astype(np.int32)).to(dev)
    half = B * S * VP * 2 // 2
    model.evaluate(f, labels)
    torch.cuda.synchronize()
    assert model._inf["ws"]["lp_chunk"].numel() * 2 < half // 2
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    out = model.evaluate(f, labels)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    assert peak < half, (peak, half)
    assert np.isfinite(out["loss"]) and out["n_tokens"] == B * (S - 1)
    torch.cuda.reset_peak_memory_stats(dev)
    logits = model(f, labels=labels, training=False)["logits"]
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated(dev) - base >= 2 * half and logits.shape == (B, S, V)


def test_full_size_evaluate(dev):
    _, whisper, _ = _mods()
    model = whisper.create_whisper_model("small", device=dev, precision="bf16")
    rng = np.random.default_rng(2)
    f = torch.from_numpy(rng.standard_normal((1, 80, 3000)).astype(np.float32)).to(dev)
    labels = torch.from_numpy(rng.integers(0, V, (1, 8)).astype(np.int32)).to(dev)
    out = model.evaluate(f, labels, return_token_logprobs=True)
    assert np.isfinite(out["loss"]) and 0.0 <= out["accuracy"] <= 1.0 and out["n_tokens"] == 7.0
    assert out["token_logprobs"].shape == (1, 7) and bool(torch.isfinite(out["token_logprobs"]).all())
    assert abs(out["loss"] - np.log(V)) < 1.0  # an untrained head: close to the uniform distribution's log V
