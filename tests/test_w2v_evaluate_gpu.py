"""``Wav2Vec2ForPreTraining.evaluate`` on the GPU: the reduced model and clips of tests/test_w2v_infer_gpu.py (B = 3, 2600
samples = 130 frames, lengths 2600 / 1700 / 330 = 130 / 85 / 17 frames), fp32 and bf16, against the float64 restatement
tests/_w2v_eval_ref.py; the same loss as ``forward_backward`` on an unmasked batch; an evaluation between two training steps
that changes nothing; one full-size call.

The projections are compared in the error form of test_w2v_infer_gpu.py with the device's own code choices fed to the
restatement (tests/test_w2v_kernels_gpu.py judges the argmin itself; a near-tie resolved differently must not mask everything
else).  Row losses and flags are recomputed in float64 from the device's own projections under the derived bounds of
tests/test_w2v_score_gpu.py; everything behind them (counts, sums, perplexity, loss) is exact host arithmetic."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _w2v_eval_ref as E  # noqa: E402
from _margins import within  # noqa: E402
from oracle import wav2vec2_oracle as V  # noqa: E402
from test_w2v_infer_gpu import B_M, CAP, SAMPLE_LENGTHS, T_IN, _train_inputs, model_err, ref_params  # noqa: E402
from test_w2v_score_gpu import TEMP, judge  # noqa: E402
from test_wav2vec2_gpu import build  # noqa: E402

T_M = 130
# Bounds at about twice what the first GPU run measured against the float64 restatement (profiles/r10_w2v_eval_margins.json;
# worst of the masked / unmasked calls, fp32 relative max: 6.8e-7, 2.1e-7; bf16 relative L2: 6.6e-3, 2.9e-3), under the caps of
# the classes (tests/test_w2v_infer_gpu.py CAP): fp32 1e-4 relative max, bf16 6e-2 relative L2 per tensor
BOUND = {"fp32": {"projected_states": 1.4e-6, "projected_quantized_features": 4.5e-7},
         "bf16": {"projected_states": 1.3e-2, "projected_quantized_features": 6e-3}}


@pytest.fixture(scope="module")
def clips():
    return torch.from_numpy(V.create_dummy_pool(seed=21, num_samples=B_M, length=T_IN))


def _negatives(model, B, T, seed=31):
    from tethys_speech_amd import wav2vec2
    return torch.from_numpy(wav2vec2.sample_negative_indices(np.random.default_rng(seed), B, T, model.config.num_negatives))


def check_evaluate(tag, precision, model, ocfg, clips, neg, mask, dev):
    out = model.evaluate(clips.to(dev), neg.to(dev), attention_mask=mask, return_rows=True)
    torch.cuda.synchronize()
    cfg = model.config
    G, Nc, pd = cfg.num_codevector_groups, cfg.num_codevectors_per_group, cfg.proj_codevector_dim
    assert out["row_loss"].shape == (B_M, T_M) and out["row_correct"].dtype == torch.int32
    assert out["code_indices"].shape == (B_M, T_M, G) and out["projected_states"].shape == (B_M, T_M, pd)
    assert all(isinstance(out[k], float) for k in ("loss", "contrastive_loss", "accuracy", "perplexity", "loss_sum", "n_correct", "n_frames"))
    codes = out["code_indices"].cpu()
    assert int(codes.min()) >= 0 and int(codes.max()) < Nc
    # the projections against the restatement, on the device's own code choices
    ref = E.forward(ref_params(model, precision), clips.double(), ocfg, None if mask is None else mask.double(), force_idx=codes.long())
    for n in ("projected_states", "projected_quantized_features"):
        e = model_err(precision, out[n], ref[n])
        print(f"w2v evaluate {tag} {precision} {n}: {e:.3e}")
        within(f"w2v evaluate {tag} {precision} {n}", e, min(BOUND[precision][n], CAP[precision]))
    # rows and flags: float64 on the device's own projections, the kernel test's derived bounds
    m = None if mask is None else mask.numpy()
    rs = E.score(out["projected_states"].double().cpu().numpy(), out["projected_quantized_features"].double().cpu().numpy(),
                 neg.numpy(), TEMP, m)
    row_loss, row_correct = out["row_loss"].cpu(), out["row_correct"].cpu()
    judge(f"evaluate {tag} {precision}", row_loss.double().numpy(), row_correct.numpy(), rs, pd, neg.shape[1], band_share=1.0)
    # counts, sums, perplexity, loss: exact host arithmetic from there
    want = E.code_counts(codes.reshape(-1, G).numpy(), Nc, None if m is None else m.reshape(-1))
    assert out["code_counts"].dtype == torch.int64 and np.array_equal(out["code_counts"].numpy(), want)
    n_frames = float(B_M * T_M if m is None else m.sum())
    assert out["n_frames"] == n_frames and (want.sum(1) == n_frames).all()
    assert out["n_correct"] == float(row_correct.sum()) and 0 < out["n_correct"] <= n_frames
    assert abs(out["loss_sum"] - float(row_loss.double().sum())) <= 1e-12 * abs(out["loss_sum"])
    assert out["contrastive_loss"] == out["loss_sum"] / n_frames and out["accuracy"] == out["n_correct"] / n_frames
    assert abs(out["perplexity"] - E.perplexity_from_counts(want)) <= 1e-12 * out["perplexity"]
    assert out["loss"] == out["contrastive_loss"] - cfg.diversity_loss_weight * out["perplexity"]
    plain = model.evaluate(clips.to(dev), neg.to(dev), attention_mask=mask)
    assert "row_loss" not in plain and plain["loss_sum"] == out["loss_sum"] and torch.equal(plain["code_counts"], out["code_counts"])
    return out


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_evaluate_matches_restatement(dev, precision, clips):
    from tethys_speech_amd import ops, wav2vec2
    model, ocfg, _ = build(precision, dev)
    mask = wav2vec2.frame_attention_mask(model.config, SAMPLE_LENGTHS, T_IN)
    assert mask.sum(1).tolist() == [130.0, 85.0, 17.0]
    neg = _negatives(model, B_M, T_M)
    was = ops.set_deterministic(True)  # (the stem's GroupNorm statistics: the two calls of check_evaluate are compared exactly)
    try:
        masked = check_evaluate("masked", precision, model, ocfg, clips, neg, mask, dev)
        assert masked["n_frames"] == 232.0
        assert bool((masked["row_loss"].cpu()[mask == 0] == 0).all()) and bool((masked["row_correct"].cpu()[mask == 0] == 0).all())
        unmasked = check_evaluate("unmasked", precision, model, ocfg, clips, neg, None, dev)
    finally:
        ops.set_deterministic(was)
    # (c) the mask matters: the shortest clip's valid rows differ between the two calls
    d = (masked["row_loss"][2, :17] - unmasked["row_loss"][2, :17]).abs().max()
    assert float(d) > 1e-3, float(d)
    # the training state was never touched: no workspace set, no step counted
    assert model._ws_key is None and model._ws_sets == {} and model._drop_step == 0


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_evaluate_loss_equals_forward_backward_loss(dev, precision, clips):
    """(b) Unmasked, dropout off, the two run the same kernels up to the projections (the quantiser's choices are compared
    exactly).  The difference of the two losses is bounded by the mean of the derived row bounds - the route from the
    projections to the rows - plus the fp32 rounding of the step's perplexity kernel, weighted by diversity_loss_weight.  That
    kernel, per group: p = count / n, + 1e-10, logf, product (4 roundings of a term), terms of one sign summed by 256 threads
    (ceil(Nc / 256) - 1 adds in a thread, 6 in the wave, 3 across waves), so s = sum p log p carries (4 + ceil(Nc / 256) + 8) U
    relative, exp(-s) that times |s| <= log(Nc), plus expf, the sum over groups and the division: 4 more."""
    from tethys_speech_amd import ops
    model, ocfg, _ = build(precision, dev)
    cfg = model.config
    neg = _negatives(model, B_M, T_M)
    was = ops.set_deterministic(True)
    try:
        step_loss = float(model.forward_backward(clips.to(dev), neg.to(dev)).item())
        step_ppl = float(model.ws["perplexity"].item())
        step_codes = model.ws["code_idx"].cpu().clone()
        out = model.evaluate(clips.to(dev), neg.to(dev), return_rows=True)
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(was)
    assert torch.equal(out["code_indices"].cpu().reshape(step_codes.shape), step_codes), "the quantiser chose other codes"
    rs = E.score(out["projected_states"].double().cpu().numpy(), out["projected_quantized_features"].double().cpu().numpy(),
                 neg.numpy(), TEMP)
    bound_rows, _ = E.bounds(rs, cfg.proj_codevector_dim, neg.shape[1])
    Nc = cfg.num_codevectors_per_group
    ppl_bound = (np.log(Nc) * (4 + -(-Nc // 256) + 8) + 4) * E.U * out["perplexity"]
    within(f"w2v evaluate {precision} perplexity vs tmi_vq_nearest / bound", abs(out["perplexity"] - step_ppl) / ppl_bound, 1.0)
    bound = float(bound_rows.mean()) + cfg.diversity_loss_weight * ppl_bound
    diff = abs(out["loss"] - step_loss)
    print(f"w2v evaluate {precision} loss {out['loss']:.6f} against the step's {step_loss:.6f}: {diff:.3e} (bound {bound:.3e})")
    within(f"w2v evaluate {precision} loss vs forward_backward / bound", diff / bound, 1.0)


def _eval_call(model, dev):
    from tethys_speech_amd import wav2vec2
    c = model.config
    clip = torch.from_numpy(V.create_dummy_pool(seed=5, num_samples=2, length=700)).to(dev)
    mask = wav2vec2.frame_attention_mask(c, (700, 250), 700)
    neg = _negatives(model, 2, mask.shape[1], seed=6).to(dev)
    out = model.evaluate(clip, neg, attention_mask=mask)
    assert np.isfinite(out["loss"]) and out["n_frames"] == float(mask.sum())


def test_evaluation_between_training_steps_changes_nothing(dev):
    """(d) eager: two teacher-forced training steps (bf16, dropout on); in the third run an evaluate call - another batch
    size, with a mask - sits between them.  The comparison form of test_inference_between_training_steps_changes_nothing."""
    from tethys_speech_amd import ops

    def run(evaluate):
        model, _, _ = build("bf16", dev)
        c = model.config
        model.enable_dropout(c.hidden_dropout, c.attention_dropout, seed=11, act_p=c.activation_dropout)
        steps = [_train_inputs(model, 3, 400, 50 + i, dev) for i in range(2)]
        model.forward_backward(steps[0][0], steps[0][1], forced_codes=steps[0][2])
        before = (model._drop_step, model._ws_key, bool(getattr(model.arena, "g_clean", False)), sorted(model._ws_sets))
        if evaluate:
            _eval_call(model, dev)
        state = (model._drop_step, model._ws_key, bool(getattr(model.arena, "g_clean", False)), sorted(model._ws_sets))
        assert state == before and model._drop_step == 1
        loss = model.forward_backward(steps[1][0], steps[1][1], forced_codes=steps[1][2])
        torch.cuda.synchronize()
        return float(loss.item()), model.arena.g.clone(), state

    was = ops.set_deterministic(True)
    try:
        l0, g0, s0 = run(False)
        l1, g1, s1 = run(False)
        l2, g2, s2 = run(True)
    finally:
        ops.set_deterministic(was)
    assert s0 == s1 == s2, (s0, s2)
    spread_g, spread_l = float((g0 - g1).abs().max()), abs(l0 - l1)
    if spread_g == 0.0 and spread_l == 0.0:
        print("plain runs agree bit for bit: comparing the run with the evaluate call bit for bit")
        assert l2 == l0 and torch.equal(g2, g0)
    else:
        print(f"plain runs differ (loss {spread_l:.2e}, gradients {spread_g:.2e}): comparing within 4 x that spread")
        assert abs(l2 - l0) <= max(4.0 * spread_l, 1e-6 * abs(l0)), (l2, l0, spread_l)
        assert float((g2 - g0).abs().max()) <= max(4.0 * spread_g, 1e-7), (float((g2 - g0).abs().max()), spread_g)


def test_recorded_plan_replays_the_same_after_an_evaluate_call(dev):
    """(d) planned: the form of test_recorded_plan_replays_the_same_after_an_inference_call."""
    from tethys_speech_amd import ops, optim, train
    from tethys_speech_amd.dist import DataParallelStrategy

    def run(evaluate):
        model, _, _ = build("bf16", dev)
        c = model.config
        model.enable_dropout(c.hidden_dropout, c.attention_dropout, seed=11, act_p=c.activation_dropout)
        opt = optim.Adam(3e-4, epsilon=1e-8)
        inputs = [_train_inputs(model, 3, 400, 60 + i, dev)[:2] for i in range(3)]
        old, train.USE_PLAN = train.USE_PLAN, True
        try:
            step = train.planned_step(DataParallelStrategy(0, 1, init=False), model, opt, "wav2vec2", pipelined=True)
            losses = []
            for i in range(8):
                if evaluate and i == 5:
                    assert step.planned is not None and step.planned.replays >= 1, "no plan was recorded before the call"
                    drop_step = model._drop_step
                    _eval_call(model, dev)
                    assert model._drop_step == drop_step
                losses.append(step(*inputs[i % 3]))
            model.finish_late()
            torch.cuda.synchronize()
            assert step.planned is not None and step.planned.replays >= 4
            return [float(x.item()) for x in losses], model.arena.p.clone()
        finally:
            train.USE_PLAN = old

    was = ops.set_deterministic(True)
    try:
        la, pa = run(False)
        lb, pb = run(False)
        lc, pc = run(True)
    finally:
        ops.set_deterministic(was)
    spread = float((pa - pb).abs().max())
    print(f"planned runs: spread {spread:.2e}, with the evaluate call {float((pa - pc).abs().max()):.2e}")
    assert float((pa - pc).abs().max()) <= max(4.0 * spread, 1e-7), (float((pa - pc).abs().max()), spread)
    assert max(abs(a - b) for a, b in zip(la, lc)) <= max(4.0 * max(abs(a - b) for a, b in zip(la, lb)), 1e-6 * abs(la[0])), (la, lc)


def test_evaluate_full_size(dev):
    """(e) Wav2Vec2-base, B = 8, 2 s clips, bf16: shapes, finiteness and the counts only."""
    from tethys_speech_amd import wav2vec2
    model = wav2vec2.create_full_model("pretraining", "base", device=dev, precision="bf16")
    cfg = model.config
    audio = torch.from_numpy(V.create_dummy_pool(seed=3, num_samples=8, length=32000)).to(dev)
    T = wav2vec2.frame_lengths(cfg, [32000])[0]
    assert T == 100
    neg = _negatives(model, 8, T).to(dev)
    out = model.evaluate(audio, neg, return_rows=True)
    torch.cuda.synchronize()
    assert out["row_loss"].shape == (8, 100) and out["row_correct"].shape == (8, 100)
    assert out["code_indices"].shape == (8, 100, 2) and out["projected_states"].shape == (8, 100, 256)
    assert out["projected_quantized_features"].shape == (8, 100, 256) and out["code_counts"].shape == (2, 320)
    assert bool(torch.isfinite(out["row_loss"]).all()) and bool(torch.isfinite(out["projected_states"].float()).all())
    assert all(np.isfinite(out[k]) for k in ("loss", "contrastive_loss", "accuracy", "perplexity", "loss_sum"))
    assert out["n_frames"] == 800 and out["code_counts"].sum(1).tolist() == [800, 800]
    assert 0 <= out["n_correct"] <= 800 and 1.0 <= out["perplexity"] <= 320.0
