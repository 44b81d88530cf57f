"""Launch plans (include/tethys_mi.h tmi_plan_*, tethys_speech_amd/plan.py): a step replayed from a plan must be the step
the host code issues - same losses, same parameters, bit for bit - including what changes per step (dropout masks, the
Adam step number) and what sits between the launches (events across the weight-gradient stream, the early / late Adam
slices).  The reference's counterpart is the traced @tf.function of speech_jobs/whisper_dist.py:818-819."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_TINY = dict(d_model=128, encoder_attention_heads=2, decoder_attention_heads=2, d_ff=256, vocab_size=160,
             encoder_layers=2, decoder_layers=2, n_mels=16, n_ctx=64, decoder_start_token_id=150, max_target_positions=32)


@pytest.fixture
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _whisper_run(dev, planned, dropout, steps=9):
    from tethys_speech_amd import whisper, optim, train, ops
    from tethys_speech_amd.dist import DataParallelStrategy
    from tethys_speech_amd.data import create_dummy_dataset
    was = ops.set_deterministic(True)
    try:
        strategy = DataParallelStrategy(0, 1, init=False)
        model = whisper.create_whisper_model("small", device=dev, precision="bf16", seed=5, **_TINY)
        model.refresh_shadows()
        if dropout:
            model.enable_dropout(0.1, 0.1, seed=77)
        opt = optim.Adam(1e-3)
        # batches of 3 out of a pool of 8: the short batch of 2 comes round every third step (its own plan / eager steps)
        it = iter(create_dummy_dataset(3, n_mels=16, seq_len=96, max_target_length=12, device=dev, seed=9, num_samples=8))
        old = train.USE_PLAN
        train.USE_PLAN = planned
        try:
            step = train.planned_step(strategy, model, opt, "whisper", pipelined=True)
            losses = []
            for _ in range(steps):
                losses.append(step(*next(it)))
            model.finish_late()
            torch.cuda.synchronize()
            info = step.planned
        finally:
            train.USE_PLAN = old
        return [float(x.item()) for x in losses], model.arena.p.clone(), model.arena.m.clone(), info
    finally:
        ops.set_deterministic(was)


@pytest.mark.parametrize("dropout", [False, True])
def test_whisper_planned_steps_equal_eager_steps_bit_for_bit(dev, dropout):
    le, pe, me, _ = _whisper_run(dev, False, dropout)
    lp, pp, mp, info = _whisper_run(dev, True, dropout)
    assert info is not None and info.replays >= 3, "the plan path did not replay"
    plans = [v["plan"] for v in info._by_sig.values() if v.get("plan") is not None]
    assert plans and all(p.launches > 50 for p in plans)
    assert le == lp, (le, lp)
    assert torch.equal(pe, pp) and torch.equal(me, mp)
    if dropout:  # masks really change from step to step under replay: the same batch comes round with another loss
        assert len(set(lp)) == len(lp)


def test_wav2vec2_planned_steps_equal_eager_steps_bit_for_bit(dev):
    from tethys_speech_amd import wav2vec2, optim, train, ops
    from tethys_speech_amd.dist import DataParallelStrategy

    def run(planned):
        strategy = DataParallelStrategy(0, 1, init=False)
        over = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                    conv_dim=(64, 64, 64), conv_stride=(5, 2, 2), conv_kernel=(10, 3, 2), num_conv_pos_embeddings=8,
                    num_conv_pos_embedding_groups=4, num_codevectors_per_group=16, codevector_dim=32,
                    proj_codevector_dim=64, num_negatives=10)  # (the small model of tests/test_wav2vec2_gpu.py)
        model = wav2vec2.create_full_model("pretraining", "base", device=dev, precision="bf16", seed=3, **over)
        model.refresh_shadows()
        c = model.config
        model.enable_dropout(c.hidden_dropout, c.attention_dropout, seed=11, act_p=c.activation_dropout)
        opt = optim.Adam(3e-4, epsilon=1e-8)
        g = torch.Generator(device="cpu").manual_seed(4)
        audio = [torch.randn(3, 400, generator=g).to(dev) for _ in range(3)]
        model._prepare(3, 400)
        rng = np.random.default_rng(8)
        negs = [torch.from_numpy(wav2vec2.sample_negative_indices(rng, 3, model.T, c.num_negatives)).to(dev) for _ in range(3)]
        old = train.USE_PLAN
        train.USE_PLAN = planned
        try:
            step = train.planned_step(strategy, model, opt, "wav2vec2", pipelined=True)
            losses = [step(audio[i % 3], negs[i % 3]) for i in range(8)]
            model.finish_late()
            torch.cuda.synchronize()
            return [float(x.item()) for x in losses], model.arena.p.clone(), step.planned
        finally:
            train.USE_PLAN = old

    was = ops.set_deterministic(True)
    try:
        le, pe, _ = run(False)
        le2, pe2, _ = run(False)
        lp, pp, info = run(True)
    finally:
        ops.set_deterministic(was)
    assert info is not None and info.replays >= 4
    # The Wav2Vec2 step keeps fp32 atomics (GroupNorm / codebook gradients: tmi_set_deterministic covers the Whisper step
    # only), so two EAGER runs already differ in the last bits; the planned run must sit inside that spread, and a wrong
    # mask or Adam step number would be off by orders of magnitude more (the masks of step k decide its loss)
    spread = float((pe - pe2).abs().max())
    tol = max(4.0 * spread, 1e-7)
    assert float((pe - pp).abs().max()) <= tol, (float((pe - pp).abs().max()), spread)
    assert max(abs(a - b) for a, b in zip(le, lp)) <= max(4.0 * max(abs(a - b) for a, b in zip(le, le2)), 1e-6 * abs(le[0])), (le, lp)


# ----------------------------------------------------------------------------- single entry points under record / replay
# The step tests above reach an entry point's recorded closure only if the step happens to launch it.  Below, every
# entry point with a per-step argument (a dropout seed, the Adam step number) and every entry point no step test replays
# is recorded ALONE: the closure must be the call that was made, with the replay's deltas added to the per-step argument
# and to nothing else, and a direct call must never see the deltas.  All comparisons are bit for bit.
_SEED = 0x1234ABCD5678
_MASK64 = 0xFFFFFFFFFFFFFFFF


def _ops_plan():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import ops, plan
    return ops, plan


def _rnd(shape, dtype, dev, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(dev)


@pytest.fixture
def deterministic():
    ops, _ = _ops_plan()
    was = ops.set_deterministic(True)
    yield
    ops.set_deterministic(was)


class _Case:
    """``run(x)`` issues the entry point(s) with per-step value ``x`` (ignored by cases without one); ``state`` are the
    tensors it reads and writes in place, restored before every run; ``outs`` the tensors it only writes, set to a
    sentinel before every run; ``launches`` the entry points one ``run`` calls."""

    def __init__(self, run, state=(), outs=(), launches=1):
        self.run, self.state, self.outs, self.launches = run, list(state), list(outs), launches
        self.state0 = [t.clone() for t in self.state]

    def reset(self):
        for t, t0 in zip(self.state, self.state0):
            t.copy_(t0)
        for t in self.outs:
            t.view(torch.uint8).fill_(0x5A)

    def snap(self):
        torch.cuda.synchronize()
        return [t.clone() for t in self.state + self.outs]


def _same(a, b):
    return all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


def _per_step_dropout(ops, dev):
    x = _rnd((8, 64), torch.bfloat16, dev, 1)
    out = torch.empty_like(x)
    return _Case(lambda s: ops.dropout(x, out, 8, 64, 0.5, s), outs=[out])


def _ln_inputs(ops, dev):
    bf = torch.bfloat16
    x = _rnd((8, 128), bf, dev, 2, 2.0) + 0.5
    gamma, beta = _rnd((128,), torch.float32, dev, 3) + 1.0, _rnd((128,), torch.float32, dev, 4)
    y, mean, rstd = torch.empty_like(x), torch.empty(8, device=dev), torch.empty(8, device=dev)
    ops.layernorm_fwd(x, gamma, beta, y, mean, rstd, 1e-5)
    dy = _rnd((8, 128), bf, dev, 5)
    dx, dg, db = torch.empty_like(x), torch.zeros(128, device=dev), torch.zeros(128, device=dev)
    return x, gamma, beta, mean, rstd, dy, dx, dg, db


def _per_step_layernorm_dropout_fwd(ops, dev):
    x, gamma, beta, _, _, _, _, _, _ = _ln_inputs(ops, dev)
    y, mean, rstd = torch.empty_like(x), torch.empty(8, device=dev), torch.empty(8, device=dev)
    return _Case(lambda s: ops.layernorm_dropout_fwd(x, gamma, beta, y, mean, rstd, 1e-5, 0.5, s), outs=[y, mean, rstd])


def _per_step_layernorm_dropout_bwd(ops, dev):
    x, gamma, _, mean, rstd, dy, dx, dg, db = _ln_inputs(ops, dev)
    return _Case(lambda s: ops.layernorm_dropout_bwd(dy, x, gamma, mean, rstd, dx, dg, db, 0.5, s), state=[dg, db], outs=[dx])


def _per_step_layernorm_bwd_emit(ops, dev):
    x, gamma, _, mean, rstd, dy, dx, dg, db = _ln_inputs(ops, dev)
    colsum, masked = _rnd((128,), torch.float32, dev, 6), torch.empty_like(x)
    return _Case(lambda s: ops.layernorm_bwd_emit(dy, x, gamma, mean, rstd, dx, dg, db, colsum, masked=masked, dropout_p=0.5,
                                                  dropout_seed=s), state=[dg, db, colsum], outs=[dx, masked])


def _per_step_gemm(ops, dev):
    bf = torch.bfloat16
    A, W = _rnd((64, 64), bf, dev, 7, 0.5), _rnd((64, 64), bf, dev, 8, 0.2)
    bias, resid = _rnd((64,), torch.float32, dev, 9, 0.1), _rnd((64, 64), bf, dev, 10)
    out = torch.empty((64, 64), dtype=bf, device=dev)
    return _Case(lambda s: ops.gemm(A, W, out, 64, 64, 64, 64, 1, 64, 1, 64, bias=bias, resid=resid, r_ld=64, dropout_p=0.5,
                                    dropout_seed=s), outs=[out])


def _per_step_attention(ops, dev):
    B, H, T = 1, 2, 64
    D, bf = H * 64, torch.bfloat16
    q, k, v, do = _rnd((B, T, D), bf, dev, 11, 0.35), _rnd((B, T, D), bf, dev, 12), _rnd((B, T, D), bf, dev, 13), _rnd((B, T, D), bf, dev, 14)
    o, dq, dk, dv = (torch.empty((B, T, D), dtype=bf, device=dev) for _ in range(4))
    stats = torch.empty((B, H, T, 2), dtype=torch.float32, device=dev)
    delta = torch.empty((B, H, T), dtype=torch.float32, device=dev)
    dmask = ops.attn_dropmask(dev, B, H, T, T)
    m = lambda t: (t, 0, T * D, D)

    def run(s):  # the backward reads the keep bits this forward stores
        ops.attn_fwd(m(q), m(k), m(v), m(o), stats, B, H, T, T, 1, dropout_p=0.5, dropout_seed=s, drop_mask=dmask)
        ops.attn_bwd(m(q), m(k), m(v), m(o), stats, m(do), m(dq), m(dk), m(dv), delta, B, H, T, T, 1, dq_scale=0.5,
                     dropout_p=0.5, dropout_seed=s, drop_mask=dmask)
    return _Case(run, outs=[o, stats, dmask, dq, dk, dv, delta], launches=2)


def _adam_state(dev, n):
    p, g = _rnd((n,), torch.float32, dev, 20), _rnd((n,), torch.float32, dev, 21, 0.05)
    m, v = _rnd((n,), torch.float32, dev, 22, 0.01), _rnd((n,), torch.float32, dev, 23, 0.01).abs()
    return p, g, m, v, torch.zeros(n, dtype=torch.bfloat16, device=dev)


def _per_step_adam(ops, dev):
    p, g, m, v, mir = _adam_state(dev, 4096)
    return _Case(lambda t: ops.adam_step(p, g, m, v, 4096, 1e-2, 0.9, 0.999, 1e-7, t, mirror=mir, zero_grad=True),
                 state=[p, g, m, v, mir])


def _per_step_adam_rows(ops, dev):
    p, g, m, v, mir = _adam_state(dev, 16 * 64)
    g.view(16, 64)[5:] = 0.0  # idle rows
    m.view(16, 64)[9:] = 0.0
    v.view(16, 64)[9:] = 0.0
    active = torch.zeros(16, dtype=torch.uint8, device=dev)
    return _Case(lambda t: ops.adam_step_rows(p, g, m, v, 16, 64, active, 1e-2, 0.9, 0.999, 1e-7, t, mirror=mir, zero_grad=True),
                 state=[p, g, m, v, mir, active])


def _per_step_adam_segments(ops, dev):
    n, offs = 4096, [0, 1000, 4096]
    p, g, m, v, mir = _adam_state(dev, n)
    chunks = ops.segment_chunks(offs, chunk=1000, device=dev)
    ss = torch.empty(2, dtype=torch.float32, device=dev)
    ops.segment_sumsq(g, torch.tensor(offs, dtype=torch.int64, device=dev), ss, 2)
    return _Case(lambda t: ops.adam_step_segments(p, g, m, v, n, chunks, ss, 2, 1.0, 1.0, 1e-2, 0.9, 0.999, 1e-8, t, mirror=mir,
                                                  zero_grad=True), state=[p, g, m, v, mir])


_PER_STEP = {"tmi_dropout": (_per_step_dropout, "seed"), "tmi_layernorm_dropout_fwd": (_per_step_layernorm_dropout_fwd, "seed"),
             "tmi_layernorm_dropout_bwd": (_per_step_layernorm_dropout_bwd, "seed"),
             "tmi_layernorm_bwd_emit": (_per_step_layernorm_bwd_emit, "seed"), "tmi_gemm": (_per_step_gemm, "seed"),
             "tmi_attn_fwd+tmi_attn_bwd": (_per_step_attention, "seed"), "tmi_adam_step": (_per_step_adam, "step"),
             "tmi_adam_step_rows": (_per_step_adam_rows, "step"), "tmi_adam_step_segments": (_per_step_adam_segments, "step")}


@pytest.mark.parametrize("entry", list(_PER_STEP))
def test_replay_moves_the_per_step_argument_and_a_direct_call_never_sees_the_deltas(dev, deterministic, entry):
    """Recorded with seed s (step 1), replayed with delta k: the outputs are those of a direct call with s + k (step 5) and
    not those of s (step 1); a direct call with s right after that replay gives what it gave before."""
    ops, plan = _ops_plan()
    make, kind = _PER_STEP[entry]
    case = make(ops, dev)
    # seeds move by the step code's own stride, which wraps modulo 2^64; the step number from 1 to 5
    base, k = (_SEED, 3 * plan.SEED_STEP & _MASK64) if kind == "seed" else (1, 4)
    moved = (base + k) & _MASK64 if kind == "seed" else base + k
    case.reset()
    case.run(base)
    eager = case.snap()
    case.reset()
    case.run(moved)
    eager_moved = case.snap()
    assert not _same(eager, eager_moved), "the per-step argument does not change the result: the case checks nothing"
    p = plan.LaunchPlan()
    case.reset()
    with p.recording():
        case.run(base)
    assert p.launches == case.launches
    assert _same(case.snap(), eager), "a recorded call is also executed, with the arguments as given"
    case.reset()
    p.replay(k if kind == "seed" else 0, k if kind == "step" else 0)
    replayed = case.snap()
    assert _same(replayed, eager_moved)
    assert not _same(replayed, eager)
    case.reset()
    case.run(base)
    assert _same(case.snap(), eager), "the deltas of the last replay leaked into a direct call"
    case.reset()
    p.replay(0, 0)
    assert _same(case.snap(), eager)


def _replay_lm_head_argmax(ops, dev):
    M, d, V = 2, 128, 160
    x, w = _rnd((M, d), torch.bfloat16, dev, 30), _rnd((d, V), torch.bfloat16, dev, 31)
    gamma, beta = _rnd((d,), torch.float32, dev, 32) + 1.0, _rnd((d,), torch.float32, dev, 33)
    ids, cnt = torch.empty(M, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    ws = torch.zeros(M + 1, dtype=torch.int64, device=dev)
    return _Case(lambda _: ops.lm_head_argmax(x, d, w, V, M, d, V, ids, 1, ws, gamma=gamma, beta=beta, eos_id=3, eos_count=cnt),
                 state=[ws], outs=[ids, cnt])


def _replay_lm_head_topk(ops, dev):
    M, d, V, N = 2, 128, 160, 4
    x, w = _rnd((M, d), torch.bfloat16, dev, 34), _rnd((d, V), torch.bfloat16, dev, 35)
    ids, lp = torch.empty((M, N), dtype=torch.int32, device=dev), torch.empty((M, N), device=dev)
    lse = torch.empty(M, device=dev)
    ws = torch.zeros(ops.lm_head_topk_workspace_elems(M, V, N), dtype=torch.int64, device=dev)
    return _Case(lambda _: ops.lm_head_topk(x, d, w, V, M, d, V, N, ids, lp, ws, temperature=0.7, lse=lse), state=[ws],
                 outs=[ids, lp, lse])


def _replay_beam_step(ops, dev):
    B, K, N, L1, t = 1, 2, 4, 8, 1
    i32 = dict(dtype=torch.int32, device=dev)
    prefix = torch.full((2, B * K, L1), 50, **i32)
    sums = torch.tensor([0.0, float("-inf")], device=dev)
    pool_ids, pool_scores, pool_len = torch.full((B, K, L1), -5, **i32), torch.zeros(B, K, device=dev), torch.zeros(B, K, **i32)
    pool_cnt, done, n_done = torch.zeros(B, **i32), torch.zeros(B, **i32), torch.zeros(1, **i32)
    cand = torch.tensor([[7, 2, 9, 11], [4, 5, 6, 8]], **i32)  # 2 = end of text: the first beam's second candidate finishes
    clp = torch.tensor([[-0.1, -0.7, -1.5, -2.5], [-0.2, -0.9, -1.1, -3.0]], device=dev)
    return _Case(lambda _: ops.beam_step(cand, clp, N, B, K, sums, prefix[t & 1], prefix[(t + 1) & 1], L1, t, 2, 1.0, False,
                                         pool_ids, pool_scores, pool_len, pool_cnt, done, n_done),
                 state=[prefix, sums, pool_ids, pool_scores, pool_len, pool_cnt, done, n_done])


def _replay_softmax_fwd(ops, dev):
    s = _rnd((32, 16), torch.float32, dev, 36, 3.0)  # [1, 2, 16, 16]
    return _Case(lambda _: ops.softmax_fwd(s, 32, 16, 16, 1), state=[s])


def _replay_softmax_bwd(ops, dev):
    p, dp = torch.softmax(_rnd((32, 16), torch.float32, dev, 37, 3.0), -1), _rnd((32, 16), torch.float32, dev, 38)
    return _Case(lambda _: ops.softmax_bwd(p, dp, 32, 16), state=[dp])


def _replay_xent(ops, dev):
    B, S, V = 1, 4, 160
    logits = _rnd((B * S, V), torch.bfloat16, dev, 39, 2.0)
    labels = torch.tensor([[150, 3, 77, 159]], dtype=torch.int32, device=dev)
    row_loss = torch.empty(B * S, device=dev)
    return _Case(lambda _: ops.xent_fwd_bwd(logits, V, labels, row_loss, B, S, V, 1.0 / 3), state=[logits], outs=[row_loss])


def _replay_adam_step_dev(ops, dev):
    p, g, m, v, mir = _adam_state(dev, 4096)
    sc = torch.tensor(ops.adam_scalars(1e-2, 0.9, 0.999, 3), dtype=torch.float32, device=dev)
    return _Case(lambda _: ops.adam_step_dev(p, g, m, v, 4096, 0.9, 0.999, 1e-7, sc, mirror=mir), state=[p, m, v, mir])


def _replay_grad_pack(ops, dev):
    src, dst = _rnd((1000,), torch.float32, dev, 40), torch.empty(1000, dtype=torch.bfloat16, device=dev)
    return _Case(lambda _: ops.grad_pack(src, dst, 1000, scale=0.5), outs=[dst])


def _replay_grad_unpack(ops, dev):
    src, dst = _rnd((2, 1000), torch.bfloat16, dev, 41), torch.empty(1000, device=dev)
    return _Case(lambda _: ops.grad_unpack(src, dst, 1000, nparts=2, part_stride=1000, scale=0.5), outs=[dst])


def _replay_transpose_cast(ops, dev):
    src, dst = _rnd((70, 40), torch.float32, dev, 42), torch.empty((40, 70), dtype=torch.bfloat16, device=dev)
    return _Case(lambda _: ops.transpose_cast_bf16(src, 40, dst, 70, 70, 40), outs=[dst])


def _replay_logmel(ops, dev):
    from tethys_speech_amd._lib import check, lib
    frames, n_bins, n_mels = 5, 33, 8
    spec, mel = _rnd((frames, 2 * n_bins), torch.float32, dev, 43), _rnd((n_bins, n_mels), torch.float32, dev, 44).abs()
    out = torch.empty((n_mels, frames), device=dev)
    return _Case(lambda _: check(lib().tmi_logmel_from_spectrum(spec.data_ptr(), 2 * n_bins, mel.data_ptr(), out.data_ptr(), frames, n_bins,
                                                                n_mels, 1e-6, 1, frames, ops.stream()), "tmi_logmel_from_spectrum"),
                 outs=[out])


def _replay_memset(ops, dev):
    t = torch.empty(1000, device=dev)
    return _Case(lambda _: ops.fill_zero(t), outs=[t])


def _replay_memset2d(ops, dev):
    t = _rnd((4, 10, 8), torch.float32, dev, 45)
    return _Case(lambda _: ops.fill_zero(t[:, 7:]), state=[t])  # the pad rows of a [B, T, C] buffer


def _replay_memcpy(ops, dev):
    src, dst = _rnd((1000,), torch.float32, dev, 46), torch.empty(1000, device=dev)
    return _Case(lambda _: ops.copy(dst, src), outs=[dst])


_REPLAY_ONLY = {"tmi_lm_head_argmax": _replay_lm_head_argmax, "tmi_lm_head_topk": _replay_lm_head_topk,
                "tmi_beam_step": _replay_beam_step, "tmi_softmax_fwd": _replay_softmax_fwd, "tmi_softmax_bwd": _replay_softmax_bwd,
                "tmi_xent_fwd_bwd": _replay_xent, "tmi_adam_step_dev": _replay_adam_step_dev, "tmi_grad_pack": _replay_grad_pack,
                "tmi_grad_unpack": _replay_grad_unpack, "tmi_transpose_cast_bf16": _replay_transpose_cast,
                "tmi_logmel_from_spectrum": _replay_logmel, "tmi_memset_async": _replay_memset,
                "tmi_memset2d_async": _replay_memset2d, "tmi_memcpy_async": _replay_memcpy}


@pytest.mark.parametrize("entry", list(_REPLAY_ONLY))
def test_a_recorded_entry_point_replays_the_call_that_was_made(dev, entry):
    """The closures no planned step replays: one call recorded, its outputs overwritten, replayed with zero deltas."""
    ops, plan = _ops_plan()
    case = _REPLAY_ONLY[entry](ops, dev)
    case.reset()
    case.run(None)
    eager = case.snap()
    p = plan.LaunchPlan()
    case.reset()
    sentinel = [t.clone() for t in case.outs]
    assert not _same(eager[len(case.state):], sentinel) or not case.outs
    with p.recording():
        before = p.launches
        case.run(None)
        assert p.launches == before + 1
    assert _same(case.snap(), eager)
    case.reset()
    p.replay(0, 0)
    assert _same(case.snap(), eager)
