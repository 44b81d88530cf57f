"""The training step on the weighted loss of W:596-598 (``decoder_attention_mask``): ``forward_backward`` /
``distributed_train_step`` / ``planned_step`` / ``train_whisper(mask_padding=True)`` against the fp64 reference of
tests/_masked_loss_ref.py.  Configuration, parameters and error measures are tests/test_whisper_step_gpu.py's
(``small_cfg()``, ``build()``, B, S = 3, 12).

The labels of that file's pool are padded in their last column only (lengths 11 of 12), which W:597 slices off; here the
tails of two samples are cut back to pad, so that ``labels != 0`` masks real positions, and one weight is fractional."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import _masked_loss_ref as M
import test_whisper_step_gpu as TW
from _margins import within
from oracle import whisper_oracle as O  # noqa: E402  (checker only)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 12


def padded_pool(seed, T_in, n, n_mels=16):
    """The oracle's dummy pool with ragged targets: sample i keeps 11 - (3 * i) % 7 tokens (EOS last, pad after), and
    mask = (labels != 0) as float32 with one fractional weight."""
    feats, labels = O.create_dummy_pool(seed=seed, n_mels=n_mels, seq_len=T_in, max_target_length=S, num_samples=n)
    for i in range(n):
        L = 11 - (3 * i) % 7
        labels[i, L - 1] = 2
        labels[i, L:] = 0
    mask = (labels != 0).astype(np.float32)
    mask[0, 3] = 0.5
    assert (mask[:, :-1] == 0).any() and (mask[:, :-1] == 1).any()
    return feats, labels, mask


def _dev(dev, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)


@pytest.mark.parametrize("T_in", [48, 47])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_masked_step_gradients_match_the_reference(dev, precision, T_in):
    """test_step_gradients_match_oracle with a mask: the same error measures and the same bounds (|dloss| 1e-6 / 2e-3,
    worst gradient 5e-5 max-norm / 6e-2 relative L2)."""
    model, ocfg, params = TW.build(precision, TW.small_cfg(), dev)
    feats, labels, mask = padded_pool(11, T_in, 3)
    if precision == "bf16":  # the oracle on the bf16-rounded kernels the step sees
        for k in params:
            if k.endswith(".kernel"):
                params[k] = params[k].to(torch.bfloat16).double()
    loss_ref, grads_ref = M.loss_and_grads(params, torch.from_numpy(feats), torch.from_numpy(labels), mask, ocfg)
    f, l, m = _dev(dev, feats, labels, mask)
    loss = model.forward_backward(f, l, decoder_attention_mask=m)
    torch.cuda.synchronize()
    lv = float(loss.item())
    got = model.arena.ref_views(model.arena.g)
    worst = {}
    for k, gr in grads_ref.items():
        gg = got[k].double().cpu()
        if precision == "fp32":
            worst[k] = float((gg - gr).abs().max() / max(float(gr.abs().max()), 1e-4))
        else:
            worst[k] = float((gg - gr).norm() / max(float(gr.norm()), 1e-2))
    print(f"masked step {precision} T_in={T_in}: |dloss| {abs(lv - float(loss_ref)):.3e}, worst gradient {max(worst.values()):.3e}")
    within(f"masked whisper step {precision} |dloss|", abs(lv - float(loss_ref)), 1e-6 if precision == "fp32" else 2e-3)  # measured 8.4e-7 / 1.5e-3
    within(f"masked whisper step {precision} worst gradient (fp32: max-norm, bf16: rel L2)", max(worst.values()),
           5e-5 if precision == "fp32" else 6e-2, sorted(worst.items(), key=lambda kv: -kv[1])[:4])  # measured 2.8e-5 / 4.3e-2
    # the model call passes the mask through, and a bool mask is the same mask (converted once, before the step)
    if precision == "fp32" and T_in == 48:
        g0 = model.arena.g.clone()
        mb = m.clone()
        mb[0, 3] = 1.0
        a = model(f, labels=l, decoder_attention_mask=mb, training=True)["loss"].clone()
        ga = model.arena.g.clone()
        b = model.forward_backward(f, l, decoder_attention_mask=mb.bool())
        assert torch.equal(a, b) and float(a) != lv
        assert not torch.equal(ga, g0)
        with pytest.raises(ValueError):
            model.forward_backward(f, l, decoder_attention_mask=m[:, :-1])
        with pytest.raises(ValueError):
            model(f, labels=l, decoder_attention_mask=m, training=False)


def test_five_step_masked_loss_curve_fp32(dev):
    """Five Adam steps (lr 1e-3) on batches of 3 from a pool of 8 (3, 3, 2, 3, 3: the short batch occurs), fp32, against the
    fp64 reference: the 1e-4 per step test_ten_step_loss_curve_fp32_small_dims holds."""
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import dist, optim, train
    model, ocfg, params = TW.build("fp32", TW.small_cfg(), dev)
    feats, labels, mask = padded_pool(5, 48, 8)
    ref_losses, _ = M.train_steps(ocfg, params, feats, labels, mask, 3, 5, lr=1e-3)
    opt, strat = optim.Adam(learning_rate=1e-3), dist.DataParallelStrategy(0, 1)
    got, sizes = [], []
    for i in range(5):
        s = (0, 3, 6)[i % 3]
        batch = _dev(dev, feats[s:s + 3], labels[s:s + 3], mask[s:s + 3])
        sizes.append(int(batch[0].shape[0]))
        got.append(float(train.distributed_train_step(strat, model, batch, opt).item()))
    assert sizes == [3, 3, 2, 3, 3]
    err = max(abs(a - b) for a, b in zip(got, ref_losses))
    print(f"masked 5-step curve fp32: max |dloss| {err:.3e}")
    within("masked whisper 5-step loss curve fp32 max |dloss|", err, 1e-4, (got, ref_losses))  # measured 3.6e-7
    assert got[-1] < got[0]


_TINY = dict(d_model=128, encoder_attention_heads=2, decoder_attention_heads=2, d_ff=256, vocab_size=160, encoder_layers=2,
             decoder_layers=2, n_mels=16, n_ctx=64, decoder_start_token_id=150, max_target_positions=32)


def _planned_run(dev, planned, dropout):
    """Seven three-input steps (batches of 3 from a pool of 8), four two-input steps of the batch-3 shape, one more
    three-input step - in ONE model, so the two plans of that shape coexist."""
    from tethys_speech_amd import whisper, optim, train, ops
    from tethys_speech_amd.dist import DataParallelStrategy
    was = ops.set_deterministic(True)
    old = train.USE_PLAN
    try:
        train.USE_PLAN = planned
        model = whisper.create_whisper_model("small", device=dev, precision="bf16", seed=5, **_TINY)
        model.refresh_shadows()
        if dropout:
            model.enable_dropout(0.1, 0.1, seed=77)
        opt = optim.Adam(1e-3)
        step = train.planned_step(DataParallelStrategy(0, 1, init=False), model, opt, "whisper", pipelined=True)
        feats, labels, mask = _dev(dev, *padded_pool(9, 96, 8))
        losses = []
        for i in range(7):
            s = (0, 3, 6)[i % 3]
            losses.append(step(feats[s:s + 3], labels[s:s + 3], mask[s:s + 3]))
        for i in range(4):
            s = (0, 3)[i % 2]
            losses.append(step(feats[s:s + 3], labels[s:s + 3]))
        losses.append(step(feats[3:6], labels[3:6], mask[3:6].bool()))  # (a bool mask: converted before the plan sees it)
        model.finish_late()
        torch.cuda.synchronize()
        return [float(x.item()) for x in losses], model.arena.p.clone(), model.arena.m.clone(), step.planned
    finally:
        train.USE_PLAN = old
        ops.set_deterministic(was)


@pytest.mark.parametrize("dropout", [False, True])
def test_masked_planned_steps_equal_eager_steps_bit_for_bit(dev, dropout):
    le, pe, me, _ = _planned_run(dev, False, dropout)
    lp, pp, mp_, info = _planned_run(dev, True, dropout)
    assert info is not None and info.replays >= 4, "the plan path did not replay"
    sigs = {len(sig): st for sig, st in info._by_sig.items() if st.get("plan") is not None and sig[0][0][0] == 3}
    assert set(sigs) == {2, 3}, "the two- and the three-input step of one shape each have a plan of their own"
    assert sigs[3]["plan"].launches == sigs[2]["plan"].launches + 1  # (the mask costs one launch: tmi_xent_weights)
    assert le == lp, (le, lp)
    assert torch.equal(pe, pp) and torch.equal(me, mp_)
    assert abs(le[7] - le[0]) > 1e-3  # (the two objectives differ on the same batch)


def test_train_whisper_with_mask_padding(dev):
    """The loop: it trains on the masked objective (its first logged loss is a direct masked forward_backward on the same
    batch), evaluates on it (the Eval lines' token counts are the mask's sums), and without the flag is what it was."""
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import dist, ops, train, whisper
    from tethys_speech_amd.data import create_dummy_dataset
    data = dict(seq_len=96, max_target_length=60)  # (targets of 50-59 tokens in 60 slots: real padding)
    lines = []
    was = ops.set_deterministic(True)
    try:
        model = train.train_whisper(dist.DataParallelStrategy(0, 1), batch_size=3, num_batches=4, precision="bf16", device=dev,
                                    log=lines.append, model_overrides=dict(_TINY, max_target_positions=64), dropout=False,
                                    mask_padding=True, eval_every=2, eval_batches=1, eval_seed=99, **data)
        twin = whisper.create_whisper_model("small", device=dev, precision="bf16", seed=1234,
                                            **dict(_TINY, max_target_positions=64))
        twin.refresh_shadows()
        f, l, m = next(iter(create_dummy_dataset(3, n_mels=16, device=dev, seed=1234, with_mask=True, **data)))
        masked = float(twin.forward_backward(f, l, decoder_attention_mask=m).item())
        plain = float(twin.forward_backward(f, l).item())
    finally:
        ops.set_deterministic(was)
    assert len(model.losses) == 4 and model.losses[0] == masked and abs(masked - plain) > 1e-3
    evals = [ln for ln in lines if ln.startswith("Eval step")]
    assert [e.split(",")[0] for e in evals] == ["Eval step 2", "Eval step 4"]
    ef, el, em = next(iter(create_dummy_dataset(3, n_mels=16, device=dev, seed=99, with_mask=True, **data)))
    n_tokens = float(em[:, :-1].sum())
    assert 0 < n_tokens < 3 * 59
    assert [r["n_tokens"] for _, r in model.eval_history] == [n_tokens, n_tokens]
    assert model.eval_history[-1][1] == train.evaluate_whisper(None, model, [(ef, el, em)])


# ---- two replicas (gloo, both on cuda:0, fresh child processes as tests/test_evaluate_two_rank_gpu.py)
STEPS, LR = 3, 1e-4   # (W:901's learning rate)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_batches(rank):
    """Per-replica batch 2, pool of 5: global batches of 4, 1, 4 - on the short one rank 0 has one sample, rank 1 none."""
    feats, labels, mask = padded_pool(7, 48, 5)
    out = []
    for s in (0, 4, 0)[:STEPS]:
        lo = s + 2 * rank
        out.append((feats[s:s + 4][2 * rank:2 * rank + 2], labels[s:s + 4][2 * rank:2 * rank + 2], mask[s:s + 4][2 * rank:2 * rank + 2]))
        assert out[-1][0].shape[0] == max(0, min(2, 5 - lo))
    return out


def _worker(rank, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import dist as D, optim, train
    torch.cuda.set_device(0)
    dev = "cuda:0"
    strat = D.DataParallelStrategy(rank, 2, backend="gloo", bucket_bytes=256 * 1024)
    model, _, _ = TW.build("fp32", TW.small_cfg(), dev)
    strat.broadcast_parameters(model.arena.p)
    model.refresh_shadows()
    opt = optim.Adam(LR)
    losses, sizes = [], []
    for batch in _rank_batches(rank):
        sizes.append(int(batch[0].shape[0]))
        losses.append(float(train.distributed_train_step(strat, model, _dev(dev, *batch), opt).item()))
    torch.cuda.synchronize()
    q.put((rank, model.arena.p.cpu().numpy(), losses, sizes))
    torch.distributed.destroy_process_group()


def test_two_rank_masked_step_matches_the_reference(dev):
    """Each replica normalises by the sum of its own weights, gradients and losses are summed (W:829-836); the replica
    whose slice of the short batch is empty contributes zeros.  Against ``train_steps(n_replicas=2)`` in fp64 at the bounds
    of test_two_rank_step_equals_accumulated_single_process (losses rtol 1e-5 + 1e-6, parameters 1e-5 of their maximum)."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, port, q)) for r in range(2)]
    for p_ in procs:
        p_.start()
    res = sorted([q.get(timeout=300) for _ in range(2)], key=lambda t: t[0])
    for p_ in procs:
        p_.join(60)
    (_, p0, l0, s0), (_, p1, l1, s1) = res
    assert np.array_equal(p0, p1) and l0 == l1
    assert s0 == [2, 1, 2] and s1 == [2, 0, 2]
    model, ocfg, params = TW.build("fp32", TW.small_cfg(), dev)
    feats, labels, mask = padded_pool(7, 48, 5)
    ref_losses, _ = M.train_steps(ocfg, params, feats, labels, mask, 2, STEPS, lr=LR, n_replicas=2)
    model.arena.load_ref(params)
    ref = model.arena.p.cpu().numpy()
    lerr = max(abs(a - b) / (1e-5 * abs(b) + 1e-6) for a, b in zip(l0, ref_losses))
    perr = float(np.abs(p0 - ref).max() / np.abs(ref).max())
    print(f"two-rank masked step: loss error / bound {lerr:.3e}, parameter error {perr:.3e}")
    within("two-rank masked step loss |err| / (1e-5 |loss| + 1e-6)", lerr, 1.0, (l0, ref_losses))
    within("two-rank masked step parameters max |err| / max |ref|", perr, 1e-5)  # measured 2.1e-7 (losses: 3.5e-3 of their bound)
