"""``train.evaluate_whisper`` over two ranks (gloo, both on cuda:0, fresh child processes as tests/test_two_rank_gpu.py):
each rank evaluates its shard of the batches and the three sums meet in ONE reduction after the loop; the result equals a
single process over the union up to the fp64 sum.  A rank whose shard is empty contributes zeros."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(d_model=128, encoder_attention_heads=2, decoder_attention_heads=2, d_ff=256, vocab_size=160,
          encoder_layers=2, decoder_layers=2, n_mels=16, n_ctx=32, decoder_start_token_id=150, max_target_positions=32)


def _batches():
    """Three global batches of 4 items; ranks take rows [0, 2) and [2, 4)."""
    rng = np.random.default_rng(17)
    return [(rng.standard_normal((4, 16, 48)).astype(np.float32), rng.integers(0, 150, (4, 9)).astype(np.int32))
            for _ in range(3)]


def _shard(rank, empty_rank):
    """This rank's batches: the usual split, or - ``empty_rank`` - everything on the other rank and zero-row batches here."""
    out = []
    for f, l in _batches():
        if empty_rank is None:
            out.append((f[2 * rank:2 * rank + 2], l[2 * rank:2 * rank + 2]))
        elif rank == empty_rank:
            out.append((f[:0], l[:0]))
        else:
            out.append((f, l))
    return out


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, port, q, empty_rank):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import dist as D, train, whisper
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dev = "cuda:0"
    strat = D.DataParallelStrategy(rank, 2, backend="gloo")
    model = whisper.create_whisper_model("small", device=dev, precision="fp32", seed=11 + rank, **KW)
    strat.broadcast_parameters(model.arena.p)
    model.refresh_shadows()
    calls, real = [0], dist.all_reduce

    def counted(*a, **kw):
        calls[0] += 1
        return real(*a, **kw)
    dist.all_reduce = counted
    lines = []
    data = [(torch.from_numpy(f).to(dev), torch.from_numpy(l).to(dev)) for f, l in _shard(rank, empty_rank)]
    out = train.evaluate_whisper(strat, model, data, log=lines.append, step=7)
    dist.all_reduce = real
    torch.cuda.synchronize()
    q.put((rank, out, calls[0], lines))
    dist.destroy_process_group()


@pytest.mark.parametrize("empty_rank", [None, 1])
def test_two_rank_evaluation_equals_one_process_over_the_union(dev, empty_rank):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, port, q, empty_rank)) for r in range(2)]
    for p_ in procs:
        p_.start()
    res = sorted([q.get(timeout=300) for _ in range(2)], key=lambda t: t[0])
    for p_ in procs:
        p_.join(60)
    (_, o0, c0, lines0), (_, o1, c1, _) = res
    assert o0 == o1, "the ranks disagree on the reduced result"
    assert c0 == 1 and c1 == 1, "one all-reduce after the loop, none per batch"

    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import train, whisper
    model = whisper.create_whisper_model("small", device=dev, precision="fp32", seed=11, **KW)
    # the union, in the batches the ranks saw (a GEMM may pick another tile for another row count: same items, other bits)
    union = [(torch.from_numpy(f).to(dev), torch.from_numpy(l).to(dev)) for r in range(2) for f, l in _shard(r, empty_rank)]
    ref = train.evaluate_whisper(None, model, union)
    assert o0["n_tokens"] == ref["n_tokens"] == 3 * 4 * 8 and o0["n_correct"] == ref["n_correct"]
    # the same fp32 token log-probabilities, added in another order in fp64: a few ulp of the sum
    assert abs(o0["loss_sum"] - ref["loss_sum"]) <= 1e-12 * abs(ref["loss_sum"])
    assert abs(o0["loss"] - ref["loss"]) <= 1e-12 * abs(ref["loss"])
    assert lines0 == [f"Eval step 7, Loss: {o0['loss']:.4f}, Accuracy: {o0['accuracy']:.4f}"]
