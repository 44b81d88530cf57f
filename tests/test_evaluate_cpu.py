"""Whisper evaluation, the parts that need no GPU: the fp64 restatement (tests/_eval_ref.py) against torch.log_softmax
and closed forms, the chunk schedule, ``check_evaluate_args``, ``evaluate_whisper``'s summing and log line with a fake
model, and the new C entry points in the built library (ABI still 31)."""
import math

import numpy as np
import pytest
import torch

import _eval_ref as E


def _cfg(**kw):
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import whisper
    return whisper, whisper.make_config("small", **kw)


# ---------------------------------------------------------------------------------------- the restatement
def test_fold_matches_log_softmax_fp64():
    g = torch.Generator().manual_seed(5)
    M, V, ld = 9, 37, 40
    z = torch.randn(M, ld, generator=g, dtype=torch.float64) * 3
    z[:, V:] = 1e30  # pad columns: never read
    targets = torch.randint(0, V, (M,), generator=g)
    targets[2] = -1
    lse, arg, lp = E.fold(z.numpy(), V, targets.numpy())
    ls = torch.log_softmax(z[:, :V], dim=1)
    assert np.allclose(lse, torch.logsumexp(z[:, :V], dim=1).numpy(), rtol=0, atol=1e-12)
    assert (arg == z[:, :V].argmax(dim=1).numpy()).all()
    want = ls[torch.arange(M), targets.clamp(min=0)].numpy()
    want[2] = 0.0
    assert np.allclose(lp, want, rtol=0, atol=1e-12) and lp[2] == 0.0


def test_fold_closed_forms():
    V = 11
    # a row of equal logits: lse = z + log V, argmax = column 0
    z = np.full((1, V), 2.5)
    lse, arg, lp = E.fold(z, V, [4])
    assert abs(lse[0] - (2.5 + math.log(V))) < 1e-14 and arg[0] == 0 and abs(lp[0] + math.log(V)) < 1e-14
    # a one-hot spike of +80 among zeros: lse = 80 + log1p((V - 1) e^-80)
    z = np.zeros((1, V))
    z[0, 7] = 80.0
    lse, arg, lp = E.fold(z, V, [7])
    assert abs(lse[0] - (80.0 + math.log1p((V - 1) * math.exp(-80.0)))) < 1e-12 and arg[0] == 7 and abs(lp[0]) < 1e-12
    lse, arg, lp = E.fold(z, V, [0])
    assert abs(lp[0] + 80.0) < 1e-12
    # -0.0 against +0.0 are equal: the smaller column wins, whichever holds which
    z = np.full((2, V), -1.0)
    z[0, 3], z[0, 8] = -0.0, 0.0
    z[1, 3], z[1, 8] = 0.0, -0.0
    assert list(E.fold(z, V, [-1, -1])[1]) == [3, 3]
    # a separately computed target logit replaces the stored one in BOTH terms: zt - log((V - 1) e^0 + e^zt)
    lse, _, lp = E.fold(np.zeros((1, V)), V, [2], zt=[0.25])
    assert abs(lse[0] - math.log(V)) < 1e-14 and abs(lp[0] - (0.25 - math.log(V - 1 + math.exp(0.25)))) < 1e-14
    assert E.fold(np.zeros((1, 1)), 1, [0], zt=[3.0])[2][0] == 0.0  # V = 1: nothing else in the sum


@pytest.mark.parametrize("V,ld,nc", [(7, 8, 64), (63, 64, 64), (64, 64, 64), (69, 72, 64), (128, 128, 64), (300, 320, 64)])
def test_chunked_fold_equals_fold(V, ld, nc):
    g = np.random.default_rng(V)
    M = 6
    z = g.standard_normal((M, ld)) * 4
    z[:, V:] = np.nan  # pad columns must not be looked at
    z[0, :V] = 1.0                                     # all equal
    z[1, :V] = -1e4; z[1, V // 2] = 0.0                 # the mask constant
    z[2, 0] = z[2, V - 1] = 50.0                        # the maximum twice: the smaller column wins
    targets = np.array([0, V - 1, V // 2, min(V - 1, nc - 1), min(V - 1, nc), -1])
    a = E.fold(z, V, targets)
    b = E.chunked_fold(z, V, ld, nc, targets)
    assert np.allclose(a[0], b[0], rtol=0, atol=1e-11) and (a[1] == b[1]).all()
    assert np.allclose(a[2], b[2], rtol=0, atol=1e-11)
    assert a[1][0] == 0 and a[1][2] == 0 and a[1][1] == V // 2


def test_weighted_loss_and_accuracy():
    lp = np.array([[-1.0, -2.0, 0.0], [-3.0, 0.0, 0.0]])
    arg = np.array([[4, 9, 0], [6, 1, 0]])
    labels = np.array([[0, 4, 5], [0, 6, 7]])
    t, w = E.shift_targets(labels)
    assert t.tolist() == [[4, 5, -1], [6, 7, -1]] and w.tolist() == [[1, 1], [1, 1]]
    loss, acc, ls, nc, nt = E.weighted(lp, arg, t, w)
    assert ls == 6.0 and nt == 4.0 and nc == 2.0 and loss == 1.5 and acc == 0.5
    # the reference's weights are mask[:, :-1] (W:597): the mask's last column never counts
    t, w = E.shift_targets(labels, mask=np.array([[1, 0, 1], [1, 1, 0]]))
    assert t.tolist() == [[4, -1, -1], [6, 7, -1]] and w.tolist() == [[1, 0], [1, 1]]
    loss, acc, ls, nc, nt = E.weighted(np.where(t >= 0, lp, 0.0), arg, t, w)
    assert ls == 4.0 and nt == 3.0 and nc == 2.0


def test_score_sums():
    lp = np.array([[-1.0, -2.0, -4.0], [-0.5, 0.0, 0.0]])
    assert E.score_sums(lp, [3, 1]).tolist() == [-7.0, -0.5] and E.score_sums(lp, [2, 0]).tolist() == [-3.0, 0.0]


# ---------------------------------------------------------------------------------------- host logic of the package
@pytest.mark.parametrize("V,ld,nc", [(51865, 51904, 8192), (7, 8, 8192), (8191, 8192, 8192), (8192, 8192, 8192),
                                     (8197, 8256, 8192), (16384, 16384, 8192), (160, 192, 64)])
def test_chunk_schedule(V, ld, nc):
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import ops
    sched = ops.logprob_chunks(V, ld, nc)
    assert sched == E.chunk_schedule(V, ld, nc)
    covered = np.zeros(V, dtype=np.int64)
    for i, (c0, n) in enumerate(sched):
        assert c0 == i * nc and 1 <= n <= nc and c0 + n <= ld and c0 < V
        covered[c0:min(c0 + n, V)] += 1
    assert (covered == 1).all()            # [0, V) exactly once
    assert sched[-1][0] + sched[-1][1] >= V and all(c0 + n < V for c0, n in sched[:-1])  # only the last chunk reaches V
    if V < nc:
        assert sched == [(0, ld)]
    if V == 51865:
        assert len(sched) == 7 and sched[-1] == (49152, 2752)  # the last chunk is partial
    with pytest.raises(ValueError):
        ops.logprob_chunks(9, 8, 64)


def test_check_evaluate_args():
    whisper, cfg = _cfg(max_target_positions=16)
    assert whisper.check_evaluate_args(cfg, (3, 9), None) == (3, 9)
    assert whisper.check_evaluate_args(cfg, (1, 2), (1, 2), mask_sum=1.0, mask_min=0.0) == (1, 2)
    for bad in (dict(labels_shape=(3,)), dict(labels_shape=(0, 4)), dict(labels_shape=(2, 1)), dict(labels_shape=(2, 17)),
                dict(labels_shape=(2, 4), mask_shape=(2, 3)), dict(labels_shape=(2, 4), mask_shape=(4, 2)),
                dict(labels_shape=(2, 4), mask_shape=(2, 4), mask_sum=0.0),
                dict(labels_shape=(2, 4), mask_shape=(2, 4), mask_sum=float("nan")),
                dict(labels_shape=(2, 4), mask_shape=(2, 4), mask_sum=2.0, mask_min=-1.0)):
        with pytest.raises(ValueError):
            whisper.check_evaluate_args(cfg, **bad)


class _FakeModel:
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def evaluate(self, features, labels, mask=None):
        self.calls.append((features.shape[0], mask is not None))
        n = float(features.shape[0])
        return {"loss": 99.0, "accuracy": 99.0, "loss_sum": 2.0 * n, "n_correct": 0.25 * n, "n_tokens": n}


class _FakeStrategy:
    world, force_collectives = 1, False

    def reduce_sum(self, x):
        raise AssertionError("one replica: no collective")


def test_evaluate_whisper_sums_and_prints():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import train
    model, lines = _FakeModel(), []
    f = lambda n: torch.zeros(n, 2, 3)  # noqa: E731
    batches = [(f(4), None), (f(0), None), (f(2), None, torch.ones(2, 2))]
    out = train.evaluate_whisper(_FakeStrategy(), model, iter(batches), log=lines.append, step=40)
    assert model.calls == [(4, False), (2, True)]  # the empty batch is skipped: it contributes zeros
    assert out["loss_sum"] == 12.0 and out["n_correct"] == 1.5 and out["n_tokens"] == 6.0
    assert out["loss"] == 2.0 and out["accuracy"] == 0.25  # the ratio of the sums, not a mean of per-batch ratios
    assert lines == ["Eval step 40, Loss: 2.0000, Accuracy: 0.2500"]

    class TwoRanks(_FakeStrategy):
        world, n = 2, 0

        def reduce_sum(self, x):
            TwoRanks.n += 1
            assert x.dtype == torch.float64 and x.shape == (3,)
            return x * 2  # the peer saw the same

    out2 = train.evaluate_whisper(TwoRanks(), _FakeModel(), iter(batches))
    assert TwoRanks.n == 1 and out2["n_tokens"] == 12.0 and out2["loss"] == 2.0  # one reduction after the loop
    # a rank with an empty shard still joins the reduction
    class Peer(TwoRanks):
        def reduce_sum(self, x):
            assert x.tolist() == [0.0, 0.0, 0.0]
            return x + torch.tensor([3.0, 1.0, 2.0], dtype=torch.float64)
    assert train.evaluate_whisper(Peer(), _FakeModel(), iter([]))["loss"] == 1.5
    with pytest.raises(ValueError):
        train.evaluate_whisper(_FakeStrategy(), _FakeModel(), iter([]))


def test_library_has_the_scoring_entry_points_and_the_abi_is_unchanged():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib, ops
    for name in ("tmi_logprob_fold", "tmi_logprob_state_bytes", "tmi_logprob_chunk_cols"):
        assert name in _lib.SIGNATURES
    h = _lib.lib()
    assert _lib.ABI_VERSION == 31 and h.tmi_abi_version() == 31
    nc = ops.logprob_chunk_cols()
    assert nc >= 256 and nc % 256 == 0  # a multiple of the fast GEMM's widest N tile
    assert h.tmi_logprob_state_bytes(5) == 160 and h.tmi_logprob_state_bytes(0) == -1 and ops.logprob_state_elems(5) == 20
    # rejected before anything is launched (no GPU needed): null pointers
    assert h.tmi_logprob_fold(None, 64, 0, 1, 7, 0, 8, None, None, 0, None, 0, 0, 0, None, 0, 1, 1, None, None, None, None) == -1
    assert b"tmi_logprob_fold" in h.tmi_last_error()
