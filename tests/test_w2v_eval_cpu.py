"""Wav2Vec2 evaluation, the parts that need no GPU: the float64 restatement (tests/_w2v_eval_ref.py) against the oracle's
``contrastive_loss`` / ``quantizer`` and a naive per-row loop, the special rows of the mask rule, ``perplexity_from_counts``,
``check_evaluate_args``, ``evaluate_wav2vec2``'s summing, single reduction and log line with a fake model, the CLI's
parser, and the new C entry points in the built library (ABI still 31)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import _w2v_eval_ref as E
from oracle import wav2vec2_oracle as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEMP = 0.1


def _w2v():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import wav2vec2
    return wav2vec2


def _inputs(B, T, pd, Nn, seed, per_time=False):
    w = _w2v()
    g = np.random.default_rng(seed)
    h = g.standard_normal((B, T, pd))
    q = 2.5 / np.sqrt(pd) * h + g.standard_normal((B, T, pd))
    neg = w.sample_negative_indices_roll(g, T, Nn) if per_time else w.sample_negative_indices(g, B, T, Nn)
    return h, q, neg


# ---------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("per_time", [False, True], ids=["[B,Nn]", "[T,Nn]"])
def test_unmasked_restatement_equals_the_oracle(per_time):
    B, T, pd, Nn = 3, 23, 16, 9
    h, q, neg = _inputs(B, T, pd, Nn, 3, per_time)
    ref = E.score(h, q, neg, TEMP, per_time=per_time)
    on = torch.from_numpy(neg).long()
    if per_time:
        on = on[None].expand(B, -1, -1)
    logits, loss = V.contrastive_loss(torch.from_numpy(h), torch.from_numpy(q), on, TEMP)
    assert np.allclose(ref["z"], logits.numpy(), rtol=0, atol=1e-11)
    assert abs(ref["row_loss"].mean() - float(loss)) < 1e-12
    # the flags are argmax(logits) == 0 - except where a negative IS frame t: there the restatement ties exactly (gap 0,
    # correct), while the oracle forms the positive and the negatives with two different sums that differ in the last bit
    tie = ref["gap"] == 0.0
    n3 = E._neg3(neg, B, T, per_time)
    assert (tie <= (n3 == np.arange(T)[None, :, None]).any(-1)).all()
    assert (np.abs(ref["gap"][~tie]) > 1e-9).all()
    assert (ref["row_correct"] == (logits.argmax(-1) == 0).numpy())[~tie].all() and (ref["row_correct"][tie] == 1).all()
    assert 0 < ref["row_correct"].sum() < B * T  # the flag goes both ways on these inputs
    assert ref["valid"].all() and ref["keep"].all()


def test_unmasked_perplexity_from_counts_equals_the_oracle_quantizer():
    w = _w2v()
    cfg = V.make_config("base", hidden_size=16, codevector_dim=8, num_codevectors_per_group=5, num_codevector_groups=2)
    p = V.init_params(cfg, seed=2, dtype=torch.float64)
    hidden = torch.from_numpy(np.random.default_rng(4).standard_normal((3, 11, 16)))
    _, idx, ppl, _ = V.quantizer(p, hidden, cfg)
    counts = E.code_counts(idx.reshape(-1, 2).numpy(), 5)
    assert counts.sum(1).tolist() == [33, 33]
    assert abs(E.perplexity_from_counts(counts) - float(ppl)) < 1e-12
    assert abs(w.perplexity_from_counts(counts) - float(ppl)) < 1e-12
    assert abs(w.perplexity_from_counts(torch.from_numpy(counts)) - E.perplexity_from_counts(counts)) < 1e-14
    # closed forms: one code only -> 1 (up to the 1e-10 of the log); all Nc codes equally -> Nc
    assert abs(w.perplexity_from_counts([[7, 0, 0, 0]]) - 1.0) < 1e-8
    assert abs(w.perplexity_from_counts([[3, 3, 3, 3], [12, 0, 0, 0]]) - 2.5) < 1e-8
    # a function of the counts of the whole set, not a mean of batch values
    a, b = np.array([[4, 0]]), np.array([[0, 4]])
    assert abs(w.perplexity_from_counts(a + b) - 2.0) < 1e-8 and abs(w.perplexity_from_counts(a) - 1.0) < 1e-8
    for bad in ([[0, 0]], [[1, -1]], [1, 2]):
        with pytest.raises(ValueError):
            w.perplexity_from_counts(bad)


@pytest.mark.parametrize("per_time", [False, True], ids=["[B,Nn]", "[T,Nn]"])
def test_masked_restatement_equals_a_naive_loop(per_time):
    B, T, pd, Nn = 3, 13, 8, 6
    h, q, neg = _inputs(B, T, pd, Nn, 5, per_time)
    lengths = (T, 8, 1)
    mask = (np.arange(T)[None, :] < np.array(lengths)[:, None]).astype(np.float32)
    ref = E.score(h, q, neg, TEMP, mask, per_time)
    loss, correct = E.score_naive(h, q, neg, TEMP, mask, per_time)
    assert np.allclose(ref["row_loss"], loss, rtol=0, atol=1e-11) and (ref["row_correct"] == correct).all()
    assert (ref["row_loss"][mask == 0] == 0).all() and (ref["row_correct"][mask == 0] == 0).all()
    # a single valid frame: every negative other than the frame itself is masked
    assert ref["valid"][2].sum() == 1 and ref["row_correct"][2, 0] == 1
    only_self = E.score(h[2:], q[2:], np.zeros((1, 2), dtype=np.int32) if not per_time else np.zeros((T, 2), dtype=np.int32),
                        TEMP, mask[2:], per_time)
    assert abs(only_self["row_loss"][0, 0] - np.log(3.0)) < 1e-12  # the positive three times: log 3, and a tie counts as correct
    assert only_self["row_correct"][0, 0] == 1 and only_self["gap"][0, 0] == 0.0
    # unmasked, the naive loop agrees as well
    l0, c0 = E.score_naive(h, q, neg, TEMP, None, per_time)
    ref0 = E.score(h, q, neg, TEMP, None, per_time)
    assert np.allclose(ref0["row_loss"], l0, rtol=0, atol=1e-11) and (ref0["row_correct"] == c0).all()


def test_special_rows():
    B, T, pd = 1, 6, 8
    h, q, _ = _inputs(B, T, pd, 3, 7)
    # a negative equal to t: the gap is exactly 0 and the row counts as correct when nothing else beats it
    q2 = q.copy()
    q2[0, 1:] = -h[0, 0] * 5      # every other frame scores far below the positive for row 0
    q2[0, 0] = h[0, 0]
    neg = np.array([[0, 3, 0]], dtype=np.int32)
    r = E.score(h, q2, neg, TEMP)
    assert r["gap"][0, 0] == 0.0 and r["row_correct"][0, 0] == 1 and r["row_loss"][0, 0] > np.log(3.0) - 1e-9
    # all negatives masked: loss 0, correct 1; the masked rows themselves: loss 0, correct 0
    mask = np.array([[1, 1, 0, 0, 0, 0]], dtype=np.float32)
    r = E.score(h, q, np.array([[2, 5, 4]], dtype=np.int32), TEMP, mask)
    assert (r["row_loss"][0, :2] == 0).all() and (r["row_correct"][0, :2] == 1).all() and np.isinf(r["gap"][0, :2]).all()
    assert (r["row_loss"][0, 2:] == 0).all() and (r["row_correct"][0, 2:] == 0).all()
    assert not r["keep"][0, :, 1:].any() and r["keep"][0, :, 0].all()
    # counts over valid rows, indices clamped as tmi_vq_assign clamps them
    idx = np.array([[0, 9], [-3, 1], [2, 2]])
    assert E.code_counts(idx, 3).tolist() == [[2, 0, 1], [0, 1, 2]]
    assert E.code_counts(idx, 3, mask=[1, 0, 1]).tolist() == [[1, 0, 1], [0, 0, 2]]
    # the bounds are built from the reference alone
    bound, band = E.bounds(E.score(h, q, neg, TEMP), pd, 3)
    assert bound.shape == (1, 6) and (bound > band).all() and (band > 0).all()


# ---------------------------------------------------------------------------------------- host logic of the package
def test_check_evaluate_args():
    w = _w2v()
    cfg = w.make_config("base", conv_dim=(8, 8), conv_stride=(5, 2), conv_kernel=(10, 3), num_codevectors_per_group=4,
                        num_codevector_groups=2)
    audio = torch.zeros(2, 100)
    T = w.frame_lengths(cfg, [100])[0]
    assert T == 10
    neg = torch.zeros(2, 3, dtype=torch.int32)
    assert w.check_evaluate_args(cfg, audio, neg)[:4] == (2, 100, 10, 3)
    mask = w.frame_attention_mask(cfg, (100, 30), 100)
    out = w.check_evaluate_args(cfg, audio, neg, mask, torch.zeros(2, 10, 2, dtype=torch.int32))
    assert out[4].dtype == torch.float32 and out[4].sum() == 13
    assert w.check_evaluate_args(cfg, audio, torch.zeros(10, 3, dtype=torch.int32), per_time=True)[3] == 3
    for bad in (dict(audio=audio.double()), dict(audio=torch.zeros(100)), dict(audio=torch.zeros(0, 100)),
                dict(neg_indices=neg.long())):
        with pytest.raises(TypeError):
            w.check_evaluate_args(cfg, **{**dict(audio=audio, neg_indices=neg), **bad})
    for bad in (dict(neg_indices=torch.zeros(3, 3, dtype=torch.int32)),                       # one row per batch row
                dict(neg_indices=torch.zeros(2, 0, dtype=torch.int32)),                       # Nn >= 1
                dict(neg_indices=torch.full((2, 3), 10, dtype=torch.int32)),                  # idx < T
                dict(neg_indices=torch.full((2, 3), -1, dtype=torch.int32)),                  # idx >= 0
                dict(neg_indices=neg, per_time=True),                                         # [T, Nn] expected
                dict(attention_mask=torch.ones(2, 9)), dict(attention_mask=torch.ones(10, 2)),
                dict(attention_mask=torch.full((2, 10), 0.5)),                                # binary here
                dict(attention_mask=torch.zeros(2, 10)),                                      # at least one valid frame
                dict(forced_codes=torch.zeros(2, 10, 1, dtype=torch.int32)),
                dict(forced_codes=torch.full((2, 10, 2), 4, dtype=torch.int32)),
                dict(forced_codes=torch.zeros(2, 10, 2))):
        with pytest.raises(ValueError):
            w.check_evaluate_args(cfg, **{**dict(audio=audio, neg_indices=neg), **bad})


class _Cfg:
    num_codevector_groups, num_codevectors_per_group, diversity_loss_weight = 2, 3, 0.1


class _FakeModel:
    device = torch.device("cpu")
    config = _Cfg()

    def __init__(self):
        self.calls = []

    def evaluate(self, audio, neg, mask=None):
        self.calls.append((audio.shape[0], mask is not None))
        n = float(audio.shape[0])
        # batch sizes 4 and 2 use different codes: a mean of per-batch perplexities (1 each) is not the set's (2)
        counts = torch.tensor([[4, 0, 0], [4, 0, 0]]) if n == 4 else torch.tensor([[0, 2, 0], [0, 0, 2]])
        return {"loss": 99.0, "accuracy": 99.0, "perplexity": 99.0, "loss_sum": 2.0 * n, "n_correct": 0.25 * n, "n_frames": n,
                "code_counts": counts}


class _FakeStrategy:
    world, force_collectives = 1, False

    def reduce_sum(self, x):
        raise AssertionError("one replica: no collective")


def test_evaluate_wav2vec2_sums_and_prints():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import train
    w = _w2v()
    model, lines = _FakeModel(), []
    f = lambda n: torch.zeros(n, 5)  # noqa: E731
    batches = [(f(4), None), (f(0), None), (f(2), None, torch.ones(2, 2))]
    out = train.evaluate_wav2vec2(_FakeStrategy(), model, iter(batches), log=lines.append, step=40)
    assert model.calls == [(4, False), (2, True)]  # the empty batch is skipped: it contributes zeros
    assert out["loss_sum"] == 12.0 and out["n_correct"] == 1.5 and out["n_frames"] == 6.0
    assert out["contrastive_loss"] == 2.0 and out["accuracy"] == 0.25  # the ratio of the sums, not a mean of ratios
    assert out["code_counts"].tolist() == [[4, 2, 0], [4, 0, 2]] and out["code_counts"].dtype == torch.int64
    ppl = w.perplexity_from_counts([[4, 2, 0], [4, 0, 2]])
    assert out["perplexity"] == ppl and 1.8 < ppl < 2.0  # from the total counts: neither batch's own value (1.0)
    assert out["code_usage"] == 4.0 / 6.0
    assert abs(out["loss"] - (2.0 - 0.1 * ppl)) < 1e-15
    assert lines == [f"Eval step 40, Loss: {2.0 - 0.1 * ppl:.4f}, Accuracy: 0.2500, Perplexity: {ppl:.4f}"]

    class TwoRanks(_FakeStrategy):
        world, n = 2, 0

        def reduce_sum(self, x):
            TwoRanks.n += 1
            assert x.dtype == torch.float64 and x.shape == (3 + 2 * 3,)
            return x * 2  # the peer saw the same

    out2 = train.evaluate_wav2vec2(TwoRanks(), _FakeModel(), iter(batches))
    assert TwoRanks.n == 1 and out2["n_frames"] == 12.0 and out2["contrastive_loss"] == 2.0  # one reduction after the loop
    assert out2["code_counts"].tolist() == [[8, 4, 0], [8, 0, 4]] and out2["perplexity"] == ppl

    # a rank with an empty shard still joins the reduction
    class Peer(TwoRanks):
        def reduce_sum(self, x):
            assert x.tolist() == [0.0] * 9
            return x + torch.tensor([3.0, 1.0, 2.0, 2, 0, 0, 1, 1, 0], dtype=torch.float64)
    out3 = train.evaluate_wav2vec2(Peer(), _FakeModel(), iter([]))
    assert out3["contrastive_loss"] == 1.5 and out3["code_counts"].tolist() == [[2, 0, 0], [1, 1, 0]]
    with pytest.raises(ValueError):
        train.evaluate_wav2vec2(_FakeStrategy(), _FakeModel(), iter([]))
    with pytest.raises(ValueError):
        train.evaluate_wav2vec2(_FakeStrategy(), _FakeModel(), iter([(f(0), None)]))


def test_train_wav2vec2_takes_the_eval_arguments():
    import inspect
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import train
    p = inspect.signature(train.train_wav2vec2).parameters
    assert (p["eval_every"].default, p["eval_batches"].default, p["eval_seed"].default) == (0, 0, 4321)


def test_library_has_the_evaluation_entry_points_and_the_abi_is_unchanged():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib
    for name in ("tmi_contrastive_score", "tmi_vq_count"):
        assert name in _lib.SIGNATURES
    h = _lib.lib()
    assert _lib.ABI_VERSION == 31 and h.tmi_abi_version() == 31
    # rejected before anything is launched (no GPU needed): null pointers, bad sizes
    assert h.tmi_contrastive_score(None, None, 8, 0, None, 3, 0, None, None, None, 2, 7, 8, 3, 0.1, None) == -1
    assert b"tmi_contrastive_score" in h.tmi_last_error()
    assert h.tmi_vq_count(None, None, None, 5, 2, 3, None) == -1
    assert b"tmi_vq_count" in h.tmi_last_error()
    import ctypes as C
    buf = (C.c_char * 4096)()
    a = (C.addressof(buf) + 63) // 64 * 64
    ok = dict(h=a, q=a + 1024, ld=8, dtype=0, neg=a + 2048, sb=3, st=0, mask=None, loss=a + 3072, corr=a + 3584, B=2, T=7, pd=8,
              Nn=3, temp=0.1)

    def score(**kw):
        v = {**ok, **kw}
        return h.tmi_contrastive_score(v["h"], v["q"], v["ld"], v["dtype"], v["neg"], v["sb"], v["st"], v["mask"], v["loss"],
                                       v["corr"], v["B"], v["T"], v["pd"], v["Nn"], v["temp"], None)

    for bad in (dict(h=a + 4), dict(q=a + 1024 + 8), dict(pd=6, ld=6), dict(dtype=1, pd=4, ld=4), dict(ld=4), dict(ld=10),
                dict(B=0), dict(T=0), dict(Nn=0), dict(T=(1 << 30) + 1), dict(B=1 << 16, T=1 << 15), dict(Nn=(1 << 30) + 1),
                dict(temp=0.0), dict(temp=-1.0), dict(temp=float("nan")), dict(dtype=2), dict(sb=-1), dict(loss=None),
                dict(corr=None), dict(neg=None), dict(mask=a + 2)):
        assert score(**bad) == -1, bad
        assert b"tmi_contrastive_score" in h.tmi_last_error()
    for bad in ((a, None, a + 1024, 0, 2, 3), (a, None, a + 1024, 5, 0, 3), (a, None, a + 1024, 5, 2, 0),
                (a, None, a + 1024, 5, 2, 8192), (a, None, a + 1024 + 4, 5, 2, 3), (a, None, a + 1024, (1 << 30) + 1, 2, 3)):
        assert h.tmi_vq_count(*bad, None) == -1, bad
        assert b"tmi_vq_count" in h.tmi_last_error()
    assert bytes(buf) == bytes(4096)  # a rejected call writes nothing


def test_cli_parser():
    spec = importlib.util.spec_from_file_location("wav2vec2_eval", os.path.join(ROOT, "speech_jobs", "wav2vec2_eval.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    a = cli.parse_args([])
    assert (a.model_size, a.weights, a.batch_size, a.num_batches, a.precision, a.clip_samples, a.seed, a.ragged) == \
        ("base", None, 8, 5, "bf16", 32000, 4321, False)
    a = cli.parse_args(["--model_size", "tiny", "--batch_size", "3", "--num_batches", "2", "--precision", "fp32",
                        "--clip_samples", "2600", "--seed", "7", "--ragged", "--out", "x.json", "--weights", "w.pt"])
    assert (a.model_size, a.batch_size, a.num_batches, a.precision, a.clip_samples, a.seed, a.ragged, a.out, a.weights) == \
        ("tiny", 3, 2, "fp32", 2600, 7, True, "x.json", "w.pt")
    for bad in (["--batch_size", "0"], ["--num_batches", "0"], ["--precision", "fp16"], ["--clip_samples", "2"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
    lens = cli.ragged_lengths(np.random.default_rng(3), 64, 2600)
    assert len(lens) == 64 and min(lens) >= 650 and max(lens) <= 2600 and len(set(lens)) > 32
    assert lens == cli.ragged_lengths(np.random.default_rng(3), 64, 2600)  # drawn from the seed
