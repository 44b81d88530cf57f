"""The reference of tmi_edit_distance (tests/_edit_ref.py) against independent checks, the planted cases against the
reference, the normalisation, the host-side validators around the kernel, and the header / binding.  No GPU."""
import itertools
import os
import re

import numpy as np
import pytest
import torch

import _edit_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pkg():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib, ops, train, wav2vec2, whisper
    return _lib, ops, train, wav2vec2, whisper


# ------------------------------------------------------------------------------------------------- the rule
def test_rule_against_the_numpy_distance_on_random_pairs():
    _, _, _, W, _ = _pkg()
    rng = np.random.default_rng(5)
    for k in range(2400):
        n, m = int(rng.integers(0, 41)), int(rng.integers(0, 41))
        A = 3 + (k & 1)
        h, r = rng.integers(0, A, n).tolist(), rng.integers(0, A, m).tolist()
        d, s, de, ins, nn, mm = E.rule(h, r)
        assert (nn, mm) == (n, m)
        assert d == W.edit_distance(np.asarray(h, np.int64), np.asarray(r, np.int64)), (h, r)
        assert s + de + ins == d and ins - de == n - m, (h, r)


def _alignments(h, r):
    """Every monotone alignment of h and r as its (d, sub, del, ins): a path of diagonal / up / left steps."""
    n, m = len(h), len(r)
    out = set()

    def walk(i, j, s, de, ins):
        if i == n and j == m:
            out.add((s + de + ins, s, de, ins))
            return
        if i < n and j < m:
            walk(i + 1, j + 1, s + (h[i] != r[j]), de, ins)
        if i < n:
            walk(i + 1, j, s, de, ins + 1)
        if j < m:
            walk(i, j + 1, s, de + 1, ins)

    walk(0, 0, 0, 0, 0)
    return out


def test_rule_against_exhaustive_alignments_over_two_symbols():
    seqs = [list(t) for k in range(5) for t in itertools.product((0, 1), repeat=k)]
    assert len(seqs) == 31
    for h in seqs:
        for r in seqs:
            al = _alignments(h, r)
            best = min(a[0] for a in al)
            got = E.rule(h, r)
            assert got[0] == best, (h, r)
            assert got[:4] in {a for a in al if a[0] == best}, (h, r, got)


# ------------------------------------------------------------------------------------------------- planted cases
@pytest.mark.parametrize("first,last", [(False, False), (True, False), (False, True), (True, True)])
def test_planted_counts_equal_the_rule(first, last):
    rng = np.random.default_rng(11 + 2 * first + last)
    for trial in range(12):
        kinds = [str(rng.choice(["s", "d", "i"])) for _ in range(int(rng.integers(2, 9)))]
        sites = [(k, int(rng.integers(1, 5))) for k in kinds]
        m = sum(run for _, run in sites) + 5 * (len(sites) + 1) + int(rng.integers(0, 40))
        hyp, ref, k = E.planted_case(m, sites, seed=trial, first=first, last=last)
        assert len(set(ref.tolist())) == m
        assert E.rule(hyp.tolist(), ref.tolist()) == (sum(k),) + k + (len(hyp), m), (sites, first, last)
    if first:  # the first site really is at the first position
        hyp, ref, _ = E.planted_case(30, [("s", 1), ("d", 1)], first=True, last=last)
        assert hyp[0] != ref[0]


@pytest.mark.parametrize("n,m", [(300, 290), (290, 300), (300, 300), (20, 300), (300, 25), (16, 16)])
def test_planted_sizes_equal_the_rule(n, m):
    hyp, ref, k = E.planted_sizes(n, m, seed=n * 1000 + m)
    assert (len(hyp), len(ref)) == (n, m)
    assert hyp[0] != ref[0] and hyp[-1] != ref[-1]  # edits at the very first and the very last position
    assert E.rule(hyp.tolist(), ref.tolist()) == (sum(k),) + k + (n, m)


def test_one_kept_token_between_sites_is_not_enough():
    """The separation the planted cases need: with ONE kept token between a deletion and an insertion a second optimal
    alignment (two substitutions) exists and the rule takes it."""
    ref, hyp = [1, 2, 3, 4], [1, 3, 9, 4]
    assert E.rule(hyp, ref)[:4] == (2, 2, 0, 0)


# ------------------------------------------------------------------------------------------------- normalisation
def test_normalisation():
    row = [5, 6, 50, 7, 101, 8]
    assert E.normalise(row) == row
    assert E.normalise(row, stop_id=50) == [5, 6]
    assert E.normalise([50] + row, stop_id=50) == []                      # a stop at position 0
    assert E.normalise(row, stop_id=49) == row                            # no stop in the row
    assert E.normalise(row, stop_id=-1) == row
    assert E.normalise([-1, 5, -1], stop_id=-1) == [-1, 5, -1]            # -1 is "none", not a token to stop at
    assert E.normalise(row, skip_lo=100, skip_hi=110) == [5, 6, 50, 7, 8]
    assert E.normalise(row, skip_lo=0, skip_hi=1000) == []                # a skip range that removes everything
    assert E.normalise(row, skip_lo=7, skip_hi=7) == row                  # skip_lo >= skip_hi: nothing is dropped
    assert E.normalise(row, skip_lo=110, skip_hi=100) == row
    assert E.normalise(row, length=99) == row                             # a length above the column count
    assert E.normalise(row, length=99, cols=4) == [5, 6, 50, 7]
    assert E.normalise(row, length=-3) == []                              # a negative length
    assert E.normalise(row, length=4, stop_id=7) == [5, 6, 50]
    assert E.normalise(row, length=3, stop_id=7) == [5, 6, 50]            # the stop lies past the length
    assert E.normalise([2 ** 31 - 1, -2 ** 31, 0], skip_lo=-2 ** 31, skip_hi=0) == [2 ** 31 - 1, 0]
    # the stop is looked for BEFORE tokens are dropped: a stop id inside the skip range still cuts
    assert E.normalise([5, 105, 6], stop_id=105, skip_lo=100, skip_hi=110) == [5]
    out = E.reference([[1, 2, 3, 50, 9]] * 2, [[1, 3, 50, 9, 9]], R=2, stop_id=50)
    assert out.tolist() == [[1, 0, 0, 1, 3, 2]] * 2  # the hypothesis holds one token more: an insertion


# ------------------------------------------------------------------------------------------------- host validators
def _cfg(**kw):
    _, _, _, _, W = _pkg()
    return W.make_config("small", d_model=128, encoder_attention_heads=2, decoder_attention_heads=2, d_ff=256, vocab_size=160,
                         encoder_layers=2, decoder_layers=2, n_mels=16, n_ctx=32, decoder_start_token_id=150,
                         max_target_positions=32, **kw)


def test_check_evaluate_generate_args():
    _, _, _, _, W = _pkg()
    cfg, chk = _cfg(), W.check_evaluate_generate_args
    assert chk(cfg, (3, 7), torch.int32) == 0
    assert chk(cfg, (3, 7), torch.int32, np.asarray([0, 7, 3]), {"num_beams": 3}) == 0
    assert chk(cfg, (3, 7), torch.int32, None, {"prompt_ids": [4, 5]}) == 2
    assert chk(cfg, (3, 7), torch.int32, None, {"prompt_ids": np.zeros((3, 5), np.int64)}) == 5
    assert chk(cfg, (3, 7), torch.int32, None, {}, n_ref_tokens=1.0) == 0
    for args, err in ((((3,), torch.int32), ValueError), (((3, 7), torch.int64), TypeError), (((0, 7), torch.int32), ValueError),
                      (((3, 0), torch.int32), ValueError), (((3, 4097), torch.int32), ValueError),
                      (((3, 7), torch.int32, np.asarray([0, 8, 3])), ValueError),
                      (((3, 7), torch.int32, np.asarray([0, -1, 3])), ValueError),
                      (((3, 7), torch.int32, np.asarray([1, 2])), ValueError),
                      (((3, 7), torch.int32, np.asarray([1.0, 2.0, 3.0])), ValueError),
                      (((3, 7), torch.int32, np.asarray([0, 0, 0])), ValueError),
                      (((3, 7), torch.int32, None, {"return_token_timestamps": True}), ValueError),
                      (((3, 7), torch.int32, None, {"return_dict_in_generate": True}), ValueError),
                      (((3, 7), torch.int32, None, {"prompt_ids": np.zeros((1, 2, 3))}), ValueError)):
        with pytest.raises(err):
            chk(cfg, *args)
    with pytest.raises(ValueError):
        chk(cfg, (3, 7), torch.int32, None, {}, n_ref_tokens=0.0)


def _fake_edit_distance(hyp, ref, hyp_len=None, ref_len=None, R=1, stop_id=-1, skip=(0, 0), out=None):
    """``ops.edit_distance`` by the reference, on host tensors."""
    t = lambda x: None if x is None else x.numpy()
    return torch.from_numpy(E.reference(hyp.numpy(), ref.numpy(), t(hyp_len), t(ref_len), R, stop_id, skip))


def test_word_error_rate_on_hand_written_sentences(monkeypatch):
    _, ops, _, _, W = _pkg()
    calls = []
    monkeypatch.setattr(ops, "edit_distance", lambda *a, **k: (calls.append(1), _fake_edit_distance(*a, **k))[1])
    hyp = ["the cat sat on mat", "hello  world", "", "a b c d"]
    ref = ["the cat sat on the mat", "hello\tworld", "one two", "a x c"]
    r = W.word_error_rate(hyp, ref, device="cpu")
    assert len(calls) == 1  # one launch for all pairs
    # pair 0: one deletion; pair 1: exact (whitespace of any kind splits); pair 2: two deletions; pair 3: b -> x, d inserted
    assert (r["n_edits"], r["n_sub"], r["n_del"], r["n_ins"]) == (5.0, 1.0, 3.0, 1.0)
    assert (r["n_ref_tokens"], r["n_hyp_tokens"], r["n_exact"], r["n_items"]) == (13.0, 11.0, 1.0, 4.0)
    assert r["token_error_rate"] == 5.0 / 13.0 and r["n_oracle_edits"] == 5.0 and r["oracle_error_rate"] == 5.0 / 13.0
    assert W.word_error_rate(["The cat"], ["the cat"], device="cpu")["n_sub"] == 1.0  # no case folding
    for bad in ((["a"], ["a", "b"]), ([], []), (["a"], [" "])):
        with pytest.raises(ValueError):
            W.word_error_rate(*bad, device="cpu")


def test_edit_counts_sums_and_oracle_minimum():
    _, ops, _, _, _ = _pkg()
    rng = np.random.default_rng(3)
    out = rng.integers(0, 50, (12, 6)).astype(np.int32)
    for R in (1, 3, 4):
        assert ops.edit_counts(torch.from_numpy(out), R) == E.counts(out, R)
    valid = np.asarray([[True, False, True], [False, False, False], [True, True, True], [True, True, False]])
    got = ops.edit_counts(torch.from_numpy(out), 3, valid=torch.from_numpy(valid))
    assert got == E.counts(out, 3, valid)
    assert got["n_oracle_edits"] == float(sum(min(out[3 * b + k, 0] for k in range(3) if k == 0 or valid[b, k]) for b in range(4)))
    assert set(got) == set(ops.EDIT_COUNT_KEYS) | {"token_error_rate", "oracle_error_rate"}


class _StubStrategy:
    def __init__(self, world=2, other=None):
        self.world, self.force_collectives, self.rank, self.calls, self.other = world, False, 0, 0, other

    def reduce_sum(self, t):
        self.calls += 1
        return t if self.other is None else t + torch.tensor(self.other, dtype=t.dtype)


class _StubModel:
    device = torch.device("cpu")

    def __init__(self):
        self.seen = []

    def evaluate_generate(self, features, labels, **kw):
        _, ops, _, _, _ = _pkg()
        self.seen.append(kw)
        b = float(features.shape[0])
        return ops.finish_edit_counts({"n_edits": 3 * b, "n_sub": b, "n_del": 2 * b, "n_ins": 0.0, "n_ref_tokens": 10 * b,
                                       "n_hyp_tokens": 8 * b, "n_exact": 1.0, "n_items": b, "n_oracle_edits": 2 * b})


def test_evaluate_generate_whisper_sums_and_reduces_once():
    _, ops, T, _, _ = _pkg()
    batches = [(torch.zeros(2, 4, 8), torch.zeros(2, 5, dtype=torch.int32)), (torch.zeros(0, 4, 8), torch.zeros(0, 5, dtype=torch.int32)),
               (torch.zeros(3, 4, 8), torch.zeros(3, 5, dtype=torch.int32), "mask")]
    model, lines = _StubModel(), []
    r = T.evaluate_generate_whisper(None, model, batches, log=lines.append, step=7, num_beams=3)
    assert model.seen == [{"num_beams": 3}] * 2  # the empty batch is skipped
    assert (r["n_edits"], r["n_sub"], r["n_del"], r["n_ins"], r["n_ref_tokens"], r["n_items"]) == (15.0, 5.0, 10.0, 0.0, 50.0, 5.0)
    assert r["n_exact"] == 2.0 and r["token_error_rate"] == 0.3 and r["oracle_error_rate"] == 0.2
    assert lines == ["Eval step 7, TER: 0.3000, Sub: 5, Del: 10, Ins: 0"]
    assert set(r) == set(ops.EDIT_COUNT_KEYS) | {"token_error_rate", "oracle_error_rate"}
    # replicas: ONE reduction after the loop; an empty shard contributes zeros and gets the others' sums
    other = [float(v) for v in (4, 1, 1, 2, 20, 21, 0, 2, 3)]
    st = _StubStrategy(other=other)
    r2 = T.evaluate_generate_whisper(st, _StubModel(), [], log=None)
    assert st.calls == 1 and r2["n_edits"] == 4.0 and r2["token_error_rate"] == 0.2 and r2["oracle_error_rate"] == 0.15
    st = _StubStrategy(other=other)
    r3 = T.evaluate_generate_whisper(st, _StubModel(), batches)
    assert st.calls == 1 and r3["n_edits"] == 19.0 and r3["n_ref_tokens"] == 70.0
    with pytest.raises(ValueError):
        T.evaluate_generate_whisper(None, _StubModel(), [])


# ------------------------------------------------------------------------------------------------- header and binding
def test_header_declares_and_binding_matches():
    L, _, _, _, _ = _pkg()
    text = open(os.path.join(ROOT, "include", "tethys_mi.h")).read()
    m = re.search(r"\bint tmi_edit_distance\(([^;]*)\);", text)
    assert m, "tmi_edit_distance is not declared in include/tethys_mi.h"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    res, args = L.SIGNATURES["tmi_edit_distance"]
    assert len(params) == len(args) == 16
    for p, a in zip(params, args):
        want = L.c_vp if "*" in p else {"int64_t": L.c_i64, "int32_t": L.c_i32}[p.split()[0]]
        assert a is want, p
    assert res is L.c_i32
    assert L.ABI_VERSION == 31
    for phrase in ("TMI_ERR_INVALID, before anything is launched", "No atomics", "the same call gives the same bits", "Not built: a backtrace"):
        assert phrase in text[text.index("Error-rate evaluation"):text.index("int tmi_edit_distance(")], phrase
    mk = open(os.path.join(ROOT, "tethys-speech_amd", "csrc", "Makefile")).read()
    assert "edit.hip" in mk and os.path.exists(os.path.join(ROOT, "tethys-speech_amd", "csrc", "edit.hip"))
