"""The reference of tmi_edit_align (tests/_edit_align_ref.py) against independent checks, ``check_path`` against planted
corruptions, the case list of the GPU test against every other order of the candidates, the header / binding of the new
symbols and the host logic around the kernels.  No GPU."""
import functools
import itertools
import json
import os
import re

import numpy as np
import pytest
import torch

import _edit_align_ref as A
import _edit_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pkg():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib, ops, train, wav2vec2, whisper
    return _lib, ops, train, wav2vec2, whisper


# ------------------------------------------------------------------------------------------------- the reference
def _all_alignments(h, r):
    """Every monotone alignment of h and r as a tuple of (op, i, j) steps, by brute force."""
    n, m = len(h), len(r)
    out = []

    def walk(i, j, path):
        if i == n and j == m:
            out.append(tuple(path))
            return
        if i < n and j < m:
            walk(i + 1, j + 1, path + [(A.SUB if h[i] != r[j] else A.MATCH, i, j)])
        if i < n:
            walk(i + 1, j, path + [(A.INS, i, -1)])
        if j < m:
            walk(i, j + 1, path + [(A.DEL, -1, j)])

    walk(0, 0, [])
    return out


def _path_top_down(h, r):
    """The rule's path, stated a second way: the distances by a memoised recursion, and from (n, m) backwards the FIRST of
    diagonal, up, left that reaches the cell's distance (a later candidate wins only when strictly smaller = the first
    among the smallest wins)."""
    @functools.lru_cache(maxsize=None)
    def d(i, j):
        if i == 0 or j == 0:
            return i + j
        return min(d(i - 1, j - 1) + (h[i - 1] != r[j - 1]), d(i - 1, j) + 1, d(i, j - 1) + 1)

    i, j, path = len(h), len(r), []
    while i > 0 or j > 0:
        if i > 0 and j > 0 and d(i - 1, j - 1) + (h[i - 1] != r[j - 1]) == d(i, j):
            i, j = i - 1, j - 1
            path.append((A.SUB if h[i] != r[j] else A.MATCH, i, j))
        elif i > 0 and d(i - 1, j) + 1 == d(i, j):
            i -= 1
            path.append((A.INS, i, -1))
        else:
            j -= 1
            path.append((A.DEL, -1, j))
    return path[::-1]


def _cost(path):
    return sum(1 for op, _, _ in path if op != A.MATCH)


def _small_pairs():
    seqs = [list(t) for k in range(5) for t in itertools.product((0, 1), repeat=k)]
    pairs = [(h, r) for h in seqs for r in seqs]
    rng = np.random.default_rng(8)
    for _ in range(150):  # and up to 5 tokens over three symbols
        pairs.append((rng.integers(0, 3, int(rng.integers(0, 6))).tolist(), rng.integers(0, 3, int(rng.integers(0, 6))).tolist()))
    return pairs


def test_reference_against_brute_force_and_a_second_statement_of_the_rule():
    for h, r in _small_pairs():
        out, path = A.align(h, r)
        every = _all_alignments(h, r)
        best = min(_cost(p) for p in every)
        assert tuple(path) in every and _cost(path) == best == out[0], (h, r)
        assert path == _path_top_down(h, r), (h, r)
        assert out == E.rule(h, r), (h, r)                     # the counts along the path are the counts of the table
        assert len(path) == len(r) + out[3] == len(h) + out[2]  # n_steps = m + ins = n + del


def test_reference_counts_equal_the_rule_on_larger_random_pairs():
    rng = np.random.default_rng(12)
    for k in range(300):
        h, r = rng.integers(0, 3 + (k & 1), int(rng.integers(0, 41))).tolist(), rng.integers(0, 3 + (k & 1), int(rng.integers(0, 41))).tolist()
        out, path = A.align(h, r)
        assert out == E.rule(h, r) and path == _path_top_down(h, r)


def test_normalise_cols_keeps_the_definition_and_the_columns():
    rng = np.random.default_rng(4)
    for _ in range(300):
        row = [int(x) for x in rng.choice([0, 1, 2, 3, E.STOP, 101, 105, -1, 2 ** 31 - 1], int(rng.integers(0, 20)))]
        kw = dict(length=int(rng.integers(-3, 25)), cols=int(rng.integers(0, len(row) + 1)), stop_id=int(rng.choice([-1, E.STOP, 2])),
                  skip_lo=int(rng.choice([0, 100, 110])), skip_hi=int(rng.choice([0, 100, 110])))
        toks, cols = A.normalise_cols(row, **kw)
        assert toks == E.normalise(row, **kw)
        assert [row[c] for c in cols] == toks and cols == sorted(set(cols))
    assert A.normalise_cols([5, 105, 6, 101, 7, E.STOP, 8], stop_id=E.STOP, skip_lo=100, skip_hi=110) == ([5, 6, 7], [0, 2, 4])


def test_reference_reports_the_columns_of_the_rows_as_passed():
    hyp = [[1, 105, 2, 101, 101, 3, E.STOP, 9]]
    ref = [[109, 1, 2, 100, 3, 3, 3, 3]]
    out, steps, ns = A.reference(hyp, ref, None, [6], stop_id=E.STOP, skip=E.SKIP)
    assert steps[0] == [(A.MATCH, 0, 1), (A.MATCH, 2, 2), (A.DEL, -1, 4), (A.MATCH, 5, 5)]
    assert out.tolist() == [[1, 0, 1, 0, 3, 4]] and ns.tolist() == [4]
    out, steps, ns = A.reference([[1, 2], [1, 3], [4, 4]], [[1, 2, 3]], [2, 2, 0], None, R=3)
    assert steps[1] == [(A.MATCH, 0, 0), (A.DEL, -1, 1), (A.MATCH, 1, 2)] and steps[2] == [(A.DEL, -1, 0), (A.DEL, -1, 1), (A.DEL, -1, 2)]
    assert steps[0] == [(A.MATCH, 0, 0), (A.MATCH, 1, 1), (A.DEL, -1, 2)] and ns.tolist() == [3, 3, 3]


# ------------------------------------------------------------------------------------------------- check_path
def test_check_path_accepts_the_reference_and_rejects_corruptions():
    rng = np.random.default_rng(21)
    kw = dict(stop_id=E.STOP, skip=E.SKIP)
    seen = set()
    for trial in range(60):
        n, m = int(rng.integers(3, 30)), int(rng.integers(3, 30))
        h_row = E.sprinkle(rng, rng.integers(0, 4, n + 3), n, stop_at=n - 1 if trial % 3 == 0 else None)
        r_row = E.sprinkle(rng, rng.integers(0, 4, m + 3), m)
        out, steps, _ = A.reference([h_row], [r_row], **kw)
        out, steps = out[0], steps[0]
        assert A.check_path(h_row, r_row, steps, out, **kw) == ""
        corrupt = {}
        k = int(rng.integers(0, len(steps)))
        op, a, b = steps[k]
        corrupt["dropped"] = steps[:k] + steps[k + 1:]
        corrupt["doubled"] = steps[:k] + [steps[k]] + steps[k:]
        corrupt["bad op"] = steps[:k] + [(4, a, b)] + steps[k + 1:]
        if op in (A.MATCH, A.SUB):
            corrupt["flipped"] = steps[:k] + [(A.SUB if op == A.MATCH else A.MATCH, a, b)] + steps[k + 1:]
            corrupt["split"] = steps[:k] + [(A.INS, a, -1), (A.DEL, -1, b)] + steps[k + 1:]  # valid, but not out's counts
            corrupt["lost side"] = steps[:k] + [(op, a, -1)] + steps[k + 1:]
        else:
            corrupt["wrong kind"] = steps[:k] + [(A.DEL if op == A.INS else A.INS, a, b)] + steps[k + 1:]
        q = max(k, 1)  # steps q - 1 and q exchanged: out of order, unless they are an insertion and a deletion (no common side)
        if len(steps) > 1 and {steps[q - 1][0], steps[q][0]} != {A.INS, A.DEL}:
            corrupt["swapped"] = steps[:q - 1] + [steps[q], steps[q - 1]] + steps[q + 1:]
        shifted = [(o, x + 1 if x >= 0 else x, y) for o, x, y in steps]  # compacted-style columns, off by one
        corrupt["shifted"] = shifted
        bad_out = out.copy()
        bad_out[1 + trial % 3] += 1
        assert A.check_path(h_row, r_row, steps, bad_out, **kw) != ""
        for name, bad in corrupt.items():
            assert A.check_path(h_row, r_row, bad, out, **kw) != "", (name, steps, bad)
            seen.add(name)
    assert seen >= {"dropped", "doubled", "bad op", "flipped", "split", "lost side", "wrong kind", "swapped", "shifted"}
    # without the normalisation arguments the skipped columns are missing from the path
    assert A.check_path([1, 105, 2], [1, 2], [(A.MATCH, 0, 0), (A.MATCH, 2, 1)], [0, 0, 0, 0, 2, 2]) != ""
    assert A.check_path([1, 105, 2], [1, 2], [(A.MATCH, 0, 0), (A.MATCH, 2, 1)], [0, 0, 0, 0, 2, 2], skip=E.SKIP) == ""


# ------------------------------------------------------------------------------------------------- the mutation check
def test_the_gpu_case_list_separates_the_rule_from_every_other_order():
    """The exhaustive pairs the GPU test launches: each of the five other orders of the three candidates gives another
    path than the rule on at least one of them (on 18, 270, 284, 466 and 474 of the 961), so a kernel that tried the
    candidates in another order could not pass."""
    hyp, ref, hl, rl = A.exhaustive_pairs()
    assert hyp.shape[0] == 961
    pairs = [(hyp[i, :hl[i]].tolist(), ref[i, :rl[i]].tolist()) for i in range(961)]
    rule = [A.align(h, r)[1] for h, r in pairs]
    differ = []
    for order in itertools.permutations(A.RULE):
        if order == A.RULE:
            continue
        n = sum(1 for (h, r), want in zip(pairs, rule) if A.align(h, r, order)[1] != want)
        assert n >= 1, order
        differ.append(n)
    assert sorted(differ) == [18, 270, 284, 466, 474]


# ------------------------------------------------------------------------------------------------- header and binding
def test_header_declares_and_binding_matches():
    L, _, _, _, _ = _pkg()
    text = open(os.path.join(ROOT, "include", "tethys_mi.h")).read()
    for name, count, ret in (("tmi_edit_align_workspace_bytes", 3, "int64_t"), ("tmi_edit_align", 21, "int"), ("tmi_edit_confusion", 16, "int")):
        m = re.search(r"\b%s %s\(([^;]*)\);" % (ret, name), text)
        assert m, f"{name} is not declared in include/tethys_mi.h"
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        res, args = L.SIGNATURES[name]
        assert len(params) == len(args) == count, name
        for p, a in zip(params, args):
            want = L.c_vp if "*" in p else {"int64_t": L.c_i64, "int32_t": L.c_i32}[p.split()[0]]
            assert a is want, (name, p)
        assert res is (L.c_i64 if ret == "int64_t" else L.c_i32)
        assert text.index("int tmi_edit_distance(") < m.start()  # declared after it, in a comment block of their own
    assert L.ABI_VERSION == 31
    block = text[text.index("/* tmi_edit_align:"):text.index("int64_t tmi_edit_align_workspace_bytes(")]
    for phrase in ("TMI_ERR_INVALID, before anything is launched", "the same call gives the same bits", "Not built: text normalisation",
                   "-1 for a deletion", "-1 for an insertion"):
        assert phrase in block, phrase
    mk = open(os.path.join(ROOT, "tethys-speech_amd", "csrc", "Makefile")).read()
    assert "edit.hip" in mk
    src = open(os.path.join(ROOT, "tethys-speech_amd", "csrc", "edit.hip")).read()
    for name in ("tmi_edit_align_workspace_bytes", "tmi_edit_align", "tmi_edit_confusion"):
        assert re.search(r'extern "C" \w+ %s\(' % name, src), name


def test_library_size_function_and_refusals_without_a_gpu():
    """What the library answers before it touches a device: the workspace size, and TMI_ERR_INVALID for every argument
    check (the refusals come before any launch, so they need no GPU)."""
    L, ops, _, _, _ = _pkg()
    lib = L.lib()
    f = lib.tmi_edit_align_workspace_bytes
    for N, hc, rc in ((1, 0, 0), (1, 1, 1), (3, 63, 64), (3, 64, 63), (2, 64, 64), (8, 448, 448), (5, 300, 200), (1, 4096, 4096),
                      (65535, 4096, 1)):
        assert f(N, hc, rc) == N * 16 * (hc + rc + 1) * ((min(hc, rc) + 64) // 64), (N, hc, rc)
        assert ops.edit_align_workspace_elems(N, hc, rc) * 4 == f(N, hc, rc)
    for N, hc, rc in ((0, 4, 4), (65536, 4, 4), (1, 4097, 4), (1, 4, 4097), (1, -1, 4), (1, 4, -1)):
        assert f(N, hc, rc) == -1
        with pytest.raises(ValueError):
            ops.edit_align_workspace_elems(N, hc, rc)
    buf = np.zeros(4096, np.int32)  # host memory: never dereferenced, every call below is refused first
    p = buf.ctypes.data
    good = dict(hyp=p, hyp_ld=8, hyp_cols=8, hyp_len=None, ref=p, ref_ld=8, ref_cols=8, ref_len=None, N=2, R=1, stop=-1, lo=0, hi=0,
                out=p, out_ld=6, steps=p, steps_ld=48, n_steps=p, ws=p, ws_bytes=f(2, 8, 8))

    def call(**over):
        a = dict(good, **over)
        return lib.tmi_edit_align(a["hyp"], a["hyp_ld"], a["hyp_cols"], a["hyp_len"], a["ref"], a["ref_ld"], a["ref_cols"],
                                  a["ref_len"], a["N"], a["R"], a["stop"], a["lo"], a["hi"], a["out"], a["out_ld"], a["steps"],
                                  a["steps_ld"], a["n_steps"], a["ws"], a["ws_bytes"], None)

    for over in (dict(hyp=None), dict(ref=None), dict(out=None), dict(steps=None), dict(n_steps=None), dict(ws=None), dict(N=0),
                 dict(N=65536), dict(R=0), dict(R=3), dict(hyp_cols=4097, hyp_ld=5000), dict(ref_cols=-1), dict(hyp_ld=7), dict(ref_ld=7),
                 dict(out_ld=5), dict(steps_ld=47), dict(ws_bytes=f(2, 8, 8) - 1), dict(hyp=p + 2), dict(steps=p + 1), dict(n_steps=p + 2),
                 dict(ws=p + 3), dict(hyp_len=p + 1)):
        assert call(**over) == -1, over
        assert b"tmi_edit_align" in lib.tmi_last_error()
    cgood = dict(steps=p, steps_ld=48, n_steps=p, hyp=p, hyp_ld=8, hyp_cols=8, ref=p, ref_ld=8, ref_cols=8, N=2, R=1, first=1, V=32,
                 counts=p, acc=0)

    def ccall(**over):
        a = dict(cgood, **over)
        return lib.tmi_edit_confusion(a["steps"], a["steps_ld"], a["n_steps"], a["hyp"], a["hyp_ld"], a["hyp_cols"], a["ref"],
                                      a["ref_ld"], a["ref_cols"], a["N"], a["R"], a["first"], a["V"], a["counts"], a["acc"], None)

    for over in (dict(steps=None), dict(n_steps=None), dict(hyp=None), dict(ref=None), dict(counts=None), dict(V=0), dict(V=1025),
                 dict(first=2), dict(acc=2), dict(N=0), dict(R=3), dict(steps_ld=47), dict(counts=p + 2), dict(ref_cols=4097)):
        assert ccall(**over) == -1, over
        assert b"tmi_edit_confusion" in lib.tmi_last_error()
    assert not buf.any()


# ------------------------------------------------------------------------------------------------- host logic
def test_chunking_arithmetic():
    _, ops, _, _, _ = _pkg()
    ch = ops.edit_align_chunks
    assert ops.EDIT_ALIGN_WORKSPACE_CAP == 256 << 20
    assert ch(10, 1, 100, 1000) == [(0, 10)]
    assert ch(25, 1, 100, 1000) == [(0, 10), (10, 10), (20, 5)]
    assert ch(24, 3, 100, 1000) == [(0, 9), (9, 9), (18, 6)]           # pieces are multiples of R
    assert ch(12, 4, 100, 350) == [(0, 4), (4, 4), (8, 4)]             # a cap below R pairs: R pairs all the same
    assert ch(5, 1, 0, 1000) == [(0, 5)]
    per = 16 * 8193 * 65                                               # a pair at the limits
    pieces = ch(100, 2, per)
    assert pieces[0] == (0, 30) and all(c * per <= 256 << 20 and c % 2 == 0 for _, c in pieces)
    assert sum(c for _, c in pieces) == 100 and [s for s, _ in pieces] == [0, 30, 60, 90]
    for N, R, pb, cap in ((65535, 1, per, 256 << 20), (60, 5, 12345, 99999), (7, 7, 1, 1)):
        got = ch(N, R, pb, cap)
        assert [s for s, _ in got] == [sum(c for _, c in got[:k]) for k in range(len(got))] and sum(c for _, c in got) == N
        assert all(c % R == 0 and (c * pb <= cap or c == R) for _, c in got)


def test_validators_learn_the_new_flags():
    _, _, _, V, W = _pkg()
    cfg = W.make_config("small", d_model=128, encoder_attention_heads=2, decoder_attention_heads=2, d_ff=256, vocab_size=160,
                        encoder_layers=2, decoder_layers=2, n_mels=16, n_ctx=32, decoder_start_token_id=150, max_target_positions=32)
    chk = W.check_evaluate_generate_args
    assert chk(cfg, (3, 7), torch.int32, None, {"prompt_ids": [4, 5]}, return_alignment=True) == 2
    assert chk(cfg, (3, 7), torch.int32, return_alignment=False) == 0
    for bad in ("out.jsonl", 1, None):
        with pytest.raises(TypeError):
            chk(cfg, (3, 7), torch.int32, return_alignment=bad)
    with pytest.raises(TypeError):
        W.word_error_rate(["a"], ["a"], device="cpu", return_alignment="yes")
    ccfg = V.Wav2Vec2Config()
    assert V.check_ctc_confusion_args(ccfg, False, False) is False and V.check_ctc_confusion_args(ccfg, False, True) is False
    assert V.check_ctc_confusion_args(ccfg, True, True) is True
    with pytest.raises(ValueError):
        V.check_ctc_confusion_args(ccfg, True, False)
    with pytest.raises(TypeError):
        V.check_ctc_confusion_args(ccfg, "table.npy", True)


def _fake_edit_align(hyp, ref, hyp_len=None, ref_len=None, R=1, stop_id=-1, skip=(0, 0), workspace=None):
    """``ops.edit_align`` by the reference, on host tensors."""
    t = lambda x: None if x is None else x.numpy()
    out, steps, ns = A.reference(hyp.numpy(), ref.numpy(), t(hyp_len), t(ref_len), R, stop_id, skip)
    st = np.full((hyp.shape[0], hyp.shape[1] + ref.shape[1], 3), 0x5A5A5A5A, np.int32)
    for i, s in enumerate(steps):
        st[i, :len(s)] = np.asarray(s, np.int32).reshape(-1, 3)
    return torch.from_numpy(out), torch.from_numpy(st), torch.from_numpy(ns)


def test_word_error_rate_alignment_on_hand_written_sentences(monkeypatch):
    _, ops, _, _, W = _pkg()
    calls = []
    monkeypatch.setattr(ops, "edit_align", lambda *a, **k: (calls.append(1), _fake_edit_align(*a, **k))[1])
    monkeypatch.setattr(ops, "edit_distance", lambda *a, **k: pytest.fail("the alignment call replaces the distance call"))
    hyp = ["the cat sat on mat", "hello  world", "", "a b c d"]
    ref = ["the cat sat on the mat", "hello\tworld", "one two", "a x c"]
    r = W.word_error_rate(hyp, ref, device="cpu", return_alignment=True)
    assert len(calls) == 1
    assert (r["n_edits"], r["n_sub"], r["n_del"], r["n_ins"]) == (5.0, 1.0, 3.0, 1.0)
    M, S, D, I = 0, 1, 2, 3
    assert ops.EDIT_OPS == ("match", "substitution", "deletion", "insertion")
    assert r["alignment"] == [
        [(M, "the", "the"), (M, "cat", "cat"), (M, "sat", "sat"), (M, "on", "on"), (D, None, "the"), (M, "mat", "mat")],
        [(M, "hello", "hello"), (M, "world", "world")],
        [(D, None, "one"), (D, None, "two")],
        [(M, "a", "a"), (S, "b", "x"), (M, "c", "c"), (I, "d", None)]]


def test_alignment_items_and_the_json_line():
    _, ops, T, _, W = _pkg()
    hyp = torch.tensor([[7, 8, 9, 4], [7, 9, 0, 0], [1, 2, 3, 4]], dtype=torch.int32)
    ref = torch.tensor([[7, 9, 4, 5]], dtype=torch.int32)
    out, steps, ns = _fake_edit_align(hyp, ref, torch.tensor([4, 2, 4], dtype=torch.int32), None, R=3)
    items = ops.edit_alignment_items(steps, ns, hyp, ref, R=3)  # the first of the R rows
    assert items == [[(0, 7, 7, 0, 0), (3, 8, None, 1, None), (0, 9, 9, 2, 1), (0, 4, 4, 3, 2), (2, None, 5, None, 3)]]
    assert len(ops.edit_alignment_items(steps, ns, hyp, ref.repeat(3, 1), R=1)) == 3
    al = {"steps": [(op, h, r) for op, h, r, _, _ in items[0]], "hyp_positions": [3, 4, 5, 6, None], "ref_positions": [0, None, 1, 2, 3]}
    line = W.alignment_record(4, al)
    assert "\n" not in line
    assert json.loads(line) == {"item": 4, "n_steps": 5, "n_errors": 2,
                                "steps": [["match", 7, 7, 3, 0], ["insertion", 8, None, 4, None], ["match", 9, 9, 5, 1],
                                          ["match", 4, 4, 6, 2], ["deletion", None, 5, None, 3]]}

    class Stub:
        device = torch.device("cpu")
        seen = []

        def evaluate_generate(self, features, labels, **kw):
            self.seen.append(kw)
            b = float(features.shape[0])
            r = ops.finish_edit_counts({"n_edits": b, "n_sub": b, "n_del": 0.0, "n_ins": 0.0, "n_ref_tokens": 4 * b, "n_hyp_tokens": 4 * b,
                                        "n_exact": 0.0, "n_items": b, "n_oracle_edits": b})
            if kw.get("return_alignment"):
                r["alignment"] = [al] * int(b)
            return r

    batches = [(torch.zeros(2, 4, 8), torch.zeros(2, 5, dtype=torch.int32)), (torch.zeros(3, 4, 8), torch.zeros(3, 5, dtype=torch.int32))]
    sink, model = [], Stub()
    T.evaluate_generate_whisper(None, model, batches, alignments=sink, num_beams=2)
    assert model.seen == [{"num_beams": 2, "return_alignment": True}] * 2 and sink == [al] * 5
    model.seen.clear()
    T.evaluate_generate_whisper(None, model, batches, num_beams=2)
    assert model.seen == [{"num_beams": 2}] * 2  # without a sink the call is the one it was
