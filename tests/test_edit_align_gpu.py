"""The callers of tmi_edit_align and tmi_edit_confusion on the GPU, tiny configurations (those of
tests/test_evaluate_generate_gpu.py and tests/test_ctc_edit_ops_gpu.py): ``evaluate_generate(return_alignment=True)``,
``word_error_rate(return_alignment=True)`` and ``Wav2Vec2ForCTC.evaluate(edit_ops=True, confusion=True)`` against the
reference of tests/_edit_align_ref.py applied on the host to the sequences and labels of that same call.  Integers
throughout: every comparison is an equality."""
import numpy as np
import pytest
import torch

import _edit_align_ref as A
from oracle import wav2vec2_oracle as V

pytestmark = pytest.mark.gpu

_TINY = dict(d_model=128, encoder_attention_heads=2, decoder_attention_heads=2, d_ff=256, vocab_size=160, encoder_layers=2,
             decoder_layers=2, n_mels=16, n_ctx=32, decoder_start_token_id=150, max_target_positions=32)
B, T_IN, S, EOS = 3, 48, 9, 2
MODES = (("greedy", dict()), ("beam-prompt", dict(num_beams=2, num_return_sequences=2, prompt_ids=[11, 22, 33])))
COUNT_KEYS = ("n_edits", "n_sub", "n_del", "n_ins", "n_ref_tokens", "n_hyp_tokens", "n_exact", "n_items", "n_oracle_edits",
              "token_error_rate", "oracle_error_rate")


@pytest.fixture(scope="module")
def whisper_setup(dev):
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import whisper
    model = whisper.create_whisper_model("small", device=dev, precision="bf16", seed=11, **_TINY)
    rng = np.random.default_rng(4)
    feats = torch.from_numpy(rng.standard_normal((B, 16, T_IN)).astype(np.float32)).to(dev)
    labels = rng.integers(3, 140, (B, S)).astype(np.int32)
    labels[0, 6] = EOS  # cut before it
    lens = np.asarray([S, 7, 4], np.int32)
    # item 1's labels: what the model generates for it, one token dropped and one changed - matches, not only substitutions
    own = model.generate(feats, max_length=8, eos_token_id=-1)[1, 1:].cpu().numpy()
    labels[1, :7] = np.concatenate([own[:2], own[3:]])[:7]
    labels[1, 4] = (labels[1, 4] + 1) % 100 + 3
    yield model, feats, labels, lens
    del model
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name,mode", MODES, ids=[m[0] for m in MODES])
def test_evaluate_generate_alignment_equals_the_reference_on_the_same_sequences(whisper_setup, name, mode):
    model, feats, labels, lens = whisper_setup
    P = len(mode.get("prompt_ids", ()))
    R = mode.get("num_return_sequences", 1)
    for eos, ll in ((EOS, lens), (-1, None)):
        kw = dict(max_length=8, eos_token_id=eos, **mode)
        args = (feats, torch.from_numpy(labels), None if ll is None else torch.from_numpy(ll))
        res = model.evaluate_generate(*args, return_items=True, return_alignment=True, **kw)
        plain = model.evaluate_generate(*args, **kw)
        assert "alignment" not in plain and {k: res[k] for k in COUNT_KEYS} == plain  # the counts do not change
        seq = res["sequences"].cpu().numpy()
        assert seq.shape[0] == B * R
        hl = None if res["lengths"] is None else res["lengths"].cpu().numpy() - P
        out, steps, ns = A.reference(seq[:, 1 + P:], labels, hl, ll, R=R, stop_id=eos)
        assert np.array_equal(res["edits"].cpu().numpy(), out) and np.array_equal(res["n_steps"].cpu().numpy(), ns)
        got = res["steps"].cpu().numpy()
        assert all([tuple(t) for t in got[i, :ns[i]].tolist()] == steps[i] for i in range(B * R))
        assert len(res["alignment"]) == B
        for b, al in enumerate(res["alignment"]):  # the item's FIRST sequence
            row, want = seq[b * R], steps[b * R]
            assert al["steps"] == [(op, None if a < 0 else int(row[1 + P + a]), None if c < 0 else int(labels[b, c])) for op, a, c in want]
            assert al["hyp_positions"] == [None if a < 0 else a + 1 + P for _, a, _ in want]
            assert al["ref_positions"] == [None if c < 0 else c for _, _, c in want]
            for (op, h, r), hp, rp in zip(al["steps"], al["hyp_positions"], al["ref_positions"]):  # the positions index the tokens
                assert (h is None) == (hp is None) == (op == A.DEL) and (r is None) == (rp is None) == (op == A.INS)
                assert (hp is None or row[hp] == h) and (rp is None or labels[b, rp] == r)
                assert op in (A.DEL, A.INS) or (h == r) == (op == A.MATCH)
            assert A.check_path(row[1 + P:], labels[b], want, out[b * R], h_len=None if hl is None else hl[b * R],
                                r_len=None if ll is None else ll[b], stop_id=eos) == ""
        if eos == -1 and name == "greedy":  # item 1's labels were cut from this very transcript
            assert any(op == A.MATCH for op, _, _ in res["alignment"][1]["steps"])
    with pytest.raises(TypeError):
        model.evaluate_generate(feats, torch.from_numpy(labels), return_alignment="items.jsonl")


def test_word_error_rate_alignment_with_known_answers(dev):
    from tethys_speech_amd import whisper
    hyp = ["the cat sat on mat", "hello  world", "", "a b c d", "one two three four five", "x"]
    ref = ["the cat sat on the mat", "hello\tworld", "one two", "a x c", "one three four six five", "x"]
    r = whisper.word_error_rate(hyp, ref, device=dev, return_alignment=True)
    plain = whisper.word_error_rate(hyp, ref, device=dev)
    assert {k: v for k, v in r.items() if k != "alignment"} == plain and "alignment" not in plain
    assert (r["n_edits"], r["n_sub"], r["n_del"], r["n_ins"], r["n_exact"]) == (7.0, 1.0, 4.0, 2.0, 2.0)
    M, SB, D, I = A.MATCH, A.SUB, A.DEL, A.INS
    assert r["alignment"] == [
        [(M, "the", "the"), (M, "cat", "cat"), (M, "sat", "sat"), (M, "on", "on"), (D, None, "the"), (M, "mat", "mat")],
        [(M, "hello", "hello"), (M, "world", "world")],
        [(D, None, "one"), (D, None, "two")],
        [(M, "a", "a"), (SB, "b", "x"), (M, "c", "c"), (I, "d", None)],
        [(M, "one", "one"), (I, "two", None), (M, "three", "three"), (M, "four", "four"), (D, None, "six"), (M, "five", "five")],
        [(M, "x", "x")]]


# ------------------------------------------------------------------------------------------------- Wav2Vec2ForCTC.evaluate
T_CTC = 800
TINY_CTC = dict(hidden_size=64, num_hidden_layers=2, num_attention_heads=1, intermediate_size=128, conv_dim=(64, 64, 64),
                conv_stride=(5, 2, 2), conv_kernel=(10, 3, 2), num_conv_pos_embeddings=8, num_conv_pos_embedding_groups=4,
                num_codevectors_per_group=16, codevector_dim=32, proj_codevector_dim=64, num_negatives=10)


@pytest.fixture(scope="module")
def ctc_setup(dev):
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import wav2vec2 as W
    m = W.create_full_model("asr", "base", device=dev, precision="bf16", seed=7, **TINY_CTC)
    g = torch.Generator().manual_seed(3)
    m.arena.param("lm_head.kernel").mul_(12.0)  # (as tests/test_ctc_gpu.py: the argmax moves between symbols)
    m.arena.param("lm_head.bias").copy_((torch.randn(m.config.vocab_size, generator=g) * 0.3).to(dev))
    m.refresh_shadows()
    mask = W.frame_attention_mask(m.config, (T_CTC, 33 * 20, 17 * 20, T_CTC), T_CTC)
    x = torch.from_numpy(V.create_dummy_pool(seed=8, num_samples=4, length=T_CTC)).to(dev)
    d = m.decode(x, attention_mask=mask)
    own = d["sequences"][0, :int(d["lengths"][0])].cpu().numpy()
    rng = np.random.default_rng(1)
    blank, Vn = m.config.ctc_blank_id, m.config.vocab_size
    L = max(len(own), 12)
    labels = np.zeros((4, L), np.int64)
    lens = [len(own), 9, 12, 0]
    labels[0, :len(own)] = own  # item 0: its own transcript with two tokens changed; 1 and 2: random labels; 3: none
    for b in (1, 2):
        labels[b, :lens[b]] = [v for v in rng.permutation(Vn) if v != blank][:lens[b]]
    for k in (0, len(own) - 1):
        labels[0, k] = next(v for v in range(Vn) if v != blank and v != own[k])
    yield m, x, mask, torch.from_numpy(labels), lens
    del m
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("num_beams", [None, 4])
def test_ctc_confusion_equals_the_reference_on_the_transcript(ctc_setup, num_beams):
    m, x, mask, labels, lens = ctc_setup
    Vn = m.config.vocab_size
    kw = dict(attention_mask=mask, num_beams=num_beams, edit_ops=True)
    base = m.evaluate(x, labels, lens, **kw)
    assert "confusion" not in base  # the default call: the keys it had
    res = m.evaluate(x, labels, lens, confusion=True, return_items=True, **kw)
    assert {k: v for k, v in res.items() if not torch.is_tensor(v)} == base  # every other key is unchanged
    table = res["confusion"]
    assert table.dtype == torch.int64 and tuple(table.shape) == (Vn + 1, Vn + 1) and table.device.type == "cuda"
    seqs, sl = (res["beam_sequences"], res["beam_lengths"]) if num_beams else (res["sequences"], res["lengths"])
    seqs, sl = seqs.cpu().numpy(), sl.cpu().numpy()
    out, steps, ns = A.reference(seqs, labels.numpy(), sl, np.asarray(lens))
    want = A.confusion(steps, seqs, labels.numpy(), Vn)
    assert want[-1] == 0 and np.array_equal(table.cpu().numpy().reshape(-1), want[:-1])
    got = table.cpu().numpy()
    assert got.sum() == ns.sum() and got[:Vn, Vn].sum() == res["n_del"] and got[Vn, :Vn].sum() == res["n_ins"]
    assert got[:Vn, :Vn].sum() - np.trace(got[:Vn, :Vn]) == res["n_sub"] and got[Vn, Vn] == 0
    assert np.array_equal(got[:Vn].sum(1), np.bincount(np.concatenate([labels[b, :lens[b]].numpy() for b in range(4)]), minlength=Vn))


def test_ctc_confusion_needs_edit_ops_and_leaves_the_default_call_alone(ctc_setup):
    m, x, mask, labels, lens = ctc_setup
    with pytest.raises(ValueError):
        m.evaluate(x, labels, lens, attention_mask=mask, confusion=True)
    with pytest.raises(TypeError):
        m.evaluate(x, labels, lens, attention_mask=mask, edit_ops=True, confusion="table.npy")
    old = m.evaluate(x, labels, lens, attention_mask=mask)
    assert set(old) == {"nll_sum", "n_items", "n_infeasible", "loss", "n_edits", "n_ref_tokens", "token_error_rate"}
    assert old == m.evaluate(x, labels, lens, attention_mask=mask, edit_ops=False, confusion=False)
