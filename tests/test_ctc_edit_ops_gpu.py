"""``Wav2Vec2ForCTC.evaluate(edit_ops=True)`` on the GPU: the tiny CTC configuration and the padded batch of
tests/test_ctc_gpu.py.  The device-side counts equal the host path's and the reference of tests/_edit_ref.py on the returned
sequences; the n-best oracle equals the host minimum over ``decode(num_beams=4, num_return_sequences=4)``.  Integers:
every comparison is an equality."""
import numpy as np
import pytest
import torch

import _edit_ref as E
from oracle import wav2vec2_oracle as V

pytestmark = pytest.mark.gpu

T_IN = 800
TINY = dict(hidden_size=64, num_hidden_layers=2, num_attention_heads=1, intermediate_size=128, conv_dim=(64, 64, 64),
            conv_stride=(5, 2, 2), conv_kernel=(10, 3, 2), num_conv_pos_embeddings=8, num_conv_pos_embedding_groups=4,
            num_codevectors_per_group=16, codevector_dim=32, proj_codevector_dim=64, num_negatives=10)
OLD_KEYS = {"nll_sum", "n_items", "n_infeasible", "loss", "n_edits", "n_ref_tokens", "token_error_rate"}
OPS_KEYS = {"n_sub", "n_del", "n_ins", "n_hyp_tokens"}


@pytest.fixture(scope="module")
def setup(dev):
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import wav2vec2 as W
    m = W.create_full_model("asr", "base", device=dev, precision="bf16", seed=7, **TINY)
    g = torch.Generator().manual_seed(3)
    m.arena.param("lm_head.kernel").mul_(12.0)  # (as tests/test_ctc_gpu.py: the argmax moves between symbols)
    m.arena.param("lm_head.bias").copy_((torch.randn(m.config.vocab_size, generator=g) * 0.3).to(dev))
    m.refresh_shadows()
    mask = W.frame_attention_mask(m.config, (T_IN, 33 * 20, 17 * 20, T_IN), T_IN)
    x = torch.from_numpy(V.create_dummy_pool(seed=8, num_samples=4, length=T_IN)).to(dev)
    # item 0 against its own greedy transcript with two tokens changed, 1 and 2 against random labels, 3 has no labels
    d = m.decode(x, attention_mask=mask)
    own = d["sequences"][0, :int(d["lengths"][0])].cpu().numpy()
    rng = np.random.default_rng(1)
    blank, Vn = m.config.ctc_blank_id, m.config.vocab_size
    L = max(len(own), 12)
    labels = np.zeros((4, L), np.int64)
    lens = [len(own), 9, 12, 0]
    labels[0, :len(own)] = own
    for b in (1, 2):
        labels[b, :lens[b]] = [v for v in rng.permutation(Vn) if v != blank][:lens[b]]
    assert len(own) >= 3
    for k in (0, len(own) - 1):
        labels[0, k] = next(v for v in range(Vn) if v != blank and v != own[k])
    yield m, x, mask, torch.from_numpy(labels), lens
    del m
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _ref_counts(seqs, seq_lens, labels, lens, R=1, valid=None):
    out = E.reference(np.asarray(seqs).reshape(-1, np.asarray(seqs).shape[-1]), labels.numpy(), np.asarray(seq_lens).reshape(-1),
                      np.asarray(lens), R=R)
    return out, E.counts(out, R, valid)


def test_greedy_counts(setup):
    m, x, mask, labels, lens = setup
    old = m.evaluate(x, labels, lens, attention_mask=mask)
    assert set(old) == OLD_KEYS  # without the argument: exactly the keys it had
    new = m.evaluate(x, labels, lens, attention_mask=mask, edit_ops=True, return_items=True)
    assert {k for k, v in new.items() if not torch.is_tensor(v)} == OLD_KEYS | OPS_KEYS
    assert all(new[k] == old[k] for k in OLD_KEYS) and old["n_edits"] >= 2.0
    _, ref = _ref_counts(new["sequences"].cpu().numpy(), new["lengths"].cpu().numpy(), labels, lens)
    for k in ("n_edits", "n_sub", "n_del", "n_ins", "n_hyp_tokens", "n_ref_tokens", "token_error_rate"):
        assert new[k] == ref[k] and isinstance(new[k], float), k
    assert new["n_sub"] + new["n_del"] + new["n_ins"] == new["n_edits"] and new["n_sub"] >= 2.0
    assert set(m.evaluate(x, labels, lens, attention_mask=mask, return_items=True)) == OLD_KEYS | {"nll", "infeasible", "sequences", "lengths"}


def test_beam_counts_and_the_n_best_oracle(setup):
    m, x, mask, labels, lens = setup
    old = m.evaluate(x, labels, lens, attention_mask=mask, num_beams=4)
    assert set(old) == OLD_KEYS
    new = m.evaluate(x, labels, lens, attention_mask=mask, num_beams=4, edit_ops=True, return_items=True)
    assert {k for k, v in new.items() if not torch.is_tensor(v)} == OLD_KEYS | OPS_KEYS | {"n_oracle_edits", "oracle_error_rate"}
    assert all(new[k] == old[k] for k in OLD_KEYS)
    _, best = _ref_counts(new["beam_sequences"].cpu().numpy(), new["beam_lengths"].cpu().numpy(), labels, lens)
    for k in ("n_edits", "n_sub", "n_del", "n_ins", "n_hyp_tokens", "n_ref_tokens"):
        assert new[k] == best[k], k
    d = m.decode(x, attention_mask=mask, num_beams=4, num_return_sequences=4)
    nb = d["n_beams"].cpu().numpy()
    assert nb.min() >= 1 and nb.max() > 1
    valid = np.arange(4)[None, :] < nb[:, None]
    table, ref = _ref_counts(d["sequences"].cpu().numpy(), d["lengths"].cpu().numpy(), labels, lens, R=4, valid=valid)
    host_min = sum(min(int(table[4 * b + k, 0]) for k in range(int(nb[b]))) for b in range(4))
    assert new["n_oracle_edits"] == float(host_min) == ref["n_oracle_edits"]
    assert new["oracle_error_rate"] == host_min / new["n_ref_tokens"] and new["n_oracle_edits"] <= new["n_edits"]
