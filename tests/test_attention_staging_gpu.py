"""The seams of the tile staging and of the output stores in csrc/attention.hip.

The forward, dQ and dK/dV kernels walk their streamed tiles in three stretches: full tiles whose successor is full too
(staged without a test, from running pointers, one LDS-DMA statement per tile), the last full tile (general staging: the
next tile may be ragged or absent), then the masked / ragged tiles.  Every output tile (o, dq, dk, dv) goes through LDS and
leaves as whole 128-byte rows.  The shapes below put one, several or no tile into each stretch, start the running pointers
behind tile 0 (key split), and end the last owner block 1, 31, 33 and 127 rows in.

Ground truth, restatement, bounds, canaries and the models' strided call forms are those of test_attention_forms_gpu.py
(``Case``, ``gaussian``, ``compare``): float64 reference, bound = twice the restatement's own error, guard rows directly
behind the last valid row of every output.  Every case also runs twice into freshly patterned output buffers: both runs'
outputs, stats, delta and stored mask must be byte-identical."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_attention_forms_gpu import Case, gaussian  # noqa: E402

# (B, H, Tq, Tk, mask): B*H = 8 takes the XCD-aware 1-D grid wherever a pair has more than one block, B*H = 3 the plain 3-D one
SEAMS = [
    # -- two-pass kernels (Tq or Tk > 256), key walk of forward / dQ: five full key tiles, then nothing / 1 key / 63 keys
    (2, 4, 300, 320, 0), (2, 4, 300, 321, 0), (2, 4, 300, 383, 0),
    # the same on the plain grid
    (1, 3, 300, 321, 0),
    # -- query walk of dK/dV: five full query tiles, then nothing / 1 row
    (2, 4, 320, 300, 0), (2, 4, 321, 300, 0),
    # causal: the masked loop only, full next tiles from the running pointers of the general staging
    (2, 4, 300, 300, 1),
    # -- one full tile: the peeled iteration alone, followed by a ragged tile (Tk = 300) or by nothing (64)
    (2, 4, 64, 300, 0), (2, 4, 300, 64, 0),
    # -- key split (Tq <= 128, >= 8 key tiles, workspace): 4 ranges of 2 full tiles, t0 = 2, 4, 6; ranges of 3, 3, 3; 3, 3, 3, 1 ragged
    (2, 4, 100, 512, 0), (2, 4, 128, 576, 0), (2, 4, 77, 577, 0),
    # -- one-launch backward (both <= 256)
    (2, 4, 128, 128, 0), (2, 4, 129, 192, 0), (2, 4, 249, 249, 0),
    # -- row stores of the two-pass kernels: the last block of 128 owner rows ends 1, 31, 33, 127 rows in; packed QKV (q, k, v
    # and dq, dk, dv side by side in one row), so a row piece in a neighbour's columns is a wrong gradient
    (2, 4, 257, 257, 0), (2, 4, 287, 287, 0), (2, 4, 289, 289, 0), (2, 4, 383, 383, 0),
    # the same ends in the cross form (q rows of their own, k | v columns of a wider cache row)
    (2, 4, 257, 383, 0), (2, 4, 289, 287, 0),
]

OUTPUTS = ("o", "dq", "dqkv", "dkv", "stats", "delta", "drop_mask", "workspace")


def _snapshot(c):
    return {n: c.bufs[n].flat.view(c.bufs[n].it).cpu().clone() for n in OUTPUTS if n in c.bufs}


@pytest.mark.parametrize("drop", [0.0, 0.1])
@pytest.mark.parametrize("B,H,Tq,Tk,mask", SEAMS)
def test_staging_seams_and_row_stores(dev, B, H, Tq, Tk, mask, drop):
    c = Case(dev, B, H, Tq, Tk, mask, drop, gaussian(B, H, Tq, Tk, 900 + 7 * Tq + Tk), dq_scale=0.5)
    c.run_and_compare(f"staging {c.form}({B},{H},{Tq}x{Tk}) mask{mask} drop{drop}")
    if drop > 0:  # the stored bits are the generator's
        from oracle import dropout as DO
        assert (c.keep()[0] == DO.keep_attention(c.seed, B, H, Tq, Tk, drop)).all()
    first = _snapshot(c)
    for n in first:  # the second launch writes into the pattern again, not onto the first one's results
        c.bufs[n].flat.view(c.bufs[n].it).fill_(c.bufs[n].pat)
    c.fwd()
    c.bwd()
    c.assert_canaries()
    second = _snapshot(c)
    for n in first:
        if n == "workspace":  # scratch of the key split: its contents are nobody's result
            continue
        assert torch.equal(first[n], second[n]), f"{n}: two identical launches differ"
