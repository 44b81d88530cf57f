"""TEST INFRASTRUCTURE: the SpecAugment span masks of include/tethys_mi.h ("SpecAugment span masks on the probes' cached
features") restated in numpy, on the generator of oracle/dropout.py (imported, not copied).  CPU only: nothing here imports
the GPU package, so tests/test_spec_augment_cpu.py checks the restatement itself - against a literal transcription of the
reference's pad-shift-OR loop, on planted starts, and on the start rate - before the GPU tests compare the kernels with it
bit for bit."""
import numpy as np

from oracle.dropout import drop_thr, keep_rows, stream_key

SITE_SPEC = 7
STREAM_TIME, STREAM_FEAT = 1, 2
MAX_LENGTH = 64


def site_seed(seed, step):
    """site = (seed + step * 0x9E3779B97F4A7C15 + SITE_SPEC * 0xD1B54A32D192ED03) mod 2^64."""
    return (int(seed) + int(step) * 0x9E3779B97F4A7C15 + SITE_SPEC * 0xD1B54A32D192ED03) % (1 << 64)


def starts(site, stream, N, cols, prob):
    """start(n, c) = !tmi_keep(tmi_stream_key(site, stream), row = n, col = c, thr) -> bool [N, cols]; prob == 0: none."""
    thr = drop_thr(prob)
    if thr == 0:
        return np.zeros((N, cols), dtype=bool)
    return ~keep_rows(stream_key(site, stream), N, cols, thr)


def spans(start, length):
    """mask(n, c) = OR over i = 0 .. length - 1 of start(n, c - i), start false for c - i < 0."""
    start = np.asarray(start, dtype=bool)
    mask = np.zeros_like(start)
    cols = start.shape[1]
    for c in range(cols):
        lo = max(0, c - (length - 1))
        mask[:, c] = start[:, lo:c + 1].any(axis=1)
    return mask


def spans_literal(start, length):
    """V:1083-1086 transcribed: for i in range(mask_length): shifted = pad(mask[:, :cols - i], [[0, 0], [i, 0]], False);
    expanded |= shifted.  (For i >= cols the reference's slice `:cols - i` would wrap around; the transcription stops there,
    as no start can reach a column from that far.)"""
    start = np.asarray(start, dtype=bool)
    cols = start.shape[1]
    expanded = np.zeros_like(start)
    for i in range(length):
        if i >= cols:
            break
        shifted = np.pad(start[:, :cols - i], [[0, 0], [i, 0]], constant_values=False)
        expanded = np.logical_or(expanded, shifted)
    return expanded


def time_mask(site, N, T_max, prob, length):
    return spans(starts(site, STREAM_TIME, N, T_max, prob), length)


def feature_mask(site, N, H, prob, length):
    return spans(starts(site, STREAM_FEAT, N, H, prob), length)


def words(cols):
    return (cols + 31) // 32


def pack_bits(mask, ld=None):
    """bool [N, cols] -> uint32 [N, ld]: column c is bit c % 32 of word c / 32; the bits past cols and the words past
    ceil(cols / 32) are 0."""
    mask = np.asarray(mask, dtype=bool)
    N, cols = mask.shape
    ld = words(cols) if ld is None else ld
    out = np.zeros((N, ld), dtype=np.uint32)
    for c in range(cols):
        out[:, c // 32] |= mask[:, c].astype(np.uint32) << np.uint32(c % 32)
    return out


def unpack_bits(bits, cols):
    bits = np.asarray(bits).view(np.uint32) if np.asarray(bits).dtype == np.int32 else np.asarray(bits, dtype=np.uint32)
    c = np.arange(cols)
    return ((bits[:, c // 32] >> (c % 32).astype(np.uint32)) & 1).astype(bool)


def apply_masks(x, tmask=None, fmask=None):
    """x [N, T, H] with the masked elements set to +0 (a copy)."""
    y = np.array(x, copy=True)
    if tmask is not None:
        y[np.asarray(tmask, dtype=bool)] = 0
    if fmask is not None:
        y[np.broadcast_to(np.asarray(fmask, dtype=bool)[:, None, :], y.shape)] = 0
    return y
