"""numpy restatement of the selection contract of include/actinon_hip.h (acn_select_above*, acn_key_histogram*, acn_key_hist_edge,
acn_key_hist_threshold): what the device and the host header (actinon_amd/csrc/acn_select_host.h) are compared with, bit for bit."""
import numpy as np

BINS, WORDS = 256, 257
LO = (1023 - 40) * 4
POISON_INDEX = np.int64(-0x5A5A5A5A5A5A5A5B)
POISON_DOUBLE = np.array([0x7FF4DEADBEEF0001], dtype=np.uint64).view(np.float64)[0]   # a NaN with a payload: compared as bits


def select(key, threshold):
    """the selected indices, ascending, int64: key[ i ] > threshold as an IEEE comparison"""
    with np.errstate(invalid="ignore"):
        return np.flatnonzero(np.asarray(key, dtype=np.float64) > threshold).astype(np.int64)


def raster_positions(idx, width, first=0):
    """pixel centres [m,2] float64 of the pixels first + idx of a raster `width` wide"""
    p = np.asarray(idx, dtype=np.uint64) + np.uint64(first)
    w = np.uint64(width)
    return np.stack([(p % w).astype(np.float64) + 0.5, (p // w).astype(np.float64) + 0.5], axis=1)


def select_above(key, threshold, capacity, src_pos=None, width=None, first=0):
    """-> ( index [m], pos [m,2], count ), m = min( count, capacity )"""
    idx = select(key, threshold)
    count = len(idx)
    idx = idx[:min(count, capacity)]
    pos = np.asarray(src_pos, dtype=np.float64).reshape(-1, 2)[idx] if src_pos is not None else raster_positions(idx, width, first)
    return idx, pos, count


def key_bin(key):
    """the histogram word of every key, from its raw bits"""
    u = np.ascontiguousarray(key, dtype=np.float64).reshape(-1).view(np.uint64)
    nan = (u & np.uint64(0x7FFFFFFFFFFFFFFF)) > np.uint64(0x7FF0000000000000)
    neg = (u >> np.uint64(63)) != 0
    e = (u >> np.uint64(50)).astype(np.int64)
    b = np.where(e < LO, 0, np.minimum(e - LO + 1, 255))
    b[neg] = 0
    b[nan] = 256
    return b.astype(np.int64)


def histogram(key):
    return np.bincount(key_bin(key), minlength=WORDS).astype(np.uint64)


def edge_bits(j):
    if j == 0:
        return 0xFFF0000000000000
    if j > 255:
        return 0x7FF8000000000000
    return (LO + j - 1) << 50


def edge(j):
    return np.array([edge_bits(j)], dtype=np.uint64).view(np.float64)[0]


def threshold(hist, budget):
    """edge( j ) of the smallest j >= 1 with hist[ j ] + ... + hist[ 255 ] <= budget, +inf if there is none (Python integers: no overflow)"""
    hh = [int(v) for v in hist]
    for j in range(1, 256):
        if sum(hh[j:256]) <= budget:
            return edge(j)
    return np.inf
