"""References of the resampler tests (tests/test_resample_refs.py on the CPU, tests/test_gpu_resample.py on the device): the geometry
and the tap table of a rate pair by the formula of vallex_amd.utils.prompt_making.resample_sinc_hann (torchaudio's published default,
unpinned: the package is not installed), a float64 evaluation on GIVEN fp32 taps, and the error bound of K fp32 fmas.

The bound is derived, not measured: an fp32 sum of K products accumulated by K fmas in ANY order (each fma rounds once, u = 2^-24)
satisfies |y^ - y| <= ((1 + u)^K - 1) a <= (K + 1) u a for K u < 0.01, with a = sum_j |k_j| |x_j| (Higham, Accuracy and Stability of
Numerical Algorithms, section 3.1; the K + 1 leaves room for the products' own rounding in an implementation that does not fuse).
"""
import math

import numpy as np

LPW, ROLLOFF = 6, 0.99
U32 = 2.0 ** -24

# orig, new -> (o, n, width, K): the table of the issue that introduced vx_resample, every pair the tests run
PAIRS = {
    (24000, 48000): (1, 2, 7, 15), (12000, 24000): (1, 2, 7, 15), (48000, 24000): (2, 1, 13, 28), (16000, 24000): (2, 3, 7, 16),
    (24000, 16000): (3, 2, 10, 23), (24000, 8000): (3, 1, 19, 41), (8000, 24000): (1, 3, 7, 15), (32000, 24000): (4, 3, 9, 22),
    (24000, 32000): (3, 4, 7, 17), (44100, 24000): (147, 80, 12, 171), (24000, 44100): (80, 147, 7, 94),
    (22050, 24000): (147, 160, 7, 161), (24000, 22050): (160, 147, 7, 174), (11025, 24000): (147, 320, 7, 161),
    (24000, 11025): (320, 147, 14, 348),
}


def geometry(orig, new):
    g = math.gcd(int(orig), int(new))
    o, n = int(orig) // g, int(new) // g
    base = min(o, n) * ROLLOFF
    width = math.ceil(LPW * o / base)
    return o, n, width, 2 * width + o


def out_len(orig, new, L):
    o, n, _, _ = geometry(orig, new)
    return (n * int(L) + o - 1) // o


def lengths(orig, new):
    """the six input lengths of the float64 tests: one sample, around one input block, one kernel, several tiles"""
    o, _, _, K = geometry(orig, new)
    return [1, max(1, o - 1), o, o + 1, K, 1007]


_TAPS = {}


def taps(orig, new):
    """(n, K) float32: the torch formula of resample_sinc_hann, word for word (the phase term divided in fp32, the rest in fp64)"""
    import torch
    o, n, width, K = geometry(orig, new)
    if (o, n) not in _TAPS:
        base = min(o, n) * ROLLOFF
        idx = torch.arange(-width, width + o, dtype=torch.float64)[None, None] / o
        t = ((torch.arange(0, -n, -1).to(torch.float32) / n).to(torch.float64)[:, None, None] + idx) * base
        t = t.clamp_(-LPW, LPW)
        window = torch.cos(t * math.pi / LPW / 2) ** 2
        t = t * math.pi
        k = (torch.where(t == 0, torch.ones_like(t), t.sin() / t) * window * (base / o)).to(torch.float32)
        _TAPS[(o, n)] = k.reshape(n, K).numpy().copy()
        _TAPS[(o, n)].setflags(write=False)
    return _TAPS[(o, n)]


def resample_ref64(x, tp, o, n, width):
    """float64 numpy on the given fp32 taps tp (n, K): returns (y, a), y[i n + p] = sum_j tp[p][j] xpad[i o + j] and the magnitude
    sum a = sum_j |tp[p][j]| |xpad[i o + j]| per element, both cut to ceil(n L / o)"""
    x = np.asarray(x, np.float64).reshape(-1)
    tp = np.asarray(tp, np.float64)
    K = tp.shape[1]
    assert tp.shape == (n, 2 * width + o)
    L = len(x)
    T = (n * L + o - 1) // o
    nblk = (T + n - 1) // n
    xpad = np.zeros(max(L + 2 * width + o, (nblk - 1) * o + K), np.float64)
    xpad[width: width + L] = x
    win = np.lib.stride_tricks.sliding_window_view(xpad, K)[: (nblk - 1) * o + 1: o]      # (nblk, K)
    y = (win @ tp.T).reshape(-1)[:T]
    a = (np.abs(win) @ np.abs(tp).T).reshape(-1)[:T]
    return y, a


def bound(a, K):
    """|fp32 result of K fmas - exact| <= (K + 1) 2^-24 a"""
    return (K + 1) * U32 * np.asarray(a, np.float64)


def ulp_diff(a, b):
    """distance in fp32 units in the last place between two float32 arrays (sign-magnitude order; equal words give 0)"""
    def key(v):
        w = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(w < 0, -(w & 0x7FFFFFFF), w)
    return np.abs(key(a) - key(b))


def noise(L, seed):
    return np.random.default_rng(seed).standard_normal(int(L)).astype(np.float32)
