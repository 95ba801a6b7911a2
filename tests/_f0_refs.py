"""The contract of vx_f0 (include/vallex_hip.h) restated in numpy: YIN with every sum, prefix, tie and rounding as the header words it.
The device (tests/test_gpu_f0.py) and the host code (tests/test_f0_host.py) are compared with this word for word;
tests/test_f0_refs.py holds it to a sequential Python loop and to its own properties.  Not a fast implementation: a checker.

Also here: the exact fp32 fma chain of the resampler (one lane, K fmaf from a zero accumulator in tap order, csrc/resample.hip) on the
taps of tests/_resample_refs.py, so that a pitch shift -- tests/_stretch_refs.py, then that resampler -- has a restatement too."""
import math
from fractions import Fraction

import numpy as np

from tests import _resample_refs as RR
from tests import _stretch_refs as SR

# (rate, hop, window, lag_min, lag_max, threshold): the two small option sets of the GPU tests and the largest options
SMALL = (8000, 40, 100, 8, 67, 0.15)
TINY = (8000, 16, 16, 2, 3, 0.5)
LARGEST = (48000, 4096, 2048, 2, 1024, 0.15)


def frames(L, H):
    return -(-int(L) // int(H))


def first(k, H, W, T):
    """s_k: Python integers floor-divide like C's for the non-negative operands here"""
    return int(k) * int(H) + int(H) // 2 - (int(W) + int(T)) // 2


def clean(x):
    x = np.asarray(x, np.float32).reshape(-1)
    return np.where(np.isfinite(x), x, np.float32(0.0)).astype(np.float32)


def nonfinite(x):
    return int((~np.isfinite(np.asarray(x, np.float32))).sum())


def take(y, start, count):
    """y[start .. start + count) as doubles, 0 outside [0, L)"""
    out = np.zeros(count, np.float64)
    lo, hi = max(start, 0), min(start + count, len(y))
    if hi > lo:
        out[lo - start: hi - start] = y[lo:hi]
    return out


def difference(seg, W, T):
    """d(t), t = 0 .. T, of one frame: seg = y[s_k .. s_k + W + T) as float64.  Row t of the window view is y[j + t]; np.cumsum adds in
    index order from the first element, one double addition per sample -- the sum `0.0 + e_0^2 + e_1^2 + ...` of the contract"""
    win = np.lib.stride_tricks.sliding_window_view(seg, W)[: T + 1]
    e = seg[None, :W] - win
    return np.cumsum(e * e, axis=1)[:, -1]


def normalise(d):
    """d'(t): c(t) = np.cumsum over d(1) .. d(t) (sequential), d'(0) = 1, d'(t) = c > 0 ? (d t) / c : 1"""
    T = len(d) - 1
    c = np.cumsum(d[1:])
    dp = np.ones(T + 1, np.float64)
    t = np.arange(1, T + 1, dtype=np.float64)
    pos = c > 0.0
    dp[1:][pos] = (d[1:][pos] * t[pos]) / c[pos]
    return dp


def pick(dp, lag_min, lag_max, thr):
    """(t, voiced)"""
    thr = float(np.float32(thr))
    under = np.flatnonzero(dp[lag_min: lag_max + 1] < thr)
    if len(under):
        t = lag_min + int(under[0])
        while t + 1 <= lag_max and dp[t + 1] < dp[t]:
            t += 1
        return t, True
    return lag_min + int(np.argmin(dp[lag_min: lag_max + 1])), False       # np.argmin: the first of equal minima


def refine(dp, t, lag_max):
    """off of the parabola through d'(t - 1), d'(t), d'(t + 1), 0 where it does not apply"""
    if t + 1 > lag_max:
        return 0.0
    a, b, c = dp[t - 1], dp[t], dp[t + 1]
    den = (a - 2.0 * b) + c
    if b <= a and b <= c and den > 0.0:
        return float((0.5 * (a - c)) / den)
    return 0.0


def f0(x, opts, tables=False):
    """(f0 float32 [M], lag int32 [M], ap float32 [M], info dict) of one row; tables: also d and d' [M][lag_max + 1] float64"""
    rate, H, W, t0, T, thr = opts
    x = np.asarray(x, np.float32).reshape(-1)
    y = clean(x).astype(np.float64)
    M = frames(len(x), H)
    f, lag, ap = np.zeros(M, np.float32), np.zeros(M, np.int32), np.zeros(M, np.float32)
    dt, dpt = np.zeros((M, T + 1), np.float64), np.zeros((M, T + 1), np.float64)
    for k in range(M):
        d = difference(take(y, first(k, H, W, T), W + T), W, T)
        dp = normalise(d)
        t, voiced = pick(dp, t0, T, thr)
        off = refine(dp, t, T)
        f[k] = np.float32(np.float64(rate) / (np.float64(t) + np.float64(off)))
        lag[k] = t if voiced else -t
        ap[k] = np.float32(dp[t])
        dt[k], dpt[k] = d, dp
    info = summary(f, lag, nonfinite(x))
    return (f, lag, ap, info, dt, dpt) if tables else (f, lag, ap, info)


def summary(f, lag, nonf):
    v = np.sort(f[lag > 0])
    out = dict(frames=len(f), voiced_frames=len(v), nonfinite=int(nonf), f0_median=0.0, f0_min=0.0, f0_max=0.0)
    if len(v):
        out.update(f0_median=float(v[(len(v) - 1) // 2]), f0_min=float(v[0]), f0_max=float(v[-1]))
    return out


def tone(freq, rate, L, harmonics=5, phase=0.3):
    """a harmonic tone: partial h at amplitude 0.5 / h"""
    n = np.arange(int(L), dtype=np.float64)
    x = sum((0.5 / h) * np.sin(2 * np.pi * h * freq * n / rate + phase * h) for h in range(1, harmonics + 1))
    return x.astype(np.float32)


def noise(L, seed):
    return (0.3 * np.random.default_rng(seed).standard_normal(int(L))).astype(np.float32)


def hot_row(L, seed=5):
    """noise plus a tone with a NaN, both infinities, -0.0 and denormals"""
    x = (noise(L, seed) + tone(310.0, 8000, L)).astype(np.float32)
    for i, v in ((3, np.nan), (L // 3, np.inf), (L // 2, -np.inf), (L // 2 + 9, np.float32(-0.0)), (L - 5, np.float32(1e-41)),
                 (L - 4, np.float32(-3e-45))):
        x[i] = v
    return x


def huge_row(L, seed=6):
    """samples at +-3e38: differences reach 6e38, their squares 3.6e77 -- nothing overflows in double"""
    s = np.random.default_rng(seed).integers(0, 2, int(L)) * 2 - 1
    return (s * 3.0e38).astype(np.float32)


def rows(H, seed=0):
    """lengths 0, 1, H-1, H, H+1 and 12 H + 3: noise under a harmonic tone that drifts a little from row to row"""
    out = []
    for i, L in enumerate((0, 1, H - 1, H, H + 1, 12 * H + 3)):
        out.append((tone(230.0 + 17.0 * i, 8000, L) + 0.1 * noise(L, seed + i)).astype(np.float32))
    return out


def cents(f, ref):
    return 1200.0 * np.log2(np.asarray(f, np.float64) / ref)


def interior(M, H, W, T, L):
    """the frames whose window reaches no zero padding: s_k >= 0 and s_k + W + T <= L"""
    return [k for k in range(M) if first(k, H, W, T) >= 0 and first(k, H, W, T) + W + T <= L]


# ---- the pitch shift: stretch (tests/_stretch_refs.py), then the resampler's fma chain on the taps of tests/_resample_refs.py ----
def fma32(a, b, c):
    """fmaf(a, b, c) of float32 arrays, exactly: the product of two fp32 values is exact in double; TwoSum gives the error of the double
    addition; the double sum rounds to fp32 as the exact sum does unless it sits on a tie of the fp32 grid with a non-zero error,
    and then the error's sign decides"""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    r = s.astype(np.float32)
    dlt = s - r.astype(np.float64)                                    # exact
    up = np.nextafter(r, np.float32(np.inf)).astype(np.float64) - r.astype(np.float64)
    dn = r.astype(np.float64) - np.nextafter(r, np.float32(-np.inf)).astype(np.float64)
    go_up = (dlt > 0) & (dlt == 0.5 * up) & (err > 0)
    go_dn = (dlt < 0) & (-dlt == 0.5 * dn) & (err < 0)
    r = np.where(go_up, np.nextafter(r, np.float32(np.inf)), r)
    r = np.where(go_dn, np.nextafter(r, np.float32(-np.inf)), r)
    return r.astype(np.float32)


def resample_bits(x, orig, new, taps=None):
    """vx_resample of one fp32 row, word for word: every output is one lane's K fmaf from +0.0 in tap order j = 0 .. K-1.  taps: the
    (n, K) fp32 table to use -- the device's own (Engine.dev_resample_taps: its libm may differ from torch's by an ulp, as
    tests/test_gpu_resample.py records); None: the torch formula of tests/_resample_refs.py"""
    x = np.asarray(x, np.float32).reshape(-1)
    o, n, width, K = RR.geometry(orig, new)
    if o == n:
        return x.copy()
    tp = RR.taps(orig, new) if taps is None else np.asarray(taps, np.float32)      # (n, K)
    assert tp.shape == (n, K)
    L = len(x)
    T = RR.out_len(orig, new, L)
    nblk = -(-T // n)
    xpad = np.zeros(max(L + 2 * width + o, (nblk - 1) * o + K) if nblk else K, np.float32)
    xpad[width: width + L] = x
    if nblk == 0:
        return np.zeros(0, np.float32)
    win = np.lib.stride_tricks.sliding_window_view(xpad, K)[: (nblk - 1) * o + 1: o]      # (nblk, K)
    acc = np.zeros((nblk, n), np.float32)
    for j in range(K):
        acc = fma32(tp[None, :, j], win[:, None, j], acc)
    return acc.reshape(-1)[:T]


def pitch_ratio(pitch):
    """the restatement of Engine.pitch_ratio for a float in semitones"""
    return Fraction(2.0 ** (float(pitch) / 12.0)).limit_denominator(256)


def shift(x, p, q, speed=(1, 1), H=240, D=150, taps=None):
    """Engine.shift of one row: stretch at speed q / p (hop 240, search 150: the defaults at 24 kHz), resample p -> q, cut"""
    x = np.asarray(x, np.float32).reshape(-1)
    sp = Fraction(int(speed[0]), int(speed[1]))
    comb = sp * Fraction(int(q), int(p))
    y = SR.stretch(x, comb.numerator, comb.denominator, H, D)[0]
    z = resample_bits(y, p, q, taps)
    return z[: -(-len(x) * sp.denominator // sp.numerator)]
