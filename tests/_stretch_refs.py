"""The contract of vx_stretch (include/vallex_hip.h) restated in numpy: WSOLA with every sum, tie and rounding as the header words
it.  The device (tests/test_gpu_stretch.py) and the host code (tests/test_stretch_host.py) are compared with this word for word;
tests/test_stretch_refs.py holds it to a sequential Python loop.  Not a fast implementation: a checker."""
import math

import numpy as np

HOPS = (16, 240, 441)
SEARCHES = (0, 5, 150, 300)
SPEEDS = ((1, 2), (2, 3), (4, 5), (5, 4), (3, 2), (2, 1), (1000, 999))


def reduce_speed(num, den):
    g = math.gcd(int(num), int(den))
    return int(num) // g, int(den) // g


def out_len(L, num, den):
    num, den = reduce_speed(num, den)
    return -(-int(L) * den // num)                       # Python integers: no width to overflow


def frames(L, num, den, H):
    return -(-out_len(L, num, den) // int(H))


def nominal(k, num, den, H):
    num, den = reduce_speed(num, den)
    return int(k) * int(H) * num // den


def fade_table(H):
    """the smoothstep crossfade table, the fade table of vx_finish: u u (3 - 2u) at u = (j + 0.5) / H in double, rounded once"""
    u = (np.arange(H, dtype=np.float64) + 0.5) / float(H)
    return (u * u * (3.0 - 2.0 * u)).astype(np.float32)


def clean(x):
    """y: the samples with every non-finite one as 0"""
    x = np.asarray(x, np.float32).reshape(-1)
    return np.where(np.isfinite(x), x, np.float32(0.0)).astype(np.float32)


class _Row:
    """y of a row as doubles, 0 outside [0, L)"""

    def __init__(self, x):
        self.y = clean(x).astype(np.float64)
        self.L = len(self.y)

    def take(self, start, count):
        out = np.zeros(count, np.float64)
        lo, hi = max(start, 0), min(start + count, self.L)
        if hi > lo:
            out[lo - start: hi - start] = self.y[lo:hi]
        return out


def frame_sums(region, t):
    """c_d and e_d of every candidate of one frame: region = y[n_k - D .. n_k + D + H) and t = the template, both float64 holding fp32
    values.  Row i of the window view is candidate d = i - D; np.cumsum adds in index order from the first element, one double
    addition per sample -- the sum `0.0 + p_0 + p_1 + ...` of the contract (0.0 + p_0 = p_0 exactly)."""
    H = len(t)
    win = np.lib.stride_tricks.sliding_window_view(region, H)
    c = np.cumsum(win * t[None, :], axis=1)[:, -1]
    e = np.cumsum(win * win, axis=1)[:, -1]
    return c, e


def pick(Dd, D):
    """index of the winner: the smallest D_d, ties to the smallest |d|, then to the negative d"""
    best = Dd.min()
    d = np.flatnonzero(Dd == best) - D
    d = d[np.abs(d) == np.abs(d).min()]
    return int(d.min()) + D


def stretch(x, num, den, H, D, shortcut=True):
    """(out float32 [Lout], pos int64 [M], cost float64 [M]) of one row.  shortcut=False runs the search at speed 1 too."""
    x = np.asarray(x, np.float32).reshape(-1)
    num, den = reduce_speed(num, den)
    L = len(x)
    Lout, M = out_len(L, num, den), frames(L, num, den, H)
    pos, cost = np.zeros(M, np.int64), np.zeros(M, np.float64)
    if num == den and shortcut:
        return x.copy(), np.arange(M, dtype=np.int64) * H, cost
    row = _Row(x)
    w = fade_table(H).astype(np.float64)
    wr = w[::-1]
    out = np.zeros(M * H, np.float32)
    for k in range(M):
        if k == 0:
            out[:H] = row.take(0, H).astype(np.float32)
            continue
        t = row.take(int(pos[k - 1]) + H, H)
        n = nominal(k, num, den, H)
        c, e = frame_sums(row.take(n - D, 2 * D + H), t)
        Dd = e - 2.0 * c
        i = pick(Dd, D)
        pos[k], cost[k] = n + i - D, Dd[i]
        out[k * H: (k + 1) * H] = (row.take(int(pos[k]), H) * w + t * wr).astype(np.float32)
    return out[:Lout], pos, cost


def rows(H):
    """the rows of the tests: lengths 0, 1, H-1, H, H+1, 3H+7, 4801, 13 001 -- a voiced-like mixture (two partials that drift, a
    little noise), so that the search has something to match and costs of neighbours differ"""
    out = []
    for i, L in enumerate((0, 1, H - 1, H, H + 1, 3 * H + 7, 4801, 13001)):
        rng = np.random.default_rng(100 + i)
        n = np.arange(L, dtype=np.float64)
        f = 110.0 + 7.0 * i
        x = 0.4 * np.sin(2 * np.pi * f * n / 24000.0 + 0.3 * np.sin(2 * np.pi * 3.0 * n / 24000.0)) + 0.2 * np.sin(2 * np.pi * 2.7 * f * n / 24000.0)
        out.append((x + 0.02 * rng.standard_normal(L)).astype(np.float32))
    return out


def hot_row():
    """4801 samples with a NaN, both infinities, -0.0 and a denormal"""
    x = rows(240)[6].copy()
    x[7], x[250], x[1003], x[1500], x[3000] = np.nan, np.inf, -np.inf, np.float32(-0.0), np.float32(1e-41)
    return x


def cases(H):
    """a thinned product for one hop: every search and every speed appears, on every length; the searches cycle along the speeds,
    and the widest search (the lane loop past 256 candidates) also meets both ends of the speed range and the speed next to 1"""
    out = [(SEARCHES[j % 4], sp) for j, sp in enumerate(SPEEDS)]
    return out + [(300, (1, 2)), (150, (2, 1)), (300, (1000, 999))]
