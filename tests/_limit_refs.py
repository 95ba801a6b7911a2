"""References of the limiter tests (tests/test_limit_refs.py and tests/test_limit_host.py on the CPU, tests/test_gpu_limit.py on the
device): a vectorised numpy restatement of the contract of vx_limit (include/vallex_hip.h), the same contract as a plain sequential
Python loop, and the rows the tests share.  Everything is defined on GIVEN taps (n, 15) float32 and a GIVEN ceiling c (float32).

Why the vectorised form equals the loop bit for bit: the detector adds exact products (two fp32 values multiply exactly in double) one
tap at a time, so an elementwise float64 `d = d + k * y` is the loop's arithmetic; the demand is one double division and a floor; hold
and smooth are integers; the gain is one double division and one rounding; the output is two float32 multiplies."""
import math

import numpy as np

from tests import _resample_refs as RS

ONE = 1 << 24
WIDTH, K = 7, 15
FLT_MAX = float(np.finfo(np.float32).max)


def taps(n):
    """(n, 15) float32, the resampler's table of the pair (1, n); (0, 15) for n = 1"""
    if n == 1:
        return np.zeros((0, K), np.float32)
    assert RS.geometry(1, n) == (1, n, WIDTH, K)
    return RS.taps(1, n)


def ceiling(ceiling_db):
    return np.float32(math.pow(10.0, float(np.float32(ceiling_db)) / 20.0))


def sanitize(x):
    x = np.asarray(x, np.float32).reshape(-1)
    fin = np.isfinite(x)
    return np.where(fin, x, np.float32(0)).astype(np.float32), int((~fin).sum())


def detector(y, tp):
    """P [L] float32 of sanitized samples y"""
    y = np.asarray(y, np.float32)
    L = len(y)
    top = np.abs(y.astype(np.float64))
    ypad = np.zeros(L + 2 * WIDTH, np.float64)
    ypad[WIDTH: WIDTH + L] = y
    for p in range(len(tp)):
        d = np.zeros(L, np.float64)
        for j in range(K):
            d = d + float(tp[p, j]) * ypad[j: j + L]
        top = np.maximum(top, np.abs(d))
    return top.astype(np.float32)


def demand(P, gs, c):
    den = np.asarray(P, np.float32).astype(np.float64) * float(np.float32(gs))
    over = den > float(c)
    r = np.ones(len(den), np.float64)
    np.divide(float(c), den, out=r, where=over)
    return np.floor(r * 16777216.0).astype(np.int64)


def hold_smooth(q, Wn):
    """s [L] int64 from the demands q [L]: the minimum over 2 Wn + 1, then the sum over 2 Wn + 1, q = 2^24 outside the row"""
    L, N = len(q), 2 * Wn + 1
    a = np.concatenate([np.full(2 * Wn, ONE, np.int64), np.asarray(q, np.int64), np.full(2 * Wn, ONE, np.int64)])
    w = 1
    while 2 * w <= N:
        a = np.minimum(a[:-w], a[w:])
        w *= 2
    m = np.minimum(a[: L + 2 * Wn], a[N - w: N - w + L + 2 * Wn])           # m of positions -Wn .. L + Wn - 1
    cs = np.concatenate([[0], np.cumsum(m)])
    return cs[N: N + L] - cs[:L]


def limit(x, gs, c, Wn, n, tp=None):
    """the whole contract of one row: dict(out, P, g, q, s, peak, min_gain, reduced, nonfinite, ceiling)"""
    tp = taps(n) if tp is None else tp
    assert len(tp) == (n if n > 1 else 0)
    y, nonfinite = sanitize(x)
    L, N = len(y), 2 * Wn + 1
    P = detector(y, tp)
    q = demand(P, gs, c)
    s = hold_smooth(q, Wn)
    g = (s.astype(np.float64) / float(N * ONE)).astype(np.float32)
    out = (y * np.float32(gs)).astype(np.float32) * g
    return dict(out=out.astype(np.float32), P=P, g=g, q=q, s=s, peak=np.float32(P.max()) if L else np.float32(0),
                min_gain=np.float32(g.min()) if L else np.float32(1), reduced=int((g < 1).sum()), nonfinite=nonfinite, ceiling=np.float32(c))


def limit_loop(x, gs, c, Wn, n, tp=None):
    """the same contract, one sample after the other over Python numbers: (out, P, g) as float32 arrays"""
    tp = taps(n) if tp is None else tp
    x = np.asarray(x, np.float32).reshape(-1)
    L, N = len(x), 2 * Wn + 1
    y = [float(v) if math.isfinite(float(v)) else 0.0 for v in x]
    gs, c = float(np.float32(gs)), float(np.float32(c))

    def Y(i):
        return y[i] if 0 <= i < L else 0.0
    P, q = [], []
    for i in range(L):
        top = abs(y[i])
        for p in range(len(tp)):
            d = 0.0
            for j in range(K):
                d = d + float(tp[p, j]) * Y(i + j - WIDTH)
            top = max(top, abs(d))
        Pi = float(np.float32(top))
        den = Pi * gs
        r = c / den if den > c else 1.0
        P.append(Pi)
        q.append(int(math.floor(r * 16777216.0)))

    def Q(k):
        return q[k] if 0 <= k < L else ONE

    def M(i):
        return min(Q(k) for k in range(i - Wn, i + Wn + 1))
    g, out = [], []
    for i in range(L):
        s = sum(M(k) for k in range(i - Wn, i + Wn + 1))
        gi = np.float32(float(s) / float(N * ONE))
        g.append(gi)
        out.append(np.float32(np.float32(np.float32(y[i]) * np.float32(gs)) * gi))
    return np.array(out, np.float32), np.array(P, np.float32), np.array(g, np.float32)


def true_peak_db(x, n=4):
    """the detector's reading of a row, dBTP"""
    y, _ = sanitize(x)
    P = detector(y, taps(n))
    return 20.0 * math.log10(float(P.max())) if len(P) and P.max() > 0 else -math.inf


def gain(loudness, target_lufs, max_gain_db):
    """the gain of vx_finish_limited: double on the host, rounded once to fp32; 1 when nothing passed the gates"""
    if loudness == -math.inf:
        return np.float32(1)
    g = math.pow(10.0, (float(np.float32(target_lufs)) - loudness) / 20.0)
    g = min(g, math.pow(10.0, float(np.float32(max_gain_db)) / 20.0))
    return np.float32(min(g, FLT_MAX))


def trapezoid(L, Wn, k0, q0):
    """s [L] of a row whose only over-ceiling demand is q0 at k0"""
    N = 2 * Wn + 1
    i = np.arange(L, dtype=np.int64)
    return N * ONE - np.maximum(0, N - np.abs(i - k0)) * (ONE - q0)


# ---- the rows the tests share ------------------------------------------------------------------------------------------------------

def noise(L, seed, amp=0.5):
    return (amp * np.random.default_rng(seed).standard_normal(int(L))).astype(np.float32)


def lengths(Wn, tile=None):
    N = 2 * Wn + 1
    ls = [0, 1, 2, Wn, N, 2 * N + 1]
    if tile:
        ls += [tile - 1, tile, tile + 1, 2 * tile + 5]
    return ls


def nonfinite_row(L=67, seed=3):
    x = noise(L, seed)
    x[5], x[L // 2], x[L - 4] = np.nan, np.inf, -np.inf
    return x


def impulse_row(L, at, amp=2.0, floor=0.05):
    """a +-floor alternation (sample peak and every interpolated reading far under any test ceiling) with samples of `amp` at `at`"""
    x = (floor * np.where(np.arange(L) % 3 == 0, 1.0, -0.5)).astype(np.float32)
    for k in at:
        x[k] = amp
    return x


def constant_row(L, v=1.5):
    return np.full(L, v, np.float32)


def sine(L, period, phase_deg, amp=1.0):
    """amp sin(2 pi i / period + phase)"""
    i = np.arange(L, dtype=np.float64)
    return (amp * np.sin(2.0 * math.pi * i / period + math.radians(phase_deg))).astype(np.float32)


def voice(L, rate, seed, amp=0.5):
    """a voice-like row: three partials under a syllable envelope, with a few sharp onsets"""
    rng = np.random.default_rng(seed)
    t = np.arange(L, dtype=np.float64) / rate
    env = 0.15 + 0.85 * np.abs(np.sin(2.0 * math.pi * 3.1 * t)) ** 3
    x = env * (np.sin(2 * math.pi * 180.0 * t) + 0.6 * np.sin(2 * math.pi * 1130.0 * t + 0.4) + 0.35 * np.sin(2 * math.pi * 2950.0 * t + 1.1))
    x = amp * x / 1.95 + 1e-4 * rng.standard_normal(L)
    return x.astype(np.float32)


def cpu_rows(Wn):
    """name -> row: the rows of the CPU suite at lookahead Wn (also run on the device)"""
    N = 2 * Wn + 1
    L = 2 * N + 1
    rows = {"len%d" % n: noise(n, 10 + n, 1.2) for n in lengths(Wn)}
    rows["nonfinite"] = nonfinite_row(max(67, L))
    rows["zero"] = np.zeros(L, np.float32)
    rows["impulse"] = impulse_row(4 * N, [2 * N])
    rows["two_impulses"] = impulse_row(4 * N, [2 * N - Wn // 2 - 1, 2 * N + Wn // 2], 3.0)
    rows["edges"] = impulse_row(3 * N, [0, 3 * N - 1])
    rows["under"] = noise(L, 7, 0.05)
    rows["constant"] = constant_row(L)
    return rows


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ulp_diff(a, b):
    return RS.ulp_diff(a, b)
