"""The numpy restatement of vx_psola's contract (include/vallex_hip.h), shared by the CPU and the GPU tests of the formant-preserving
pitch shift.  Options are a tuple (hop, period_min, period_max, unvoiced_period, ratio_q16).  Every sum of the mark search is a
float64 np.cumsum along the sample axis (sequential, from 0.0), every output sample receives its grains in order of j, and every
floating-point operation is one numpy operation: nothing is contracted.  The mark walk and the synthesis marks are serial by contract
and stay Python loops over marks and grains; what is vectorised is the candidates of a mark and the samples of a grain."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

SMALL = (80, 16, 160, 40)        # 8 kHz: hop, period_min, period_max, U
TINY = (16, 16, 24, 16)
LARGEST = (4096, 16, 1024, 1024)
LENGTHS = (0, 1, 15, 16, 17, 12 * 80 + 3)
RATIOS = (43691, 65536, 131072)


def frames(L, H):
    return -(-int(L) // int(H))


def clean(x):
    y = np.array(x, np.float32).reshape(-1)
    bad = ~np.isfinite(y)
    y[bad] = 0
    return y, int(bad.sum())


def identity(x):
    """what a call returns whose grains all lie where they were taken (every ratio 65536, or no voiced mark): the cleaned samples bit
    for bit, a -0.0 as +0.0 (num starts from +0.0, and +0.0 + -0.0 = +0.0)"""
    return clean(x)[0] + np.float32(0.0)


def period(lag, a, o):
    """(P, voiced) at sample a"""
    H, pmin, pmax, U = o[:4]
    t = int(lag[min(a // H, len(lag) - 1)])
    v = pmin <= t <= pmax
    return (t if v else U), v


def marks(x, lag, o):
    """(marks a_0 .. a_N int32, cost (N + 1,) float64: the winning cost of every voiced mark below L, 0 elsewhere)"""
    y, _ = clean(x)
    L = len(y)
    pmax = o[2]
    yd = np.concatenate([y.astype(np.float64), np.zeros(2 * pmax + pmax // 8 + 1)])
    a, out, cost = 0, [], []
    while True:
        out.append(a)
        if a >= L:
            cost.append(0.0)
            break
        P, v = period(lag, a, o)
        if not v:
            cost.append(0.0)
            a += o[3]
            continue
        D = P // 8
        t = yd[a: a + P]
        lo = a + P - D
        if lo < 0:                                   # never: D < P
            raise AssertionError
        win = sliding_window_view(yd[lo: lo + 2 * D + P], P)             # (2D + 1, P): row c is candidate d = c - D
        c = np.cumsum(win * t, axis=1)[:, -1]
        e = np.cumsum(win * win, axis=1)[:, -1]
        cd = e - 2.0 * c
        d = np.arange(-D, D + 1)
        best = np.lexsort((d, np.abs(d), cd))[0]                         # cost, then |d|, then the negative d
        cost.append(float(cd[best]))
        a += P + int(d[best])
    return np.array(out, np.int32), np.array(cost, np.float64)


def grains(mk, lag, o, L, ratio=None):
    """((J, 4) int32 = (s, a, Wl, Wr), voiced_marks)"""
    H, r_all = o[0], o[4]
    N = len(mk) - 1
    a = [int(v) for v in mk]
    nv = sum(1 for i in range(N) if period(lag, a[i], o)[1])
    out, S, i = [], 0, 0
    while N >= 1:
        s = (S + 32768) >> 16
        if s >= L:
            break
        while i + 1 <= N - 1 and abs(a[i + 1] - s) < abs(a[i] - s):
            i += 1
        g = a[i + 1] - a[i]
        v = period(lag, a[i], o)[1]
        k = min(a[i] // H, len(lag) - 1)
        r = (int(ratio[k]) if ratio is not None else r_all) if v else 65536
        out.append((s, a[i], a[i] - a[i - 1] if i else a[1] - a[0], g))
        S += (g << 32) // r
    return np.array(out, np.int32).reshape(-1, 4), nv


def weights(rr, Wl, Wr):
    rr = np.asarray(rr, np.int64)
    left = rr < 0
    u = np.where(left, ((rr + Wl).astype(np.float64) + 0.5) / np.float64(Wl), ((Wr - rr).astype(np.float64) - 0.5) / np.float64(Wr))
    return ((u * u) * (3.0 - 2.0 * u)).astype(np.float32)


def synth(x, gr):
    """(out float32 (L,), gaps)"""
    y, _ = clean(x)
    L = len(y)
    yd = y.astype(np.float64)
    num, den = np.zeros(L, np.float64), np.zeros(L, np.float64)
    for s, a, Wl, Wr in gr.tolist():
        n = np.arange(max(0, s - Wl), min(L, s + Wr), dtype=np.int64)
        if not n.size:
            continue
        rr = n - s
        w = weights(rr, Wl, Wr).astype(np.float64)
        src = a + rr
        ok = (src >= 0) & (src < L)
        ys = np.where(ok, yd[np.clip(src, 0, max(L - 1, 0))], 0.0)
        num[n] = num[n] + ys * w
        den[n] = den[n] + w
    has = den > 0
    out = np.zeros(L, np.float32)
    out[has] = (num[has] / den[has]).astype(np.float32)
    return out, int(L - has.sum())


def psola(x, lag, o, ratio=None):
    """the whole contract of one row: dict(out, marks, cost, grains, info)"""
    y, bad = clean(x)
    L = len(y)
    lag = np.asarray(lag, np.int32).reshape(-1)
    assert len(lag) == frames(L, o[0])
    mk, cost = marks(y, lag, o)
    gr, nv = grains(mk, lag, o, L, ratio)
    out, gaps = synth(y, gr)
    info = dict(marks=len(mk) - 1, voiced_marks=nv, grains=len(gr), gaps=gaps, nonfinite=bad)
    return dict(out=out, marks=mk, cost=cost, grains=gr, info=info)


# ---- rows ---------------------------------------------------------------------------------------------------------------------------

def vowel(f0, F1, rate, n, bw=80.0, amp=0.5):
    """harmonics of f0 under a two-pole resonance at F1 with `bw` Hz of bandwidth, the peak at `amp`"""
    t = np.arange(n, dtype=np.float64) / rate
    r, th = np.exp(-np.pi * bw / rate), 2 * np.pi * F1 / rate
    x = np.zeros(n, np.float64)
    h = 1
    while h * f0 < 0.45 * rate:
        z = np.exp(-1j * 2 * np.pi * h * f0 / rate)
        x += np.sin(2 * np.pi * h * f0 * t) / abs(1 - 2 * r * np.cos(th) * z + r * r * z * z)
        h += 1
    return (amp * x / np.abs(x).max()).astype(np.float32)


def glide(fa, fb, F1, rate, n, bw=80.0, amp=0.5):
    """a vowel whose f0 runs linearly from fa to fb"""
    f = np.linspace(fa, fb, n)
    ph = 2 * np.pi * np.cumsum(f) / rate
    r, th = np.exp(-np.pi * bw / rate), 2 * np.pi * F1 / rate
    x = np.zeros(n, np.float64)
    h = 1
    while h * max(fa, fb) < 0.45 * rate:
        z = np.exp(-1j * 2 * np.pi * h * f / rate)
        x += np.sin(h * ph) / np.abs(1 - 2 * r * np.cos(th) * z + r * r * z * z)
        h += 1
    return (amp * x / np.abs(x).max()).astype(np.float32)


def hot_row(n, seed=5):
    """noise with a NaN, both infinities, -0.0 and denormals in it"""
    x = np.random.default_rng(seed).standard_normal(n).astype(np.float32) * np.float32(0.3)
    x[n // 7] = np.nan
    x[n // 3] = np.inf
    x[n // 2] = -np.inf
    x[n // 5] = -0.0
    x[n // 4: n // 4 + 3] = np.array([1e-40, -1e-45, 3e-39], np.float32)
    return x


def huge_row(n, seed=6):
    s = np.random.default_rng(seed).integers(0, 2, n).astype(np.float32) * 2 - 1
    return (s * np.float32(3e38)).astype(np.float32)


def length_rows(seed=1):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(n) * 0.25).astype(np.float32) for n in LENGTHS]


def lag_sets(L, o):
    """the lag arrays of a row of L samples: all voiced, all unvoiced, alternating, jumping between the period bounds"""
    H, pmin, pmax = o[:3]
    M = frames(L, H)
    mid = (pmin + pmax) // 2
    k = np.arange(M)
    return dict(voiced=np.full(M, mid, np.int32), unvoiced=np.full(M, -mid, np.int32),
                alternating=np.where(k % 2 == 0, mid, -mid).astype(np.int32),
                jumping=np.where(k % 2 == 0, pmin, pmax).astype(np.int32))


def frame_ratios(M, seed=9):
    """a per-frame Q16 array over the whole legal range, its ends included"""
    r = np.random.default_rng(seed).integers(43691, 131073, M).astype(np.int32)
    if M > 1:
        r[0], r[-1] = 43691, 131072
    return r


def cases(name):
    """(tag, row, lags, options with the ratio, per-frame ratios or None) of an option set: every row length and content with every
    lag array, the ratios going round; the vowel with every ratio on the jumping lags"""
    if name == "largest":
        x = vowel(8.0, 40.0, 8000, 3 * 1024)
        return [("largest", x, np.full(frames(len(x), 4096), 1000, np.int32), LARGEST + (43691,), None)]
    o4 = dict(small=SMALL, tiny=TINY)[name]
    out = []
    rows = length_rows() + [hot_row(483), np.zeros(200, np.float32), huge_row(331), vowel(110.0, 700.0, 8000, 963)]
    for i, x in enumerate(rows):
        for j, (lname, lag) in enumerate(lag_sets(len(x), o4).items()):
            q = RATIOS[(i + j) % 3]
            per = frame_ratios(len(lag)) if (i + j) % 4 == 3 else None
            out.append((f"{name}_{i}_{lname}", x, lag, o4 + (q,), per))
    x = rows[-1]
    lag = lag_sets(len(x), o4)["jumping"]
    for q in RATIOS:
        out.append((f"{name}_vowel_jumping_{q}", x, lag, o4 + (q,), None))
    out.append((f"{name}_vowel_jumping_frames", x, lag, o4 + (65536,), frame_ratios(len(lag), seed=10)))
    return out


# ---- yardsticks ---------------------------------------------------------------------------------------------------------------------

def strongest_harmonic(x, rate, f0):
    """the frequency in Hz of the strongest harmonic of f0 in a float64 DFT of the middle half of x"""
    x = np.asarray(x, np.float64)
    n = len(x)
    seg = x[n // 4: n // 4 + n // 2]
    t = np.arange(len(seg), dtype=np.float64) / rate
    hs = np.arange(1, int(0.45 * rate / f0) + 1)
    mag = [abs(np.sum(seg * np.exp(-2j * np.pi * h * f0 * t))) for h in hs]
    return float(hs[int(np.argmax(mag))] * f0)


def cents(f, g):
    return 1200.0 * np.log2(np.asarray(f, np.float64) / g)
