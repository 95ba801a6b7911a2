"""The contracts of vx_pauses and vx_retime (include/vallex_hip.h) restated in numpy: the pause rule on top of _finish_refs' frame
table, and the piecewise time map -- copies and WSOLA with both ends pinned, every sum, tie and rounding as the header words it, on
top of _stretch_refs.  The device (tests/test_gpu_retime.py) and the host code (tests/test_retime_host.py) are compared with this
word for word; tests/test_retime_refs.py holds it to a sequential Python loop and to its properties.  Not fast: a checker."""
import numpy as np

from tests import _finish_refs as F
from tests import _stretch_refs as S

H = 80                                                   # the hop of the tests: 10 ms at 8 kHz
RATE = 8000


# ---- vx_pauses -------------------------------------------------------------------------------------------------------------------
def pauses(x, frame, silence_db=-50.0, min_frames=1, keep=0, table=None):
    """the pause spans of a row, int32 (n, 2): maximal runs of at least min_frames quiet frames strictly between the first and the
    last active frame, as [f_a F + keep, f_b F - keep), the empty ones dropped"""
    x = np.asarray(x, np.float32).reshape(-1)
    L = len(x)
    e, _, _ = F.frames(x, frame) if table is None else table
    active = e > F.thr2(silence_db) * F.frame_counts(L, frame).astype(np.float64)
    idx = np.flatnonzero(active)
    out = []
    if len(idx):
        f, last = int(idx[0]) + 1, int(idx[-1])
        while f < last:
            if active[f]:
                f += 1
                continue
            g = f
            while g < last and not active[g]:
                g += 1
            if g - f >= min_frames and f * frame + keep < g * frame - keep:
                out.append((f * frame + keep, g * frame - keep))
            f = g
    return np.array(out, np.int32).reshape(-1, 2)


# ---- vx_retime -------------------------------------------------------------------------------------------------------------------
def seg_frames(lb, hop):
    return int(lb) // int(hop)


def seg_nominal(la, lb, hop, k):
    """n_k - a_i of a walked segment: floor(k (la - lb + (M - 1) H) / (M - 1))"""
    M = seg_frames(lb, hop)
    return int(k) * (int(la) - int(lb) + (M - 1) * int(hop)) // (M - 1)


def check_anchors(anchors, L, hop):
    """None, or what is wrong with the anchors of a row of L samples -- the refusals of the header, in its order"""
    an = np.asarray(anchors, np.int64).reshape(-1, 2)
    if len(an) < 1:
        return "n_anchors"
    if tuple(an[0]) != (0, 0):
        return "anchors[0]"
    for i in range(1, len(an)):
        la, lb = int(an[i, 0] - an[i - 1, 0]), int(an[i, 1] - an[i - 1, 1])
        if la <= 0 or lb <= 0:
            return f"anchors[{i}]"
        if la != lb and (la < 2 * hop or lb < 2 * hop):
            return f"segment {i - 1} is walked"
        if la != lb and (la > 4 * lb or lb > 4 * la):
            return f"segment {i - 1}: la / lb"
    if int(an[-1, 0]) != L:
        return f"anchors[{len(an) - 1}]"
    return None


def frame_count(anchors, hop):
    an = np.asarray(anchors, np.int64).reshape(-1, 2)
    d = np.diff(an, axis=0)
    return int(sum(seg_frames(lb, hop) for la, lb in d if la != lb))


def _pick(Dd, dlo):
    """offset of the winner among the candidates d = dlo + index: the smallest D_d, ties to the smallest |d|, then to the negative d"""
    d = np.flatnonzero(Dd == Dd.min()) + dlo
    d = d[np.abs(d) == np.abs(d).min()]
    return int(d.min())


def walk(row, a, a1, lb, hop, D):
    """one walked segment of a _stretch_refs._Row: (out float32 [lb], pos int64 [M], cost float64 [M])"""
    la, M = a1 - a, seg_frames(lb, hop)
    rem = lb - M * hop
    w = S.fade_table(hop).astype(np.float64)
    wr = w[::-1]
    out, pos, cost = np.zeros(lb, np.float32), np.zeros(M, np.int64), np.zeros(M, np.float64)
    pos[0] = a
    out[:hop] = row.take(a, hop).astype(np.float32)
    for k in range(1, M):
        t = row.take(int(pos[k - 1]) + hop, hop)
        n = a + seg_nominal(la, lb, hop, k)
        dlo, dhi = (0, 0) if k == M - 1 else (max(-D, a - n), min(D, a1 - hop - n))
        c, e = S.frame_sums(row.take(n + dlo, dhi - dlo + hop), t)
        Dd = e - 2.0 * c
        d = _pick(Dd, dlo)
        pos[k], cost[k] = n + d, Dd[d - dlo]
        out[k * hop: (k + 1) * hop] = (row.take(int(pos[k]), hop) * w + t * wr).astype(np.float32)
    assert pos[M - 1] == a1 - hop - rem
    out[M * hop:] = row.take(int(pos[M - 1]) + hop, rem).astype(np.float32)
    return out, pos, cost


def retime(x, anchors, hop, D):
    """(out float32 [Lout], pos int64 [frames], cost float64 [frames]) of one row under its anchors (k, 2)"""
    x = np.asarray(x, np.float32).reshape(-1)
    an = np.asarray(anchors, np.int64).reshape(-1, 2)
    assert check_anchors(an, len(x), hop) is None, check_anchors(an, len(x), hop)
    row = S._Row(x)
    out = np.zeros(int(an[-1, 1]), np.float32)
    pos, cost = [np.zeros(0, np.int64)], [np.zeros(0, np.float64)]
    for (a, b), (a1, b1) in zip(an[:-1], an[1:]):
        a, b, a1, b1 = int(a), int(b), int(a1), int(b1)
        if a1 - a == b1 - b:
            out[b:b1] = x[a:a1]                          # the bits, non-finite ones included
            continue
        o, p, c = walk(row, a, a1, b1 - b, hop, D)
        out[b:b1] = o
        pos.append(p)
        cost.append(c)
    return out, np.concatenate(pos), np.concatenate(cost)


# ---- the inputs of the tests -----------------------------------------------------------------------------------------------------
def voiced(L, seed, f=140.0, rate=RATE):
    """a voiced-like mixture (two partials that drift, a little noise), as _stretch_refs.rows"""
    rng = np.random.default_rng(seed)
    n = np.arange(L, dtype=np.float64)
    x = 0.4 * np.sin(2 * np.pi * f * n / rate + 0.3 * np.sin(2 * np.pi * 3.0 * n / rate)) + 0.2 * np.sin(2 * np.pi * 2.7 * f * n / rate)
    return (x + 0.02 * rng.standard_normal(L)).astype(np.float32)


def bursts(gaps, burst=2000, lead=400, tail=400, seed=5, floor=1e-4, rate=RATE):
    """voiced bursts of `burst` samples separated by the given gaps of noise floor, between a lead and a tail of it: (x, [(g0, g1)])"""
    rng = np.random.default_rng(seed)
    L = lead + tail + burst * (len(gaps) + 1) + sum(gaps)
    x = (floor * rng.standard_normal(L)).astype(np.float32)
    s, spans = lead, []
    for i in range(len(gaps) + 1):
        x[s: s + burst] += voiced(burst, seed + 1 + i, rate=rate)
        s += burst
        if i < len(gaps):
            spans.append((s, s + gaps[i]))
            s += gaps[i]
    return x, spans


ABOVE_MIN_WINDOW = ("whole row walked",)                 # its one segment does not fit the smallest development window


def cases():
    """(name, row, anchors, D) of the kernel tests at hop 80: the row lengths 0, 1, 400, 4001 and 20 011 and the maps of the issue.
    Every walked segment but the one of ABOVE_MIN_WINDOW fits a launch of 2048 input samples (la + 2 D + H)."""
    h = H
    x0, x1, x400, x4001, x20011 = (voiced(L, 40 + i) for i, L in enumerate((0, 1, 400, 4001, 20011)))
    hot = x4001.copy()
    hot[100], hot[900], hot[2500], hot[3300] = np.nan, np.inf, -np.inf, np.nan     # 100, 3300 in copies; 900, 2500 walked
    z = x4001.copy()
    z[1000:2600] = 0.0
    out = [
        ("empty", x0, [(0, 0)], 50),
        ("one sample", x1, [(0, 0), (1, 1)], 50),
        ("identity 400", x400, [(0, 0), (400, 400)], 50),
        ("identity 20011", x20011, [(0, 0), (20011, 20011)], 50),
        ("many anchors all copy", x4001, [(i, i) for i in range(0, 4001, 137)] + [(4001, 4001)], 50),
        ("4:1", x4001, [(0, 0), (500, 500), (2100, 900), (4001, 2801)], 50),
        ("1:4", x4001, [(0, 0), (500, 500), (900, 2100), (4001, 5201)], 50),
        ("lb = 2H", x400, [(0, 0), (100, 100), (400, 100 + 2 * h)], 50),
        ("la = 2H", x400, [(0, 0), (2 * h, 399), (400, 639)], 0),
        ("rem = 0", x4001, [(0, 0), (1000, 1000), (2000, 1000 + 7 * h), (4001, 3001 + 7 * h)], 50),
        ("rem = H - 1", x4001, [(0, 0), (1000, 1000), (2000, 1000 + 8 * h - 1), (4001, 3001 + 8 * h - 1)], 50),
        ("back to back", x4001, [(0, 0), (1500, 900), (2900, 2900), (4001, 4001)], 50),
        ("back to back D 0", x4001, [(0, 0), (1500, 900), (2900, 2900), (4001, 4001)], 0),
        ("whole row walked", x20011, [(0, 0), (20011, 16009)], 50),
        ("many walked", x20011, [(0, 0)] + [(1000 * i, 800 * i if i % 3 else 800 * i + 50) for i in range(1, 20)] + [(20011, 16011)], 50),
        ("non-finite", hot, [(0, 0), (500, 500), (1500, 1000), (2300, 1800), (3000, 3000), (4001, 4001)], 50),
        ("all-zero walked", z, [(0, 0), (1000, 1000), (2600, 2000), (4001, 3401)], 50),
    ]
    return [(n, x, np.array(a, np.int32).reshape(-1, 2), D) for n, x, a, D in out]
