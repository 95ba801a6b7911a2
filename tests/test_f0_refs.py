"""CPU: the numpy restatement of vx_f0's contract (tests/_f0_refs.py) held to a sequential Python loop and to its own properties,
the pitch-ratio tabulation behind `pitch=`, the exact fma chain that restates the resampler for the pitch shift, and
utils.alignment.token_pitch.  No GPU, no library."""
import math
from fractions import Fraction

import numpy as np
import pytest

import vallex_amd  # noqa: F401
from tests import _f0_refs as R
from tests import _resample_refs as RR
from vallex_amd._capi import Engine
from vallex_amd.utils.alignment import token_pitch


def _loop_frame(y, s, W, T, t0, thr, rate):
    """one frame by plain Python floats (IEEE doubles), statement by statement as the header has it"""
    def at(i):
        return float(y[i]) if 0 <= i < len(y) else 0.0
    d = []
    for t in range(T + 1):
        acc = 0.0
        for j in range(W):
            e = at(s + j) - at(s + j + t)
            acc = acc + e * e
        d.append(acc)
    dp, c = [1.0], 0.0
    for t in range(1, T + 1):
        c = c + d[t]
        dp.append((d[t] * float(t)) / c if c > 0.0 else 1.0)
    thr = float(np.float32(thr))
    t, voiced = None, False
    for u in range(t0, T + 1):
        if dp[u] < thr:
            t, voiced = u, True
            break
    if voiced:
        while t + 1 <= T and dp[t + 1] < dp[t]:
            t += 1
    else:
        t = t0
        for u in range(t0 + 1, T + 1):
            if dp[u] < dp[t]:
                t = u
    off = 0.0
    if t + 1 <= T:
        a, b, cc = dp[t - 1], dp[t], dp[t + 1]
        den = (a - 2.0 * b) + cc
        if b <= a and b <= cc and den > 0.0:
            off = (0.5 * (a - cc)) / den
    return d, dp, (t if voiced else -t), np.float32(float(rate) / (float(t) + off)), np.float32(dp[t]), off


@pytest.mark.parametrize("opts,x", [(R.SMALL, R.rows(40)[5]), (R.SMALL, R.hot_row(483)), (R.TINY, R.rows(16)[5]), (R.SMALL, R.huge_row(131)),
                                    (R.SMALL, R.tone(200.0, 8000, 203))], ids=["mix", "hot", "tiny", "huge", "tone"])
def test_restatement_equals_a_sequential_loop(opts, x):
    rate, H, W, t0, T, thr = opts
    f, lag, ap, info, d, dp = R.f0(x, opts, tables=True)
    y = R.clean(x)
    assert len(f) == R.frames(len(x), H)
    for k in sorted({0, 1, len(f) // 2, len(f) - 1}):
        ld, ldp, ll, lf, la, off = _loop_frame(y, R.first(k, H, W, T), W, T, t0, thr, rate)
        assert d[k].tolist() == ld and dp[k].tolist() == ldp, k
        assert (int(lag[k]), f[k], ap[k]) == (ll, lf, la), k
        assert abs(off) <= 0.5                                          # the parabola's guard


def test_restatement_properties():
    rate, H, W, t0, T, thr = R.SMALL
    # an all-zero row: unvoiced at lag_min, aperiodicity 1, the candidate rate / lag_min, no summary
    f, lag, ap, info = R.f0(np.zeros(3 * H, np.float32), R.SMALL)
    assert (lag == -t0).all() and (ap == 1.0).all() and (f == np.float32(rate / t0)).all()
    assert info == dict(frames=3, voiced_frames=0, nonfinite=0, f0_median=0.0, f0_min=0.0, f0_max=0.0)
    assert R.f0(np.zeros(0, np.float32), R.SMALL)[3]["frames"] == 0
    # NaN and Inf count as 0 and are counted
    x = R.rows(40)[5].copy()
    z = x.copy()
    x[[5, 100, 300]] = np.nan, np.inf, -np.inf
    z[[5, 100, 300]] = 0.0
    a, b = R.f0(x, R.SMALL, tables=True), R.f0(z, R.SMALL, tables=True)
    assert a[3]["nonfinite"] == 3 and b[3]["nonfinite"] == 0
    for u, v in zip(a[:3] + a[4:], b[:3] + b[4:]):
        assert np.array_equal(u, v)
    # frames reach before 0 and behind L: the first and the last frame read padding, and the row's length alone decides M
    assert R.first(0, H, W, T) < 0 and R.first(12, H, W, T) + W + T > 12 * H + 3
    assert len(R.f0(R.rows(40)[5], R.SMALL)[0]) == 13 and len(R.f0(np.ones(1, np.float32), R.SMALL)[0]) == 1
    y = R.clean(R.rows(40)[5]).astype(np.float64)
    assert R.take(y, -5, 8).tolist() == [0.0] * 5 + y[:3].tolist() and R.take(y, len(y) - 2, 4).tolist() == y[-2:].tolist() + [0.0, 0.0]
    # summary: the lower median over the voiced frames
    s = R.summary(np.array([5, 1, 9, 3, 7, 100], np.float32), np.array([1, 2, 3, 4, -5, -6], np.int32), 2)
    assert s == dict(frames=6, voiced_frames=4, nonfinite=2, f0_median=3.0, f0_min=1.0, f0_max=9.0)


def test_tie_rules_and_the_parabola_guard():
    # unvoiced: the first of equal minima wins
    dp = np.array([1.0, 0.9, 0.7, 0.5, 0.8, 0.5, 0.6])
    assert R.pick(dp, 2, 6, 0.15) == (3, False)
    # voiced: the first lag under the threshold, then downhill only while strictly smaller
    dp = np.array([1.0, 0.9, 0.14, 0.10, 0.10, 0.05, 0.3])
    assert R.pick(dp, 2, 6, 0.15) == (3, True)
    assert R.pick(dp, 4, 6, 0.15) == (5, True)
    # the threshold is the fp32 value widened: (double)(float)0.14 lies above 0.14, so d' = 0.14 is under it
    assert float(np.float32(0.14)) > 0.14 and R.pick(np.array([1.0, 1.0, 0.14, 0.5]), 2, 3, 0.14) == (2, True)
    assert R.pick(np.array([1.0, 1.0, float(np.float32(0.14)), 0.5]), 2, 3, 0.14) == (2, False)
    assert R.pick(np.array([1.0, 1.0, 1.0, 1.0]), 2, 3, 1.0) == (2, False)      # d' = 1 is not under a threshold of 1
    # refinement: at the last lag, on a rising or falling flank and on a plateau the offset is 0; else it stays within half a lag
    assert R.refine(np.array([1.0, 0.5, 0.2, 0.1]), 3, 3) == 0.0
    assert R.refine(np.array([1.0, 0.1, 0.2, 0.3]), 2, 3) == 0.0        # b > a
    assert R.refine(np.array([1.0, 0.3, 0.2, 0.1]), 2, 3) == 0.0        # b > c
    assert R.refine(np.array([1.0, 0.2, 0.2, 0.2]), 2, 3) == 0.0        # den = 0
    assert R.refine(np.array([1.0, 0.2, 0.2, 0.9]), 2, 3) == -0.5 and R.refine(np.array([1.0, 0.9, 0.2, 0.2]), 2, 3) == 0.5
    rng = np.random.default_rng(3)
    for _ in range(2000):
        b = rng.random()
        a, c = b + rng.random() * 10.0 ** rng.integers(-17, 1), b + rng.random() * 10.0 ** rng.integers(-17, 1)
        assert abs(R.refine(np.array([1.0, a, b, c]), 2, 3)) <= 0.5


def test_accuracy_of_the_restatement_on_the_small_tones():
    """the measurement behind WORST_CENTS of tests/test_gpu_f0.py"""
    rate, H, W, t0, T, thr = R.SMALL
    L = 12 * H + 3
    worst = 0.0
    for fr in (130.0, 150.0, 200.0, 310.0, 440.0, 620.0):
        f, lag, ap, info = R.f0(R.tone(fr, rate, L), R.SMALL)
        ks = R.interior(len(f), H, W, T, L)
        assert ks == list(range(2, 10)) and (lag[ks] > 0).all()
        worst = max(worst, float(np.abs(R.cents(f[ks], fr)).max()))
    assert 4.545 <= worst <= 4.546


def test_pitch_ratio_tabulation():
    """the 1-cent grid over +-12 semitones: within 3 cents of the request, terms at most 512, the resampler's n K under its 2^18 cap"""
    worst, terms, nk = 0.0, 0, 0
    for c in range(-1200, 1201):
        r = Engine.pitch_ratio(c / 100.0)
        assert r == R.pitch_ratio(c / 100.0)
        assert Fraction(1, 2) <= r <= 2
        worst = max(worst, abs(1200.0 * math.log2(float(r)) - c))
        terms = max(terms, r.numerator, r.denominator)
        o, n, width, K = RR.geometry(r.numerator, r.denominator)
        nk = max(nk, n * K)
    assert worst <= 3.0 and terms <= 512 and nk <= 137472 < 2 ** 18
    assert Engine.pitch_ratio(0.0) == 1 and Engine.pitch_ratio(12) == 2 and Engine.pitch_ratio(-12.0) == Fraction(1, 2)
    assert Engine.pitch_ratio(Fraction(3, 2)) == Fraction(3, 2) and Engine.pitch_ratio((6, 4)) == Fraction(3, 2)
    assert Engine.pitch_ratio((512, 511)) == Fraction(512, 511)
    for bad in (12.01, -12.5, float("nan"), float("inf"), (513, 512), Fraction(1, 3), (3, 1), (0, 5), (5, 0), (-3, 2), (1, 2, 3)):
        with pytest.raises(ValueError):
            Engine.pitch_ratio(bad)


def test_shift_plan_refuses_before_any_launch():
    r, comb, sp = Engine._shift_plan(3.0, None)
    assert (r, comb, sp) == (Fraction(44, 37), Fraction(37, 44), 1)
    r, comb, sp = Engine._shift_plan((3, 2), 1.25)
    assert (r, comb, sp) == (Fraction(3, 2), Fraction(5, 6), Fraction(5, 4))
    assert Engine._shift_plan(Fraction(1), (4, 5))[1] == Fraction(4, 5)
    for pitch, speed in ((12.0, 0.9), (-12.0, 1.1), ((3, 2), (4, 6)), (1.0, 2.5), (1.0, 0.0), (1.0, (1, 0)), (1.0, Fraction(997, 1000))):
        with pytest.raises(ValueError):
            Engine._shift_plan(pitch, speed)


def test_fma32_is_the_exact_fused_multiply_add():
    rng = np.random.default_rng(11)
    a = rng.standard_normal(4000).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32)
    c = (rng.standard_normal(4000) * 10.0 ** rng.integers(-8, 3, 4000)).astype(np.float32)
    # ties of the fp32 grid that only the error term resolves: a b = 1 + 2^-24 + 2^-46 exactly with c = 0 and friends
    a[:4] = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12), np.float32(1.0), np.float32(3.0)
    b[:4] = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12), np.float32(1.0), np.float32(0.5)
    c[:4] = np.float32(-2.0 ** -11 + 2.0 ** -24), np.float32(2.0 ** -60), np.float32(2.0 ** -24), np.float32(2.0 ** -23)
    got = R.fma32(a, b, c)

    def exact32(v):                                                    # a Fraction to the nearest fp32, ties to even
        if v == 0:
            return np.float32(0.0)
        e = math.floor(math.log2(abs(v)))
        while Fraction(2) ** e > abs(v):
            e -= 1
        while Fraction(2) ** (e + 1) <= abs(v):
            e += 1
        q = v / Fraction(2) ** (e - 23)
        n = math.floor(q)
        rem = q - n
        if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2):
            n += 1
        return np.float32(float(n * Fraction(2) ** (e - 23)))
    for i in range(len(a)):
        want = exact32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
        assert got[i] == want, (i, a[i], b[i], c[i], got[i], want)


def test_resample_bits_is_within_the_fma_bound_of_the_float64_sum():
    x = R.tone(210.0, 24000, 1007)
    for p, q in ((44, 37), (37, 44), (3, 2), (2, 3)):
        o, n, width, K = RR.geometry(p, q)
        y = R.resample_bits(x, p, q)
        y64, mag = RR.resample_ref64(x, RR.taps(p, q), o, n, width)
        assert len(y) == RR.out_len(p, q, len(x)) and (np.abs(y - y64) <= RR.bound(mag, K)).all()
    assert R.resample_bits(x, 5, 5) is not x and np.array_equal(R.resample_bits(x, 5, 5), x)
    assert len(R.shift(x, 44, 37)) == len(x) and len(R.shift(x, 3, 2, (5, 4))) == -(-len(x) * 4 // 5)


def test_headers_declare_and_the_library_exports_the_entries():
    """what tests/test_abi.py does for the other entries: its scan reads names of letters and underscores, these carry a digit"""
    import ctypes as C
    import os
    import re
    from vallex_amd import _capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = vallex_amd.load_library()
    for header, syms in (("vallex_hip.h", _capi.F0_SYMBOLS), ("vallex_hip_dev.h", _capi.F0_DEV_SYMBOLS)):
        hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", header)).read(), flags=re.S)
        declared = set(re.findall(r"\b(vx_\w+)\s*\(", hdr))
        assert {s for s in declared if re.search(r"\d", s)} == set(syms), header
        for s in syms:
            assert hasattr(lib, s), s
    hdr = open(os.path.join(root, "include", "vallex_hip.h")).read()
    for st in (_capi.vx_f0_opts, _capi.vx_f0_info):                    # field names and order of the two structs == the binding
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (st.__name__, st.__name__), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in re.findall(r"\w+\s+([^;]+);", body) for n in re.findall(r"\w+", decl)]
        assert names == [f[0] for f in st._fields_], (st.__name__, names)
    assert C.sizeof(_capi.vx_f0_opts) == 28 and C.sizeof(_capi.vx_f0_info) == 24
    assert int(re.search(r"#define VX_ABI_VERSION (\d+)", hdr).group(1)) == _capi.ABI_VERSION == 6
    dev = open(os.path.join(root, "include", "vallex_hip_dev.h")).read()
    assert int(re.search(r"#define VX_DEV_F0_WINDOW_MIN (\d+)", dev).group(1)) == _capi.DEV_F0_WINDOW_MIN
    assert "#define VX_F0_WINDOW (1 << 23)" in hdr and _capi.F0_WINDOW == 1 << 23


def test_token_pitch():
    hop = 240
    f0 = np.array([100, 110, 120, 130, 140, 150, 160, 170], np.float32)          # centres 120, 360, 600, .. 1800
    voiced = np.array([1, 1, 0, 1, 1, 1, 0, 0], bool)
    seg = np.array([[0, 0], [1, 2], [3, 4], [5, 5]], np.int32)                   # samples [0, 320) [320, 960) [960, 1600) [1600, 1920)
    got = token_pitch(seg, f0, voiced, hop)
    assert got.dtype == np.float64 and got[:3].tolist() == [100.0, 110.0, 140.0] and np.isnan(got[3])
    assert token_pitch(seg, f0, voiced, hop, frame=640)[:2].tolist() == [100.0, 140.0]      # [0, 640) and [640, 1920): 130 140 150
    assert token_pitch(np.zeros((0, 2), np.int32), f0, voiced, hop).shape == (0,)
    with pytest.raises(ValueError):
        token_pitch(seg, f0, voiced[:5], hop)
    with pytest.raises(ValueError):
        token_pitch(seg, f0, voiced, 0)
