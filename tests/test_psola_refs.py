"""CPU: the numpy restatement of vx_psola's contract (tests/_psola_refs.py) held to a plain sequential Python loop of the header's
words and to its own properties; utils.alignment.range_contour, the refusals of utils.generation.Pitch, and the build lists.  No GPU,
no library."""
import math
import os
import struct
from fractions import Fraction

import numpy as np
import pytest

import vallex_amd  # noqa: F401
from tests import _psola_refs as R
from vallex_amd import _build, _capi
from vallex_amd._capi import Engine
from vallex_amd.utils.alignment import range_contour
from vallex_amd.utils.generation import Pitch


def _f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


def _loop(x, lag, o, ratio=None):
    """the contract, one scalar operation at a time (Python floats are IEEE doubles, every operation rounds once)"""
    H, pmin, pmax, U, r_all = o
    L = len(x)
    y = [float(v) if math.isfinite(v) else 0.0 for v in x]
    bad = sum(0 if math.isfinite(v) else 1 for v in x)

    def at(s):
        return y[s] if 0 <= s < L else 0.0

    def period(a):
        t = int(lag[min(a // H, len(lag) - 1)])
        return (t, True) if pmin <= t <= pmax else (U, False)
    marks, cost, a = [], [], 0
    while True:
        marks.append(a)
        if a >= L:
            cost.append(0.0)
            break
        P, v = period(a)
        if not v:
            cost.append(0.0)
            a += U
            continue
        D = P // 8
        best = None
        for d in range(-D, D + 1):
            c = e = 0.0
            for j in range(P):
                p = at(a + P + d + j)
                c = c + p * at(a + j)
                e = e + p * p
            key = (e - 2.0 * c, abs(d), d)
            if best is None or key < best:
                best = key
        cost.append(best[0])
        a += P + best[2]
    N = len(marks) - 1
    nv = sum(1 for i in range(N) if period(marks[i])[1])
    gr, S, j = [], 0, 0
    while N >= 1:
        s = (S + 32768) >> 16
        if s >= L:
            break
        i = min(range(N), key=lambda q: (abs(marks[q] - s), q))                 # nearest, ties to the lower index
        g = marks[i + 1] - marks[i]
        k = min(marks[i] // H, len(lag) - 1)
        r = (int(ratio[k]) if ratio is not None else r_all) if period(marks[i])[1] else 65536
        gr.append((s, marks[i], marks[i] - marks[i - 1] if i else marks[1] - marks[0], g))
        S += (g << 32) // r
        j += 1
    out, gaps = [], 0
    for n in range(L):
        num = den = 0.0
        for s, a, Wl, Wr in gr:
            rr = n - s
            if not -Wl <= rr < Wr:
                continue
            u = (float(rr + Wl) + 0.5) / float(Wl) if rr < 0 else (float(Wr - rr) - 0.5) / float(Wr)
            w = _f32((u * u) * (3.0 - 2.0 * u))
            num = num + at(a + rr) * w
            den = den + w
        out.append(_f32(num / den) if den > 0 else 0.0)
        gaps += 0 if den > 0 else 1
    info = dict(marks=N, voiced_marks=nv, grains=len(gr), gaps=gaps, nonfinite=bad)
    return dict(out=np.array(out, np.float32), marks=np.array(marks, np.int32), cost=np.array(cost, np.float64),
                grains=np.array(gr, np.int32).reshape(-1, 4), info=info)


def _same(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    view = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    np.testing.assert_array_equal(a.view(view), b.view(view), err_msg=str(what))


def test_restatement_equals_the_sequential_loop_word_for_word():
    cs = R.cases("tiny") + [c for c in R.cases("small") if len(c[1]) <= 500 or "jumping" in c[0]]
    assert len(cs) > 60
    for tag, x, lag, o, per in cs:
        got, want = R.psola(x, lag, o, per), _loop(x, lag, o, per)
        assert got["info"] == want["info"], (tag, got["info"], want["info"])
        for key in ("marks", "cost", "grains", "out"):
            _same(got[key], want[key], (tag, key))


def test_an_all_zero_row_steps_by_exactly_the_period():
    lag = np.full(R.frames(400, 80), 57, np.int32)
    got = R.psola(np.zeros(400, np.float32), lag, R.SMALL + (98304,))
    assert (np.diff(got["marks"]) == 57).all() and not got["cost"].any() and not got["out"].any()
    assert got["info"] == dict(marks=8, voiced_marks=8, grains=got["info"]["grains"], gaps=0, nonfinite=0)


def test_non_finite_samples_equal_zeros_and_are_counted():
    hot = R.hot_row(483)
    zeroed = R.clean(hot)[0]
    lag = R.lag_sets(483, R.SMALL)["alternating"]
    a, b = R.psola(hot, lag, R.SMALL + (80000,)), R.psola(zeroed, lag, R.SMALL + (80000,))
    assert a["info"]["nonfinite"] == 3 and b["info"]["nonfinite"] == 0
    for key in ("marks", "cost", "grains", "out"):
        _same(a[key], b[key], key)


def test_both_tie_rules():
    # a constant row: every candidate of a mark costs the same, |d| = 0 wins
    lag = np.full(R.frames(300, 80), 40, np.int32)
    x = np.full(300, 0.25, np.float32)
    mk = R.marks(x, lag, R.SMALL + (65536,))[0]
    assert (np.diff(mk)[: 300 // 40 - 2] == 40).all()
    # a template that d = -1 and d = +1 match equally and d = 0 does not: the negative d wins
    P = 16
    x = np.zeros(3 * P, np.float32)
    x[4] = 1.0
    x[P + 3] = x[P + 5] = 1.0
    mk, cost = R.marks(x, np.full(1, P, np.int32), (4096, 16, 160, 40, 65536))
    assert mk[1] == P - 1 and cost[0] == 0.0                                     # e = 2, c = 1 at d = -1 and at d = +1; 2 elsewhere
    # the synthesis marks: a centre half-way between two analysis marks takes the lower one
    gr, _ = R.grains(np.array([0, 40, 80, 120], np.int32), np.full(2, -1, np.int32), (80, 16, 160, 40, 65536), 100)
    assert gr[:, 0].tolist() == [0, 40, 80] and gr[:, 1].tolist() == [0, 40, 80]
    gr, _ = R.grains(np.array([0, 30, 60, 120], np.int32), np.array([30, 30], np.int32), (80, 16, 160, 40, 131072), 110)
    assert (15, 0, 30, 30) in [tuple(g) for g in gr.tolist()]                   # |0 - 15| == |30 - 15|: the lower index


def test_a_lag_outside_the_period_bounds_is_unvoiced():
    x = R.vowel(110.0, 700.0, 8000, 500)
    M = R.frames(500, 80)
    for t in (15, 161, 0, -73, 10 ** 6):
        got, want = R.psola(x, np.full(M, t, np.int32), R.SMALL + (131072,)), R.psola(x, np.full(M, -1, np.int32), R.SMALL + (131072,))
        assert got["info"]["voiced_marks"] == 0 and (np.diff(got["marks"]) == 40).all()
        _same(got["out"], want["out"], t)
    for t in (16, 160):
        assert R.psola(x, np.full(M, t, np.int32), R.SMALL + (131072,))["info"]["voiced_marks"] > 0


TONES = ((110.0, 700.0), (150.0, 900.0), (120.0, 800.0))                        # rows 1, 2 and 4 of the issue's table: periods >= 53


def _true_lags(f0, n, rate=8000, hop=80):
    return np.full(R.frames(n, hop), int(round(rate / f0)), np.int32)


def test_ratio_one_returns_the_samples_and_unvoiced_rows_do_at_any_ratio():
    for x in (R.vowel(110.0, 700.0, 8000, 963), R.hot_row(483), R.huge_row(331)):
        y = R.identity(x)
        sets = R.lag_sets(len(x), R.SMALL)
        for lname in ("voiced", "alternating", "jumping"):
            got = R.psola(x, sets[lname], R.SMALL + (65536,))
            _same(got["out"], y, lname)
            assert got["info"]["gaps"] == 0
        for q in R.RATIOS + (50000,):
            _same(R.psola(x, sets["unvoiced"], R.SMALL + (q,))["out"], y, q)
        assert (y.view(np.uint32) == R.clean(x)[0].view(np.uint32)).sum() >= len(x) - 1        # all but the one -0.0 of the hot row
        per = np.full(len(sets["voiced"]), 65536, np.int32)
        _same(R.psola(x, sets["voiced"], R.SMALL + (131072,), per)["out"], y, "per-frame ones override the call's ratio")


TABLE = ((110.0, 700.0, 98304), (150.0, 900.0, 43691), (130.0, 700.0, 77935), (120.0, 800.0, 131072), (100.0, 700.0, 52017),
         (160.0, 1000.0, 81920))                                                 # the issue's table: f0, F1, the ratio in Q16


def test_no_gaps_at_two_thirds_on_the_test_tones():
    """the grains overlap down to 2/3: no sample is uncovered in front of the last grain's end, at any ratio, on any tone.  What the
    contract leaves open is the END of a row: grains stop at s_j < L, so below ratio 1 the last grain's right side may end up to half an
    output period before L (the 120 Hz tone at 2/3: 14 samples of 4 000) -- `gaps` is exactly that tail."""
    for f0, F1, q in TABLE:                                                      # every row of the table at its own ratio: none
        got = R.psola(R.vowel(f0, F1, 8000, 4000), _true_lags(f0, 4000), R.SMALL + (q,))
        assert got["info"]["gaps"] == 0, (f0, q)
    tails = {}
    for f0, F1, _ in TABLE:
        x = R.vowel(f0, F1, 8000, 4000)
        for q in R.RATIOS:
            got = R.psola(x, _true_lags(f0, 4000), R.SMALL + (q,))
            s, _, _, Wr = got["grains"][-1].tolist()
            tails[f0, q] = max(0, 4000 - (s + Wr))                               # samples behind the last grain
            assert got["info"]["gaps"] == tails[f0, q] and tails[f0, q] < 0.5 * (8000 / f0) * 65536 / q, (f0, q, got["info"])
            if q >= 65536:
                assert got["info"]["gaps"] == 0, (f0, q)
    assert tails[150.0, 43691] == 0 and tails[120.0, 43691] == 14 and sum(1 for v in tails.values() if v) == 1


def test_formants_stay_and_the_pitch_moves_in_the_restatement():
    """what the GPU tests rely on, checked here first: the strongest output harmonic stays within one output harmonic spacing of F1,
    which excludes F1 * ratio"""
    for (f0, F1), q in zip(TONES, (98304, 43691, 131072)):
        ratio = q / 65536.0
        x = R.vowel(f0, F1, 8000, 4000)
        out = R.psola(x, _true_lags(f0, 4000), R.SMALL + (q,))["out"]
        peak = R.strongest_harmonic(out, 8000, f0 * ratio)
        assert abs(peak - F1) <= f0 * ratio, (f0, F1, ratio, peak)
        assert abs(F1 * ratio - F1) > f0 * ratio, (f0, F1, ratio)
        grains = R.psola(x, _true_lags(f0, 4000), R.SMALL + (q,))["grains"]
        mean = np.diff(grains[:, 0]).mean()
        assert abs(mean - (8000 / f0) / ratio) < 0.02 * (8000 / f0) / ratio


def test_range_contour():
    f0 = np.array([100.0, 110.0, 120.0, 130.0, 0.0, 140.0], np.float32)
    lag = np.array([80, 73, 67, 62, -40, 57], np.int32)
    flat = range_contour(f0, lag, 1.0, 0.0)
    assert flat.dtype == np.int32 and flat.shape == (6,)
    med = 120.0                                                                  # the lower median of the five voiced values
    want = np.rint(med / f0[[0, 1, 2, 3, 5]].astype(np.float64) * 65536).astype(np.int32)
    assert flat[[0, 1, 2, 3, 5]].tolist() == want.tolist() and flat[4] == 65536 and flat[2] == 65536
    assert range_contour(f0, lag, 1.25, 1.0).tolist() == [81920] * 6              # scale 1: the ratio alone
    wide = range_contour(f0, lag, 1.0, 2.0)
    assert wide[0] < 65536 < wide[5] and wide[5] == int(np.rint(140.0 / 120.0 * 65536))
    assert range_contour(f0, lag, 1.9, 3.0).max() == 131072 and range_contour(f0, lag, 0.7, 3.0).min() == 43691      # clipped
    assert range_contour(f0, -np.abs(lag), 1.5, 0.0).tolist() == [98304] * 6      # no voiced frame: the ratio
    assert range_contour([], [], 1.0, 0.0).shape == (0,)
    for bad in (dict(ratio=0.0), dict(ratio=float("nan")), dict(scale=float("inf"))):
        a = dict(f0=f0, lag=lag, ratio=1.0, scale=0.0)
        a.update(bad)
        with pytest.raises(ValueError):
            range_contour(**a)
    with pytest.raises(ValueError):
        range_contour(f0, lag[:5], 1.0, 0.0)


def test_pitch_refusals_and_what_it_carries():
    p = Pitch(3.0)
    assert p.formants is True and p.range is None and Engine._pitch_parts(p) == (3.0, True, None)
    assert Engine._pitch_parts(3.0) == (3.0, False, None) and Engine._pitch_parts(Fraction(3, 2), True, 0.5) == (Fraction(3, 2), True, 0.5)
    r, comb, sp = Engine._shift_plan(Pitch((3, 2)), (5, 4))
    assert (r, comb, sp) == (Fraction(3, 2), Fraction(5, 4), Fraction(5, 4))      # with formants the stretch runs at the speed alone
    assert Engine._shift_plan((3, 2), (5, 4)) == (Fraction(3, 2), Fraction(5, 6), Fraction(5, 4))     # as before
    assert Engine._shift_plan(Pitch((3, 2), formants=False), (5, 4)) == (Fraction(3, 2), Fraction(5, 6), Fraction(5, 4))
    Pitch((2, 3)), Pitch((2, 1)), Pitch(-7.0), Pitch(0.0, range=0.0), Pitch(2.0, range=4.0), Pitch((1, 2), formants=False)
    for a, kw in (((13.0,), {}), (((1, 2),), {}), (((3, 5),), {}), ((-7.1,), {}), ((3.0,), dict(formants=False, range=0.5)),
                  ((3.0,), dict(range=-0.1)), ((3.0,), dict(range=4.1)), ((3.0,), dict(range=float("nan"))), (((1, 0),), {})):
        with pytest.raises(ValueError):
            Pitch(*a, **kw)
    assert Engine.psola_q16(1.0) == 65536 and Engine.psola_q16(Fraction(2, 3)) == 43691 and Engine.psola_q16((2, 1)) == 131072
    assert Engine.psola_q16(Fraction(44, 37)) == round(Fraction(44, 37) * 65536)
    for bad in (0.66, 2.0001, float("inf"), (1, 0)):
        with pytest.raises(ValueError):
            Engine.psola_q16(bad)


def test_build_lists_symbols_and_constants():
    assert "psola.hip" in _build.SOURCES and "psola.hip" in _build.ENGINE_TUS and "psola_host.h" in _build.ENGINE_HEADERS
    assert os.path.exists(os.path.join(_build.CSRC, "psola.hip")) and os.path.exists(os.path.join(_build.CSRC, "psola_host.h"))
    assert "vx_psola" in _capi.SYMBOLS and {"vx_dev_psola_table", "vx_dev_psola_window"} <= set(_capi.DEV_SYMBOLS)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "vallex_hip.h")).read()
    dev = open(os.path.join(root, "include", "vallex_hip_dev.h")).read()
    assert "#define VX_PSOLA_WINDOW (1 << 23)" in hdr and _capi.PSOLA_WINDOW == 1 << 23
    assert f"#define VX_DEV_PSOLA_WINDOW_MIN {_capi.DEV_PSOLA_WINDOW_MIN}\n" in dev
    assert "#define VX_ABI_VERSION 6" in hdr and _capi.ABI_VERSION == 6
    import ctypes as C
    assert C.sizeof(_capi.vx_psola_opts) == 24 and C.sizeof(_capi.vx_psola_info) == 20
    src = open(os.path.join(_build.CSRC, "psola.hip")).read()
    assert "atomic" not in src.split("#include", 1)[1].replace("No atomics", "") and "asm" not in src.replace("assembly", "")
