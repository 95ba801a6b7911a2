"""CPU: the numpy restatement of vx_pauses and vx_retime (tests/_retime_refs.py) held to a sequential Python loop and to its
properties, and the integer time-map builders of utils.alignment (pause_map, pace_map, retimed_sample).  No GPU, no library beyond
the symbol lists."""
from fractions import Fraction

import numpy as np
import pytest

import vallex_amd  # noqa: F401
from tests import _f0_refs as F0
from tests import _finish_refs as FR
from tests import _retime_refs as R
from tests import _stretch_refs as S
from vallex_amd.utils.alignment import pace_map, pause_map, retimed_sample

H = R.H


def test_symbols_and_structs_are_bound():
    import ctypes as C
    from vallex_amd import _capi
    assert "vx_pauses" in _capi.SYMBOLS and "vx_retime" in _capi.SYMBOLS and "vx_dev_retime_window" in _capi.DEV_SYMBOLS
    assert C.sizeof(_capi.vx_pause_opts) == 20 and C.sizeof(_capi.vx_retime_opts) == 12
    assert _capi.ABI_VERSION == 6


def _loop_walk(x, a, a1, lb, hop, D):
    """one walked segment by a plain Python loop over candidates and samples: Python floats are doubles"""
    L = len(x)
    y = lambda s: float(x[s]) if 0 <= s < L and np.isfinite(x[s]) else 0.0
    w = [float(v) for v in S.fade_table(hop)]
    la, M = a1 - a, lb // hop
    rem = lb - M * hop
    out, pos, cost = [np.float32(y(a + j)) for j in range(hop)], [a], [0.0]
    for k in range(1, M):
        n = a + k * (la - lb + (M - 1) * hop) // (M - 1)
        ds = [0] if k == M - 1 else [d for d in range(-D, D + 1) if a <= n + d <= a1 - hop]
        best = None
        for d in ds:
            c = e = 0.0
            for j in range(hop):
                u, t = y(n + d + j), y(pos[-1] + hop + j)
                c += u * t
                e += u * u
            key = (e - 2.0 * c, abs(d), d)
            if best is None or key < best:
                best = key
        p = n + best[2]
        out += [np.float32(y(p + j) * w[j] + y(pos[-1] + hop + j) * w[hop - 1 - j]) for j in range(hop)]
        pos.append(p)
        cost.append(best[0])
    out += [np.float32(y(pos[-1] + hop + j)) for j in range(rem)]
    return np.array(out, np.float32), np.array(pos, np.int64), np.array(cost, np.float64)


def test_restatement_equals_a_sequential_loop():
    x = R.voiced(1200, 3)
    x[300], x[700] = np.nan, np.inf
    for a, a1, lb, hop, D in ((100, 900, 2 * 16 + 5, 16, 5), (0, 1200, 700, 16, 0), (200, 500, 900, 32, 7), (0, 64, 16 * 16 - 1, 16, 300)):
        out, pos, cost = R.walk(S._Row(x), a, a1, lb, hop, D)
        lout, lpos, lcost = _loop_walk(x, a, a1, lb, hop, D)
        np.testing.assert_array_equal(out.view(np.uint32), lout.view(np.uint32))
        np.testing.assert_array_equal(pos, lpos)
        np.testing.assert_array_equal(cost.view(np.uint64), lcost.view(np.uint64))
        M = lb // hop
        assert pos[0] == a and pos[-1] == a1 - hop - (lb - M * hop) and ((pos >= a) & (pos <= a1 - hop)).all()


def test_pins_and_copies():
    for name, x, an, D in R.cases():
        out, pos, cost = R.retime(x, an, H, D)
        assert len(out) == an[-1, 1] and len(pos) == len(cost) == R.frame_count(an, H)
        f = 0
        for (a, b), (a1, b1) in zip(an[:-1], an[1:]):
            if a1 - a == b1 - b:                                                       # a copy: the bits, NaN and Inf included
                np.testing.assert_array_equal(out[b:b1].view(np.uint32), x[a:a1].view(np.uint32), err_msg=name)
                continue
            M = (b1 - b) // H
            y = S.clean(x)
            np.testing.assert_array_equal(out[b: b + H], y[a: a + H], err_msg=name)     # the start pin: the input itself
            rem = b1 - b - M * H
            if rem:                                                                    # behind the end pin: the input up to the anchor
                np.testing.assert_array_equal(out[b1 - rem: b1], y[a1 - rem: a1], err_msg=name)
            assert pos[f] == a and pos[f + M - 1] == a1 - H - rem and cost[f] == 0.0
            # the last crossfade ends on the input: w[H-1] of y[a1 - rem - 1] and w[0] of the template's end
            f += M
        assert np.isfinite(out[np.isfinite(out)]).all()
    name, x, an, D = next(c for c in R.cases() if c[0] == "all-zero walked")
    _, pos, cost = R.retime(x, an, H, D)
    a, a1, lb = 1000, 2600, 1000
    assert pos.tolist() == [a + R.seg_nominal(a1 - a, lb, H, k) if k else a for k in range(lb // H)]      # the tie rule: d = 0
    # the identity map returns the bits; a segment walked at la == lb would find the self-match
    x = R.voiced(2000, 9)
    np.testing.assert_array_equal(R.retime(x, [(0, 0), (2000, 2000)], H, 50)[0].view(np.uint32), x.view(np.uint32))
    out, pos, cost = R.walk(S._Row(x), 0, 2000, 2000, H, 50)
    np.testing.assert_array_equal(out, x)
    assert pos.tolist() == [k * H for k in range(25)]


def test_pause_rule_edges():
    F = 80
    loud = R.voiced(F, 1)
    q = np.zeros(F, np.float32)
    row = lambda pattern: np.concatenate([q[:0]] + [loud if c == "x" else q for c in pattern])
    P = lambda pattern, **kw: R.pauses(row(pattern), F, -50.0, **kw).tolist()
    assert P("..xx..") == [] and P("......") == [] and P("") == [] and P("x") == [] and P("xx") == []
    assert P("x.x") == [[80, 160]] and P(".x.x.") == [[160, 240]]
    assert P("x..x.xx...x..") == [[80, 240], [320, 400], [560, 800]]
    assert P("x..x.xx...x..", min_frames=2) == [[80, 240], [560, 800]]
    assert P("x..x.xx...x..", min_frames=3, keep=10) == [[570, 790]]
    assert P("x..x", keep=80) == [] and P("x..x", keep=79) == [[159, 161]]         # an empty span is dropped
    # a short last frame: n_f counts its samples
    x = np.concatenate([row("x.x"), loud[:7]])
    assert R.pauses(x, F, -50.0).tolist() == [[80, 160]]
    # quiet is the negation of vx_finish's active rule: the pauses lie inside trim's span and hold no active frame
    x, gaps = R.bursts([4800, 900, 4800])
    e, _, _ = FR.frames(x, F)
    active = e > FR.thr2(-50.0) * FR.frame_counts(len(x), F)
    info = FR.measure(x, F, silence_db=-50.0, trim=3)
    for b, en in R.pauses(x, F, -50.0):
        assert info["begin"] < b < en < info["end"] and not active[b // F: en // F].any() and active[b // F - 1] and active[en // F]


def test_bursts_pauses_and_pause_map():
    """voiced bursts separated by 600 ms of noise floor at 8 kHz: the detector returns exactly the gaps inside the guards, pause_map
    shortens each to 1600 samples, and every output sample outside the walked segments has the input's bits"""
    x, gaps = R.bursts([4800, 4800, 4800])
    keep = 160
    p = R.pauses(x, H, -50.0, min_frames=15, keep=keep)
    assert p.tolist() == [[g0 + keep, g1 - keep] for g0, g1 in gaps]
    an = pause_map(len(x), p, max_len=1600, hop=H)
    assert R.check_anchors(an, len(x), H) is None
    d = np.diff(an, axis=0)
    assert [tuple(v) for v in d[d[:, 0] != d[:, 1]]] == [(4800 - 2 * keep, 1600)] * 3
    out, pos, cost = R.retime(x, an, H, 50)
    assert len(out) == len(x) - 3 * (4800 - 2 * keep - 1600)
    for (a, b), (a1, b1) in zip(an[:-1], an[1:]):
        if a1 - a == b1 - b:
            np.testing.assert_array_equal(out[b:b1].view(np.uint32), x[a:a1].view(np.uint32))
    assert np.abs(out[an[1, 1]: an[2, 1]]).max() < 1e-3                             # the walked pause is still a pause
    assert R.pauses(out, H, -50.0, min_frames=15, keep=keep).tolist() == [[b + 0, b1 - 0] for (a, b), (a1, b1) in zip(an[:-1], an[1:]) if a1 - a != b1 - b]


def test_pause_map_and_pace_map_are_integer_rules():
    L, hop = 100000, 240
    pauses = [(1000, 1400), (5000, 9800), (20000, 20481), (30000, 40000)]
    an = pause_map(L, pauses, max_len=2400, hop=hop)
    # 400 < 2 hop: a copy; 4800 -> 2400; 481 stays (below the bound); 10000 -> 2400 is outside 1/4: 2500
    assert np.diff(an, axis=0).tolist() == [[1000, 1000], [400, 400], [3600, 3600], [4800, 2400], [10200, 10200], [481, 481], [9519, 9519],
                                            [10000, 2500], [60000, 60000]]
    assert an.dtype == np.int32 and an[0].tolist() == [0, 0] and an[-1].tolist() == [L, L - 2400 - 7500]
    an = pause_map(L, pauses, min_len=6000, hop=hop)
    assert [v[1] for v in np.diff(an, axis=0).tolist()][1::2] == [400, 6000, 4 * 481, 10000]
    an = pause_map(L, pauses, scale=Fraction(1, 2), hop=hop)
    assert [v[1] for v in np.diff(an, axis=0).tolist()][1::2] == [400, 2400, 480, 5000]          # 240.5 -> 240 (half to even) -> 2 hop
    an = pause_map(L, [(5000, 5961)], scale=0.5, hop=hop)
    assert np.diff(an, axis=0).tolist()[1] == [961, 480]                                        # 480.5 -> 480
    an = pause_map(L, [(5000, 5963)], scale=0.5, hop=hop)
    assert np.diff(an, axis=0).tolist()[1] == [963, 482]                                        # 481.5 -> 482
    assert pause_map(L, [], max_len=10).tolist() == [[0, 0], [L, L]] and pause_map(0, []).tolist() == [[0, 0]]
    assert pause_map(L, [(0, 4800)], max_len=2400, hop=hop).tolist() == [[0, 0], [4800, 2400], [L, L - 2400]]
    assert pause_map(L, [(L - 4800, L)], max_len=2400, hop=hop).tolist() == [[0, 0], [L - 4800, L - 4800], [L, L - 2400]]
    for bad in ([(5, 5)], [(10, 5)], [(100, 200), (150, 300)], [(L - 1, L + 1)], [(-1, 5)]):
        with pytest.raises(ValueError):
            pause_map(L, bad, max_len=10)
    for an in (pause_map(L, pauses, max_len=2400, hop=hop), pause_map(L, pauses, scale=3, hop=hop)):
        assert R.check_anchors(an, L, hop) is None
    seg = [(1000, 2000), (2000, 2100), (5000, 9000)]
    an = pace_map(10000, seg, [2, 0.5, Fraction(4, 5)], hop=80)
    assert an.tolist() == [[0, 0], [1000, 1000], [2000, 1500], [2100, 1600], [5000, 4500], [9000, 9500], [10000, 10500]]
    assert pace_map(10000, seg, [8, 1, 0.125], hop=80).tolist() == [[0, 0], [1000, 1000], [2000, 1250], [2100, 1350], [5000, 4250], [9000, 20250],
                                                                       [10000, 21250]]
    assert R.check_anchors(pace_map(10000, seg, [8, 1, 0.125], hop=80), 10000, 80) is None
    with pytest.raises(ValueError):
        pace_map(10000, seg, [1, 1])
    with pytest.raises(ValueError):
        pace_map(10000, seg, [1, 0, 1])


def test_retimed_sample_round_trips_every_anchor():
    for name, x, an, _ in R.cases():
        np.testing.assert_array_equal(retimed_sample(an, an[:, 0]), an[:, 1], err_msg=name)
        np.testing.assert_array_equal(retimed_sample(an, an[:, 1], inverse=True), an[:, 0], err_msg=name)
    an = [(0, 0), (1000, 1000), (2600, 1400), (4000, 2800)]
    assert retimed_sample(an, 500) == 500 and retimed_sample(an, 1800) == 1200 and retimed_sample(an, 1801) == 1200
    assert retimed_sample(an, 1300, inverse=True) == 2200 and retimed_sample(an, 3000) == 1800
    assert retimed_sample(an, -5) == 0 and retimed_sample(an, 99999) == 2800 and isinstance(retimed_sample(an, 7), int)
    t = np.arange(0, 4001, 7)
    assert (np.diff(retimed_sample(an, t)) >= 0).all()
    # inside a walked segment (here la / lb = 4) the true positions stay within D + 2 H |la / lb - 1| of the line
    x, D = R.voiced(4000, 12), 50
    out, pos, _ = R.retime(x, an, H, D)
    k = np.arange(len(pos))
    assert (np.abs(retimed_sample(an, 1000 + k * H, inverse=True) - pos) <= D + 2 * H * 3).all()


def _median_cents(x, ref):
    f, lag, _, info = F0.f0(x, F0.SMALL)
    assert info["voiced_frames"] > 0.8 * info["frames"]
    return abs(float(F0.cents(info["f0_median"], ref)))


@pytest.mark.parametrize("la,lb,speed", [(4000, 8000, (1, 2)), (8000, 4000, (2, 1))])
def test_a_tone_keeps_its_pitch(la, lb, speed):
    """a 200 Hz five-harmonic tone inside one segment walked 1:2 and 2:1: its median F0 stays within MARGIN of what vx_stretch's
    restatement does at the same ratio, which is computed here.  MARGIN: the tracker reads a lag of 40 samples at 8 kHz, where one
    sample of lag is 43 cents; its parabolic refinement resolves a steady tone to a few cents, and 5 cents is the smallest pitch step
    commonly taken as audible.
    Measured: 1:2 retime 1.097 cents, stretch 1.097 cents; 2:1 retime 1.097 cents, stretch 1.097 cents off 200 Hz (the tracker's own
    bias on this tone: both walks leave the period alone)."""
    MARGIN = 5.0
    x = np.concatenate([F0.tone(200.0, 8000, la + 800)])
    an = [(0, 0), (400, 400), (400 + la, 400 + lb), (la + 800, lb + 800)]
    out, _, _ = R.retime(x, an, H, 50)
    st, _, _ = S.stretch(x[400: 400 + la], speed[0], speed[1], H, 50)
    rt_c, st_c = _median_cents(out[400: 400 + lb], 200.0), _median_cents(st, 200.0)
    print(f"la {la} lb {lb}: retime {rt_c:.3f} cents, stretch {st_c:.3f} cents off 200 Hz")
    assert rt_c <= st_c + MARGIN
