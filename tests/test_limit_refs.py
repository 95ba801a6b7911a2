"""CPU: the numpy restatement of the limiter's contract (tests/_limit_refs.py) against a plain sequential loop, the gain by
construction, the sample-peak bound, the detector against EBU Tech 3341's tolerance, the true peak after limiting, and the ABI."""
import ctypes as C
import dataclasses
import math
import os
import re

import numpy as np
import pytest

import vallex_amd  # noqa: F401
from tests import _limit_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C1 = R.ceiling(-1.0)
BOUND = 1.0 + 2.0 ** -22


def _all_rows():
    for Wn in (1, 3, 16):
        for name, x in R.cpu_rows(Wn).items():
            yield Wn, name, x


@pytest.mark.parametrize("Wn", [1, 3, 16])
@pytest.mark.parametrize("n", [1, 2, 4, 8])
def test_restatement_equals_the_sequential_loop(Wn, n):
    rows = [R.noise(L, 100 + L, 1.2) for L in R.lengths(Wn)] + [R.nonfinite_row(max(67, 4 * Wn + 3))]
    for x in rows:
        for gs in (1.0, 2.5):
            want = R.limit(x, gs, C1, Wn, n)
            out, P, g = R.limit_loop(x, gs, C1, Wn, n)
            assert np.array_equal(R.bits(out), R.bits(want["out"])), (len(x), gs)
            assert np.array_equal(R.bits(P), R.bits(want["P"])) and np.array_equal(R.bits(g), R.bits(want["g"]))
    assert R.limit(R.nonfinite_row(), 1.0, C1, Wn, n)["nonfinite"] == 3


def test_trapezoid_of_an_isolated_impulse():
    for Wn in (1, 3, 16):
        N = 2 * Wn + 1
        x = R.impulse_row(4 * N, [2 * N])
        r = R.limit(x, 1.0, C1, Wn, 1)
        q0 = int(r["q"][2 * N])
        assert q0 == math.floor(float(C1) / 2.0 * 16777216.0) and int((r["q"] < R.ONE).sum()) == 1
        assert np.array_equal(r["s"], R.trapezoid(len(x), Wn, 2 * N, q0))
        assert r["reduced"] == 2 * N - 1 and r["g"][2 * N] == np.float32(q0 / R.ONE)
        far = np.abs(np.arange(len(x)) - 2 * N) >= N
        assert np.array_equal(R.bits(r["out"][far]), R.bits(x[far]))


def test_two_impulses_closer_than_the_window_merge():
    Wn = 16
    N = 2 * Wn + 1
    a, b = 2 * N - Wn // 2 - 1, 2 * N + Wn // 2
    x = R.impulse_row(4 * N, [a, b], 3.0)
    r = R.limit(x, 1.0, C1, Wn, 1)
    q0 = int(r["q"][a])
    assert b - a < N and int(r["q"][b]) == q0
    # the hold is one plateau from a - Wn to b + Wn: between the impulses the gain stays at the floor q0 / 2^24
    assert np.all(r["g"][a: b + 1] == np.float32(q0 / R.ONE))
    lone = R.trapezoid(len(x), Wn, a, q0)
    assert np.all(r["s"] <= lone) and r["s"][b] < lone[b]


def test_impulses_at_the_first_and_the_last_sample():
    Wn = 3
    N = 2 * Wn + 1
    L = 3 * N
    x = R.impulse_row(L, [0, L - 1])
    r = R.limit(x, 1.0, C1, Wn, 1)
    q0 = int(r["q"][0])
    want = R.trapezoid(L, Wn, 0, q0) + R.trapezoid(L, Wn, L - 1, q0) - N * R.ONE
    assert np.array_equal(r["s"], want)
    assert r["g"][0] == np.float32(q0 / R.ONE) and r["g"][L - 1] == np.float32(q0 / R.ONE)


def test_a_row_under_the_ceiling_keeps_its_bits():
    for Wn in (1, 3, 16):
        for n in (1, 2, 4, 8):
            x = R.cpu_rows(Wn)["under"]
            r = R.limit(x, 1.0, C1, Wn, n)
            assert np.array_equal(R.bits(r["out"]), R.bits(x)) and r["reduced"] == 0 and r["min_gain"] == 1.0
            assert np.all(R.bits(r["g"]) == R.bits(np.float32(1)))


def test_a_constant_row_above_the_ceiling():
    Wn = 3
    x = R.constant_row(40)
    r = R.limit(x, 1.0, C1, Wn, 1)
    q0 = math.floor(float(C1) / 1.5 * 16777216.0)
    assert np.all(r["q"] == q0)
    # every window of the hold that the smoothing of a row sample reaches contains that sample: the gain is flat up to both ends
    assert np.all(r["g"] == np.float32(q0 / R.ONE)) and r["reduced"] == 40
    assert np.all(np.abs(r["out"]) <= float(C1) * BOUND)


def test_sample_peak_bound_on_every_row():
    n_checked = 0
    for Wn, name, x in _all_rows():
        for n in (1, 4):
            for gs, db in ((1.0, -1.0), (2.5, -1.0), (2.5, 0.0)):
                c = R.ceiling(db)
                r = R.limit(x, gs, c, Wn, n)
                assert np.all(np.abs(r["out"].astype(np.float64)) <= float(c) * BOUND), (Wn, name, n, gs, db)
                assert np.all(r["g"].astype(np.float64) * R.ONE <= r["q"])            # g <= q / 2^24
                n_checked += 1
    assert n_checked == (12 + 13 + 13) * 2 * 3                       # at lookahead 1 the lengths Wn and 1 coincide


SINES = [(4, 45.0, -3.01), (6, 60.0, -1.25), (8, 67.5, -0.69)]        # period, phase, sample peak in dBFS


def test_detector_reads_intersample_peaks_within_ebu_tech_3341(capsys):
    got = []
    for period, phase, sample_db in SINES:
        x = R.sine(480, period, phase)
        tp = 20.0 * math.log10(float(R.detector(x, R.taps(4))[32:-32].max()))
        sp = 20.0 * math.log10(float(np.abs(x).max()))
        got.append((period, tp, sp))
        assert abs(sp - sample_db) <= 0.01
        assert -0.4 <= tp <= 0.2, (period, tp)
    with capsys.disabled():
        print("\n[limit] detector at n = 4, fs/4, fs/6, fs/8:", ", ".join(f"{tp:+.3f} dBTP (sample peak {sp:+.2f})" for _, tp, sp in got))


# measured on the restatement (docs/log_r25.md): the worst reading, at n = 4, of a limited test row over the ceiling, in dB, at a
# look-ahead of 5 ms at 8 kHz (the default of finish_limited) and at 3 samples (far shorter than any use: the gain then moves within the
# span of the interpolation kernel)
WORST_EXCESS_DB = {40: 0.0146, 3: 0.5037}


def _limited_rows():
    rows = [R.voice(4000, 8000, 1, 0.9), R.sine(960, 6, 60.0) * np.hanning(960).astype(np.float32), R.sine(960, 4, 45.0),
            R.noise(2000, 42, 0.6)]
    return rows + [x for _, _, x in _all_rows() if len(x) > 16]


def test_true_peak_after_limiting(capsys):
    """not derivable: the time-varying gain can move an intersample peak.  Measured over the test rows, asserted at the measured worst
    plus 0.01 dB; a sample-peak limiter (n = 1) leaves the fs/4 sine 3 dB over"""
    c = C1
    worst = {40: -math.inf, 3: -math.inf}
    for x in _limited_rows():
        for gs in (1.0, 2.5):
            for Wn in worst:
                r = R.limit(x, gs, c, Wn, 4)
                if r["reduced"]:
                    worst[Wn] = max(worst[Wn], R.true_peak_db(r["out"], 4) - 20.0 * math.log10(float(c)))
    x = R.sine(960, 4, 45.0)
    tp4 = R.true_peak_db(R.limit(x, 1.5, c, 40, 4)["out"], 4)
    tp1 = R.true_peak_db(R.limit(x, 1.5, c, 40, 1)["out"], 4)
    with capsys.disabled():
        print(f"\n[limit] worst true-peak excess over the ceiling at n = 4: {worst[40]:+.4f} dB (look-ahead 40), {worst[3]:+.4f} dB (look-ahead 3); "
              f"fs/4 sine at 1.5: {tp4:+.3f} dBTP (n = 4), {tp1:+.3f} dBTP (n = 1)")
    for Wn in worst:
        assert worst[Wn] <= WORST_EXCESS_DB[Wn] + 0.01, Wn
    assert tp4 <= -1.0 + WORST_EXCESS_DB[40] + 0.01 and tp1 > tp4 + 1.0


def test_gain_of_finish_limited():
    assert R.gain(-math.inf, -16.0, 20.0) == 1.0
    assert R.gain(-20.0, -16.0, 20.0) == np.float32(10.0 ** 0.2)
    assert R.gain(-60.0, -16.0, 20.0) == np.float32(10.0)
    assert R.gain(-10.0, -16.0, 20.0) == np.float32(10.0 ** -0.3)


def test_abi_symbols_sources_and_layouts():
    from vallex_amd import _build, _capi
    from vallex_amd.utils import generation as G
    for s in ("vx_limit_taps", "vx_limit", "vx_finish_limited"):
        assert s in _capi.SYMBOLS
    for s in ("vx_dev_limit_gain", "vx_dev_limit_window"):
        assert s in _capi.DEV_SYMBOLS
    assert "limit.hip" in _build.SOURCES and "limit.hip" in _build.ENGINE_TUS and "limit_host.h" in _build.ENGINE_HEADERS
    assert (_capi.LIMIT_WINDOW, _capi.DEV_LIMIT_WINDOW_MIN) == (1 << 23, 8192)
    assert C.sizeof(_capi.vx_limit_opts) == 12 and [f[0] for f in _capi.vx_limit_opts._fields_] == ["struct_size", "lookahead", "oversample"]
    assert C.sizeof(_capi.vx_limit_info) == 20
    assert [f[0] for f in _capi.vx_limit_info._fields_] == ["peak", "min_gain", "ceiling", "reduced", "nonfinite"]
    assert C.sizeof(_capi.vx_finish_opts) == 44 and C.sizeof(_capi.vx_loudness_opts) == 16
    assert C.sizeof(_capi.vx_wave_info) == 40 and C.sizeof(_capi.vx_loudness_info) == 40
    assert [f.name for f in dataclasses.fields(G.Finish)][-2:] == ["lufs", "ceiling_db"]
    assert [f.name for f in dataclasses.fields(G.LimitedFinish)][-2:] == ["lookahead", "oversample"]
    assert issubclass(G.LimitedFinish, G.Finish)
    with pytest.raises(ValueError):
        G.LimitedFinish()
    assert G.LimitedFinish(lufs=-16.0).oversample == 4 and G.LimitedFinish(lufs=-16.0).lookahead is None
    hdr = open(os.path.join(ROOT, "include", "vallex_hip.h")).read()
    dev = open(os.path.join(ROOT, "include", "vallex_hip_dev.h")).read()
    assert "#define VX_ABI_VERSION 6 " in hdr and "#define VX_LIMIT_WINDOW (1 << 23)" in hdr
    assert "#define VX_DEV_LIMIT_WINDOW_MIN 8192" in dev
    m = re.search(r"typedef struct vx_limit_info \{(.*?)\} vx_limit_info;", hdr, re.S)
    order = [hdr.find(w, m.start()) for w in ("float peak;", "float min_gain;", "float ceiling;", "int32_t reduced;", "int32_t nonfinite;")]
    assert all(o > 0 for o in order) and order == sorted(order)
    for s in ("vx_limit_taps(", "vx_limit(", "vx_finish_limited("):
        assert s in hdr
    for s in ("vx_dev_limit_gain(", "vx_dev_limit_window("):
        assert s in dev
