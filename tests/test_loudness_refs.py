"""CPU: the numpy restatement of the loudness contract (tests/_loudness_refs.py) against itself, against a sequential full-history
filter, against the standard's coefficient table and calibration point, and against hand-computed block tables; the symbols, source
lists, constants and struct layouts of the feature."""
import dataclasses
import inspect
import math
import re

import numpy as np
import pytest

import vallex_amd  # noqa: F401
from tests import _loudness_refs as R

EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def tables():
    """rate -> (coefficients, rows, step tables): computed once"""
    d = {}
    for rate in (8000, 24000, 11025):
        c = R.coeffs(rate)
        rows = R.rows(rate)
        d[rate] = (c, rows, [R.steps(x, rate, c) for x in rows])
    return d


def test_coefficients_are_the_table_of_the_standard():
    c = R.coeffs(48000)
    want = [1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585, 1.0, -2.0, 1.0,
            -1.99004745483398, 0.99007225036621]
    worst = float(np.max(np.abs(c - np.array(want))))
    print(f"48 kHz: worst |c - table| = {worst:.2e}")
    assert worst <= 1e-13


def test_vectorised_steps_equal_the_sequential_loop_bit_for_bit():
    rate = 8000
    c = R.coeffs(rate)
    x = R.rows(rate)[8].copy()                                          # 7 S + 13: a cut last step
    x[5], x[2000], x[2001] = np.nan, np.inf, -np.inf
    a, b = R.steps(x, rate, c), R.steps_loop(x, rate, c)
    assert len(a) == 8
    np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64))


def _abs_impulse(b, a, n):
    """|h_k|, k < n, of a biquad b / (1, a1, a2)"""
    h = np.zeros(n)
    s1 = s2 = 0.0
    for k in range(n):
        x = 1.0 if k == 0 else 0.0
        y = b[0] * x + s1
        s1 = b[1] * x - a[0] * y + s2
        s2 = b[2] * x - a[1] * y
        h[k] = abs(y)
    return h


def test_steps_against_a_sequential_full_history_filter(tables):
    """every z_j against scipy.signal.lfilter run once over the whole row.  The bound is worked out from the coefficients:
    truncation: a step starts from rest at j S - W, so it misses the response to everything at a lag of W or more: at most
      max|x| * sum_{k >= W} |h_k|, h the impulse response of the chain (summed here until it is below 1e-40);
    rounding: either filter injects, per sample and stage, at most 3 eps (|b0| + |b1| + |b2| + |a1| + |a2| + 1) max|signal| into its
      recursion, which the recursive part amplifies by at most g = sum |impulse response of 1 / A|; the shelf's error also passes the
      high-pass (sum |h_hp|).  Two filters, so twice;
    a sum of S squares: |dz| <= 2 sqrt(z S) E + S E^2 (Cauchy-Schwarz) plus (S + 1) eps z of the additions."""
    sig = pytest.importorskip("scipy.signal")
    rate = 8000
    c, rows, zs = tables[rate]
    S, W = rate // 10, 2 * (rate // 10)
    rho = math.sqrt(c[9])
    n_imp = W + int(120 / (1 - rho))                                    # rho^(n_imp - W) < 1e-50
    h2 = _abs_impulse(c[5:8], c[8:10], n_imp)
    chain = np.abs(np.convolve(_signed(c[0:3], c[3:5], n_imp), _signed(c[5:8], c[8:10], n_imp))[:n_imp])
    tail = float(chain[W:].sum())
    g1, g2 = float(_abs_impulse([1, 0, 0], c[3:5], n_imp).sum()), float(_abs_impulse([1, 0, 0], c[8:10], n_imp).sum())
    k1, k2 = 3 * (np.abs(c[0:5]).sum() + 1), 3 * (np.abs(c[5:10]).sum() + 1)
    print(f"rho = {rho:.5f}, W rho^W = {W * rho ** W:.2e}, tail = {tail:.2e}, g = {g1:.1f}, {g2:.1f}")
    assert W * rho ** W < 1e-16 and tail < 1e-15                        # the header's claim at this rate
    worst = 0.0
    for x, z in zip(rows[8:], zs[8:]):                                  # 7 S + 13 and 20 S + 5
        xd = x.astype(np.float64)
        u = sig.lfilter(c[0:3], [1.0, c[3], c[4]], xd)
        v = sig.lfilter(c[5:8], [1.0, c[8], c[9]], u)
        xmax, umax = float(np.abs(xd).max()), float(np.abs(u).max())
        E = xmax * tail + 2 * EPS * (k1 * xmax * g1 * float(h2.sum()) + k2 * umax * g2)
        for j in range(len(z)):
            ref = float(np.sum(v[j * S:(j + 1) * S] ** 2))
            n_j = min(S, len(x) - j * S)
            bound = 2 * math.sqrt(ref * n_j) * E + n_j * E * E + 2 * (n_j + 1) * EPS * ref
            assert abs(z[j] - ref) <= bound, (len(x), j, z[j], ref, bound)
            worst = max(worst, abs(z[j] - ref) / ref)
    print(f"worst relative error against lfilter = {worst:.2e}")


def _signed(b, a, n):
    h = np.zeros(n)
    s1 = s2 = 0.0
    for k in range(n):
        x = 1.0 if k == 0 else 0.0
        y = b[0] * x + s1
        s1 = b[1] * x - a[0] * y + s2
        s2 = b[2] * x - a[1] * y
        h[k] = y
    return h


def test_calibration_sine_measures_minus_3_01_lufs():
    """the standard's calibration point: a 0 dBFS 997 Hz sine at 48 kHz reads -3.01 LUFS"""
    rate = 48000
    x = np.sin(2 * np.pi * 997.0 * np.arange(2 * rate) / rate).astype(np.float32)
    got = R.measure(x, rate, R.coeffs(rate))
    print(f"0 dBFS 997 Hz: {got['loudness']:.4f} LUFS")
    assert abs(got["loudness"] - (-3.01)) <= 0.01
    assert got["blocks"] == 17 and got["gated"] == 17


def test_every_input_stays_clear_of_both_gates(tables):
    """log10 and pow may differ by an ulp between libraries: no block of any test input is within 0.1 dB of a gate.  The set holds
    rows the absolute gate cuts, rows the relative gate cuts further, a row nothing of which passes and rows below four steps."""
    for rate, (c, rows, zs) in tables.items():
        S = rate // 10
        assert [len(r) for r in rows] == R.lengths(rate)
        for x, z in zip(rows, zs):
            m = R.gate_margin_db(z, len(x), S)
            print(f"rate {rate}, row of {len(x)}: nearest block {m:.2f} dB from a gate")
            assert m >= 0.1
    c, rows, zs = tables[8000]
    S = 800
    info = [R.reduce(z, len(x), S) for x, z in zip(rows, zs)]
    assert [i["blocks"] for i in info] == [0, 1, 1, 1, 1, 1, 1, 1, 4, 17]
    assert info[8]["above_abs"] < info[8]["blocks"]                     # the absolute gate removes blocks
    assert info[9]["gated"] < info[9]["above_abs"] < info[9]["blocks"]    # ... and the relative one removes more
    q = R.quiet_row(6 * S + 1, 8000)
    zq = R.steps(q, 8000, c)
    assert R.gate_margin_db(zq, len(q), S) >= 0.1
    iq = R.reduce(zq, len(q), S)
    assert iq["blocks"] == 3 and iq["above_abs"] == 0 and iq["loudness"] == -math.inf and iq["max_momentary"] > -math.inf
    # the round-trip row of the GPU test: no block within 25 dB of the absolute gate
    assert all(10 * math.log10(v / R.ABS_GATE) >= 25 for v in R.blocks(zs[7], len(rows[7]), S))


def test_gates_and_short_rows_by_hand():
    S = 800
    e = lambda *v: np.array(v, np.float64) * S                          # noqa: E731  step energies of S samples at mean square v
    # one standard block
    i = R.reduce(e(1e-3, 1e-3, 1e-3, 1e-3), 4 * S, S)
    assert (i["blocks"], i["above_abs"], i["gated"]) == (1, 1, 1) and abs(i["loudness"] - (-30.691)) < 1e-9
    # complete blocks only: 5 S - 1 samples are still one block, the cut fifth step is not read
    i = R.reduce(np.append(e(1e-3, 1e-3, 1e-3, 1e-3), 1e30), 5 * S - 1, S)
    assert i["blocks"] == 1 and abs(i["loudness"] - (-30.691)) < 1e-9
    # the relative gate: blocks 1e-5 | 0.0250075 0.050005 0.0750025 0.1; 0.1 * their mean = 0.0050003 removes the first
    i = R.reduce(e(1e-5, 1e-5, 1e-5, 1e-5, 0.1, 0.1, 0.1, 0.1), 8 * S, S)
    assert (i["blocks"], i["above_abs"], i["gated"]) == (5, 5, 4)
    assert abs(i["mean_square"] - 0.06250375) < 1e-12 and abs(i["max_momentary"] - (-10.691)) < 1e-9
    # the absolute gate (1.172e-7): the first block, 1e-8, does not count in the relative threshold; the others are
    # (3e-8 + 0.01) / 4, (2e-8 + 0.02) / 4, (1e-8 + 0.03) / 4 and 0.01: their mean is 0.00625000375
    i = R.reduce(e(1e-8, 1e-8, 1e-8, 1e-8, 1e-2, 1e-2, 1e-2, 1e-2), 8 * S, S)
    assert (i["blocks"], i["above_abs"], i["gated"]) == (5, 4, 4)
    assert abs(i["mean_square"] - 0.00625000375) < 1e-12
    # nothing passes: -inf, but the loudest block is still reported; the gain is 1
    i = R.reduce(e(1e-9, 1e-9, 1e-9, 1e-9, 1e-9), 5 * S, S)
    assert (i["blocks"], i["above_abs"], i["gated"]) == (2, 0, 0) and i["loudness"] == -math.inf and i["mean_square"] == 0.0
    assert abs(i["max_momentary"] - (-90.691)) < 1e-9
    assert R.gain(i["loudness"], -16.0, -1.0, 20.0, 0.5) == np.float32(1)
    # below four steps: one block over the n samples
    i = R.reduce(np.array([S * 1e-3, 1 * 1e-3]), S + 1, S)
    assert (i["blocks"], i["gated"]) == (1, 1) and abs(i["loudness"] - (-30.691)) < 1e-9
    i = R.reduce(np.array([3 * 1e-3]), 3, S)
    assert i["blocks"] == 1 and abs(i["loudness"] - (-30.691)) < 1e-9
    # no sample: no block
    i = R.reduce(np.zeros(0), 0, S)
    assert i["blocks"] == 0 and i["loudness"] == -math.inf and i["max_momentary"] == -math.inf
    # an all-zero row has blocks of energy 0
    i = R.reduce(np.zeros(4), 4 * S, S)
    assert i["blocks"] == 1 and i["max_momentary"] == -math.inf


def test_gain_takes_the_smallest_of_target_cap_and_ceiling():
    L = -30.0
    assert R.gain(L, -16.0, -1.0, 20.0, 0.01) == np.float32(10 ** (14 / 20))              # the target
    assert R.gain(L, -6.0, -1.0, 20.0, 0.01) == np.float32(10.0)                           # max_gain_db
    assert R.gain(L, -16.0, -1.0, 20.0, 0.5) == np.float32(10 ** (-1 / 20) / 0.5)          # the ceiling
    assert R.gain(L, -16.0, -1.0, 20.0, 0.0) == np.float32(10 ** (14 / 20))                # no peak: no ceiling term
    assert R.gain(L, -40.0, -1.0, 20.0, 0.5) == np.float32(10 ** (-10 / 20))               # a cut


def test_abi_lists_the_loudness_entries():
    from vallex_amd import _build, _capi
    from vallex_amd.utils import generation as G
    from vallex_amd.utils import prompt_making as PM
    assert {"vx_loudness_coeffs", "vx_loudness", "vx_finish_loud"} <= set(_capi.SYMBOLS)
    assert {"vx_dev_loudness_steps", "vx_dev_loudness_window"} <= set(_capi.DEV_SYMBOLS)
    assert "loudness.hip" in _build.SOURCES and "loudness.hip" in _build.ENGINE_TUS and "loudness_host.h" in _build.ENGINE_HEADERS
    for f in ("loudness", "finish_loud", "loudness_coeffs", "dev_loudness_steps", "dev_loudness_window"):
        assert callable(getattr(_capi.Engine, f))
    assert _capi.Engine.last_loudness_info is None
    sig = inspect.signature(_capi.Engine.finish_loud).parameters
    assert list(sig)[1:] == ["wavs", "sample_rate", "lufs", "ceiling_db", "frame", "silence_db", "trim", "keep", "max_gain_db", "fade_in",
                             "fade_out", "pcm16"]
    assert [sig[k].default for k in list(sig)[4:]] == [-1.0, None, -40.0, 0, 0, 20.0, 0, 0, False]
    assert list(inspect.signature(_capi.Engine.loudness).parameters)[1:] == ["wavs", "sample_rate"]
    f = G.Finish()
    assert f.lufs is None and f.ceiling_db == -1.0
    assert [x.name for x in dataclasses.fields(G.Finish)][-2:] == ["lufs", "ceiling_db"]        # behind the existing fields
    assert G.Finish(lufs=-16.0).lufs == -16.0
    with pytest.raises(ValueError, match="level_mode"):
        G.Finish(lufs=-16.0, level_mode=2)
    for fn in (PM.make_prompt, PM.tokenize_audio):
        assert inspect.signature(fn).parameters["lufs"].default is None
    root = _capi.os.path.dirname(_capi._HERE)
    hdr = open(_capi.os.path.join(root, "include", "vallex_hip.h")).read()
    dev = open(_capi.os.path.join(root, "include", "vallex_hip_dev.h")).read()
    assert f"#define VX_LOUDNESS_WINDOW (1 << {_capi.LOUDNESS_WINDOW.bit_length() - 1})" in hdr and _capi.LOUDNESS_WINDOW == 1 << 23
    assert f"#define VX_DEV_LOUDNESS_WINDOW_MIN {_capi.DEV_LOUDNESS_WINDOW_MIN}" in dev and _capi.DEV_LOUDNESS_WINDOW_MIN == 4096
    assert "#define VX_ABI_VERSION 6 " in hdr
    for st in (_capi.vx_loudness_opts, _capi.vx_loudness_info):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (st.__name__, st.__name__), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
        assert names == [f[0] for f in st._fields_], (st.__name__, names)
    assert _capi.C.sizeof(_capi.vx_loudness_opts) == 16 and _capi.C.sizeof(_capi.vx_loudness_info) == 40
    assert _capi.vx_loudness_info.blocks.offset == 24
    assert _capi.C.sizeof(_capi.vx_finish_opts) == 44                   # the output stage's struct did not grow


def test_lufs_needs_a_loaded_model(monkeypatch):
    from vallex_amd.utils import generation as G
    from vallex_amd.utils import prompt_making as PM
    monkeypatch.setattr(G, "model", None)
    with pytest.raises(RuntimeError, match="preload_models"):
        PM.level_loudness(np.zeros((1, 480), np.float32), -20.0, 24000)
