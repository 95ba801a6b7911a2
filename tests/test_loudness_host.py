"""CPU: the loudness host code (csrc/loudness_host.h: option checking, coefficients, step-table reduction, gain, launch planner),
compiled into the stand-alone program tools/loudness_host_check.cpp and run here -- no GPU, no library.  Counts and mean squares must
equal the numpy restatement (tests/_loudness_refs.py) exactly, loudness within 1e-12 (log10 may differ between libraries), gains within
1 fp32 ulp (pow); the planner must cover every step exactly once, in order, every job holding its warm-up, inside the capacities it
was given."""
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import vallex_amd  # noqa: F401
from tests import _loudness_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "loudness_host_check.cpp")


def _compile(exe, *flags):
    from vallex_amd import _build
    cxx = shutil.which("g++") or shutil.which("c++")
    cmd = [cxx] if cxx else [_build._hipcc(), "-x", "c++"]
    subprocess.run(cmd + ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, SRC, "-o", exe], check=True, cwd=ROOT)
    return exe


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return _compile(str(tmp_path_factory.mktemp("ln") / "loudness_host_check"))


def _run(prog, *args, stdin=None):
    r = subprocess.run([prog] + [str(a) for a in args], capture_output=True, text=True, input=stdin)
    return r.returncode, r.stdout.split("\n"), r.stderr


def _f64(word):
    return struct.unpack("<d", struct.pack("<Q", int(word, 16)))[0]


def _hex64(v):
    return f"{struct.unpack('<Q', struct.pack('<d', float(v)))[0]:016x}"


def _hex32(v):
    return f"{int(np.float32(v).view(np.uint32)):08x}"


def _coeffs(prog, rate):
    rc, out, _ = _run(prog, "coeffs", rate)
    assert rc == 0
    return np.array([_f64(w) for w in out if w], np.float64)


def test_coefficients(prog):
    """the standard's 48 kHz table to 1e-13, and the restatement's formulas within an ulp or two of tan / pow at every test rate"""
    c = _coeffs(prog, 48000)
    want = [1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585, 1.0, -2.0, 1.0,
            -1.99004745483398, 0.99007225036621]
    assert len(c) == 10 and float(np.max(np.abs(c - np.array(want)))) <= 1e-13
    for rate in (8000, 11025, 24000, 44100, 192000):
        assert float(np.max(np.abs(_coeffs(prog, rate) - R.coeffs(rate)))) <= 1e-14, rate
    assert _run(prog, "coeffs", 7999)[0] == 3 and _run(prog, "coeffs", 192001)[0] == 3


def _cases():
    S = 800
    c = R.coeffs(8000)
    cases = [(x, R.steps(x, 8000, c)) for x in R.rows(8000)]
    q = R.quiet_row(6 * S + 1, 8000)
    cases.append((q, R.steps(q, 8000, c)))
    hot = R.rows(8000)[9].copy()
    hot[3], hot[9000], hot[9001] = np.nan, np.inf, -np.inf
    cases.append((hot, R.steps(hot, 8000, c)))
    return cases


def test_reduction_and_gain_equal_the_restatement(prog):
    S = 800
    n = 0
    for x, z in _cases():
        assert R.gate_margin_db(z, len(x), S) >= 0.1                    # a last bit of log10 / pow cannot move a block across a gate
        want = R.reduce(z, len(x), S, R.sanitize(x)[1])
        peak = np.float32(np.abs(R.sanitize(x)[0]).max()) if len(x) else np.float32(0)
        txt = "".join(_hex64(v) + "\n" for v in z)
        for target, ceiling, cap in ((-16.0, -1.0, 20.0), (-23.0, -1.0, 20.0), (-6.0, -1.0, 3.0), (-10.0, -6.0, 40.0), (0.0, 0.0, 0.0)):
            rc, out, err = _run(prog, "reduce", 8000, len(x), want["nonfinite"], target, ceiling, cap, _hex32(peak), stdin=txt)
            assert rc == 0, err
            b, a, g, nf, loud, ms, mom, gain = out[0].split()
            assert (int(b), int(a), int(g), int(nf)) == (want["blocks"], want["above_abs"], want["gated"], want["nonfinite"])
            assert ms == _hex64(want["mean_square"])                    # exact
            for got, w in ((_f64(loud), want["loudness"]), (_f64(mom), want["max_momentary"])):
                assert got == w if math.isinf(w) else abs(got - w) <= 1e-12, (len(x), got, w)
            assert R.ulp_diff([np.array([int(gain, 16)], np.uint32).view(np.float32)[0]],
                              [R.gain(want["loudness"], target, ceiling, cap, peak)])[0] <= 1, (len(x), target)
            n += 1
    assert n == 12 * 5


def test_option_ranges(prog):
    ok = dict(sample_rate=24000, target_lufs=-16.0, ceiling_db=-1.0)
    assert _run(prog, "opts", *ok.values())[:2] == (0, ["ok", ""])
    for field, bad in (("sample_rate", 7999), ("sample_rate", 192001), ("sample_rate", 0), ("sample_rate", -8000),
                       ("target_lufs", 0.5), ("target_lufs", -70.5), ("target_lufs", "nan"), ("target_lufs", "-inf"),
                       ("ceiling_db", 0.1), ("ceiling_db", "nan"), ("ceiling_db", "inf"), ("ceiling_db", "-inf")):
        rc, out, _ = _run(prog, "opts", *dict(ok, **{field: bad}).values())
        assert rc == 3 and out[0].startswith(field), (field, bad, out[0])
    for field, edge in (("sample_rate", 8000), ("sample_rate", 192000), ("target_lufs", 0.0), ("target_lufs", -70.0), ("ceiling_db", 0.0),
                        ("ceiling_db", -120.0)):
        assert _run(prog, "opts", *dict(ok, **{field: edge}).values())[0] == 0, (field, edge)


S8 = 800


@pytest.mark.parametrize("rate,win,max_jobs,spans", [
    (8000, 4096, 4096, [(0, 20 * S8 + 5), (0, 7 * S8 + 13), (0, 0), (0, 1), (0, S8)]),
    (8000, 5000, 4096, [(0, 20 * S8 + 5), (0, 7 * S8 + 13), (3, 4 * S8 + 4)]),
    (8000, 4096, 4096, [(1000, 1000 + 20 * S8 + 5), (17, 17 + 7 * S8 + 13)]),             # kept spans: step 0 starts at begin
    (8000, 2400, 4096, [(0, 5 * S8 + 1)]),                                                  # the smallest window: one step per job
    (11025, 5000, 4096, [(0, 9 * 1102 + 3)]),
    (8000, 1 << 23, 3, [(0, 10), (0, 20), (0, 30), (0, 40), (0, 50), (0, 60), (0, 70)]),    # the job cap cuts
    (8000, 1 << 23, 4096, [(0, 20 * S8 + 5), (0, 0), (0, 7 * S8 + 13)]),                  # everything in one launch
])
def test_planner_covers_every_step_once(prog, rate, win, max_jobs, spans):
    S = rate // 10
    W = 2 * S
    rc, out, err = _run(prog, "plan", rate, win, max_jobs, *[f"{a}:{b}" for a, b in spans])
    assert rc == 0, err
    jobs = [tuple(int(v) for v in ln.split()) for ln in out if ln]
    nxt = [0] * len(spans)                                              # next step of every row
    by_launch = {}
    for launch, row, j0, pre, cnt, off, z_off in jobs:
        n = spans[row][1] - spans[row][0]
        assert j0 == nxt[row] and cnt > 0                               # rows in order, steps in order, none twice, none skipped
        assert pre == min(W, j0 * S)                                    # the job holds its warm-up (what lies before the span is 0)
        assert cnt % S == 0 or j0 * S + cnt == n                        # only the row's last step may be cut
        nxt[row] = j0 + -(-cnt // S)
        assert j0 * S + cnt <= n
        by_launch.setdefault(launch, []).append((off, pre + cnt, z_off, -(-cnt // S)))
    assert nxt == [-(-(b - a) // S) for a, b in spans]
    assert [row for _, row, *_ in jobs] == sorted(row for _, row, *_ in jobs)
    assert sorted(by_launch) == list(range(len(by_launch)))
    for js in by_launch.values():
        assert len(js) <= max_jobs
        end = z_end = 0
        for off, size, z_off, nz in js:                                 # packed back to back, inside the window
            assert off == end and z_off == z_end
            end += size
            z_end += nz
        assert end <= win
    if win == 1 << 23 and max_jobs == 4096:
        assert len(by_launch) == 1
    if win <= 5000:
        assert len(by_launch) >= sum(b - a for a, b in spans) / win


def test_planner_refuses_a_window_below_three_steps(prog):
    rc, _, err = _run(prog, "plan", 8000, 2399, 4096, "0:10000")
    assert rc == 3 and "below 3 S" in err
    rc, _, err = _run(prog, "plan", 24000, 4096, 4096, "0:10000")
    assert rc == 3 and "below 3 S" in err
    assert _run(prog, "plan", 24000, 7200, 4096, "0:10000")[0] == 0


def test_the_program_runs_clean_under_sanitizers(tmp_path):
    """the same program under AddressSanitizer and UBSan (host code only; nothing here is loaded into Python)"""
    exe = _compile(str(tmp_path / "loudness_host_check_san"), "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    S = 800
    x = R.rows(8000)[9]
    z = R.steps(x, 8000, R.coeffs(8000))
    txt = "".join(_hex64(v) + "\n" for v in z)
    for args, stdin in ((("coeffs", 48000), None), (("opts", 24000, -16.0, -1.0), None),
                        (("reduce", 8000, len(x), 0, -16.0, -1.0, 20.0, _hex32(0.3)), txt),
                        (("reduce", 8000, 0, 0, -16.0, -1.0, 20.0, _hex32(0.0)), ""),
                        (("reduce", 8000, 5, 0, -16.0, -1.0, 20.0, _hex32(0.3)), _hex64(1e-3) + "\n"),
                        (("plan", 8000, 4096, 4096, f"0:{20 * S + 5}", "5:5", f"17:{7 * S + 30}"), None),
                        (("plan", 8000, 2400, 2, "0:9000", "0:1"), None)):
        rc, out, err = _run(exe, *args, stdin=stdin)
        assert rc == 0 and "runtime error" not in err and "Sanitizer" not in err, (args, err)
