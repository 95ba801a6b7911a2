"""CPU: the equaliser's host code (csrc/eq_host.h: the cookbook designs, the checks of a cascade, the warm-up W, the launch planner, the
sequential reference of the contract), compiled into the stand-alone program tools/eq_host_check.cpp and run here -- no GPU, no
library.  Designs, W and the program's sequential recursion must equal the numpy restatement (tests/_eq_refs.py) word for word; the
planner must put every step of every row into exactly one job, give it the warm-up pre = min(W, start), stage every sample a job
reads and stay inside the window and the caps.  The same program runs the same inputs once more under the address and
undefined-behaviour sanitizers, stand-alone."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import vallex_amd  # noqa: F401
from tests import _eq_refs as R
from vallex_amd._capi import DEV_EQ_WINDOW_MIN, EQ_WINDOW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = int(re.search(r"#define VX_EQ_STEP (\d+)", open(os.path.join(ROOT, "include", "vallex_hip.h")).read()).group(1))
TILE = 64


def _build(tmp, name, extra):
    from vallex_amd import _build
    exe = str(tmp / name)
    src = os.path.join(ROOT, "tools", "eq_host_check.cpp")
    cxx = shutil.which("g++") or shutil.which("c++")
    cmd = [cxx] if cxx else [_build._hipcc(), "-x", "c++"]
    subprocess.run(cmd + ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + extra + [src, "-o", exe], check=True, cwd=ROOT)
    return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def prog(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("eq")
    if request.param == "plain":
        return _build(tmp, "eq_host_check", [])
    return _build(tmp, "eq_host_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _run(prog, *args):
    r = subprocess.run([prog] + [str(a) for a in args], capture_output=True, text=True)
    return r.returncode, r.stdout.split("\n"), r.stderr


def _design(prog, kind, rate, f0, q, g):
    rc, out, err = _run(prog, "design", R.KINDS[kind], rate, repr(float(f0)), repr(float(q)), repr(float(g)))
    assert rc == 0, (out, err)
    return np.array([int(w, 16) for w in out[0].split()], np.uint64).view(np.float64)


def _sections(prog, specs, rate):
    return np.stack([_design(prog, k, rate, f, q, g) for k, f, q, g in specs])


def test_designs_equal_the_restatement(prog):
    """word for word: the program and the restatement call the same C library here, in the same order of operations"""
    for kind in R.KINDS:
        for rate, f0, q, g in ((8000, 20.0, 0.7071, 6.0), (24000, 80.0, 0.5, -12.0), (24000, 3000.0, 1.0, 4.0), (48000, 1000.0, 8.0, 24.0),
                               (16000, 7900.0, 0.3, -24.0)):
            np.testing.assert_array_equal(_design(prog, kind, rate, f0, q, g).view(np.uint64), R.design(kind, rate, f0, q, g).view(np.uint64),
                                          err_msg=str((kind, rate, f0, q, g)))
    for field, args in (("f0", (0, 24000, 12000, 0.7, 0)), ("f0", (0, 24000, 0, 0.7, 0)), ("f0", (0, 24000, "nan", 0.7, 0)), ("q", (1, 24000, 100, 0, 0)),
                        ("q", (1, 24000, 100, "inf", 0)), ("gain_db", (4, 24000, 100, 1, 24.01)), ("gain_db", (4, 24000, 100, 1, "nan")),
                        ("sample_rate", (0, 7999, 100, 1, 0)), ("sample_rate", (0, 192001, 100, 1, 0)), ("kind", (7, 24000, 100, 1, 0)),
                        ("kind", (-1, 24000, 100, 1, 0))):
        rc, out, _ = _run(prog, "design", *args)
        assert rc == 3 and out[0].startswith(field + " "), (field, args, out[0])


def test_warm_equals_the_restatement(prog, tmp_path):
    path = tmp_path / "sec.f64"
    cascades = [_sections(prog, specs, rate) for _, rate, specs in R.FILTERS] + [R.IDENTITY]
    cascades.append(np.concatenate([cascades[2], cascades[3], _sections(prog, [("peak", 500.0, 2.0, -6.0), ("peak", 6000.0, 3.0, 5.0)], 24000)]))
    for s in cascades:
        s.tofile(path)
        rc, out, err = _run(prog, "warm", path)
        assert rc == 0 and out[0].split() == [str(R.warm(s)), str(S)], (out, err)
    rate, (k, f, q, g) = R.HUM_NOTCH
    bad = [(_sections(prog, [(k, f, q, g)], rate), "the filter's memory is too long"), (np.array([[1.0, 0.0, 0.0, 0.0, 1.0]]), "section 0 is unstable"),
           (np.array([[1.0, 0.0, 0.0, 2.0, 0.99]]), "section 0 is unstable"), (np.array([[1.0, 0.0, np.nan, 0.0, 0.0]]), "section 0: coefficient 2"),
           (np.stack([cascades[0][0], [np.inf, 0.0, 0.0, 0.0, 0.0]]), "section 1: coefficient 0"), (np.zeros((0, 5)), "nsections 0"),
           (np.tile(cascades[0], (9, 1)), "nsections 9")]
    for s, want in bad:
        s.tofile(path)
        rc, out, _ = _run(prog, "warm", path)
        assert rc == 3 and out[0].startswith(want), (want, out[0])
        with pytest.raises(ValueError):
            R.warm(s)


def _rows():
    x = R.noise_row(3 * S + 1, seed=5, dc=0.3)
    hot = R.noise_row(2 * S + 9, seed=6)
    hot[[0, S - 1, S, 2 * S + 8]] = [np.nan, np.inf, -np.inf, np.nan]
    big = np.full(S + 3, 3e38, np.float32)
    big[1::2] *= -1
    return [x, hot, big, x[:0], x[:1], x[:S - 1], x[:S], x[:S + 1]]


def test_reference_equals_the_restatement(prog, tmp_path):
    sec, src, dst = tmp_path / "sec.f64", tmp_path / "in.f32", tmp_path / "out.f32"
    shelf = _sections(prog, [("high_shelf", 1000.0, 0.7071, 24.0)], 24000)
    cascades = [_sections(prog, specs, 24000) for _, rate, specs in R.FILTERS if rate == 24000 and len(specs) > 1] + [R.IDENTITY, shelf]
    checked = zeroed = 0
    for s in cascades:
        s.tofile(sec)
        W = R.warm(s)
        for x in _rows():
            x.tofile(src)
            rc, out, err = _run(prog, "run", src, sec, dst)
            assert rc == 0, err
            want, info = R.eq(x, s, W, S)
            got = np.fromfile(dst, np.float32)
            np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
            assert out[0].split() == [str(W), str(info["nonfinite"]), str(info["nonfinite_out"]), "%08x" % np.float32(info["peak"]).view(np.uint32)]
            assert np.isfinite(got).all()
            checked += len(x)
            zeroed += info["nonfinite_out"]
    assert checked > 30 * S and zeroed > 0                                # the +24 dB shelf does overflow fp32 on the 3e38 row


def _plan(prog, W, win, out_cap, max_jobs, lens, step=None):
    rc, out, err = _run(prog, "plan", step or S, W, win, out_cap, max_jobs, *lens)
    return rc, [tuple(int(v) for v in ln.split()) for ln in out if ln], err


def _check_plan(jobs, lens, W, win, out_cap, max_jobs, step):
    assert [j[0] for j in jobs] == sorted(j[0] for j in jobs)
    by_launch = {}
    for j in jobs:
        by_launch.setdefault(j[0], []).append(j)
    assert sorted(by_launch) == list(range(len(by_launch)))
    covered = [np.zeros(-(-n // step), np.int32) for n in lens]
    for js in by_launch.values():
        assert len(js) <= max_jobs
        i_end = o_end = r_end = 0
        for _, row, j0, pre, cnt, off, out_off, rec_off in js:           # packed back to back, inside the window and the caps
            assert (off, out_off, rec_off) == (i_end, o_end, r_end)
            start = j0 * step
            assert cnt > 0 and pre == min(W, start) and start + cnt <= lens[row]
            assert cnt % step == 0 or start + cnt == lens[row]           # a job never splits a step
            # every sample a lane of the job reads is staged: step t reads row samples [start + t step - W, ..), 0 before the row
            assert start - pre == max(0, start - W)
            nst = -(-cnt // step)
            covered[row][j0: j0 + nst] += 1
            i_end, o_end, r_end = i_end + pre + cnt, o_end + cnt, r_end + -(-nst // TILE)
        assert i_end <= win and o_end <= out_cap
    for c in covered:
        assert (c == 1).all()                                            # every step of every row in exactly one job
    return by_launch


@pytest.mark.parametrize("W", [0, 64, 1120, 8960])
def test_planner_invariants(prog, W):
    lens = [0, 1, S - 1, S, S + 1, 777, 63 * S + 5, 64 * S, 64 * S + 1, 70 * S, 0, 200 * S + 3]
    small = max(DEV_EQ_WINDOW_MIN, -(-(W + S) // 1024) * 1024)          # the smallest window of this filter the dev entry can set
    for win in (EQ_WINDOW, small, W + S):
        rc, jobs, err = _plan(prog, W, win, EQ_WINDOW, 4096, lens)
        assert rc == 0, err
        by_launch = _check_plan(jobs, lens, W, win, EQ_WINDOW, 4096, S)
        assert len(by_launch) == 1 if win == EQ_WINDOW else len(by_launch) >= sum(lens) / win
    rc, _, err = _plan(prog, W, W + S - 1, EQ_WINDOW, 4096, lens)       # below a warm-up and one step: refused
    assert rc == 3 and "warm-up" in err
    for out_cap, max_jobs in ((3 * S, 4096), (EQ_WINDOW, 2), (S, 1)):
        rc, jobs, err = _plan(prog, W, EQ_WINDOW, out_cap, max_jobs, lens)
        assert rc == 0, err
        assert len(_check_plan(jobs, lens, W, EQ_WINDOW, out_cap, max_jobs, S)) >= 5      # ten rows with samples, two jobs a launch at the most
    rc, jobs, _ = _plan(prog, W, EQ_WINDOW, EQ_WINDOW, 4096, [0, 0])
    assert rc == 0 and jobs == []
    rc, jobs, _ = _plan(prog, W + 31, 4 * (W + 31 + 512), EQ_WINDOW, 4096, lens, step=512)      # another step, a W that is no multiple of it
    assert rc == 0
    _check_plan(jobs, lens, W + 31, 4 * (W + 31 + 512), EQ_WINDOW, 4096, 512)
