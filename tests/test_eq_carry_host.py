"""CPU: the carried-state equaliser's host code (csrc/eq_carry_host.h: the step matrix M, the launch planner, the sequential reference
of the contract's three passes), compiled into the stand-alone program tools/eq_carry_host_check.cpp and run here -- no GPU, no
library.  M, the reference's outputs, end states and counts must equal the numpy restatement (tests/_eq_carry_refs.py) word for word;
the planner must put every step of every row into exactly one job, cut rows at steps only, hand a cut row's state on (cont / cut /
last) through a carry slot that no launch both reads and writes, and stay inside the window and the job cap.  The same program runs the same inputs once more under the address and
undefined-behaviour sanitizers, stand-alone."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import vallex_amd  # noqa: F401
from tests import _eq_carry_refs as R
from tests import _eq_refs as E
from vallex_amd._capi import DEV_EQ_WINDOW_MIN, EQ_WINDOW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Sc = int(re.search(r"#define VX_EQ_CARRY_STEP (\d+)", open(os.path.join(ROOT, "include", "vallex_hip.h")).read()).group(1))
TILE = 64


def _build(tmp, name, extra):
    from vallex_amd import _build
    exe = str(tmp / name)
    src = os.path.join(ROOT, "tools", "eq_carry_host_check.cpp")
    cxx = shutil.which("g++") or shutil.which("c++")
    cmd = [cxx] if cxx else [_build._hipcc(), "-x", "c++"]
    subprocess.run(cmd + ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + extra + [src, "-o", exe], check=True, cwd=ROOT)
    return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def prog(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("eq_carry")
    if request.param == "plain":
        return _build(tmp, "eq_carry_host_check", [])
    return _build(tmp, "eq_carry_host_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _run(prog, *args):
    r = subprocess.run([prog] + [str(a) for a in args], capture_output=True, text=True)
    return r.returncode, r.stdout.split("\n"), r.stderr


def _words(line):
    return np.array([int(w, 16) for w in line.split()], np.uint64).view(np.float64)


def _sections(specs, rate=24000):
    return np.stack([E.design(k, rate, f, q, g) for k, f, q, g in specs])


CASCADES = {
    "hum 50 x 1 Q 100": _sections(R.hum_specs(50.0, 1, 100.0, 24000)),
    "hum 60 x 4 Q 30 + rumble": _sections(R.hum_specs(60.0, 4, 30.0, 24000) + [("highpass", 80.0, 0.7071, 0.0)]),
    "hum 50 x 8 Q 100": _sections(R.hum_specs(50.0, 8, 100.0, 24000)),
    "shelf +24 dB": _sections([("high_shelf", 1000.0, 0.7071, 24.0)]),
    "identity": E.IDENTITY,
}


def test_matrix_equals_the_restatement(prog, tmp_path):
    path = tmp_path / "sec.f64"
    for name, s in CASCADES.items():
        s.tofile(path)
        rc, out, err = _run(prog, "matrix", path)
        assert rc == 0 and out[0].split() == [str(Sc), str(2 * len(s))], (name, out, err)
        got = np.stack([_words(ln) for ln in out[1: 1 + 2 * len(s)]])
        np.testing.assert_array_equal(got.view(np.uint64), R.matrix(s, Sc).view(np.uint64), err_msg=name)
    # a section's state is reached from its own and from earlier sections' states only: M is block lower triangular (the structural
    # zeros the chain multiplies like any other entry), and a stable cascade's M contracts
    m = R.matrix(CASCADES["hum 50 x 8 Q 100"], Sc)
    assert all((m[2 * k: 2 * k + 2, 2 * k + 2:] == 0).all() for k in range(8)) and np.abs(np.linalg.eigvals(m)).max() < 1
    rumble = _sections([("highpass", 80.0, 0.7071, 0.0)])
    bad = [(np.array([[1.0, 0.0, 0.0, 0.0, 1.0]]), "section 0 is unstable"), (np.array([[1.0, 0.0, 0.0, 2.0, 0.99]]), "section 0 is unstable"),
           (np.array([[1.0, 0.0, np.nan, 0.0, 0.0]]), "section 0: coefficient 2"), (np.stack([rumble[0], [np.inf, 0.0, 0.0, 0.0, 0.0]]), "section 1: coefficient 0"),
           (np.zeros((0, 5)), "nsections 0"), (np.tile(rumble, (9, 1)), "nsections 9")]
    for s, want in bad:
        s.tofile(path)
        rc, out, _ = _run(prog, "matrix", path)
        assert rc == 3 and out[0].startswith(want), (want, out[0])
        with pytest.raises(ValueError):
            R.matrix(s, Sc)


def _rows():
    x = R.hum_row(3 * Sc + 1, dc=0.3, seed=5)[0]
    hot = R.hum_row(2 * Sc + 9, seed=6)[0]
    hot[[0, Sc - 1, Sc, 2 * Sc + 8]] = [np.nan, np.inf, -np.inf, np.nan]
    big = np.full(Sc + 3, 3e38, np.float32)
    big[1::2] *= -1
    return [x, hot, big, x[:0], x[:1], x[:Sc - 1], x[:Sc], x[:Sc + 1]]


def test_reference_equals_the_restatement(prog, tmp_path):
    sec, src, dst, zin = tmp_path / "sec.f64", tmp_path / "in.f32", tmp_path / "out.f32", tmp_path / "z.f64"
    checked = zeroed = 0
    for name, s in CASCADES.items():
        s.tofile(sec)
        D = 2 * len(s)
        m = R.matrix(s, Sc)
        for i, x in enumerate(_rows()):
            x.tofile(src)
            z = None if i % 2 else np.random.default_rng(i).standard_normal(D)
            args = [src, sec, dst]
            if z is not None:
                z.tofile(zin)
                args.append(zin)
            rc, out, err = _run(prog, "run", *args)
            assert rc == 0, err
            want, wstate, info = R.eq_carry(x, s, Sc, z, m)
            got = np.fromfile(dst, np.float32)
            np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=f"{name} row {i}")
            assert out[0].split() == [str(info["nonfinite"]), str(info["nonfinite_out"]), "%08x" % np.float32(info["peak"]).view(np.uint32)]
            np.testing.assert_array_equal(_words(out[1]).view(np.uint64), wstate.view(np.uint64), err_msg=f"{name} row {i}")
            assert np.isfinite(got).all()
            checked += len(x)
            zeroed += info["nonfinite_out"]
    assert checked > 30 * Sc and zeroed > 0                               # the +24 dB shelf does overflow fp32 on the 3e38 row
    CASCADES["identity"].tofile(sec)
    _rows()[0].tofile(src)
    for bad in (np.array([np.nan, 0.0]), np.array([0.0, -np.inf])):      # a state that is not finite is refused
        bad.tofile(zin)
        rc, out, _ = _run(prog, "run", src, sec, dst, zin)
        assert rc == 3 and out[0].startswith("state_in of row 0: component"), out


def _plan(prog, win, max_jobs, lens, step=None):
    rc, out, err = _run(prog, "plan", step or Sc, win, max_jobs, *lens)
    return rc, [tuple(int(v) for v in ln.split()) for ln in out if ln], err


def _check_plan(jobs, lens, win, max_jobs, step):
    assert [j[0] for j in jobs] == sorted(j[0] for j in jobs)
    by_launch = {}
    for j in jobs:
        by_launch.setdefault(j[0], []).append(j)
    assert sorted(by_launch) == list(range(len(by_launch)))
    covered = [np.zeros(-(-n // step), np.int32) for n in lens]
    at = [0] * len(lens)                                                 # the next sample of every row, in job order
    handed = None                                                        # the slot the launch before wrote a cut row's z into
    for js in by_launch.values():
        assert len(js) <= max_jobs
        reads, writes = set(), set()
        i_end = s_end = r_end = 0
        for q, (_, row, j0, cnt, off, st_off, rec_off, cont, cut, last, rslot, wslot) in enumerate(js):      # packed back to back, inside the window
            assert (off, st_off, rec_off) == (i_end, s_end, r_end)
            start = j0 * step
            assert cnt > 0 and start == at[row] and start + cnt <= lens[row]
            assert cnt % step == 0 or start + cnt == lens[row]           # a job never splits a step
            assert cont == (start > 0) and last == (start + cnt == lens[row]) and cut == 1 - last
            assert not cut or q == len(js) - 1                            # a cut job is the last of its launch: one carry slot serves
            assert not cont or q == 0                                     # ... and the part behind it opens the next one
            assert rslot in (0, 1) and wslot in (0, 1)
            if cont:
                assert rslot == handed                                    # what the cut in the launch before wrote
                reads.add(rslot)
            if cut:
                writes.add(wslot)
            nst = -(-cnt // step)
            covered[row][j0: j0 + nst] += 1
            at[row] = start + cnt
            i_end, s_end, r_end = i_end + cnt, s_end + nst, r_end + -(-nst // TILE)
        assert i_end <= win and s_end <= win // step + len(js)
        assert not (reads & writes)                                      # no launch reads and writes the same carry slot: its workgroups run in no order
        handed = next(iter(writes)) if writes else None
    for c in covered:
        assert (c == 1).all()                                            # every step of every row in exactly one job
    assert at == list(lens)
    return by_launch


def test_planner_invariants(prog):
    lens = [0, 1, Sc - 1, Sc, Sc + 1, 777, 63 * Sc + 5, 64 * Sc, 64 * Sc + 1, 70 * Sc, 0, 200 * Sc + 3]
    for win in (EQ_WINDOW, DEV_EQ_WINDOW_MIN, Sc):                       # the default, the smallest the dev entry sets, one step
        rc, jobs, err = _plan(prog, win, 4096, lens)
        assert rc == 0, err
        by_launch = _check_plan(jobs, lens, win, 4096, Sc)
        assert len(by_launch) == 1 if win == EQ_WINDOW else len(by_launch) >= sum(lens) / win
    rc, _, err = _plan(prog, Sc - 1, 4096, lens)                         # below one step: refused
    assert rc == 3 and "step" in err
    for max_jobs in (2, 1):
        rc, jobs, err = _plan(prog, EQ_WINDOW, max_jobs, lens)
        assert rc == 0, err
        assert len(_check_plan(jobs, lens, EQ_WINDOW, max_jobs, Sc)) >= 5      # ten rows with samples, two jobs a launch at the most
    rc, jobs, _ = _plan(prog, EQ_WINDOW, 4096, [0, 0])
    assert rc == 0 and jobs == []
    rc, jobs, _ = _plan(prog, 4 * 96 + 5, 3, lens, step=96)              # another step, a window that is no multiple of it
    assert rc == 0
    _check_plan(jobs, lens, 4 * 96 + 5, 3, 96)
