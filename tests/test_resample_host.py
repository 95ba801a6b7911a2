"""CPU: the resampler's host code (csrc/resample_host.h: geometry, tap builder, window planner), compiled into the stand-alone program
tools/resample_host_check.cpp and run here -- no GPU, no library.  The taps a C++ builder makes with libm must be the torch table of
resample_sinc_hann (within the 1 fp32 ulp the device test allows; the differing words are printed); the planner must cover every
block of every row exactly once, inside the capacities it was given, with the samples each window's taps reach."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import vallex_amd  # noqa: F401
from tests import _resample_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    from vallex_amd import _build
    exe = str(tmp_path_factory.mktemp("rs") / "resample_host_check")
    src = os.path.join(ROOT, "tools", "resample_host_check.cpp")
    cxx = shutil.which("g++") or shutil.which("c++")
    cmd = [cxx] if cxx else [_build._hipcc(), "-x", "c++"]
    subprocess.run(cmd + ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", src, "-o", exe], check=True, cwd=ROOT)
    return exe


def _run(prog, *args):
    r = subprocess.run([prog] + [str(a) for a in args], capture_output=True, text=True)
    return r.returncode, r.stdout.split("\n"), r.stderr


def test_host_taps_are_the_torch_taps(prog):
    total = 0
    for (orig, new), want in sorted(R.PAIRS.items()):
        rc, out, err = _run(prog, "taps", orig, new)
        assert rc == 0, err
        assert tuple(int(v) for v in out[0].split()) == want
        got = np.array([int(w, 16) for w in out[1:] if w], np.uint32).view(np.float32).reshape(want[1], want[3])
        d = R.ulp_diff(got, R.taps(orig, new))
        total += int((d != 0).sum())
        print(f"{orig} -> {new}: {int((d != 0).sum())} of {d.size} words differ from the torch table, at most {int(d.max())} ulp")
        assert d.max() <= 1, (orig, new, int(d.max()))
    print(f"host taps: {total} differing words in the fifteen tables")


def test_tap_cap(prog):
    rc, out, _ = _run(prog, "taps", 44101, 24000)
    assert rc == 3 and [int(v) for v in out[0].split()][:2] == [44101, 24000]
    rc, out, _ = _run(prog, "taps", 24000, 24000)
    assert rc == 0 and out[0].split() == ["1", "1", "7", "15"]


@pytest.mark.parametrize("orig,new,win,out_cap,max_jobs,lens", [
    (24000, 44100, 512, 1 << 24, 4096, [1007, 2015, 0, 1, 94]),
    (44100, 24000, 513, 1 << 24, 4096, [1007, 2015]),
    (24000, 11025, 512, 1 << 24, 4096, [1007, 2015, 348]),
    (24000, 16000, 777, 1 << 24, 4096, [1007, 2015, 5]),
    (24000, 48000, 1 << 23, 1000, 4096, [1007, 300]),            # the output capacity cuts
    (24000, 16000, 1 << 23, 1 << 24, 3, [10, 20, 30, 40, 50, 60, 70]),      # the job count cuts
    (24000, 16000, 1 << 23, 1 << 24, 4096, [1007, 0, 2015]),     # everything in one launch
])
def test_planner_invariants(prog, orig, new, win, out_cap, max_jobs, lens):
    o, n, width, K = R.geometry(orig, new)
    rc, out, err = _run(prog, "plan", orig, new, win, out_cap, max_jobs, *lens)
    assert rc == 0, err
    jobs = [tuple(int(v) for v in ln.split()) for ln in out if ln]
    next_blk = [0] * len(lens)
    by_launch = {}
    for launch, row, a, b, s_lo, s_hi, in_off, out_off, out_cnt in jobs:
        L = lens[row]
        olen = R.out_len(orig, new, L)
        assert a == next_blk[row] and b > a                       # rows in order, blocks in order, none twice, none skipped
        next_blk[row] = b
        assert s_lo == max(0, a * o - width) and s_hi == max(s_lo, min(L, (b - 1) * o - width + K))      # what the taps reach, inside the row
        assert out_cnt == min(b * n, olen) - a * n and out_cnt > 0
        by_launch.setdefault(launch, []).append((in_off, s_hi - s_lo, out_off, out_cnt))
    for row, L in enumerate(lens):
        assert next_blk[row] == -(-R.out_len(orig, new, L) // n), row
    assert sorted(by_launch) == list(range(len(by_launch)))
    for js in by_launch.values():
        assert len(js) <= max_jobs
        i_end = o_end = 0
        for in_off, in_cnt, out_off, out_cnt in js:               # packed back to back, inside the capacities
            assert in_off == i_end and out_off == o_end
            i_end, o_end = in_off + in_cnt, out_off + out_cnt
        assert i_end <= win and o_end <= out_cap
    if win == 1 << 23 and out_cap == 1 << 24 and max_jobs == 4096:
        assert len(by_launch) == 1
    if win < 1007:
        assert len(by_launch) > 1


def test_planner_refuses_a_window_below_one_kernel(prog):
    rc, _, err = _run(prog, "plan", 24000, 11025, 300, 1 << 24, 4096, 1007)
    assert rc == 3 and "no block fits" in err
