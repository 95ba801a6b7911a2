"""CPU: the time-stretch's host code (csrc/stretch_host.h: option checking, lengths, nominal positions, launch planner), compiled
into the stand-alone program tools/stretch_host_check.cpp and run here -- no GPU, no library.  Lengths and positions must equal the
numpy restatement (tests/_stretch_refs.py); every option range is refused with its field named; the planner must cover every frame
of every row exactly once, in order, with every sample those frames can read inside the job's span and inside the capacities.  The
same program runs the same inputs once more under the address and undefined-behaviour sanitizers, stand-alone."""
import os
import shutil
import subprocess

import pytest

import vallex_amd  # noqa: F401
from tests import _stretch_refs as R
from vallex_amd._capi import DEV_STRETCH_WINDOW_MIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp, name, extra):
    from vallex_amd import _build
    exe = str(tmp / name)
    src = os.path.join(ROOT, "tools", "stretch_host_check.cpp")
    cxx = shutil.which("g++") or shutil.which("c++")
    cmd = [cxx] if cxx else [_build._hipcc(), "-x", "c++"]
    subprocess.run(cmd + ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + extra + [src, "-o", exe], check=True, cwd=ROOT)
    return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def prog(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("st")
    if request.param == "plain":
        return _build(tmp, "stretch_host_check", [])
    return _build(tmp, "stretch_host_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _run(prog, *args):
    r = subprocess.run([prog] + [str(a) for a in args], capture_output=True, text=True)
    return r.returncode, r.stdout.split("\n"), r.stderr


def test_lengths_and_nominal_positions_equal_the_restatement(prog):
    n = 0
    for H in R.HOPS:
        for L in (0, 1, H - 1, H, H + 1, 3 * H + 7, 4801, 13001):
            for num, den in R.SPEEDS + ((6, 4), (32767, 32767)):
                M = R.frames(L, num, den, H)
                ks = sorted({0, 1, 2, M // 2, max(M - 1, 0)})
                rc, out, err = _run(prog, "geom", num, den, H, L, *ks)
                assert rc == 0, err
                assert out[0].split() == [str(R.out_len(L, num, den)), str(M)]
                assert [int(v) for v in out[1: 1 + len(ks)]] == [R.nominal(k, num, den, H) for k in ks]
                n += 1
    assert n == 3 * 8 * 9
    big = 2 ** 31 - 1                                       # no overflow
    for num, den, H in ((1, 2, 16), (2, 1, 16), (1, 2, 2048), (32767, 16384, 16), (16384, 32767, 2048)):
        M = R.frames(big, num, den, H)
        rc, out, err = _run(prog, "geom", num, den, H, big, M - 1, M)
        assert rc == 0, err
        assert out[0].split() == [str(R.out_len(big, num, den)), str(M)]
        assert [int(out[1]), int(out[2])] == [R.nominal(M - 1, num, den, H), R.nominal(M, num, den, H)]
    assert R.out_len(big, 1, 2) == 2 ** 32 - 2


def test_option_ranges(prog):
    ok = dict(speed_num=5, speed_den=4, hop=240, search=150)
    assert _run(prog, "opts", *ok.values())[:2] == (0, ["ok 5 4", ""])
    assert _run(prog, "opts", 32766, 16383, 16, 0)[1][0] == "ok 2 1"
    for field, bad in (("hop", 15), ("hop", 2049), ("hop", -1), ("search", -1), ("search", 1025), ("speed_num", 0), ("speed_num", 32768),
                       ("speed_num", -4), ("speed_den", 0), ("speed_den", 32768), ("speed_den", -1)):
        rc, out, _ = _run(prog, "opts", *dict(ok, **{field: bad}).values())
        assert rc == 3 and out[0].startswith(field + " "), (field, bad, out[0])
    for num, den in ((1, 3), (3, 1), (999, 2000), (2001, 1000), (32767, 16383)):
        rc, out, _ = _run(prog, "opts", num, den, 240, 150)
        assert rc == 3 and out[0].startswith("speed_num / speed_den"), (num, den, out[0])
    for edge in (dict(hop=16), dict(hop=2048), dict(search=0), dict(search=1024), dict(speed_num=1, speed_den=1),
                 dict(speed_num=32767, speed_den=32767), dict(speed_num=1, speed_den=2), dict(speed_num=2, speed_den=1),
                 dict(speed_num=16383, speed_den=32766), dict(speed_num=32766, speed_den=16383)):
        assert _run(prog, "opts", *dict(ok, **edge).values())[0] == 0, edge


def _check_plan(jobs, lens, num, den, H, D, win, out_cap, frame_cap, max_jobs):
    nxt = [0] * len(lens)
    by_launch = {}
    last_launch_of_row = {}
    for launch, row, k0, k1, s_lo, s_hi, in_off, out_off, out_cnt, f_off in jobs:
        L = lens[row]
        Lout, M = R.out_len(L, num, den), R.frames(L, num, den, H)
        assert k0 == nxt[row] and k0 < k1 <= M                       # frames in order, none twice, none skipped
        nxt[row] = k1
        if k0 > 0:                                                   # a later window of a row: a LATER launch, p of frame k0 - 1 is known
            assert launch > last_launch_of_row[row]
        last_launch_of_row[row] = launch
        assert out_cnt == min(k1 * H, Lout) - k0 * H and 0 <= s_lo <= s_hi <= L
        # every sample the frames can read for any admissible p lies in [s_lo, s_hi) or outside the row
        need = []
        for k in {k0, k0 + 1, (k0 + k1) // 2, k1 - 2, k1 - 1}:
            if not k0 <= k < k1:
                continue
            if k == 0:
                need.append((0, 2 * H))                              # the frame itself and the template of frame 1
                continue
            n = R.nominal(k, num, den, H)
            need.append((n - D, n + D + 2 * H))                      # search region, new segment, the next template
            if k == k0:
                n1 = R.nominal(k - 1, num, den, H)
                need.append((n1 - D + H, n1 + D + 2 * H))            # the first template, wherever p_{k0-1} lies
        for a, b in need:
            a, b = max(a, 0), min(b, L)
            assert b <= a or (s_lo <= a and b <= s_hi), (row, k0, k1, a, b, s_lo, s_hi)
        by_launch.setdefault(launch, []).append((s_hi - s_lo, in_off, out_cnt, out_off, k1 - k0, f_off))
    assert nxt == [R.frames(L, num, den, H) for L in lens]
    assert [j[1] for j in jobs] == sorted(j[1] for j in jobs)         # rows in order
    assert sorted(by_launch) == list(range(len(by_launch)))
    for js in by_launch.values():
        assert len(js) <= max_jobs
        i_end = o_end = f_end = 0
        for cnt, in_off, out_cnt, out_off, nf, f_off in js:          # packed back to back, inside the capacities
            assert (in_off, out_off, f_off) == (i_end, o_end, f_end)
            i_end, o_end, f_end = i_end + cnt, o_end + out_cnt, f_end + nf
        assert i_end <= win and o_end <= out_cap and f_end <= frame_cap
    return by_launch


@pytest.mark.parametrize("win", [DEV_STRETCH_WINDOW_MIN, DEV_STRETCH_WINDOW_MIN + 1, 7777, 1 << 23])
@pytest.mark.parametrize("H,D", [(16, 0), (16, 300), (240, 150), (441, 300), (441, 5)])
def test_planner_covers_every_frame_once_with_its_span(prog, win, H, D):
    lens = [4801, 0, 13001, 1, H - 1, H, H + 1, 3 * H + 7]
    for num, den in ((1, 2), (4, 5), (5, 4), (2, 1), (1000, 999)):
        rc, out, err = _run(prog, "plan", num, den, H, D, win, 2 * win, 1 << 18, 2048, *lens)
        assert rc == 0, err
        jobs = [tuple(int(v) for v in ln.split()) for ln in out if ln]
        by_launch = _check_plan(jobs, lens, num, den, H, D, win, 2 * win, 1 << 18, 2048)
        if win == 1 << 23:
            assert len(by_launch) == 1 and len(jobs) == 7            # the empty row has no job
        else:
            assert len(by_launch) >= 13001 / win


def test_planner_respects_the_caps(prog):
    lens = [100, 200, 300, 400, 500, 600, 700]
    rc, out, err = _run(prog, "plan", 4, 5, 16, 5, 1 << 23, 1 << 24, 1 << 18, 3, *lens)
    assert rc == 0, err
    jobs = [tuple(int(v) for v in ln.split()) for ln in out if ln]
    by_launch = _check_plan(jobs, lens, 4, 5, 16, 5, 1 << 23, 1 << 24, 1 << 18, 3)
    assert [len(v) for v in by_launch.values()] == [3, 3, 1]
    for out_cap, frame_cap in ((1000, 1 << 18), (1 << 24, 7)):       # the output and the frame capacities cut as well
        rc, out, err = _run(prog, "plan", 1, 2, 16, 5, 1 << 23, out_cap, frame_cap, 2048, 4801, 333)
        assert rc == 0, err
        jobs = [tuple(int(v) for v in ln.split()) for ln in out if ln]
        assert len(_check_plan(jobs, [4801, 333], 1, 2, 16, 5, 1 << 23, out_cap, frame_cap, 2048)) > 5


def test_planner_refuses_a_window_below_one_frame(prog):
    rc, _, err = _run(prog, "plan", 4, 5, 441, 300, 1000, 1 << 24, 1 << 18, 2048, 4801)
    assert rc == 3 and "no frame fits" in err
    rc, _, err = _run(prog, "plan", 2, 1, 2048, 1024, DEV_STRETCH_WINDOW_MIN, 1 << 24, 1 << 18, 2048, 100000)
    assert rc == 3 and "no frame fits" in err
    assert _run(prog, "plan", 4, 5, 441, 300, 1000, 1 << 24, 1 << 18, 2048, 0)[0] == 0        # nothing to place
