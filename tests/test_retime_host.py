"""CPU: the time map's host code (csrc/retime_host.h: option checking, pause reduction, anchor checks, frames and nominal positions,
launch planner), compiled into the stand-alone program tools/retime_host_check.cpp and run here -- no GPU, no library.  Pauses,
anchor verdicts and the program's sequential walk must equal the numpy restatement (tests/_retime_refs.py) word for word; the planner
must make every walked segment exactly one job, partition the copy spans into tiles, stage every sample a job reads and stay inside
the window and the caps.  The same program runs the same inputs once more under the address and undefined-behaviour sanitizers,
stand-alone."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import vallex_amd  # noqa: F401
from tests import _retime_refs as R
from vallex_amd._capi import DEV_RETIME_WINDOW_MIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = R.H


def _build(tmp, name, extra):
    from vallex_amd import _build
    exe = str(tmp / name)
    src = os.path.join(ROOT, "tools", "retime_host_check.cpp")
    cxx = shutil.which("g++") or shutil.which("c++")
    cmd = [cxx] if cxx else [_build._hipcc(), "-x", "c++"]
    subprocess.run(cmd + ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + extra + [src, "-o", exe], check=True, cwd=ROOT)
    return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def prog(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("rt")
    if request.param == "plain":
        return _build(tmp, "retime_host_check", [])
    return _build(tmp, "retime_host_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _run(prog, *args):
    r = subprocess.run([prog] + [str(a) for a in args], capture_output=True, text=True)
    return r.returncode, r.stdout.split("\n"), r.stderr


def test_option_ranges(prog):
    assert _run(prog, "popts", 80, -50, 1, 0)[:2] == (0, ["ok", ""])
    for field, args in (("frame", (15, -50, 1, 0)), ("frame", (4097, -50, 1, 0)), ("silence_db", (80, 1, 1, 0)), ("silence_db", (80, "nan", 1, 0)),
                        ("silence_db", (80, "-inf", 1, 0)), ("min_frames", (80, -50, 0, 0)), ("keep", (80, -50, 1, -1))):
        rc, out, _ = _run(prog, "popts", *args)
        assert rc == 3 and out[0].startswith(field + " "), (field, args, out[0])
    for ok in ((16, 0, 1, 0), (4096, -120, 1000, 100000)):
        assert _run(prog, "popts", *ok)[0] == 0, ok
    assert _run(prog, "opts", 80, 50)[:2] == (0, ["ok", ""])
    for field, args in (("hop", (15, 5)), ("hop", (2049, 5)), ("search", (80, -1)), ("search", (80, 1025))):
        rc, out, _ = _run(prog, "opts", *args)
        assert rc == 3 and out[0].startswith(field + " "), (field, args, out[0])
    for ok in ((16, 0), (2048, 1024)):
        assert _run(prog, "opts", *ok)[0] == 0, ok


def _pause_rows():
    x, _ = R.bursts([4800, 4800, 900])
    first = x[400:].copy()                                  # the first frame is active, a pause follows
    only = np.concatenate([x[2320:2400], x[2400:7200], x[7200:7280]])      # one active frame, a pause, one active frame
    quiet = (1e-5 * np.random.default_rng(3).standard_normal(3000)).astype(np.float32)
    hot = x.copy()
    hot[3000], hot[3001], hot[1000] = np.nan, np.inf, -np.inf
    return [x, first, only, quiet, hot, x[:0], x[:1], x[: 7 * 80 + 3]]


def test_pauses_equal_the_restatement(prog, tmp_path):
    n = 0
    for i, x in enumerate(_pause_rows()):
        path = tmp_path / f"row{i}.f32"
        x.tofile(path)
        for F, db, mf, keep in ((80, -50.0, 1, 0), (80, -50.0, 15, 160), (80, -50.0, 12, 480), (80, -50.0, 61, 0), (240, -40.0, 2, 30), (16, -60.0, 3, 8)):
            rc, out, err = _run(prog, "pauses", path, F, db, mf, keep)
            assert rc == 0, err
            got = np.array([[int(v) for v in ln.split()] for ln in out if ln], np.int32).reshape(-1, 2)
            np.testing.assert_array_equal(got, R.pauses(x, F, db, mf, keep), err_msg=str((i, F, db, mf, keep)))
            n += len(got)
    assert n > 20


def _flat(an):
    return [int(v) for v in np.asarray(an).reshape(-1)]


def test_anchor_checks_equal_the_restatement(prog):
    for name, x, an, _ in R.cases():
        rc, out, _ = _run(prog, "anchors", H, len(x), *_flat(an))
        assert rc == 0 and out[0].split() == ["ok", str(int(an[-1, 1])), str(R.frame_count(an, H))], (name, out[0])
    L = 4001
    bad = [
        ([(1, 0), (L, L)], "anchors[0]"), ([(0, 1), (L, L)], "anchors[0]"),
        ([(0, 0), (500, 500), (500, 600), (L, L)], "anchors[2]"), ([(0, 0), (500, 500), (600, 500), (L, L)], "anchors[2]"),
        ([(0, 0), (500, 500), (400, 600), (L, L)], "anchors[2]"),
        ([(0, 0), (L - 1, L - 1)], "anchors[1]"), ([(0, 0), (L + 1, L + 1)], "anchors[1]"), ([(0, 0)], "anchors[0]"),
        ([(0, 0), (159, 200), (L, L)], "segment 0 is walked"), ([(0, 0), (200, 159), (L, L)], "segment 0 is walked"),
        ([(0, 0), (1000, 1000), (2000, 1249), (L, L)], "segment 1: la / lb"), ([(0, 0), (1000, 1000), (1250, 2001), (L, L)], "segment 1: la / lb"),
    ]
    for an, want in bad:
        assert (R.check_anchors(an, L, H) or "").startswith(want), (an, R.check_anchors(an, L, H))
        rc, out, _ = _run(prog, "anchors", H, L, *_flat(an))
        assert rc == 3 and out[0].startswith(want), (an, out[0])
    rc, out, _ = _run(prog, "anchors", H, 0)
    assert rc == 3 and out[0].startswith("n_anchors")
    for an in ([(0, 0), (160, 161), (L, L + 1)], [(0, 0), (1000, 250), (L, L - 750)], [(0, 0), (250, 1000), (L, L + 750)]):      # the edges
        assert R.check_anchors(an, L, H) is None
        assert _run(prog, "anchors", H, L, *_flat(an))[0] == 0, an
    big = 2 ** 31 - 1
    rc, out, _ = _run(prog, "anchors", 2048, big, 0, 0, big, big // 4 + 1)
    assert rc == 0 and out[0].split() == ["ok", str(big // 4 + 1), str((big // 4 + 1) // 2048)]


def _check_plan(jobs, rows, D, win, out_cap, frame_cap, max_jobs, tile):
    by_launch, by_row = {}, {}
    assert [j[0] for j in jobs] == sorted(j[0] for j in jobs)
    for j in jobs:
        by_launch.setdefault(j[0], []).append(j)
        by_row.setdefault(j[1], []).append(j)
    assert sorted(by_launch) == list(range(len(by_launch)))
    for js in by_launch.values():
        assert len(js) <= max_jobs
        i_end = o_end = f_end = 0
        for _, _, walk, a, a1, b, lb, s_lo, s_hi, in_off, out_off, f_off, f_row in js:      # packed back to back, inside the capacities
            assert (in_off, out_off, f_off) == (i_end, o_end, f_end)
            i_end, o_end, f_end = i_end + s_hi - s_lo, o_end + lb, f_end + (lb // H if walk else 0)
        assert i_end <= win and o_end <= out_cap and f_end <= frame_cap
    for r, (L, an) in enumerate(rows):
        js = by_row.get(r, [])
        walked = [(int(a), int(a1), int(b), int(b1 - b)) for (a, b), (a1, b1) in zip(an[:-1], an[1:]) if a1 - a != b1 - b]
        copies = [(int(a), int(a1), int(b)) for (a, b), (a1, b1) in zip(an[:-1], an[1:]) if a1 - a == b1 - b]
        wj = [j for j in js if j[2] == 1]
        assert [(j[3], j[4], j[5], j[6]) for j in wj] == walked                      # every walked segment is exactly one job, in order
        f_row = 0
        for (_, _, _, a, a1, b, lb, s_lo, s_hi, _, _, _, fr) in wj:
            assert (s_lo, s_hi) == (max(0, a - D), min(L, a1 + D + H)) and fr == f_row
            f_row += lb // H
            for k in range(1, lb // H):                                              # every region a frame loads is staged
                n = a + R.seg_nominal(a1 - a, lb, H, k)
                assert a <= n <= a1 - H
                lo, hi = max(n - D, 0), min(n + D + 2 * H, L)
                assert hi <= lo or (s_lo <= lo and hi <= s_hi)
        cj = sorted((j[3], j[4], j[5], j[6], j[7], j[8]) for j in js if j[2] == 0)
        covered = np.zeros(L, np.int32)
        want_out = np.full(L, -1, np.int64)
        for a, a1, b in copies:
            want_out[a:a1] = np.arange(b, b + a1 - a)
        for a, a1, b, lb, s_lo, s_hi in cj:                                          # the copy tiles partition the copy spans
            assert 0 < a1 - a == lb <= tile and (s_lo, s_hi) == (a, a1)
            covered[a:a1] += 1
            np.testing.assert_array_equal(want_out[a:a1], np.arange(b, b + lb))
        np.testing.assert_array_equal(covered, (want_out >= 0).astype(np.int32))
    return by_launch


def _plan(prog, tmp_path, rows, D, win, out_cap, frame_cap, max_jobs, tile):
    path = tmp_path / "rows.txt"
    path.write_text("".join(f"{L} {len(an)} " + " ".join(str(v) for v in _flat(an)) + "\n" for L, an in rows))
    rc, out, err = _run(prog, "plan", H, D, win, out_cap, frame_cap, max_jobs, tile, path)
    return rc, [tuple(int(v) for v in ln.split()) for ln in out if ln], err


@pytest.mark.parametrize("win", [DEV_RETIME_WINDOW_MIN, 5000, 1 << 23])
@pytest.mark.parametrize("D", [0, 50])
def test_planner_invariants(prog, tmp_path, win, D):
    cases = [c for c in R.cases() if c[0] not in R.ABOVE_MIN_WINDOW]                 # that one is above the small windows: refused below
    rows = [(len(x), an) for _, x, an, _ in cases]
    for tile in (16384, 1000):
        rc, jobs, err = _plan(prog, tmp_path, rows, D, win, 2 * win, 1 << 18, 2048, tile)
        assert rc == 0, err
        by_launch = _check_plan(jobs, rows, D, win, 2 * win, 1 << 18, 2048, tile)
        if win == 1 << 23:
            assert len(by_launch) == 1
        else:
            assert len(by_launch) >= sum(L for L, _ in rows) / win


def test_planner_respects_the_caps_and_refuses_a_segment_above_the_window(prog, tmp_path):
    cases = R.cases()
    rows = [(len(x), an) for _, x, an, _ in cases]
    for out_cap, frame_cap, max_jobs in ((21000, 1 << 18, 2048), (1 << 24, 201, 2048), (1 << 24, 1 << 18, 3)):
        rc, jobs, err = _plan(prog, tmp_path, rows, 50, 1 << 23, out_cap, frame_cap, max_jobs, 16384)
        assert rc == 0, err
        assert len(_check_plan(jobs, rows, 50, 1 << 23, out_cap, frame_cap, max_jobs, 16384)) > 2
    whole = [(len(x), an) for n, x, an, _ in cases if n in ("identity 400", "whole row walked")]
    rc, _, err = _plan(prog, tmp_path, whole, 50, 5000, 1 << 24, 1 << 18, 2048, 16384)
    assert rc == 3 and "row 1 segment 0" in err
    rc, _, err = _plan(prog, tmp_path, whole, 50, 1 << 23, 16008, 1 << 18, 2048, 16384)        # its outputs above the cap
    assert rc == 3 and "row 1 segment 0" in err
    rc, _, err = _plan(prog, tmp_path, whole, 50, 1 << 23, 1 << 24, 199, 2048, 16384)          # its 200 frames above the cap
    assert rc == 3 and "row 1 segment 0" in err
    rc, jobs, err = _plan(prog, tmp_path, whole, 50, 20011, 16009, 200, 1, 16384)              # ... and exactly inside all of them
    assert rc == 0 and len(jobs) == 2, err


def test_sequential_walk_equals_the_restatement(prog, tmp_path):
    frames = 0
    for i, (name, x, an, D) in enumerate(R.cases()):
        if name in ("whole row walked", "many walked", "identity 20011"):
            continue                                         # the long ones: the device tests compare them; here the loop is sequential
        want, wpos, wcost = R.retime(x, an, H, D)
        src, dst = tmp_path / f"in{i}.f32", tmp_path / f"out{i}.bin"
        x.tofile(src)
        rc, out, err = _run(prog, "walk", src, dst, H, D, *_flat(an))
        assert rc == 0, err
        assert out[0].split() == [str(len(want)), str(len(wpos))]
        raw = dst.read_bytes()
        n, m = len(want), len(wpos)
        assert len(raw) == 4 * n + 12 * m
        np.testing.assert_array_equal(np.frombuffer(raw[: 4 * n], np.uint32), want.view(np.uint32), err_msg=name)
        np.testing.assert_array_equal(np.frombuffer(raw[4 * n: 4 * n + 4 * m], np.int32), wpos.astype(np.int32), err_msg=name)
        np.testing.assert_array_equal(np.frombuffer(raw[4 * n + 4 * m:], np.uint64), wcost.view(np.uint64), err_msg=name)
        frames += m
    assert frames >= 100                                     # the walk did run
