"""CPU: the pitch tracker's host code (csrc/f0_host.h: option checking, frame geometry, launch planner, summary, the sequential
reference of the contract), compiled into the stand-alone program tools/f0_host_check.cpp and run here -- no GPU, no library.  The
sequential reference must equal the numpy restatement (tests/_f0_refs.py) word for word; every option range is refused with its field
named; the planner must put every frame of every row into exactly one job, in order, with every sample the job's frames read inside
its span and inside the capacities.  The same program runs the same inputs once more under the address and undefined-behaviour
sanitizers, stand-alone."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import vallex_amd  # noqa: F401
from tests import _f0_refs as R
from vallex_amd._capi import DEV_F0_WINDOW_MIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp, name, extra):
    from vallex_amd import _build
    exe = str(tmp / name)
    src = os.path.join(ROOT, "tools", "f0_host_check.cpp")
    cxx = shutil.which("g++") or shutil.which("c++")
    cmd = [cxx] if cxx else [_build._hipcc(), "-x", "c++"]
    subprocess.run(cmd + ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + extra + [src, "-o", exe], check=True, cwd=ROOT)
    return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def prog(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("f0")
    if request.param == "plain":
        return _build(tmp, "f0_host_check", [])
    return _build(tmp, "f0_host_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _run(prog, *args):
    r = subprocess.run([prog] + [str(a) for a in args], capture_output=True, text=True)
    return r.returncode, r.stdout.split("\n"), r.stderr


def _same(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    view = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    np.testing.assert_array_equal(a.view(view), b.view(view), err_msg=str(what))


def _ref(prog, tmp_path, x, opts, tag):
    rate, H, W, t0, T, thr = opts
    fin, fout = tmp_path / f"{tag}.in", tmp_path / f"{tag}.out"
    np.asarray(x, np.float32).tofile(fin)
    rc, _, err = _run(prog, "ref", rate, H, W, t0, T, repr(float(np.float32(thr))), fin, fout)
    assert rc == 0, err
    raw = fout.read_bytes()
    M, T1 = R.frames(len(x), H), T + 1
    at = 0

    def cut(dtype, n):
        nonlocal at
        v = np.frombuffer(raw, dtype, n, at)
        at += v.nbytes
        return v
    f, lag, ap = cut(np.float32, M), cut(np.int32, M), cut(np.float32, M)
    d, dp = cut(np.float64, M * T1).reshape(M, T1), cut(np.float64, M * T1).reshape(M, T1)
    ints, fl = cut(np.int32, 3), cut(np.float32, 3)
    assert at == len(raw)
    info = dict(frames=int(ints[0]), voiced_frames=int(ints[1]), nonfinite=int(ints[2]), f0_median=float(fl[0]), f0_min=float(fl[1]),
                f0_max=float(fl[2]))
    return f, lag, ap, info, d, dp


def test_sequential_reference_equals_the_restatement_word_for_word(prog, tmp_path):
    voiced = 0
    cases = [(R.SMALL, x) for x in R.rows(40)] + [(R.TINY, x) for x in R.rows(16)]
    cases += [(R.SMALL, R.hot_row(483)), (R.SMALL, np.zeros(200, np.float32)), (R.SMALL, R.huge_row(331)), (R.TINY, R.hot_row(100)),
              (R.SMALL, R.tone(200.0, 8000, 483)), (R.LARGEST, R.tone(101.0, 48000, 2 * 4096 + 5))]
    for i, (opts, x) in enumerate(cases):
        want = R.f0(x, opts, tables=True)
        got = _ref(prog, tmp_path, x, opts, f"c{i}")
        for name, g, w in zip(("f0", "lag", "ap"), got[:3], want[:3]):
            _same(g, w, (i, name))
        assert got[3] == want[3], i
        _same(got[4], want[4], (i, "d"))
        _same(got[5], want[5], (i, "dp"))
        voiced += want[3]["voiced_frames"]
    assert voiced > 20


def test_geometry(prog):
    for rate, H, W, t0, T, _ in (R.SMALL, R.TINY, R.LARGEST, (24000, 240, 600, 48, 400, 0.15), (24000, 241, 601, 48, 401, 0.15)):
        for L in (0, 1, H - 1, H, H + 1, 12 * H + 3, 2 ** 31 - 1):
            M = R.frames(L, H)
            ks = sorted({0, 1, M // 2, max(M - 1, 0)})
            rc, out, err = _run(prog, "geom", rate, H, W, t0, T, L, *ks)
            assert rc == 0, err
            assert out[0].split() == [str(M), str(W + T)]
            assert [int(v) for v in out[1: 1 + len(ks)]] == [R.first(k, H, W, T) for k in ks]
    assert R.first(0, 40, 100, 67) == 20 - 83 and R.first(0, 241, 601, 401) == 120 - 501


def test_option_ranges(prog):
    ok = dict(rate=24000, hop=240, window=600, lag_min=48, lag_max=400, threshold=0.15)
    assert _run(prog, "opts", *ok.values())[:2] == (0, ["ok", ""])
    for field, bad in (("sample_rate", dict(rate=7999)), ("sample_rate", dict(rate=192001)), ("hop", dict(hop=15)), ("hop", dict(hop=4097)),
                       ("window", dict(window=15)), ("window", dict(window=2049)), ("lag_min", dict(lag_min=1)),
                       ("lag_min", dict(lag_min=1024, lag_max=1024)), ("lag_max", dict(lag_max=48)), ("lag_max", dict(lag_max=47)),
                       ("lag_max", dict(lag_max=1025)), ("lag_min", dict(lag_min=-3)), ("threshold", dict(threshold=0.0)),
                       ("threshold", dict(threshold=-0.1)), ("threshold", dict(threshold=1.0000001)), ("threshold", dict(threshold="nan")),
                       ("threshold", dict(threshold="inf"))):
        rc, out, _ = _run(prog, "opts", *dict(ok, **bad).values())
        assert rc == 3 and out[0].startswith(field + " "), (field, bad, out[0])
    for edge in (dict(rate=8000), dict(rate=192000), dict(hop=16), dict(hop=4096), dict(window=16), dict(window=2048),
                 dict(lag_min=2, lag_max=3), dict(lag_min=1023, lag_max=1024), dict(threshold=1.0), dict(threshold=1e-30)):
        assert _run(prog, "opts", *dict(ok, **edge).values())[0] == 0, edge


def _check_plan(jobs, lens, H, W, T, win, frame_cap, max_jobs):
    nxt = [0] * len(lens)
    by_launch = {}
    for launch, row, k0, k1, s_lo, s_hi, in_off, f_off in jobs:
        L = lens[row]
        M = R.frames(L, H)
        assert k0 == nxt[row] and k0 < k1 <= M                       # frames in order, none twice, none skipped
        nxt[row] = k1
        assert 0 <= s_lo <= s_hi <= L
        for k in {k0, (k0 + k1) // 2, k1 - 1}:                       # every sample a frame reads lies in [s_lo, s_hi) or outside the row
            a, b = max(R.first(k, H, W, T), 0), min(R.first(k, H, W, T) + W + T, L)
            assert b <= a or (s_lo <= a and b <= s_hi), (row, k0, k1, k, a, b, s_lo, s_hi)
        by_launch.setdefault(launch, []).append((s_hi - s_lo, in_off, k1 - k0, f_off))
    assert nxt == [R.frames(L, H) for L in lens]                     # every frame in exactly one job
    assert [(j[0], j[1]) for j in jobs] == sorted((j[0], j[1]) for j in jobs)      # launches and rows in order
    assert sorted(by_launch) == list(range(len(by_launch)))
    for js in by_launch.values():
        assert len(js) <= max_jobs
        i_end = f_end = 0
        for cnt, in_off, nf, f_off in js:                            # packed back to back, inside the capacities
            assert (in_off, f_off) == (i_end, f_end)
            i_end, f_end = i_end + cnt, f_end + nf
        assert i_end <= win and f_end <= frame_cap
    return by_launch


@pytest.mark.parametrize("win", [DEV_F0_WINDOW_MIN, DEV_F0_WINDOW_MIN + 1, 7777, 1 << 23])
@pytest.mark.parametrize("opts", [R.SMALL, R.TINY, (24000, 240, 600, 48, 400, 0.15), R.LARGEST])
def test_planner_covers_every_frame_once_with_its_span(prog, win, opts):
    rate, H, W, t0, T, _ = opts
    lens = [4801, 0, 13001, 1, H - 1, H, H + 1, 12 * H + 3]
    rc, out, err = _run(prog, "plan", rate, H, W, t0, T, win, 1 << 20, 4096, *lens)
    assert rc == 0, err
    jobs = [tuple(int(v) for v in ln.split()) for ln in out if ln]
    by_launch = _check_plan(jobs, lens, H, W, T, win, 1 << 20, 4096)
    if win == 1 << 23:
        assert len(by_launch) == 1 and len(jobs) == 7                # the empty row has no job
    elif H < 4096:
        assert len(by_launch) >= 2


def test_planner_respects_the_caps(prog):
    lens = [100, 200, 300, 400, 500, 600, 700]
    rc, out, err = _run(prog, "plan", 8000, 16, 16, 2, 3, 1 << 23, 1 << 20, 3, *lens)
    assert rc == 0, err
    jobs = [tuple(int(v) for v in ln.split()) for ln in out if ln]
    assert [len(v) for v in _check_plan(jobs, lens, 16, 16, 3, 1 << 23, 1 << 20, 3).values()] == [3, 3, 1]
    rc, out, err = _run(prog, "plan", 8000, 16, 16, 2, 3, 1 << 23, 7, 4096, 4801, 333)      # the frame capacity cuts as well
    assert rc == 0, err
    jobs = [tuple(int(v) for v in ln.split()) for ln in out if ln]
    assert len(_check_plan(jobs, [4801, 333], 16, 16, 3, 1 << 23, 7, 4096)) == -(-(301 + 21) // 7)


def test_planner_refuses_a_window_below_one_frame(prog):
    rc, _, err = _run(prog, "plan", 48000, 4096, 2048, 2, 1024, 3071, 1 << 20, 4096, 100000)
    assert rc == 3 and "no frame fits" in err
    assert _run(prog, "plan", 48000, 4096, 2048, 2, 1024, DEV_F0_WINDOW_MIN, 1 << 20, 4096, 100000)[0] == 0
    assert _run(prog, "plan", 48000, 4096, 2048, 2, 1024, 100, 1 << 20, 4096, 0)[0] == 0        # nothing to place
