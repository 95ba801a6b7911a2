"""CPU: the host code of the formant-preserving pitch shift (csrc/psola_host.h: option checking, period lookup, synthesis marks and
grain table, gap count, launch planner, the sequential reference of the contract), compiled into the stand-alone program
tools/psola_host_check.cpp and run here -- no GPU, no library.  The sequential reference must equal the numpy restatement
(tests/_psola_refs.py) word for word; every option range is refused with its field named and accepted at its edges; the planner must
put every row into exactly one launch, in order, inside the capacities.  The same program runs the same inputs once more under the
address and undefined-behaviour sanitizers, stand-alone."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import vallex_amd  # noqa: F401
from tests import _psola_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp, name, extra):
    from vallex_amd import _build
    exe = str(tmp / name)
    src = os.path.join(ROOT, "tools", "psola_host_check.cpp")
    cxx = shutil.which("g++") or shutil.which("c++")
    cmd = [cxx] if cxx else [_build._hipcc(), "-x", "c++"]
    subprocess.run(cmd + ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + extra + [src, "-o", exe], check=True, cwd=ROOT)
    return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def prog(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("psola")
    if request.param == "plain":
        return _build(tmp, "psola_host_check", [])
    return _build(tmp, "psola_host_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _run(prog, *args):
    r = subprocess.run([prog] + [str(a) for a in args], capture_output=True, text=True)
    return r.returncode, r.stdout.split("\n"), r.stderr


def _same(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    view = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    np.testing.assert_array_equal(a.view(view), b.view(view), err_msg=str(what))


def _ref(prog, tmp_path, x, lag, o, ratio, tag):
    fin, flag, fout = tmp_path / f"{tag}.in", tmp_path / f"{tag}.lag", tmp_path / f"{tag}.out"
    np.asarray(x, np.float32).tofile(fin)
    words = np.asarray(lag, np.int32) if ratio is None else np.concatenate([np.asarray(lag, np.int32), np.asarray(ratio, np.int32)])
    words.tofile(flag)
    rc, _, err = _run(prog, "ref", *o, 0 if ratio is None else 1, fin, flag, fout)
    assert rc == 0, err
    raw = fout.read_bytes()
    at = 0

    def cut(dtype, n):
        nonlocal at
        v = np.frombuffer(raw, dtype, n, at)
        at += v.nbytes
        return v
    ints = cut(np.int32, 5)
    info = dict(zip(("marks", "voiced_marks", "grains", "gaps", "nonfinite"), (int(v) for v in ints)))
    mk, cost = cut(np.int32, info["marks"] + 1), cut(np.float64, info["marks"] + 1)
    gr, out = cut(np.int32, 4 * info["grains"]).reshape(-1, 4), cut(np.float32, len(x))
    assert at == len(raw)
    return dict(out=out, marks=mk, cost=cost, grains=gr, info=info)


def _cases():
    return R.cases("small") + R.cases("tiny") + R.cases("largest")


def test_sequential_reference_equals_the_restatement_word_for_word(prog, tmp_path):
    for tag, x, lag, o, per in _cases():
        got, want = _ref(prog, tmp_path, x, lag, o, per, tag), R.psola(x, lag, o, per)
        assert got["info"] == want["info"], (tag, got["info"], want["info"])
        for key in ("marks", "cost", "grains", "out"):
            _same(got[key], want[key], (tag, key))


EDGES = [((16, 16, 16, 16, 43691), None), ((4096, 1024, 1024, 1024, 131072), None), ((16, 16, 1024, 16, 65536), None),
         ((15, 16, 160, 40, 65536), "hop"), ((4097, 16, 160, 40, 65536), "hop"),
         ((80, 15, 160, 40, 65536), "period_min"), ((80, 1025, 1025, 1025, 65536), "period_min"),
         ((80, 48, 47, 47, 65536), "period_max"), ((80, 16, 1025, 40, 65536), "period_max"),
         ((80, 16, 160, 15, 65536), "unvoiced_period"), ((80, 16, 160, 161, 65536), "unvoiced_period"),
         ((80, 16, 160, 40, 43690), "ratio_q16"), ((80, 16, 160, 40, 131073), "ratio_q16")]


@pytest.mark.parametrize("o,field", EDGES, ids=[f"{'_'.join(map(str, o))}" for o, _ in EDGES])
def test_every_option_range_at_its_edges(prog, o, field):
    rc, out, _ = _run(prog, "opts", *o)
    if field is None:
        assert rc == 0 and out[0] == "ok", out
    else:
        assert rc == 3 and out[0].startswith(field + " "), out


def _plan(prog, o4, win, mark_cap, grain_cap, lag_cap, max_jobs, lens):
    rc, out, err = _run(prog, "plan", *o4, win, mark_cap, grain_cap, lag_cap, max_jobs, *lens)
    return rc, [tuple(int(v) for v in ln.split()) for ln in out if ln.strip()], err


def test_planner_puts_every_row_into_exactly_one_launch(prog):
    lens = [0, 963, 1, 1024, 17, 500, 524, 0, 0, 1000, 24, 1]
    big = 1 << 30
    for win, mc, gc, lc, mj in ((1024, big, big, big, big), (1 << 23, big, big, big, big), (1 << 23, 80, big, big, big),
                                (1 << 23, big, 150, big, big), (1 << 23, big, big, 14, big), (1 << 23, big, big, big, 2)):
        rc, jobs, err = _plan(prog, R.SMALL, win, mc, gc, lc, mj, lens)
        assert rc == 0, err
        assert [j[1] for j in jobs] == list(range(len(lens)))                       # every row once, in order
        launches = [j[0] for j in jobs]
        assert launches[0] == 0 and all(b - a in (0, 1) for a, b in zip(launches, launches[1:]))
        for launch in set(launches):
            mine = [j for j in jobs if j[0] == launch]
            at = [0, 0, 0, 0]
            for _, row, in_off, lag_off, m_off, g_off in mine:                      # packed without holes or overlap
                L = lens[row]
                assert [in_off, lag_off, m_off, g_off] == at, (win, row)
                at = [at[0] + L, at[1] + R.frames(L, R.SMALL[0]), at[2] + L // 14 + 2, at[3] + L // 7 + 2]
            assert at[0] <= win and at[2] <= mc and at[3] <= gc and at[1] <= lc and len(mine) <= mj
        if win == 1024:
            assert len(set(launches)) >= 5
    rc, _, err = _plan(prog, R.SMALL, 1024, big, big, big, big, [5, 1025])
    assert rc == 3 and "does not fit" in err
    rc, jobs, _ = _plan(prog, R.SMALL, 1024, big, big, big, big, [])
    assert rc == 0 and jobs == []


def test_bounds_of_marks_and_grains_hold_on_the_test_rows(prog, tmp_path):
    """L / 14 + 2 marks and L / 7 + 2 grains: what the planner reserves and the dev header promises"""
    for tag, x, lag, o, per in _cases():
        got = R.psola(x, lag, o, per)
        assert len(got["marks"]) <= len(x) // 14 + 2 and len(got["grains"]) <= len(x) // 7 + 2, tag
