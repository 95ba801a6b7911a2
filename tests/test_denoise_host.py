"""CPU: the host code of the noise suppression (csrc/denoise_host.h: tables, option checking, frame counts, K, the choice of the noise
frames with its ties, launch planner, the sequential reference of the contract), compiled into the stand-alone program
tools/denoise_host_check.cpp and run here -- no GPU, no library.  The sequential reference must equal the numpy restatement
(tests/_denoise_refs.py) word for word on the program's own tables; every option range is refused with its field named and accepted
at its edges; the planner must put every row into exactly one launch, in order, inside the capacities.  The same program runs the same
inputs once more under the address and undefined-behaviour sanitizers, stand-alone."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import vallex_amd  # noqa: F401
from tests import _denoise_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp, name, extra):
    from vallex_amd import _build
    exe = str(tmp / name)
    src = os.path.join(ROOT, "tools", "denoise_host_check.cpp")
    cxx = shutil.which("g++") or shutil.which("c++")
    cmd = [cxx] if cxx else [_build._hipcc(), "-x", "c++"]
    subprocess.run(cmd + ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + extra + [src, "-o", exe], check=True, cwd=ROOT)
    return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def prog(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("denoise")
    if request.param == "plain":
        return _build(tmp, "denoise_host_check", [])
    return _build(tmp, "denoise_host_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _run(prog, *args):
    r = subprocess.run([prog] + [str(a) for a in args], capture_output=True, text=True)
    return r.returncode, r.stdout.split("\n"), r.stderr


def _tables(prog, tmp_path):
    rc, _, err = _run(prog, "tables", tmp_path / "tab")
    assert rc == 0, err
    return np.fromfile(tmp_path / "tab", np.float64)


def _ref(prog, tmp_path, x, o, psd, tag):
    fin, fpsd, fout = tmp_path / f"{tag}.in", tmp_path / f"{tag}.psd", tmp_path / f"{tag}.out"
    np.asarray(x, np.float32).tofile(fin)
    if psd is not None:
        np.asarray(psd, np.float64).tofile(fpsd)
    rc, _, err = _run(prog, "ref", *[repr(float(np.float32(v))) for v in o[:3]], o[3], 0 if psd is None else 1, fin, fpsd, fout)
    assert rc == 0, err
    raw = fout.read_bytes()
    at = 0

    def cut(dtype, n):
        nonlocal at
        v = np.frombuffer(raw, dtype, n, at)
        at += v.nbytes
        return v
    info = dict(zip(("frames", "full_frames", "k", "nonfinite"), (int(v) for v in cut(np.int32, 4))))
    T = info["frames"]
    sel = cut(np.int32, int(cut(np.int32, 1)[0]))
    P, E, Nz, g = cut(np.float64, T * R.B).reshape(T, R.B), cut(np.float64, T), cut(np.float64, R.B), cut(np.float64, T * R.B).reshape(T, R.B)
    out = cut(np.float32, len(x))
    assert at == len(raw)
    return dict(out=out, P=P, E=E, sel=sel, psd=Nz, gain=g, info=info)


def test_tables_are_numpys_to_one_ulp(prog, tmp_path):
    got, want = _tables(prog, tmp_path), R.tables()
    assert got.shape == want.shape and (np.abs(got - want) <= np.spacing(np.abs(want))).all()


def test_sequential_reference_equals_the_restatement_word_for_word(prog, tmp_path):
    tab = _tables(prog, tmp_path)
    cases = [(f"len{len(x)}", x, R.DEFAULTS, None) for x in R.length_rows()]
    cases.append(("odd", R.odd_row(), R.DEFAULTS, None))
    cases.append(("zero", np.zeros(700, np.float32), R.DEFAULTS, None))
    cases.append(("strong", R.length_rows()[-1], (7.5, 0.01, 0.5, 0), None))
    cases.append(("nothing_chosen", R.length_rows()[-1], (2.0, 0.5, 0.0, 0), None))
    cases.append(("identity", R.length_rows()[-1], (0.0, 1.0, 1.0, 3), None))
    cases.append(("given", R.length_rows()[-1], R.DEFAULTS, R.denoise(R.length_rows(seed=8)[-1], R.DEFAULTS, tab)["psd"]))
    for tag, x, o, psd in cases:
        got, want = _ref(prog, tmp_path, x, o, psd, tag), R.denoise(x, o, tab, psd)
        assert got["info"] == want["info"], (tag, got["info"], want["info"])
        assert list(got["sel"]) == list(want["sel"]), tag
        for key in ("P", "E", "psd", "gain", "out"):
            R.same(got[key], want[key], (tag, key))


EDGES = [((0.0, 1.0, 0.0, 0), None), ((3.0e38, 1e-30, 1.0, 2 ** 31 - 1), None), ((2.0, 0.126, 0.1, 8), None),
         ((-0.001, 0.126, 0.1, 8), "alpha"), (("nan", 0.126, 0.1, 8), "alpha"), (("inf", 0.126, 0.1, 8), "alpha"),
         ((2.0, 0.0, 0.1, 8), "floor"), ((2.0, 1.001, 0.1, 8), "floor"), ((2.0, "nan", 0.1, 8), "floor"), ((2.0, -0.5, 0.1, 8), "floor"),
         ((2.0, 0.126, -0.001, 8), "frac"), ((2.0, 0.126, 1.001, 8), "frac"), ((2.0, 0.126, "nan", 8), "frac"),
         ((2.0, 0.126, 0.1, -1), "kmin")]


@pytest.mark.parametrize("o,field", EDGES, ids=["_".join(map(str, o)) for o, _ in EDGES])
def test_every_option_range_at_its_edges(prog, o, field):
    rc, out, _ = _run(prog, "opts", *o)
    if field is None:
        assert rc == 0 and out[0] == "ok", out
    else:
        assert rc == 3 and out[0].startswith(field + " "), out


def test_frame_counts_and_k(prog):
    lens = list(R.LENGTHS) + [383, 384, 511, 640, 48000, 1 << 22]
    for o in (R.DEFAULTS, (2.0, 0.5, 1.0, 0), (2.0, 0.5, 0.0, 0), (2.0, 0.5, 0.5, 3)):
        rc, out, err = _run(prog, "k", *[repr(float(np.float32(v))) for v in o[:3]], o[3], *lens)
        assert rc == 0, err
        got = [tuple(int(v) for v in ln.split()) for ln in out if ln.strip()]
        assert got == [(R.frames(L), R.full(L), R.k_of(o, R.full(L))) for L in lens], o
    assert R.frames(1 << 22) == 32771 and R.full(384) == 0 and R.full(512) == 1


def test_selection_and_its_ties(prog, tmp_path):
    rng = np.random.default_rng(2)
    for L, K in ((1024, 1), (1024, 3), (1024, 5), (1024, 9), (1024, 0), (300, 2), (3000, 8)):
        T = R.frames(L)
        for name, E in (("ties", rng.integers(0, 3, T).astype(np.float64)), ("distinct", rng.random(T)), ("equal", np.ones(T))):
            E.tofile(tmp_path / "E")
            rc, out, err = _run(prog, "select", L, K, tmp_path / "E")
            assert rc == 0, err
            assert [int(v) for v in out if v.strip()] == list(R.select(E, L, K)), (L, K, name)


def _plan(prog, win, frame_cap, max_jobs, lens):
    rc, out, err = _run(prog, "plan", win, frame_cap, max_jobs, *lens)
    return rc, [tuple(int(v) for v in ln.split()) for ln in out if ln.strip()], err


def test_planner_puts_every_row_into_exactly_one_launch(prog):
    lens = [0, 963, 1, 3000, 17, 500, 524, 0, 0, 1000, 128, 1]
    big = 1 << 30
    for win, fc, mj in ((3072, big, big), (1 << 22, big, big), (1 << 22, 30, big), (1 << 22, big, 2), (3072, 30, 3)):
        rc, jobs, err = _plan(prog, win, fc, mj, lens)
        assert rc == 0, err
        assert [j[1] for j in jobs] == list(range(len(lens)))                       # every row once, in order
        launches = [j[0] for j in jobs]
        assert launches[0] == 0 and all(b - a in (0, 1) for a, b in zip(launches, launches[1:]))
        for launch in set(launches):
            mine = [j for j in jobs if j[0] == launch]
            at = [0, 0, 0]
            for _, row, in_off, f_off, h_off in mine:                               # packed without holes or overlap
                L = lens[row]
                assert [in_off, f_off, h_off] == at, (win, row)
                at = [at[0] + L, at[1] + R.frames(L), at[2] + -(-L // R.H)]
            assert at[0] <= win and at[1] <= fc and len(mine) <= mj
        if win == 3072:
            assert len(set(launches)) >= 3
    rc, _, err = _plan(prog, 3072, big, big, [5, 3073])
    assert rc == 3 and "does not fit" in err
    rc, _, err = _plan(prog, 1 << 22, 26, big, [5, 3000])
    assert rc == 3 and "does not fit" in err
    rc, jobs, _ = _plan(prog, 3072, big, big, [])
    assert rc == 0 and jobs == []
