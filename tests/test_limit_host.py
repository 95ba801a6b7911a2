"""CPU: the limiter's host code (csrc/limit_host.h: option checking, taps, ceiling, gain, launch planner and the sequential reference of
the contract), compiled into the stand-alone program tools/limit_host_check.cpp and run here -- no GPU, no library.  The reference must
equal the numpy restatement (tests/_limit_refs.py) word for word at the ceiling the program reports; the taps must be the resampler's;
the planner must cover every sample exactly once, in order, every part holding its halos, inside the capacities it was given."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import vallex_amd  # noqa: F401
from tests import _limit_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "limit_host_check.cpp")


def _compile(exe, *flags):
    from vallex_amd import _build
    cxx = shutil.which("g++") or shutil.which("c++")
    cmd = [cxx] if cxx else [_build._hipcc(), "-x", "c++"]
    subprocess.run(cmd + ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, SRC, "-o", exe], check=True, cwd=ROOT)
    return exe


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return _compile(str(tmp_path_factory.mktemp("lm") / "limit_host_check"))


def _run(prog, *args, stdin=None):
    r = subprocess.run([prog] + [str(a) for a in args], capture_output=True, text=True, input=stdin)
    return r.returncode, r.stdout.split("\n"), r.stderr


def _hex32(v):
    return f"{int(np.float32(v).view(np.uint32)):08x}"


def _f32(words):
    return np.array([int(w, 16) for w in words], np.uint32).view(np.float32)


def _taps(prog, n):
    rc, out, _ = _run(prog, "taps", n)
    assert rc == 0
    return out[0], _f32([w for w in out[1:] if w]).reshape(-1, 15)


def test_taps_are_the_resamplers(prog):
    for n in (2, 4, 8):
        geom, t = _taps(prog, n)
        assert geom == "7 15" and t.shape == (n, 15)
        assert np.array_equal(t.view(np.uint32), R.RS.taps(1, n).view(np.uint32)), n
    assert _taps(prog, 1)[1].shape == (0, 15)
    for bad in (0, 3, 16, -4):
        assert _run(prog, "taps", bad)[0] == 3


def _ref(prog, x, gs, db, Wn, n):
    txt = "".join(_hex32(v) + "\n" for v in x)
    rc, out, err = _run(prog, "ref", _hex32(gs), db, Wn, n, len(x), stdin=txt)
    assert rc == 0, err
    head = out[0].split()
    rows = [ln.split() for ln in out[1:] if ln]
    assert len(rows) == len(x)
    cols = [_f32([r[k] for r in rows]) if rows else np.zeros(0, np.float32) for k in range(3)]
    info = dict(ceiling=_f32(head[:1])[0], peak=_f32(head[1:2])[0], min_gain=_f32(head[2:3])[0], reduced=int(head[3]), nonfinite=int(head[4]))
    return cols, info


def test_reference_equals_the_restatement_word_for_word(prog):
    cases = 0
    for Wn in (1, 3, 16):
        rows = R.cpu_rows(Wn)
        for n in (1, 2, 4, 8):
            tp = _taps(prog, n)[1]
            for name, x in rows.items():
                gs, db = ((1.0, -1.0), (2.5, -1.0), (2.5, 0.0))[cases % 3]
                (out, P, g), info = _ref(prog, x, gs, db, Wn, n)
                want = R.limit(x, gs, info["ceiling"], Wn, n, tp)
                assert R.ulp_diff([info["ceiling"]], [R.ceiling(db)])[0] <= 1
                for got, key in ((out, "out"), (P, "P"), (g, "g")):
                    assert np.array_equal(R.bits(got), R.bits(want[key])), (Wn, n, name, key)
                for key in ("peak", "min_gain"):
                    assert R.bits(info[key]) == R.bits(want[key]), (Wn, n, name, key)
                assert (info["reduced"], info["nonfinite"]) == (want["reduced"], want["nonfinite"])
                cases += 1
    assert cases == (12 + 13 + 13) * 4                                    # at lookahead 1 the lengths Wn and 1 coincide


def test_gain_drops_the_ceiling_term(prog):
    for loud, target, cap in ((-20.0, -16.0, 20.0), (-60.0, -16.0, 20.0), (-10.0, -16.0, 20.0), (-23.456, -14.0, 6.0), (float("-inf"), -16.0, 20.0)):
        w = f"{struct.unpack('<Q', struct.pack('<d', loud))[0]:016x}"
        rc, out, _ = _run(prog, "gain", w, target, cap)
        assert rc == 0 and R.ulp_diff(_f32(out[:1]), [R.gain(loud, target, cap)])[0] <= 1, (loud, out)


def test_option_ranges(prog):
    ok = dict(pre_gain=1.0, ceiling_db=-1.0, lookahead=120, oversample=4)
    assert _run(prog, "opts", *ok.values())[:2] == (0, ["ok", ""])
    for field, bad in (("pre_gain", 0.0), ("pre_gain", -1.0), ("pre_gain", "nan"), ("pre_gain", "inf"), ("ceiling_db", 0.1), ("ceiling_db", "nan"),
                       ("ceiling_db", "inf"), ("ceiling_db", "-inf"), ("lookahead", 0), ("lookahead", 1025), ("lookahead", -5),
                       ("oversample", 0), ("oversample", 3), ("oversample", 16), ("oversample", -4)):
        rc, out, _ = _run(prog, "opts", *dict(ok, **{field: bad}).values())
        assert rc == 3 and out[0].startswith(field), (field, bad, out[0])
    for field, edge in (("pre_gain", 1e-30), ("pre_gain", 3e38), ("ceiling_db", 0.0), ("ceiling_db", -120.0), ("lookahead", 1), ("lookahead", 1024),
                        ("oversample", 1), ("oversample", 2), ("oversample", 8)):
        assert _run(prog, "opts", *dict(ok, **{field: edge}).values())[0] == 0, (field, edge)


@pytest.mark.parametrize("Wn,win,max_jobs,tile,lens", [
    (120, 8192, 4096, 2048, [20000, 0, 1, 8192, 500]),
    (120, 9000, 4096, 2048, [20000, 7000, 3000]),
    (1024, 8192, 4096, 2048, [30000, 5]),
    (16, 1237, 4096, 100, [5000, 1237, 1238, 0, 77]),                      # a window that is no multiple of anything
    (3, 1 << 23, 3, 2048, [10, 20, 30, 40, 50, 60, 70]),                    # the job cap cuts
    (120, 1 << 23, 4096, 2048, [192000, 0, 48000]),                        # everything in one launch
    (1024, 4111, 4096, 2048, [9000]),                                       # the smallest window: one sample per cut part
])
def test_planner_covers_every_sample_once(prog, Wn, win, max_jobs, tile, lens):
    H = 2 * Wn + 7
    rc, out, err = _run(prog, "plan", Wn, win, max_jobs, tile, *lens)
    assert rc == 0, err
    jobs = [tuple(int(v) for v in ln.split()) for ln in out if ln]
    nxt = [0] * len(lens)
    by_launch = {}
    for launch, row, s, cnt, hl, hr, off, out_off, rec_off in jobs:
        L = lens[row]
        assert s == nxt[row] and cnt > 0                                    # rows in order, samples in order, none twice, none skipped
        assert hl == min(H, s) and hr == min(H, L - s - cnt)                # real samples on both sides, cut to the row
        nxt[row] = s + cnt
        by_launch.setdefault(launch, []).append((off, hl + cnt + hr, out_off, cnt, rec_off, -(-cnt // tile)))
    assert nxt == list(lens)
    assert [j[1] for j in jobs] == sorted(j[1] for j in jobs)
    assert sorted(by_launch) == list(range(len(by_launch)))
    for js in by_launch.values():
        assert len(js) <= max_jobs
        end = o_end = r_end = 0
        for off, size, out_off, cnt, rec_off, nrec in js:                   # packed back to back, inside the window
            assert (off, out_off, rec_off) == (end, o_end, r_end)
            end += size
            o_end += cnt
            r_end += nrec
        assert end <= win
    if win == 1 << 23 and max_jobs == 4096:
        assert len(by_launch) == 1
    if win < 10000:
        assert len(by_launch) >= sum(lens) / win


def test_planner_refuses_a_window_below_two_halos_and_a_sample(prog):
    rc, _, err = _run(prog, "plan", 1024, 4110, 4096, 2048, 9000)
    assert rc == 3 and "two halos" in err
    assert _run(prog, "plan", 1024, 4111, 4096, 2048, 9000)[0] == 0
    assert _run(prog, "plan", 1, 18, 4096, 2048, 100)[0] == 3 and _run(prog, "plan", 1, 19, 4096, 2048, 100)[0] == 0


def test_the_program_runs_clean_under_sanitizers(tmp_path):
    """the same program under AddressSanitizer and UBSan (host code only; nothing here is loaded into Python)"""
    exe = _compile(str(tmp_path / "limit_host_check_san"), "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    rows = R.cpu_rows(3)
    for args, stdin in ((("taps", 8), None), (("taps", 1), None), (("opts", 1.0, -1.0, 120, 4), None), (("gain", "c030000000000000", -16.0, 20.0), None),
                        (("ref", _hex32(2.5), -1.0, 3, 4, len(rows["nonfinite"])), "".join(_hex32(v) + "\n" for v in rows["nonfinite"])),
                        (("ref", _hex32(1.0), -1.0, 16, 1, len(rows["edges"])), "".join(_hex32(v) + "\n" for v in rows["edges"])),
                        (("ref", _hex32(1.0), 0.0, 1024, 8, 0), ""), (("ref", _hex32(1.0), -1.0, 5, 2, 1), _hex32(3.0) + "\n"),
                        (("plan", 120, 8192, 4096, 2048, 20000, 0, 1, 8192), None), (("plan", 1024, 4111, 2, 2048, 9000, 1), None)):
        rc, out, err = _run(exe, *args, stdin=stdin)
        assert rc == 0 and "runtime error" not in err and "Sanitizer" not in err, (args, err)
