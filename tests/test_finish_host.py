"""CPU: the output stage's host code (csrc/finish_host.h: option checking, threshold, frame-table reduction, fade tables, launch
planner), compiled into the stand-alone program tools/finish_host_check.cpp and run here -- no GPU, no library.  Tables, spans and
counts must equal the numpy restatement (tests/_finish_refs.py) word for word, gains within 1 fp32 ulp (pow may differ between
libraries); the planner must cover every frame and every output element exactly once, inside the capacities it was given."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import vallex_amd  # noqa: F401
from tests import _finish_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    from vallex_amd import _build
    exe = str(tmp_path_factory.mktemp("fn") / "finish_host_check")
    src = os.path.join(ROOT, "tools", "finish_host_check.cpp")
    cxx = shutil.which("g++") or shutil.which("c++")
    cmd = [cxx] if cxx else [_build._hipcc(), "-x", "c++"]
    subprocess.run(cmd + ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", src, "-o", exe], check=True, cwd=ROOT)
    return exe


def _run(prog, *args, stdin=None):
    r = subprocess.run([prog] + [str(a) for a in args], capture_output=True, text=True, input=stdin)
    return r.returncode, r.stdout.split("\n"), r.stderr


def _f32(word):
    return np.array([int(word, 16)], np.uint32).view(np.float32)[0]


def _f64(word):
    return struct.unpack("<d", struct.pack("<Q", int(word, 16)))[0]


@pytest.mark.parametrize("n", [0, 1, 2, 7, 240, 4801, 20000, 1 << 20])
def test_fade_tables_word_for_word(prog, n):
    rc, out, err = _run(prog, "table", n)
    assert rc == 0, err
    got = np.array([int(w, 16) for w in out if w], np.uint32)
    np.testing.assert_array_equal(got, R.fade_table(n).view(np.uint32))


def test_threshold(prog):
    for db in (-40.0, -60.0, 0.0, -33.3, -96.33):
        rc, out, _ = _run(prog, "thr2", db)
        got, want = _f64(out[0]), R.thr2(db)
        assert rc == 0 and abs(got - want) <= abs(want) * 2.0 ** -52, db       # one ulp of a double: pow


def _table_text(x, F):
    e, p, z = R.frames(x, F)
    return "".join(f"{struct.unpack('<Q', struct.pack('<d', float(a)))[0]:016x} {int(np.float32(b).view(np.uint32)):08x} {int(c)}\n"
                   for a, b, c in zip(e, p, z))


@pytest.mark.parametrize("F", R.FRAMES)
def test_spans_and_gains_equal_the_restatement(prog, F):
    rows = R.rows(F)
    rows.append(np.zeros(3 * F + 1, np.float32))                     # all silent
    hot = rows[5].copy()
    hot[F + 3], hot[2] = np.nan, np.inf
    rows.append(hot)
    n = 0
    for x in rows:
        assert R.margin(x, F, -40.0) >= 0.25                         # no frame near the threshold: a last bit of pow cannot flip one
        txt = _table_text(x, F)
        for trim in (0, 1, 2, 3):
            for keep in (0, 5, 100000):
                for mode, level_db, cap in ((R.NONE, -1.0, 20.0), (R.PEAK, -1.0, 20.0), (R.RMS, -20.0, 20.0), (R.RMS, 0.0, 3.0)):
                    rc, out, err = _run(prog, "reduce", F, -40.0, trim, keep, mode, level_db, cap, len(x), stdin=txt)
                    assert rc == 0, err
                    b, e, act, nonf, pk, g, ms = out[0].split()
                    want = R.measure(x, F, silence_db=-40.0, trim=trim, keep=keep, level_mode=mode, level_db=level_db, max_gain_db=cap)
                    assert (int(b), int(e), int(act), int(nonf)) == (want["begin"], want["end"], want["active_frames"], want["nonfinite"])
                    assert _f32(pk).view(np.uint32) == np.float32(want["peak"]).view(np.uint32)
                    assert struct.pack("<d", _f64(ms)) == struct.pack("<d", want["mean_square"])
                    assert R.ulp_diff([_f32(g)], [want["gain"]])[0] <= 1, (trim, keep, mode)
                    n += 1
    assert n == len(rows) * 48


def test_option_ranges(prog):
    ok = dict(frame=240, silence_db=-40.0, trim=3, keep=0, mode=2, level_db=-1.0, max_gain_db=20.0, fade_in=7, fade_out=1 << 20, format=1)
    assert _run(prog, "opts", *ok.values())[:2] == (0, ["ok", ""])
    for field, bad in (("frame", 15), ("frame", 4097), ("silence_db", 0.5), ("silence_db", "nan"), ("silence_db", "-inf"), ("trim", 4),
                       ("trim", -1), ("keep", -1), ("mode", 3), ("mode", -1), ("level_db", 0.1), ("level_db", "inf"),
                       ("max_gain_db", -0.1), ("max_gain_db", "nan"), ("fade_in", -1), ("fade_in", (1 << 20) + 1), ("fade_out", -1),
                       ("fade_out", (1 << 20) + 1), ("format", 2), ("format", -1)):
        rc, out, _ = _run(prog, "opts", *dict(ok, **{field: bad}).values())
        assert rc == 3 and out[0].startswith("level_mode" if field == "mode" else field), (field, bad, out[0])
    for field, edge in (("frame", 16), ("frame", 4096), ("silence_db", 0.0), ("level_db", 0.0), ("max_gain_db", 0.0), ("keep", 2 ** 31 - 1)):
        assert _run(prog, "opts", *dict(ok, **{field: edge}).values())[0] == 0, (field, edge)


@pytest.mark.parametrize("win,max_jobs,frame,spans", [
    (512, 4096, 16, [(0, 4801), (0, 13001), (0, 0), (0, 1), (0, 15)]),
    (513, 4096, 240, [(0, 4801), (0, 13001), (0, 239)]),
    (777, 4096, 441, [(0, 4801), (0, 13001), (0, 442)]),
    (777, 4096, 240, [(0, 4801), (0, 13001)]),
    (512, 4096, 0, [(1000, 4101), (2395, 10085), (5, 5), (0, 1)]),          # the apply pass: kept spans, cut anywhere
    (513, 4096, 0, [(0, 4801), (2491, 9909)]),
    (777, 4096, 0, [(12, 4801), (0, 13001), (7, 8)]),
    (1 << 23, 3, 16, [(0, 10), (0, 20), (0, 30), (0, 40), (0, 50), (0, 60), (0, 70)]),      # the job count cuts
    (1 << 23, 4096, 240, [(0, 4801), (0, 0), (0, 13001)]),              # everything in one launch
])
def test_planner_covers_everything_once(prog, win, max_jobs, frame, spans):
    rc, out, err = _run(prog, "plan", win, max_jobs, frame, *[f"{a}:{b}" for a, b in spans])
    assert rc == 0, err
    jobs = [tuple(int(v) for v in ln.split()) for ln in out if ln]
    nxt = [a for a, _ in spans]
    by_launch = {}
    for launch, row, s_lo, cnt, off, f_off in jobs:
        assert s_lo == nxt[row] and cnt > 0                         # rows in order, samples in order, none twice, none skipped
        nxt[row] = s_lo + cnt
        assert nxt[row] <= spans[row][1]
        if frame:
            assert s_lo % frame == 0                                # a measure job starts at a frame of its row ...
            assert cnt % frame == 0 or nxt[row] == spans[row][1]    # ... and only the row's last frame may be cut
        by_launch.setdefault(launch, []).append((off, cnt, f_off))
    assert nxt == [b for _, b in spans]
    assert [row for _, row, *_ in jobs] == sorted(row for _, row, *_ in jobs)
    assert sorted(by_launch) == list(range(len(by_launch)))
    for js in by_launch.values():
        assert len(js) <= max_jobs
        end = f_end = 0
        for off, cnt, f_off in js:                                  # packed back to back, inside the window
            assert off == end and f_off == f_end
            end += cnt
            f_end += -(-cnt // frame) if frame else 0
        assert end <= win
    if win == 1 << 23 and max_jobs == 4096:
        assert len(by_launch) == 1
    if win < 4801:
        assert len(by_launch) >= sum(b - a for a, b in spans) / win


def test_planner_refuses_a_window_below_one_frame(prog):
    rc, _, err = _run(prog, "plan", 200, 4096, 240, "0:1000")
    assert rc == 3 and "no frame fits" in err
