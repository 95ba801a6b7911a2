"""GPU: the time map (vx_pauses and vx_retime, csrc/retime.hip) against tests/_retime_refs.py, the numpy restatement of the header's
contract, at 8 kHz with hop 80.

Everything is compared word for word: outputs, lengths, positions, the winning cost of every frame as doubles, pause spans.  Nothing
goes through a transcendental but the threshold of the pause rule, which both sides compute from the same double.  One un-finalized
context serves the kernel tests: the entries need no weights.  The restatement of every case is computed once and shared."""
import ctypes as C

import numpy as np
import pytest

from tests import _finish_refs as FR
from tests import _retime_refs as R
from tests import _stretch_refs as S
from vallex_amd import _capi
from vallex_amd._capi import VX_EINVAL, Engine, VallexHipError, _ptr
from vallex_amd.utils.alignment import pause_map

pytestmark = pytest.mark.gpu

H = R.H
SENT_F = np.float32(-1.0e30)
SENT_I = -123456789
SENT_D = -7.5e300


@pytest.fixture(scope="module")
def eng():
    e = Engine(num_layers=2, max_batch=1, max_text=8, max_prompt=8, max_new=8, with_vocos=False)      # created, never finalized
    yield e
    e.close()


@pytest.fixture(scope="module")
def ref():
    """(name, row, anchors, D, (out, pos, cost)) of every case"""
    return [(n, x, an, D, R.retime(x, an, H, D)) for n, x, an, D in R.cases()]


def _opts(hop, search):
    return _capi.vx_retime_opts(C.sizeof(_capi.vx_retime_opts), hop, search)


def _raw(eng, rows, maps, hop, D, pad=5):
    """vx_retime on sentinel-filled outputs: (rc, message, out (n, stride + pad), out_lens, pos (n, pstride + pad), cost likewise)"""
    n = len(rows)
    ln = np.array([len(r) for r in rows], np.int32)
    ws = max(1, int(ln.max()))
    buf = np.zeros((n, ws), np.float32)
    for i, r in enumerate(rows):
        buf[i, : len(r)] = r
    na = np.array([len(m) for m in maps], np.int32)
    ast = 2 * int(na.max()) + 3
    anc = np.full((n, ast), SENT_I, np.int32)
    for i, m in enumerate(maps):
        anc[i, : 2 * len(m)] = np.asarray(m, np.int32).reshape(-1)
    os_ = max(1, max(int(np.asarray(m)[-1, 1]) for m in maps))
    ps = max(1, max(R.frame_count(m, hop) for m in maps))
    out = np.full((n, os_ + pad), SENT_F, np.float32)
    pos = np.full((n, ps + pad), SENT_I, np.int32)
    cost = np.full((n, ps + pad), SENT_D, np.float64)
    ol = np.full(n, -7, np.int32)
    o = _opts(hop, D)
    rc = eng.lib.vx_retime(eng.ctx, _ptr(buf, C.c_float), ws, _ptr(ln, C.c_int32), n, _ptr(anc, C.c_int32), ast, _ptr(na, C.c_int32), C.byref(o),
                           _ptr(out, C.c_float), os_ + pad, _ptr(ol, C.c_int32), _ptr(pos, C.c_int32), _ptr(cost, C.c_double), ps + pad)
    return rc, eng.lib.vx_last_error(eng.ctx).decode(), out, ol, pos, cost


def _same(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    view = {4: np.uint32, 8: np.uint64, 2: np.uint16}[a.dtype.itemsize]
    np.testing.assert_array_equal(a.view(view), b.view(view), err_msg=str(what))


def _check_rows(got, want, what):
    rc, msg, out, ol, pos, cost = got
    assert rc == 0, (what, msg)
    for i, (wo, wp, wc) in enumerate(want):
        assert ol[i] == len(wo), (what, i)
        _same(out[i, : len(wo)], wo, (what, i, "out"))
        _same(pos[i, : len(wp)], wp.astype(np.int32), (what, i, "pos"))
        _same(cost[i, : len(wc)], wc, (what, i, "cost"))
        assert (out[i, len(wo):] == SENT_F).all() and (pos[i, len(wp):] == SENT_I).all() and (cost[i, len(wc):] == SENT_D).all(), (what, i)


def _batches(ref):
    """the cases in batches of five rows that share a search radius; the last batch of a radius is filled up with cases whose maps
    only copy (their words do not depend on it)"""
    copies = [c for c in ref if R.frame_count(c[2], H) == 0]
    out = []
    for D in sorted({c[3] for c in ref}):
        group = [c for c in ref if c[3] == D]
        for i in range(0, len(group), 5):
            b = group[i: i + 5]
            out.append((D, b + [c for c in copies if all(c is not g for g in b)][: 5 - len(b)]))
    assert all(len(b) == 5 for _, b in out)
    return out


def test_cases_cover_the_issue(ref):
    names = {c[0] for c in ref}
    assert {len(c[1]) for c in ref} == {0, 1, 400, 4001, 20011} and {c[3] for c in ref} == {0, 50}
    assert {"identity 400", "many anchors all copy", "4:1", "1:4", "lb = 2H", "rem = 0", "rem = H - 1", "back to back", "non-finite",
            "all-zero walked"} <= names
    by = {c[0]: c for c in ref}
    d = lambda n: np.diff(by[n][2], axis=0)
    assert [1600, 400] in d("4:1").tolist() and [400, 1600] in d("1:4").tolist() and [300, 2 * H] in d("lb = 2H").tolist()
    assert d("rem = 0")[1, 1] % H == 0 and d("rem = H - 1")[1, 1] % H == H - 1
    w = d("back to back")
    assert (w[0, 0] != w[0, 1]) and (w[1, 0] != w[1, 1])
    x, an = by["non-finite"][1], by["non-finite"][2]
    seg = np.searchsorted(an[:, 0], np.flatnonzero(~np.isfinite(x)), side="right") - 1
    assert [bool(d("non-finite")[i, 0] != d("non-finite")[i, 1]) for i in seg] == [False, True, True, False]      # in copies and in walked segments
    assert np.isnan(x[100]) and np.isinf(x[900]) and np.isinf(x[2500]) and np.isnan(x[3300])
    moved = 0
    for c in ref:
        nominal = [[a] + [a + R.seg_nominal(a1 - a, b1 - b, H, k) for k in range(1, (b1 - b) // H)]
                   for (a, b), (a1, b1) in zip(c[2][:-1].tolist(), c[2][1:].tolist()) if a1 - a != b1 - b]
        moved += int((c[4][1] != np.array(sum(nominal, []), np.int64)).sum()) if c[3] == 50 else 0
    assert moved > 100                                               # the search does move frames off their nominal positions


def test_word_for_word_alone_and_across_windows(eng, ref):
    """every case alone, at the default window and at the smallest one, where the segments of a row land in different launches"""
    try:
        for name, x, an, D, want in ref:
            eng.dev_retime_window(0)
            got = _raw(eng, [x], [an], H, D)
            _check_rows(got, [want], (name, "default window"))
            again = _raw(eng, [x], [an], H, D)                        # two calls give the same bits
            for a, b in zip(got[2:], again[2:]):
                _same(a, b, (name, "second call"))
            eng.dev_retime_window(_capi.DEV_RETIME_WINDOW_MIN)
            small = _raw(eng, [x], [an], H, D)
            if name in R.ABOVE_MIN_WINDOW:                           # a walked segment is never cut: refused, nothing written
                assert small[0] == VX_EINVAL and "vx_dev_retime_window" in small[1] and "row 0: segment 0" in small[1], small[1]
                assert (small[2] == SENT_F).all() and small[3][0] == -7 and (small[4] == SENT_I).all() and (small[5] == SENT_D).all()
                continue
            _check_rows(small, [want], (name, "smallest window"))
            for a, b in zip(got[2:], small[2:]):
                _same(a, b, (name, "windows"))
    finally:
        eng.dev_retime_window(0)
    by = {c[0]: c for c in ref}
    for name in ("identity 400", "identity 20011", "many anchors all copy", "one sample"):
        _same(eng.retime([by[name][1]], [by[name][2]], H, 50)[0], by[name][1], name)          # the bits come back
    name, x, an, D, (wo, wp, wc) = by["all-zero walked"]
    a, a1, lb = 1000, 2600, 1000
    assert wp.tolist() == [a] + [a + R.seg_nominal(a1 - a, lb, H, k) for k in range(1, lb // H)]        # the tie rule keeps d = 0
    name, x, an, D, (wo, wp, wc) = by["non-finite"]
    out = eng.retime([x], [an], H, D)[0]
    assert np.isnan(out[100]) and np.isnan(out[3300]) and np.isfinite(np.delete(out, [100, 3300])).all()


def test_word_for_word_in_batches_of_five(eng, ref):
    """the same rows inside ragged batches of five, at the default and at the smallest window: the words of the row alone"""
    try:
        for win in (0, _capi.DEV_RETIME_WINDOW_MIN):
            eng.dev_retime_window(win)
            for D, batch in _batches(ref):
                if win and any(c[0] in R.ABOVE_MIN_WINDOW for c in batch):
                    batch = [c for c in batch if c[0] not in R.ABOVE_MIN_WINDOW]
                got = _raw(eng, [c[1] for c in batch], [c[2] for c in batch], H, D)
                _check_rows(got, [c[4] for c in batch], (win, D, [c[0] for c in batch]))
    finally:
        eng.dev_retime_window(0)


def test_engine_retime_and_other_hops(eng, ref):
    by = {c[0]: c for c in ref}
    rows, maps = [by[n][1] for n in ("4:1", "empty", "back to back")], [by[n][2] for n in ("4:1", "empty", "back to back")]
    out, pos, cost = eng.retime(rows, maps, H, 50, positions=True)
    for i, n in enumerate(("4:1", "empty", "back to back")):
        _same(out[i], by[n][4][0], n)
        _same(pos[i], by[n][4][1].astype(np.int32), n)
        _same(cost[i], by[n][4][2], n)
    assert eng.last_retime_info == [dict(segments=3, walked=1, frames=5, out_len=2801), dict(segments=0, walked=0, frames=0, out_len=0),
                                    dict(segments=3, walked=2, frames=36, out_len=4001)]
    assert [len(o) for o in eng.retime(rows, maps, H, 50)] == [2801, 0, 4001]
    assert eng.retime([], []) == []
    # the largest options (the 24-register prefetch, the largest LDS layout) and a hop that is no multiple of the wavefront
    x = R.voiced(30011, 77, rate=24000)
    for hop, D, an in ((2048, 1024, [(0, 0), (3000, 3000), (20000, 12001), (30011, 22012)]), (441, 300, [(0, 0), (9000, 13999), (30011, 35010)])):
        wo, wp, wc = R.retime(x, an, hop, D)
        go, gp, gc = eng.retime([x], [an], hop, D, positions=True)
        _same(go[0], wo, (hop, D))
        _same(gp[0], wp.astype(np.int32), (hop, D))
        _same(gc[0], wc, (hop, D))


def test_stretch_and_retime_share_their_tables(eng):
    """vx_stretch and vx_retime keep one crossfade table (rebuilt when the hop changes) and one pair of position / cost tables in a
    context.  One row through both, the hops alternating: a table left over from the other stage or the other hop would show in the
    words.  The map has a copy, a walked segment with a searched frame and a pinned end with a tail at both hops, and another copy."""
    x = S.rows(240)[6][:2000]
    an = np.array([(0, 0), (300, 300), (1500, 1200), (2000, 1700)], np.int32)
    assert [(900 // h, 900 % h) for h in (160, 240)] == [(5, 100), (3, 180)]      # frames and tail of the walked segment

    def stretched(costs, hop, D):
        want = S.stretch(x, 4, 5, hop, D)
        if costs:
            out, pos, cost = eng.dev_stretch_costs(x, (4, 5), hop, D)
            _same(cost, want[2], ("stretch", hop, "cost"))
        else:
            (out,), (pos,) = eng.stretch([x], (4, 5), hop, D, return_positions=True)
        _same(out, want[0], ("stretch", hop, "out"))
        _same(pos, want[1].astype(np.int32), ("stretch", hop, "pos"))

    stretched(False, 240, 150)
    _check_rows(_raw(eng, [x], [an], 160, 100), [R.retime(x, an, 160, 100)], "retime 160 behind stretch 240")
    stretched(False, 240, 150)
    _check_rows(_raw(eng, [x], [an], 240, 150), [R.retime(x, an, 240, 150)], "retime 240 behind stretch 240")
    stretched(True, 160, 100)


def test_refusals(eng, ref):
    by = {c[0]: c for c in ref}
    x, an = by["4:1"][1], by["4:1"][2].copy()
    L, Lout, M = len(x), int(an[-1, 1]), R.frame_count(an, H)
    lib, ctx = eng.lib, eng.ctx
    buf = x[None].copy()
    ln = np.array([L], np.int32)
    na = np.array([len(an)], np.int32)
    out = np.full((1, Lout), SENT_F, np.float32)
    pos = np.full((1, M), SENT_I, np.int32)
    cost = np.full((1, M), SENT_D, np.float64)
    ol = np.full(1, -7, np.int32)
    fp, ip, dp = lambda a: _ptr(a, C.c_float), lambda a: _ptr(a, C.c_int32), lambda a: _ptr(a, C.c_double)
    o = C.byref(_opts(H, 50))
    A = lambda m: np.ascontiguousarray(np.asarray(m, np.int32).reshape(1, -1))

    def refused(field, *args):
        rc = lib.vx_retime(ctx, *args)
        msg = lib.vx_last_error(ctx).decode()
        assert rc == VX_EINVAL and field in msg and "vx_retime" in msg, (field, rc, msg)
        assert (out == SENT_F).all() and ol[0] == -7 and (pos == SENT_I).all() and (cost == SENT_D).all(), field    # nothing written

    def check(field, wav=fp(buf), ws=L, lens=ip(ln), batch=1, anchors=an, n=None, ast=None, opts=o, outp=fp(out), ost=Lout, olp=ip(ol),
              posp=ip(pos), costp=dp(cost), pst=M, null=""):
        a = A(anchors)
        n_ = np.array([a.size // 2 if n is None else n], np.int32)
        args = (wav, ws, lens, batch, None if null == "anchors" else ip(a), a.size if ast is None else ast, None if null == "n_anchors" else ip(n_),
                opts, outp, ost, olp, posp, costp, pst)
        if field is None:
            return args, (a, n_)                                      # the arrays stay alive with the caller
        refused(field, *args)

    check("wav", wav=None)
    check("lens", lens=None)
    check("anchors is NULL", null="anchors")
    check("n_anchors is NULL", null="n_anchors")
    check("o is NULL", opts=None)
    check("out is NULL", outp=None)
    check("out_lens", olp=None)
    args, alive = check(None)
    assert lib.vx_retime(None, *args) == VX_EINVAL
    check("batch", batch=0)
    check("batch", batch=-1)
    check("lens[0]", lens=ip(np.array([-1], np.int32)))
    check("wav_stride", lens=ip(np.array([L + 1], np.int32)))
    short = _opts(H, 50)
    short.struct_size -= 4
    check("struct_size", opts=C.byref(short))
    for field, hop, D in (("hop", 15, 50), ("hop", 2049, 50), ("search", H, -1), ("search", H, 1025)):
        check(field, opts=C.byref(_opts(hop, D)))
    check("n_anchors", n=0)
    check("anchor_stride", ast=2 * len(an) - 1)
    check("anchors[0]", anchors=[(1, 0), (L, L)])
    check("anchors[0]", anchors=[(0, 1), (L, L)])
    check("does not increase", anchors=[(0, 0), (500, 500), (500, 600), (L, L)])
    check("does not increase", anchors=[(0, 0), (500, 500), (600, 500), (L, L)])
    check("a_m is not the row's length", anchors=[(0, 0), (L - 1, L - 1)])
    check("a_m is not the row's length", anchors=[(0, 0)])
    check("shorter than 2 hop", anchors=[(0, 0), (159, 200), (L, L + 41)])
    check("shorter than 2 hop", anchors=[(0, 0), (200, 159), (L, L - 41)])
    check("outside 1/4 .. 4", anchors=[(0, 0), (1000, 249), (L, L - 751)])
    check("outside 1/4 .. 4", anchors=[(0, 0), (250, 1001), (L, L + 751)])
    check("out_stride", ost=Lout - 1)
    check("pos_stride", pst=M - 1)
    check("pos_stride", pst=M - 1, posp=None)                      # cost alone needs its records too
    try:
        eng.dev_retime_window(_capi.DEV_RETIME_WINDOW_MIN)
        check("vx_dev_retime_window", anchors=[(0, 0), (2100, 900), (L, L - 1200)], posp=None, costp=None)      # 2230 staged samples above 2048
        for bad in (1, _capi.DEV_RETIME_WINDOW_MIN - 1, -5, _capi.RETIME_WINDOW + 1):
            with pytest.raises(VallexHipError) as ei:
                eng.dev_retime_window(bad)
            assert ei.value.code == VX_EINVAL and "input_samples" in str(ei.value)
    finally:
        eng.dev_retime_window(0)
    with pytest.raises(VallexHipError) as ei:
        eng.retime([x], [[(0, 0), (L, 4 * L + 1)]], H, 50)
    assert ei.value.code == VX_EINVAL and "la / lb" in str(ei.value)
    with pytest.raises(ValueError):
        eng.retime([x], [], H, 50)
    # pos and cost of NULL are allowed, each alone too: the same bits
    args, alive = check(None, posp=None, costp=None, pst=0)
    assert lib.vx_retime(ctx, *args) == 0 and ol[0] == Lout and (pos == SENT_I).all() and (cost == SENT_D).all()
    _same(out[0], by["4:1"][4][0])
    args, alive = check(None, costp=None)
    assert lib.vx_retime(ctx, *args) == 0 and (cost == SENT_D).all()
    _same(pos[0], by["4:1"][4][1].astype(np.int32))
    args, alive = check(None, posp=None)
    pos[:] = SENT_I
    assert lib.vx_retime(ctx, *args) == 0 and (pos == SENT_I).all()
    _same(cost[0], by["4:1"][4][2])


def _pause_rows():
    x, gaps = R.bursts([4800, 4800, 900])
    first = x[400:].copy()                                  # the first frame is active and a pause follows it at frame 25
    one = np.concatenate([x[2320:7280]])                    # one active frame, the pause, one active frame: it touches both ends
    last = x[: 2400 + 4800 + 80].copy()                     # the last frame is the one active frame behind the pause
    quiet = (1e-5 * np.random.default_rng(3).standard_normal(3000)).astype(np.float32)
    lead = np.concatenate([quiet[:800], x[400:2400], quiet[:800]])       # quiet at both ends and no pause inside
    hot = x.copy()
    hot[3000], hot[3001], hot[1000] = np.nan, np.inf, -np.inf
    return [x, first, one, last, quiet, lead, hot, x[:0], x[:1]]


def _raw_pauses(eng, rows, frame, db, mf, keep, stride=None, pad=3):
    n = len(rows)
    ln = np.array([len(r) for r in rows], np.int32)
    ws = max(1, int(ln.max()))
    buf = np.zeros((n, ws), np.float32)
    for i, r in enumerate(rows):
        buf[i, : len(r)] = r
    want = [R.pauses(r, frame, db, mf, keep) for r in rows]
    st = (2 * max(len(w) for w in want) + pad) if stride is None else stride
    spans = np.full((n, max(st, 1)), SENT_I, np.int32)
    counts = np.full(n, -7, np.int32)
    o = _capi.vx_pause_opts(C.sizeof(_capi.vx_pause_opts), frame, db, mf, keep)
    rc = eng.lib.vx_pauses(eng.ctx, _ptr(buf, C.c_float), ws, _ptr(ln, C.c_int32), n, C.byref(o), _ptr(spans, C.c_int32), st, _ptr(counts, C.c_int32))
    return rc, eng.lib.vx_last_error(eng.ctx).decode(), spans, counts, want


def test_pauses_word_for_word(eng):
    rows = _pause_rows()
    found = 0
    try:
        for win in (0, _capi.DEV_FINISH_WINDOW_MIN):         # 512 samples: the frame table of a row is cut inside its pauses
            eng.dev_finish_window(win)
            for frame, db, mf, keep in ((80, -50.0, 1, 0), (80, -50.0, 15, 160), (80, -50.0, 61, 0), (240, -40.0, 2, 30)):
                rc, msg, spans, counts, want = _raw_pauses(eng, rows, frame, db, mf, keep)
                assert rc == 0, msg
                for i, w in enumerate(want):
                    assert counts[i] == len(w), (win, frame, mf, keep, i)
                    np.testing.assert_array_equal(spans[i, : 2 * len(w)], w.reshape(-1), err_msg=str((win, frame, mf, keep, i)))
                    assert (spans[i, 2 * len(w):] == SENT_I).all()
                    found += len(w)
                for i in (1, 2, 6):                          # alone: the same spans
                    rc, msg, s1, c1, w1 = _raw_pauses(eng, [rows[i]], frame, db, mf, keep)
                    assert rc == 0 and c1[0] == len(want[i]), msg
                    np.testing.assert_array_equal(s1[0, : 2 * c1[0]], want[i].reshape(-1))
    finally:
        eng.dev_finish_window(0)
    assert found > 40
    want = [R.pauses(r, 80, -50.0, 1, 0).tolist() for r in rows]
    assert want[1][0] == [2000, 6800] and want[2] == [[80, 4880]] and want[3][-1] == [2400, 7200]       # touching the first / last frame
    assert want[4] == [] and want[5] == [] and want[7] == [] and want[8] == []                           # all quiet; silence at the ends only
    # the detector agrees with trim: every pause lies inside the span vx_finish keeps and holds none of its active frames
    for x, w in zip(rows[:4], want[:4]):
        info = eng.measure([x], 80, -50.0)[0]
        e, _, _ = FR.frames(x, 80)
        active = e > FR.thr2(-50.0) * FR.frame_counts(len(x), 80)
        assert info["active_frames"] == int(active.sum())
        for b, en in w:
            assert info["begin"] <= b - 80 and en + 80 <= info["end"] and not active[b // 80: en // 80].any()
    # Engine.pauses: milliseconds at a rate
    got = eng.pauses(rows, 8000, silence_db=-50.0, min_ms=150.0, keep_ms=20.0)
    for g, x in zip(got, rows):
        np.testing.assert_array_equal(g, R.pauses(x, 80, -50.0, 15, 160))
    assert eng.pauses([], 8000) == []


def test_pauses_refusals(eng):
    rows = _pause_rows()[:2]
    rc, msg, spans, counts, want = _raw_pauses(eng, rows, 80, -50.0, 1, 0, stride=5)
    assert rc == VX_EINVAL and "span_stride" in msg and "row 0" in msg and "6 ints" in msg and "3 pauses" in msg, msg
    assert (spans == SENT_I).all() and (counts == -7).all()
    rc, msg, spans, counts, want = _raw_pauses(eng, [_pause_rows()[2], rows[0]], 80, -50.0, 1, 0, stride=5)      # one pause fits, the second row's three do not
    assert rc == VX_EINVAL and "row 1" in msg and (spans == SENT_I).all() and (counts == -7).all()
    assert _raw_pauses(eng, rows, 80, -50.0, 1, 0, stride=6)[0] == 0
    for field, (frame, db, mf, keep) in (("frame", (15, -50.0, 1, 0)), ("frame", (4097, -50.0, 1, 0)), ("silence_db", (80, 1.0, 1, 0)),
                                         ("silence_db", (80, float("nan"), 1, 0)), ("min_frames", (80, -50.0, 0, 0)), ("keep", (80, -50.0, 1, -1))):
        o = _capi.vx_pause_opts(C.sizeof(_capi.vx_pause_opts), frame, db, mf, keep)
        x = rows[0][None].copy()
        ln = np.array([x.shape[1]], np.int32)
        sp, ct = np.full((1, 16), SENT_I, np.int32), np.full(1, -7, np.int32)
        rc = eng.lib.vx_pauses(eng.ctx, _ptr(x, C.c_float), x.shape[1], _ptr(ln, C.c_int32), 1, C.byref(o), _ptr(sp, C.c_int32), 16, _ptr(ct, C.c_int32))
        msg = eng.lib.vx_last_error(eng.ctx).decode()
        assert rc == VX_EINVAL and field in msg and "vx_pauses" in msg and (sp == SENT_I).all() and ct[0] == -7, (field, msg)
    x = rows[0][None].copy()
    ln = np.array([x.shape[1]], np.int32)
    sp, ct = np.full((1, 16), SENT_I, np.int32), np.full(1, -7, np.int32)
    good = _capi.vx_pause_opts(C.sizeof(_capi.vx_pause_opts), 80, -50.0, 1, 0)
    short = _capi.vx_pause_opts(C.sizeof(_capi.vx_pause_opts) - 4, 80, -50.0, 1, 0)
    fp, ip = lambda a: _ptr(a, C.c_float), lambda a: _ptr(a, C.c_int32)
    for field, args in (("wav", (None, x.shape[1], ip(ln), 1, C.byref(good), ip(sp), 16, ip(ct))),
                        ("lens", (fp(x), x.shape[1], None, 1, C.byref(good), ip(sp), 16, ip(ct))),
                        ("o is NULL", (fp(x), x.shape[1], ip(ln), 1, None, ip(sp), 16, ip(ct))),
                        ("spans is NULL", (fp(x), x.shape[1], ip(ln), 1, C.byref(good), None, 16, ip(ct))),
                        ("counts is NULL", (fp(x), x.shape[1], ip(ln), 1, C.byref(good), ip(sp), 16, None)),
                        ("batch", (fp(x), x.shape[1], ip(ln), 0, C.byref(good), ip(sp), 16, ip(ct))),
                        ("wav_stride", (fp(x), x.shape[1] - 1, ip(ln), 1, C.byref(good), ip(sp), 16, ip(ct))),
                        ("struct_size", (fp(x), x.shape[1], ip(ln), 1, C.byref(short), ip(sp), 16, ip(ct)))):
        rc = eng.lib.vx_pauses(eng.ctx, *args)
        msg = eng.lib.vx_last_error(eng.ctx).decode()
        assert rc == VX_EINVAL and field in msg and "vx_pauses" in msg and (sp == SENT_I).all() and ct[0] == -7, (field, msg)


def test_pauses_then_pause_map_then_retime(eng):
    """the three steps by hand on bursts with 600 ms gaps: the gaps come out at 1600 samples and everything else keeps its bits"""
    x, gaps = R.bursts([4800, 4800, 4800])
    p = eng.pauses([x], 8000, silence_db=-50.0, min_ms=150.0, keep_ms=20.0)[0]
    assert p.tolist() == [[g0 + 160, g1 - 160] for g0, g1 in gaps]
    an = pause_map(len(x), p, max_len=1600, hop=H)
    out = eng.retime([x], [an], H, 50)[0]
    _same(out, R.retime(x, an, H, 50)[0])
    assert len(out) == len(x) - 3 * (4480 - 1600)

    class P:
        max_ms, min_ms, scale, silence_db, at_least_ms, keep_ms = 200.0, None, None, -50.0, 150.0, 20.0
    _same(eng._paused([x], P, 8000)[0], out)
    assert eng._paused([x], None, 8000)[0] is x


def test_generate_audio_batch_with_pauses():
    """one end-to-end cell on the synthetic 2-layer model: pauses=Pauses(...) equals the vocoder output plus Engine.pauses, pause_map and
    Engine.retime applied by hand; pauses=None returns the bits of a call without the argument.  The synthetic vocoder's output has
    no silence of its own, so the threshold is taken from its frame levels: at their 60th percentile, runs of quieter frames between
    louder ones are the 'pauses' of this waveform."""
    from oracle import synth
    from vallex_amd.utils import generation as G
    G.preload_models(state_dict=synth.vallex_state_dict(2, 11), vocos_state_dict=synth.vocos_state_dict(2), num_layers=2, max_new=64,
                     max_prompt=128, max_text=64, max_batch=2)
    e = G.model.engine
    ids = [synth.synth_text(6, 1), synth.synth_text(5, 2)]
    us = synth.uniforms(64, 2, 5)
    kw = dict(language="en", uniforms=us, force_eos_at=40)
    w24 = G.generate_audio_batch(ids, **kw)
    for a, b in zip(G.generate_audio_batch(ids, pauses=None, **kw), w24):
        _same(a, b)

    def by_hand(ws, ps):
        spans = e.pauses(ws, 24000, silence_db=ps.silence_db, min_ms=ps.at_least_ms, keep_ms=ps.keep_ms)
        mf, keep = -(-int(round(ps.at_least_ms * 24)) // 240), int(round(ps.keep_ms * 24))
        for w, sp in zip(ws, spans):
            np.testing.assert_array_equal(sp, R.pauses(w, 240, ps.silence_db, mf, keep))
        maps = [pause_map(len(w), sp, max_len=None if ps.max_ms is None else int(round(ps.max_ms * 24)), hop=240) for w, sp in zip(ws, spans)]
        out = e.retime(ws, maps)
        return out, maps, [r["walked"] for r in e.last_retime_info]

    ps200 = G.Pauses(max_ms=200)                                     # the defaults: -50 dB, 150 ms
    want, maps, walked = by_hand(w24, ps200)
    for a, b in zip(G.generate_audio_batch(ids, pauses=ps200, **kw), want):
        _same(a, b)
    lev = np.concatenate([10.0 * np.log10(np.maximum(FR.frames(w, 240)[0] / 240.0, 1e-30)) for w in w24])
    db = min(0.0, float(np.percentile(lev, 60)))
    ps = G.Pauses(max_ms=20, silence_db=db, at_least_ms=30, keep_ms=0)
    want, maps, walked = by_hand(w24, ps)
    print("lengths:", [len(w) for w in w24], "walked segments per row:", walked, "threshold dB:", db)
    assert sum(walked) >= 1                                          # this cell does walk
    got = G.generate_audio_batch(ids, pauses=ps, **kw)
    for a, b, w, m in zip(got, want, w24, maps):
        _same(a, b)
        _same(b, R.retime(w, m, 240, 150)[0])
        assert len(b) < len(w)
    fin = G.Finish(trim=3, keep=80, level_mode=2, level_db=-20.0, fade_in=32, fade_out=32, pcm16=True)
    fk = {k: getattr(fin, k) for k in ("silence_db", "trim", "keep", "level_mode", "level_db", "max_gain_db", "fade_in", "fade_out", "pcm16")}
    got16 = G.generate_audio_batch(ids, pauses=ps, speed=(5, 4), sample_rate=16000, finish=fin, **kw)
    want16 = e.finish(e.resample(e.stretch(want, (5, 4)), 24000, 16000), 160, **fk)[0]
    for a, b in zip(got16, want16):                                  # behind the vocoder, in front of speed, resample and finish
        _same(a, b)
    w1 = G.generate_audio(ids[0], language="en", uniforms=us[:, 0], force_eos_at=40)
    _same(G.generate_audio(ids[0], language="en", uniforms=us[:, 0], force_eos_at=40, pauses=ps), by_hand([w1], ps)[0][0])
    _same(e.vocos_decode([_codes12()], 2, pauses=None)[0], e.vocos_decode([_codes12()], 2)[0])
    # max_pause_ms= at the enrolment end: behind denoise and pitch, in front of the trim (a stand-in tokenizer returns what it is given)
    from vallex_amd.utils import prompt_making as PM

    class Tok:
        sample_rate = 24000
        encode = staticmethod(lambda wav: wav)

    x, gaps = R.bursts([14400, 2400], burst=6000, lead=1200, tail=1200, rate=24000)
    short = PM.shorten_pauses(x[None], 200.0, 24000)
    hand, maps, walked = by_hand([x], G.Pauses(max_ms=200))
    _same(short[0], hand[0])
    assert walked == [1] and short.shape == (1, len(x) - (14400 - 2 * 480 - 4800))      # 600 ms -> 200 ms inside the guards; 100 ms is no pause
    _same(PM.tokenize_audio(Tok, (x[None], 24000))[0, 0], x)
    _same(PM.tokenize_audio(Tok, (x[None], 24000), max_pause_ms=200.0)[0, 0], short[0])
    _same(PM.tokenize_audio(Tok, (x[None], 24000), max_pause_ms=200.0, trim_db=-50.0)[0, 0], PM.trim_silence(short, -50.0)[0])


def _codes12():
    from tests._util import golden
    return golden("nl2_bestof3")["codes"][0].astype(np.int64)
