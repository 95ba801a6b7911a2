"""GPU: the formant-preserving pitch shift (vx_psola, csrc/psola.hip) against tests/_psola_refs.py, the numpy restatement of the
header's contract.

Everything is compared word for word: the analysis marks, the winning cost of every mark and the grain table (vx_dev_psola_table), the
output samples and the infos.  Nothing goes through a transcendental or a library that could differ, so there is no tolerance
anywhere.  One un-finalized context serves all tests: the entry needs no weights.  The restatement of every case is computed once and
shared."""
import ctypes as C

import numpy as np
import pytest

from tests import _psola_refs as R
from vallex_amd import _capi
from vallex_amd._capi import VX_EINVAL, Engine, _ptr

pytestmark = pytest.mark.gpu

SENT_F = np.float32(-1.0e30)
SENT_I = -123456789
INFO = ("marks", "voiced_marks", "grains", "gaps", "nonfinite")


@pytest.fixture(scope="module")
def eng():
    e = Engine(num_layers=2, max_batch=1, max_text=8, max_prompt=8, max_new=8, with_vocos=False)      # created, never finalized
    yield e
    e.close()


@pytest.fixture(scope="module")
def ref():
    """per option set: the cases and the restatement of each"""
    return {name: [(c, R.psola(c[1], c[2], c[3], c[4])) for c in R.cases(name)] for name in ("small", "tiny", "largest")}


def _opts(o):
    return _capi.vx_psola_opts(C.sizeof(_capi.vx_psola_opts), *[int(v) for v in o])


def _same(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    view = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    np.testing.assert_array_equal(a.view(view), b.view(view), err_msg=str(what))


def _raw(eng, rows, lags, o, ratios=None, pad=5, with_marks=True, **kw):
    """vx_psola on sentinel-filled outputs: (rc, message, out (n, stride + pad), marks (n, mstride), info structs).  ratios: per row a
    Q16 array, or an int that fills the row's frames, or None for no `ratio` argument at all."""
    n = len(rows)
    ln = np.array([len(r) for r in rows], np.int32)
    ws = max(1, int(ln.max()))
    buf = np.zeros((n, ws), np.float32)
    for i, r in enumerate(rows):
        buf[i, : len(r)] = r
    fs = max([1] + [len(lg) for lg in lags]) + 2
    lag = np.full((n, fs), 10 ** 6, np.int32)
    rat = None if ratios is None else np.full((n, fs), 7, np.int32)              # 7: out of range behind a row's frames, never read
    for i, lg in enumerate(lags):
        lag[i, : len(lg)] = lg
        if rat is not None:
            rat[i, : len(lg)] = ratios[i]
    out = np.full((n, ws + pad), SENT_F, np.float32)
    ms = ws // 14 + 2 + pad
    marks = np.full((n, ms), SENT_I, np.int32)
    info = (_capi.vx_psola_info * n)()
    for w in info:
        w.marks = SENT_I
    a = dict(wav=_ptr(buf, C.c_float), wav_stride=ws, lens=_ptr(kw.pop("lens_arr", ln), C.c_int32), batch=n, lag=_ptr(lag, C.c_int32),
             lag_stride=fs, ratio=None if rat is None else _ptr(rat, C.c_int32), opts=C.byref(o), out=_ptr(out, C.c_float), out_stride=ws + pad,
             marks=_ptr(marks, C.c_int32) if with_marks else None, marks_stride=ms, info=info)
    a.update(kw)
    rc = eng.lib.vx_psola(eng.ctx, a["wav"], a["wav_stride"], a["lens"], a["batch"], a["lag"], a["lag_stride"], a["ratio"], a["opts"], a["out"],
                          a["out_stride"], a["marks"], a["marks_stride"], a["info"])
    return rc, eng.lib.vx_last_error(eng.ctx).decode(), out, marks, info


def _info(w):
    return {k: getattr(w, k) for k in INFO}


def _check(res, wants, what, with_marks=True):
    rc, msg, out, marks, info = res
    assert rc == 0, msg
    for i, want in enumerate(wants):
        L, N = len(want["out"]), want["info"]["marks"]
        _same(out[i, :L], want["out"], (what, "out", i))
        assert (out[i, L:] == SENT_F).all(), (what, "behind the row", i)
        if with_marks:
            _same(marks[i, : N + 1], want["marks"], (what, "marks", i))
            assert (marks[i, N + 1:] == SENT_I).all(), (what, "behind the marks", i)
        else:
            assert (marks == SENT_I).all()
        assert _info(info[i]) == want["info"], (what, i, _info(info[i]), want["info"])


@pytest.mark.parametrize("name", ["small", "tiny"], ids=["hop80_p16_160_u40", "hop16_p16_24_u16"])
def test_kernels_word_for_word_alone_and_as_one_ragged_batch(eng, ref, name):
    cs = ref[name]
    assert {0, 1, 15, 16, 17, 12 * 80 + 3} <= {len(c[1]) for c, _ in cs}
    assert any(w["info"]["nonfinite"] == 3 for _, w in cs) and any(not c[1].any() and len(c[1]) for c, _ in cs)
    assert max(w["info"]["grains"] for _, w in cs) > 40                    # the jumping lags at ratio 2: many grains over one sample
    for (tag, x, lag, o, per), want in cs:                                 # every case alone
        res = _raw(eng, [x], [lag], _opts(o), None if per is None else [per])
        _check(res, [want], tag)
        cost, gr = eng.dev_psola_table(x, lag, _opts(o), per)
        _same(cost, want["cost"], (tag, "cost"))
        _same(gr, want["grains"], (tag, "grains"))
    # all of them as one ragged batch: the call's ratio is one word, so every row brings its own as a per-frame array
    rows, lags, wants = [c[1] for c, _ in cs], [c[2] for c, _ in cs], [w for _, w in cs]
    ratios = [c[3][4] if c[4] is None else c[4] for c, _ in cs]
    o = _opts(cs[0][0][3][:4] + (65536,))
    first = _raw(eng, rows, lags, o, ratios)
    _check(first, wants, name + " batch")
    again = _raw(eng, rows, lags, o, ratios)
    _same(again[2], first[2], "twice: out")
    _same(again[3], first[3], "twice: marks")
    _check(_raw(eng, rows, lags, o, ratios, with_marks=False), wants, name + " batch without marks", with_marks=False)


def test_largest_options_on_a_row_of_three_periods(eng, ref):
    (tag, x, lag, o, per), want = ref["largest"][0]
    assert len(x) == 3 * 1024 and want["info"]["voiced_marks"] == want["info"]["marks"] >= 3
    _check(_raw(eng, [x], [lag], _opts(o)), [want], tag)
    cost, gr = eng.dev_psola_table(x, lag, _opts(o), per)
    _same(cost, want["cost"], "cost")
    _same(gr, want["grains"], "grains")


def test_ratio_one_and_unvoiced_rows_return_the_samples(eng):
    x, hot = R.vowel(110.0, 700.0, 8000, 963), R.hot_row(483)
    for row in (x, hot):
        sets = R.lag_sets(len(row), R.SMALL)
        y = R.identity(row)
        for lname in ("voiced", "jumping", "alternating"):
            res = _raw(eng, [row], [sets[lname]], _opts(R.SMALL + (65536,)))
            assert res[0] == 0, res[1]
            _same(res[2][0, : len(row)], y, lname)
        for q in R.RATIOS:
            res = _raw(eng, [row], [sets["unvoiced"]], _opts(R.SMALL + (q,)))
            assert res[0] == 0, res[1]
            _same(res[2][0, : len(row)], y, ("unvoiced", q))


def test_a_row_alone_equals_the_row_among_others_and_through_small_windows(eng, ref):
    cs = ref["small"]
    pick = [k for k, (c, _) in enumerate(cs) if len(c[1]) == 963][:8]
    assert len(pick) == 8
    (tag, x, lag, o, per), want = cs[pick[0]]
    o1 = _opts(o[:4] + (65536,))
    others = [cs[k] for k in pick[1:]]
    for place in (0, 3, 7):
        batch = others[:place] + [cs[pick[0]]] + others[place:]
        rows, lags = [c[1] for c, _ in batch], [c[2] for c, _ in batch]
        ratios = [c[3][4] if c[4] is None else c[4] for c, _ in batch]
        res = _raw(eng, rows, lags, o1, ratios)
        _check(res, [w for _, w in batch], ("place", place))
        _same(res[2][place, :963], want["out"], ("the row at", place))
    # the smallest window: 963-sample rows go one per launch, the short ones share launches; every word equals the single pass
    rows, lags, wants = [c[1] for c, _ in cs], [c[2] for c, _ in cs], [w for _, w in cs]
    ratios = [c[3][4] if c[4] is None else c[4] for c, _ in cs]
    assert sum(len(r) for r in rows) > 8 * _capi.DEV_PSOLA_WINDOW_MIN
    eng.dev_psola_window(_capi.DEV_PSOLA_WINDOW_MIN)
    try:
        _check(_raw(eng, rows, lags, o1, ratios), wants, "smallest window")
        big = np.zeros(_capi.DEV_PSOLA_WINDOW_MIN + 1, np.float32)
        rc, msg, out, marks, _ = _raw(eng, [big], [np.full(R.frames(len(big), 80), 60, np.int32)], o1)
        assert rc == VX_EINVAL and "lens[0]" in msg and (out == SENT_F).all() and (marks == SENT_I).all()
    finally:
        eng.dev_psola_window(0)
    for bad in (1, _capi.DEV_PSOLA_WINDOW_MIN - 1, _capi.PSOLA_WINDOW + 1, -1):
        assert eng.lib.vx_dev_psola_window(eng.ctx, bad) == VX_EINVAL
        assert "samples" in eng.lib.vx_last_error(eng.ctx).decode()


REFUSALS = [("hop", dict(hop=15)), ("hop", dict(hop=4097)), ("period_min", dict(period_min=15)), ("period_max", dict(period_max=1025)),
            ("period_max", dict(period_min=100, period_max=99, unvoiced_period=99)), ("unvoiced_period", dict(unvoiced_period=15)),
            ("unvoiced_period", dict(unvoiced_period=161)), ("ratio_q16", dict(ratio_q16=43690)), ("ratio_q16", dict(ratio_q16=131073)),
            ("struct_size", dict(struct_size=20))]


def _untouched(res):
    _, _, out, marks, info = res
    return (out == SENT_F).all() and (marks == SENT_I).all() and all(w.marks == SENT_I for w in info)


@pytest.mark.parametrize("field,change", REFUSALS, ids=[f"{f}_{'_'.join(str(v) for v in c.values())}" for f, c in REFUSALS])
def test_options_are_refused_with_their_field_and_nothing_is_written(eng, field, change):
    x = R.vowel(110.0, 700.0, 8000, 400)
    lag = R.lag_sets(400, R.SMALL)["voiced"]
    o = _opts(R.SMALL + (65536,))
    for k, v in change.items():
        setattr(o, k, v)
    res = _raw(eng, [x], [lag], o)
    assert res[0] == VX_EINVAL and field in res[1], res[:2]
    assert _untouched(res)


def test_arguments_are_refused_with_their_field_and_nothing_is_written(eng):
    x, y = R.vowel(110.0, 700.0, 8000, 400), R.vowel(150.0, 900.0, 8000, 300)
    rows = [x, y]
    lags = [R.lag_sets(400, R.SMALL)["voiced"], R.lag_sets(300, R.SMALL)["jumping"]]
    o = _opts(R.SMALL + (65536,))
    ok = _raw(eng, rows, lags, o)
    assert ok[0] == 0, ok[1]
    N = max(_info(w)["marks"] for w in ok[4])
    cases = [("wav", dict(wav=None)), ("lens", dict(lens=None)), ("lag", dict(lag=None)), ("o is", dict(opts=None)), ("out", dict(out=None)),
             ("info", dict(info=None)), ("batch", dict(batch=0)), ("batch", dict(batch=-1)),
             ("lens[1]", dict(lens_arr=np.array([400, -1], np.int32))), ("lens[0]", dict(lens_arr=np.array([401, 300], np.int32))),
             ("lag_stride", dict(lag_stride=4)), ("out_stride", dict(out_stride=399)), ("marks_stride", dict(marks_stride=N))]
    for field, kw in cases:
        res = _raw(eng, rows, lags, o, **kw)
        assert res[0] == VX_EINVAL and field in res[1], (field, res[:2])
        assert _untouched(res), field
    for bad, at in ((43690, 0), (131073, 4)):                                    # a ratio element within a row's frames
        per = [np.full(len(lags[0]), 65536, np.int32), np.full(len(lags[1]), 65536, np.int32)]
        per[1][at if at < len(per[1]) else -1] = bad
        res = _raw(eng, rows, lags, o, per)
        assert res[0] == VX_EINVAL and "ratio[1]" in res[1], res[:2]
        assert _untouched(res)
    assert _raw(eng, rows, lags, o, marks_stride=N + 1)[0] == 0                  # N + 1 marks fit exactly
    # the dev table: capacities below N + 1 / J, nothing written
    lag = lags[0]
    cost, gr = eng.dev_psola_table(x, lag, o)
    cbuf, gbuf = np.full(len(cost), -1.0), np.full((len(gr), 4), SENT_I, np.int32)
    nm, ng = C.c_int32(SENT_I), C.c_int32(SENT_I)
    for ccap, gcap, field in ((len(cost) - 1, len(gr), "cost_cap"), (len(cost), len(gr) - 1, "grain_cap")):
        rc = eng.lib.vx_dev_psola_table(eng.ctx, _ptr(x, C.c_float), len(x), _ptr(lag, C.c_int32), None, C.byref(o), _ptr(cbuf, C.c_double), ccap,
                                        _ptr(gbuf, C.c_int32), gcap, C.byref(nm), C.byref(ng))
        assert rc == VX_EINVAL and field in eng.lib.vx_last_error(eng.ctx).decode()
        assert (cbuf == -1.0).all() and (gbuf == SENT_I).all() and nm.value == SENT_I and ng.value == SENT_I


def test_python_refusals_come_before_any_call():
    class NoLaunch(Engine):
        def __init__(self):                                            # no context: any launch would fail on the missing attributes
            pass

        def __del__(self):
            pass
    e = NoLaunch()
    x = np.zeros(400, np.float32)
    lag = np.full(5, 60, np.int32)
    for kw in (dict(hop=8), dict(ratio=0.6), dict(ratio=2.01), dict(ratio=float("nan")), dict(period_min=8), dict(period_max=2000),
               dict(unvoiced_period=10), dict(contour=[np.full(5, 43690, np.int32)]), dict(contour=[np.full(4, 65536, np.int32)]),
               dict(contour=[]), dict(lags=[lag[:4]]), dict(lags=[])):
        a = dict(wavs=[x], lags=[lag], hop=80, period_min=16, period_max=160, unvoiced_period=40)
        a.update(kw)
        with pytest.raises(ValueError):
            e.psola(**a)
    for kw in (dict(pitch=(1, 2), formants=True), dict(pitch=3.0, range=0.5), dict(pitch=3.0, formants=True, range=-1.0),
               dict(pitch=3.0, formants=True, range=float("inf")), dict(pitch=13.0, formants=True)):
        with pytest.raises(ValueError):
            e.shift([x], **kw)
