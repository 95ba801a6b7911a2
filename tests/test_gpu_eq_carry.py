"""GPU: the carried-state equaliser (vx_eq_carry, csrc/eq_carry.hip) against tests/_eq_carry_refs.py, the numpy restatement of the
header's contract, on the coefficients the library designs.

Outputs, end states, counts and peaks are compared word for word: the contract fixes every operation of the three passes, so there is
no tolerance on them.  The two places with one are the ones the header names: a row filtered in two calls against the one call, and the
carried stage against vx_eq on filters both accept; both bounds are 2^-24 of the input peak per truncation plus the rounding of the
outputs.  Sc comes from vx_eq_carry_plan and is never written down here.  One engine serves all tests; the restatement of every row
is computed once."""
import ctypes as C
import types

import numpy as np
import pytest

from tests import _eq_carry_refs as R
from tests import _eq_refs as E
from vallex_amd import _capi
from vallex_amd._capi import VX_EINVAL, Engine, _ptr
from vallex_amd.utils.generation import CarriedEq, Eq

pytestmark = pytest.mark.gpu

SENT_F = np.float32(-1.0e30)
SENT_D = -1.0e300
U = 2.0 ** -24
INFO = ("warm", "nonfinite", "nonfinite_out", "peak")
FILTERS = {"hum 50 x 1 Q 100": Eq.hum(50.0, 1, 100.0), "hum 60 x 4 Q 30 + rumble": Eq.hum(60.0, 4, 30.0) + Eq.rumble(),
           "hum 50 x 8 Q 100": Eq.hum(50.0, 8, 100.0)}


@pytest.fixture(scope="module")
def eng():
    from tests._util import get_model
    return get_model(2, 0, 2.5, vocos=True).engine


@pytest.fixture(scope="module")
def filt():
    """name -> sections; Sc"""
    f = {k: e.sections(24000) for k, e in FILTERS.items()}
    assert [len(s) for s in f.values()] == [1, 5, 8]
    return f, Engine.eq_carry_plan(E.IDENTITY)[1]


def _same(got, want, tag=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (tag, got.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=str(tag))


def _same64(got, want, tag=""):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64), err_msg=str(tag))


def _info_same(got, want, tag=""):
    assert {k: got[k] for k in INFO[:3]} == {k: want[k] for k in INFO[:3]}, (tag, got, want)
    assert np.float32(got["peak"]).view(np.uint32) == np.float32(want["peak"]).view(np.uint32), (tag, got, want)


def _rows(Sc):
    """the ragged batch: 0, 1, Sc - 1, Sc, Sc + 1, 5000 and 20011 samples of hum + noise + DC, with NaN / +-Inf in the long ones"""
    rows = [R.hum_row(L, dc=0.05, seed=60 + i)[0] for i, L in enumerate((0, 1, Sc - 1, Sc, Sc + 1, 5000, 20011))]
    rows[2][[0, Sc - 2]] = [np.nan, np.inf]
    rows[5][[7, Sc - 1, Sc, 4999]] = [np.inf, np.nan, -np.inf, np.nan]
    rows[6][[0, 3 * Sc + 5, 20011 // Sc // 2 * Sc, 20010]] = [-np.inf, np.nan, np.inf, np.nan]
    return rows


def _states(name, n, D):
    return None if name == "rest" else np.random.default_rng(77).standard_normal((n, D))


@pytest.fixture(scope="module")
def refs(filt):
    """(filter, "rest" | "state") -> the restatement (out, state_out, info) of every row of the batch"""
    f, Sc = filt
    rows = _rows(Sc)
    out = {}
    for name, s in f.items():
        m = R.matrix(s, Sc)
        for st in ("rest", "state"):
            z = _states(st, len(rows), 2 * len(s))
            out[(name, st)] = [R.eq_carry(x, s, Sc, None if z is None else z[i], m) for i, x in enumerate(rows)]
    return rows, out


def _check_batch(eng, s, rows, z, want, tag):
    got, sout = eng.eq_carry(rows, s, state=z, return_state=True)
    infos = eng.last_eq_info
    for i, (w, ws, wi) in enumerate(want):
        _same(got[i], w, (tag, i))
        _same64(sout[i], ws, (tag, i))
        _info_same(infos[i], wi, (tag, i))
        assert np.isfinite(got[i]).all() and infos[i]["warm"] == 0
    return got, sout, infos


@pytest.mark.parametrize("start", ["rest", "state"])
@pytest.mark.parametrize("name", sorted(FILTERS))
def test_ragged_batch_word_for_word(eng, filt, refs, name, start):
    f, Sc = filt
    rows, want = refs
    z = _states(start, len(rows), 2 * len(f[name]))
    got, sout, infos = _check_batch(eng, f[name], rows, z, want[(name, start)], (name, start))
    assert len(got[0]) == 0 and infos[0]["peak"] == 0.0 and sum(i["nonfinite"] for i in infos) == 10
    _same64(sout[0], np.zeros_like(sout[0]) if z is None else z[0])       # a row of length 0 hands its state_in on
    np.testing.assert_array_equal(Engine.eq_carry_plan(f[name])[0].view(np.uint64), R.matrix(f[name], Sc).view(np.uint64))


@pytest.mark.parametrize("name", sorted(FILTERS))
def test_smallest_window_gives_the_same_bits(eng, filt, refs, name):
    """many launches per row: the 20011-sample row is cut at step multiples and the chain's z carried on the device"""
    f, Sc = filt
    rows, want = refs
    assert _capi.DEV_EQ_WINDOW_MIN < 5000
    eng.dev_eq_window(_capi.DEV_EQ_WINDOW_MIN)
    try:
        for start in ("rest", "state"):
            _check_batch(eng, f[name], rows, _states(start, len(rows), 2 * len(f[name])), want[(name, start)], (name, start, "window"))
    finally:
        eng.dev_eq_window(0)


def test_every_row_alone_has_the_bits_it_had_in_the_batch(eng, filt, refs):
    f, Sc = filt
    rows, want = refs
    name = "hum 60 x 4 Q 30 + rumble"
    z = _states("state", len(rows), 2 * len(f[name]))
    for i, x in enumerate(rows):
        _check_batch(eng, f[name], [x], z[i: i + 1], want[(name, "state")][i: i + 1], (name, i, "alone"))
    assert eng.eq_carry([], f[name]) == [] and eng.last_eq_info == []


@pytest.mark.parametrize("name", sorted(FILTERS))
def test_two_calls_with_the_state_handed_over(eng, filt, refs, name):
    """the 20011-sample row cut at 40 Sc (at a step above 250 samples that lies behind the row: then at half its steps): within
    2^-24 peak(x) + 2^-24 |y| of the one call (in fact within rounding in double: the outputs are almost always the same fp32 words),
    the end states within 1e-9 relative to the state's largest component (not component by component: a component near 0 has no
    digits to agree in)"""
    f, Sc = filt
    rows, _ = refs
    x, s = rows[6], f[name]
    cut = min(40, len(x) // Sc // 2) * Sc
    one, zone = eng.eq_carry([x], s, return_state=True)
    a, za = eng.eq_carry([x[:cut]], s, return_state=True)
    b, zb = eng.eq_carry([x[cut:]], s, state=za, return_state=True)
    two = np.concatenate([a[0], b[0]]).astype(np.float64)
    y = one[0].astype(np.float64)
    peak = float(np.abs(x[np.isfinite(x)]).max())
    d = np.abs(two - y)
    print(f"{name}: largest distance of the two calls {d.max():.3e} (bound {U * peak:.3e} + 2^-24 |y|), "
          f"end state {np.abs(zb - zone).max() / np.abs(zone).max():.3e} relative")
    assert (d <= U * peak + U * np.abs(y)).all(), (name, float(d.max()))
    assert np.abs(zb - zone).max() <= 1e-9 * np.abs(zone).max(), (name, zb, zone)
    _same(a[0], one[0][:cut], name)                                  # in front of the cut the steps are the one call's


def test_short_filters_agree_with_vx_eq(eng):
    """the six filters vx_eq's W table was drawn up with: carried against Engine.eq within 2 x 2^-24 peak(x) + 2^-24 |y|: the
    truncation of the one (vx_eq's bound, at most 2^-24 peak) plus the one rounding of both outputs (half an fp32 ulp each)"""
    x = E.noise_row(12000, seed=33, dc=0.3)
    peak = float(np.abs(x).max())
    for name, rate, specs in E.FILTERS:
        eq = Eq(specs)
        plain = eng.eq([x], eq, sample_rate=rate)[0].astype(np.float64)
        car = eng.eq_carry([x], eq, sample_rate=rate)[0].astype(np.float64)
        d = np.abs(car - plain)
        print(f"{name}: largest distance {d.max():.3e}")
        assert (d <= 2 * U * peak + U * np.abs(plain)).all(), (name, float(d.max()))
        assert eng.last_eq_info[0]["warm"] == 0


def test_refusals_write_nothing(eng, filt):
    f, Sc = filt
    s = f["hum 50 x 1 Q 100"]
    x = E.noise_row(Sc, seed=91)
    out = np.full(Sc, SENT_F, np.float32)
    sout = np.full(2, SENT_D)
    lens = np.array([Sc], np.int32)
    info = (_capi.vx_eq_info * 1)()
    info[0].warm = -7
    px, po, pl, ps, pz = _ptr(x, C.c_float), _ptr(out, C.c_float), _ptr(lens, C.c_int32), _ptr(s, C.c_double), _ptr(sout, C.c_double)
    unstable = np.array([[1.0, 0.0, 0.0, 0.0, 1.0]])
    nan = np.array([[1.0, np.nan, 0.0, 0.0, 0.0]])
    neg = np.array([-1], np.int32)
    zbad = [np.array([0.0, np.nan]), np.array([np.inf, 0.0])]
    for args, why in (((None, Sc, pl, 1, ps, 1, None, po, Sc, pz, info), "wav"), ((px, Sc, None, 1, ps, 1, None, po, Sc, pz, info), "lens"),
                      ((px, Sc, pl, 0, ps, 1, None, po, Sc, pz, info), "batch"), ((px, Sc, pl, 1, None, 1, None, po, Sc, pz, info), "sections"),
                      ((px, Sc, pl, 1, ps, 1, None, None, Sc, pz, info), "out"), ((px, Sc, pl, 1, ps, 1, None, po, Sc, pz, None), "info"),
                      ((px, Sc - 1, pl, 1, ps, 1, None, po, Sc, pz, info), "wav_stride"), ((px, Sc, pl, 1, ps, 1, None, po, Sc - 1, pz, info), "out_stride"),
                      ((px, Sc, _ptr(neg, C.c_int32), 1, ps, 1, None, po, Sc, pz, info), "lens"),
                      ((px, Sc, pl, 1, ps, 0, None, po, Sc, pz, info), "nsections 0"), ((px, Sc, pl, 1, ps, 9, None, po, Sc, pz, info), "nsections 9"),
                      ((px, Sc, pl, 1, _ptr(unstable, C.c_double), 1, None, po, Sc, pz, info), "section 0 is unstable"),
                      ((px, Sc, pl, 1, _ptr(nan, C.c_double), 1, None, po, Sc, pz, info), "section 0: coefficient 1"),
                      ((px, Sc, pl, 1, ps, 1, _ptr(zbad[0], C.c_double), po, Sc, pz, info), "state_in of row 0: component 1"),
                      ((px, Sc, pl, 1, ps, 1, _ptr(zbad[1], C.c_double), po, Sc, pz, info), "state_in of row 0: component 0")):
        assert eng.lib.vx_eq_carry(eng.ctx, *args) == VX_EINVAL, why
        msg = eng.lib.vx_last_error(eng.ctx).decode()
        assert why in msg and "vx_eq_carry" in msg, (why, msg)
        assert (out == SENT_F).all() and (sout == SENT_D).all() and info[0].warm == -7      # nothing written
    m = np.full((2, 2), SENT_D)
    st = C.c_int32(-7)
    for a in ((None, 1, _ptr(m, C.c_double), C.byref(st)), (ps, 1, None, C.byref(st)), (ps, 1, _ptr(m, C.c_double), None),
              (_ptr(unstable, C.c_double), 1, _ptr(m, C.c_double), C.byref(st)), (ps, 0, _ptr(m, C.c_double), C.byref(st))):
        assert eng.lib.vx_eq_carry_plan(*a) == VX_EINVAL and eng.lib.vx_eq_last_error() != b""
        assert st.value == -7
    with pytest.raises(ValueError, match="unstable"):
        eng.eq_carry([x], unstable)
    with pytest.raises(ValueError, match="state of shape"):
        eng.eq_carry([x], s, state=np.zeros((1, 4)))
    with pytest.raises(_capi.VallexHipError, match="state_in"):
        eng.eq_carry([x], s, state=np.array([[np.nan, 0.0]]))
    # the stage still works, without a state_out too
    lib_out = np.full(Sc, SENT_F, np.float32)
    assert eng.lib.vx_eq_carry(eng.ctx, px, Sc, pl, 1, ps, 1, None, _ptr(lib_out, C.c_float), Sc, None, info) == 0
    _same(lib_out, R.eq_carry(x, s, Sc)[0])


def test_through_python_priming_and_both_audio_ends(eng, monkeypatch, tmp_path):
    from tests._util import golden
    from vallex_amd.utils import generation as G
    from vallex_amd.utils import prompt_making as PM
    hum = Eq.hum()
    assert isinstance(hum, CarriedEq) and hum.prime_hz == 50.0
    s = hum.sections(24000)
    Sc = Engine.eq_carry_plan(s)[1]
    x, _ = R.hum_row(72000, seed=35)                                      # 3 s
    want, wstate, winfo = R.primed(x, s, Sc, 24000, 50.0)
    got, state = eng.eq_carry([x], hum, return_state=True)
    _same(got[0], want)
    _same64(state[0], wstate)
    _info_same(eng.last_eq_info[0], winfo)
    rest = eng.eq_carry([x], s)[0]                                        # sections carry no prime_hz: from rest
    _same(rest, R.eq_carry(x, s, Sc)[0])
    _same(eng.eq_carry([x], hum.carried(), state=np.zeros((1, 12)))[0], rest)      # a given state is the state
    lvl = lambda v: 10 * np.log10(np.mean(v[:6000].astype(np.float64) ** 2))
    assert lvl(rest) > lvl(got[0]) + 10                                   # the notches ring in from rest, not when primed

    calls = []
    real_carry, real_eq = eng.eq_carry, eng.eq
    monkeypatch.setattr(eng, "eq_carry", lambda *a, **k: (calls.append("eq_carry"), real_carry(*a, **k))[1])
    monkeypatch.setattr(eng, "eq", lambda *a, **k: (calls.append("eq"), real_eq(*a, **k))[1])
    codes = [golden("nl2_bestof3")["codes"][0].astype(np.int64)]
    w24 = [w.copy() for w in eng.vocos_decode(codes, 2)]
    out = eng.vocos_decode(codes, 2, eq=hum)
    assert calls == ["eq_carry"]                                          # 3840 samples are below ten periods: no lead, one call
    _same(out[0], real_carry(w24, s)[0])
    calls.clear()
    _same(eng.vocos_decode(codes, 2, eq=Eq.rumble())[0], real_eq(w24, Eq.rumble())[0])
    assert calls == ["eq"]
    with pytest.raises(ValueError, match="too long"):
        eng.vocos_decode(codes, 2, eq=Eq.notch(50.0, 100.0))
    calls.clear()
    _same(eng.vocos_decode(codes, 2, eq=Eq.notch(50.0, 100.0).carried())[0], real_carry(w24, Eq.notch(50.0, 100.0).sections(24000))[0])
    assert calls == ["eq_carry"]

    seen = []

    class Tok:
        sample_rate = 24000

        def encode(self, w):
            seen.append(np.array(w))
            return [(np.zeros((1, 8, 2), np.int64), None)]

    monkeypatch.setattr(G, "model", types.SimpleNamespace(engine=eng))
    monkeypatch.setattr(PM, "codec", Tok())
    monkeypatch.setattr(G, "language_detector", lambda t: "en")
    monkeypatch.setattr(G, "text_tokenizer", lambda t: ([7] * 4, ["en"] * 4))
    calls.clear()
    PM.make_prompt("hum", (x[None], 24000), transcript="hello", save_dir=str(tmp_path), eq=hum)
    assert calls == ["eq_carry", "eq_carry"]                              # the lead's call, then the clip's
    _same(seen[0][0, 0], want)
    calls.clear()
    PM.make_prompt("plain", (x[None], 24000), transcript="hello", save_dir=str(tmp_path), eq=Eq.rumble())
    assert calls == ["eq"]
    _same(seen[1][0, 0], real_eq([x], Eq.rumble())[0])
