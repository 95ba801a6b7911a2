"""CPU: the carried-state equaliser's contract without a GPU -- the binding and the header, vx_eq_carry_plan's M against the numpy
restatement (tests/_eq_carry_refs.py), the restatement's three passes against the unbounded recursion they restate, the Eq.hum /
CarriedEq objects, the dispatch of a carried `eq=` at both audio ends on stub engines, and what priming buys on a hum row."""
import inspect
import os
import re
import types

import numpy as np
import pytest

import vallex_amd  # noqa: F401
from tests import _eq_carry_refs as R
from tests import _eq_refs as E
from vallex_amd import _capi
from vallex_amd._capi import Engine
from vallex_amd.utils import generation as G
from vallex_amd.utils import prompt_making as PM
from vallex_amd.utils.generation import CarriedEq, Eq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "vallex_hip.h")).read()
U = 2.0 ** -24
LONG = {"hum 50 x 6 Q 35": Eq.hum(50.0, 6, 35.0), "hum 50 x 8 Q 100": Eq.hum(50.0, 8, 100.0),
        "hum 60 x 4 Q 30 + rumble": Eq.hum(60.0, 4, 30.0) + Eq.rumble(), "rumble": Eq.rumble().carried(), "highpass 5 Hz": Eq.highpass(5.0).carried()}


def test_binding_and_header_constants():
    step = int(re.search(r"#define VX_EQ_CARRY_STEP (\d+)", HEADER).group(1))
    m, sc = Engine.eq_carry_plan(E.IDENTITY)
    assert sc == step and step % 32 == 0 and step >= 32
    np.testing.assert_array_equal(m, np.zeros((2, 2)))                    # the identity section keeps no state
    assert {"vx_eq_carry", "vx_eq_carry_plan"} <= set(_capi.SYMBOLS)
    lib = vallex_amd.load_library()
    assert len(lib.vx_eq_carry.argtypes) == 12 and len(lib.vx_eq_carry_plan.argtypes) == 4
    for name in ("vx_eq_carry", "vx_eq_carry_plan"):
        assert re.search(r"\bint " + name + r"\(", HEADER), name
    assert int(re.search(r"#define VX_ABI_VERSION (\d+)", HEADER).group(1)) == _capi.ABI_VERSION == lib.vx_abi_version()
    assert "vx_eq_info" in inspect.getsource(Engine.eq_carry) and Engine.last_eq_info is None
    assert lib.vx_eq_carry_plan(None, 1, None, None) == _capi.VX_EINVAL and b"NULL" in lib.vx_eq_last_error()


def test_matrix_equals_the_restatement():
    sc = Engine.eq_carry_plan(E.IDENTITY)[1]
    for name, eq in LONG.items():
        for rate in (24000, 16000):
            s = eq.sections(rate)
            m, step = Engine.eq_carry_plan(eq, rate)
            assert step == sc and m.shape == (2 * len(s), 2 * len(s))
            np.testing.assert_array_equal(m.view(np.uint64), R.matrix(s, sc).view(np.uint64), err_msg=f"{name} at {rate}")
    for bad, why in ((np.array([[1.0, 0.0, 0.0, 0.0, 1.0]]), "unstable"), (np.array([[1.0, np.nan, 0.0, 0.0, 0.0]]), "coefficient 1"),
                     (np.zeros((0, 5)), "nsections 0"), (np.tile(E.IDENTITY, (9, 1)), "nsections 9")):
        with pytest.raises(ValueError, match=why):
            Engine.eq_carry_plan(bad)
        with pytest.raises(ValueError):
            R.matrix(bad, sc)


@pytest.fixture(scope="module")
def long_rows():
    a = R.hum_row(72077, dc=0.05, noise=0.05, hum_db=-20.0, seed=34)[0]  # hum + noise + DC
    b = R.hum_row(20011, f0=60.0, harmonics=4, dc=-0.02, noise=0.05, hum_db=-20.0, seed=35)[0]
    return a, b


@pytest.mark.parametrize("name", sorted(LONG))
def test_restatement_is_the_unbounded_recursion(long_rows, name):
    """every sample within 2^-24 peak(x) + 2^-24 |y| of _eq_refs.full, the bound vx_eq's restatement is held to -- here the first
    term has nothing to cover but rounding in double (there is no truncation), the second is the one rounding of the output to fp32"""
    sc = Engine.eq_carry_plan(E.IDENTITY)[1]
    s = LONG[name].sections(24000)
    worst = 0.0
    for x in long_rows:
        got, state, info = R.eq_carry(x, s, sc)
        want = E.full(x, s)
        d = np.abs(got.astype(np.float64) - want)
        bound = U * float(np.abs(x).max()) + U * np.abs(want)
        assert (d <= bound).all(), (name, len(x), float((d / bound).max()))
        assert info["nonfinite"] == info["nonfinite_out"] == 0 and info["warm"] == 0 and state.shape == (2 * len(s),)
        worst = max(worst, float((d - U * np.abs(want)).max()))
    assert worst < 1e-9                                                   # beyond the output's own rounding: double roundoff alone


def test_a_plain_notch_is_still_refused_and_the_same_specs_carried_are_accepted():
    with pytest.raises(ValueError, match="too long"):
        Engine.eq_plan(Eq.notch(50.0, 100.0))
    m, sc = Engine.eq_carry_plan(Eq.notch(50.0, 100.0).carried())
    assert m.shape == (2, 2) and np.isfinite(m).all() and np.abs(np.linalg.eigvals(m)).max() < 1
    assert tuple(Eq.notch(50.0, 100.0).carried()) == tuple(Eq.notch(50.0, 100.0))
    for name in ("Eq", "README"):
        text = Eq.__doc__ if name == "Eq" else open(os.path.join(ROOT, "README.md")).read()
        assert "CarriedEq" in text, name


def test_hum_and_carried_eq_objects():
    h = Eq.hum()
    assert isinstance(h, CarriedEq) and isinstance(h, Eq) and h.prime_hz == 50.0 and h.is_carried
    assert tuple(h) == tuple(("notch", 50.0 * k, 35.0, 0.0) for k in range(1, 7))
    assert tuple(Eq.hum(60.0, 4, 30.0)) == tuple(("notch", 60.0 * k, 30.0, 0.0) for k in range(1, 5))
    assert not getattr(Eq.rumble(), "is_carried", False) and type(Eq.rumble() + Eq.presence()) is Eq
    for both in (h + Eq.rumble(), Eq.rumble() + h):
        assert isinstance(both, CarriedEq) and both.prime_hz == 50.0 and len(both) == 7
    assert (Eq.rumble() + h)[0] == ("highpass", 80.0, 0.7071, 0.0) and (h + Eq.rumble())[6] == ("highpass", 80.0, 0.7071, 0.0)
    c = Eq.telephone().carried()
    assert isinstance(c, CarriedEq) and c.prime_hz is None and tuple(c) == tuple(Eq.telephone()) and c.carried() is c
    assert Eq.rumble().carried(prime_hz=60.0).prime_hz == 60.0 and (c + Eq.hum(60.0, 2)).prime_hz == 60.0
    with pytest.raises(AttributeError):
        h.prime_hz = 60.0
    with pytest.raises(ValueError, match="sections"):
        Eq.hum(50.0, 6) + Eq.telephone()                                  # the limits are Eq's: 8 sections
    for bad in (0, 9, 2.5):
        with pytest.raises(ValueError, match="harmonics"):
            Eq.hum(50.0, bad)
    with pytest.raises(ValueError, match="prime_hz"):
        CarriedEq([("notch", 50.0, 35.0, 0.0)], prime_hz=0.0)
    # the Nyquist drop: at the rate of the call, of the harmonics only
    assert len(h.sections(24000)) == 6 and len(Eq.hum(1000.0, 8, 35.0).sections(8000)) == 3 and len(Eq.hum(1000.0, 8, 35.0).sections(24000)) == 8
    np.testing.assert_array_equal(Eq.hum(1000.0, 8, 35.0).sections(8000), Eq([("notch", 1000.0 * k, 35.0, 0.0) for k in (1, 2, 3)]).sections(8000))
    assert len((Eq.hum(3000.0, 4) + Eq.rumble()).sections(16000)) == 3
    with pytest.raises(ValueError, match="f0"):
        (Eq.hum(3000.0, 2) + Eq.highpass(9000.0)).sections(16000)         # a spec of the caller's own is never dropped
    with pytest.raises(ValueError, match="f0"):
        Eq.notch(9000.0).carried().sections(16000)
    with pytest.raises(ValueError, match="no section"):
        Eq.hum(9000.0, 2).sections(16000)


# ---- dispatch on stub engines --------------------------------------------------------------------------------------------------------

class _StageEngine(Engine):
    """an Engine without a context: the vocoder entries of the library answer 0 and write nothing, every stage records its name"""

    def __init__(self):
        self.calls = []
        self.ctx = None
        self.lib = types.SimpleNamespace(vx_vocos_decode=lambda *a: 0, vx_encodec_decode=lambda *a: 0)

    def denoise(self, rows, **kw):
        self.calls.append("denoise")
        return rows, []

    def _paused(self, rows, pauses, rate=24000):
        if pauses is not None:
            self.calls.append("pauses")
        return rows

    def stretch(self, rows, speed):
        self.calls.append("stretch")
        return rows

    def eq(self, rows, sections, sample_rate=24000, return_info=False):
        self.calls.append(("eq", sample_rate, len(self._eq_sections(sections, sample_rate))))
        return rows

    def eq_carry(self, rows, eq, sample_rate=24000, state=None, return_state=False):
        self.calls.append(("eq_carry", sample_rate, len(self._eq_sections(eq, sample_rate)), getattr(eq, "prime_hz", None)))
        return rows

    def resample(self, rows, a, b):
        self.calls.append(("resample", a, b))
        return rows


def test_engine_order_of_the_stages_with_a_carried_eq():
    codes = [np.zeros((12, 8), np.int64)]
    for decode in ("vocos_decode", "encodec_decode"):
        kw = dict(bandwidth_id=2) if decode == "vocos_decode" else {}
        e = _StageEngine()
        getattr(e, decode)(codes, sample_rate=8000, denoise=True, pauses=G.Pauses(max_ms=300.0), speed=1.25, eq=Eq.hum(), **kw)
        assert e.calls == ["denoise", "pauses", "stretch", ("eq_carry", 24000, 6, 50.0), ("resample", 24000, 8000)]
        e = _StageEngine()
        out = getattr(e, decode)(codes, eq=Eq.notch(50.0, 100.0).carried(), **kw)
        assert e.calls == [("eq_carry", 24000, 1, None)] and len(out) == 1 and len(out[0]) == 12 * 320
        e = _StageEngine()
        getattr(e, decode)(codes, eq=Eq.rumble(), **kw)                   # a plain Eq runs what it ran
        assert e.calls == [("eq", 24000, 1)]
        e = _StageEngine()
        with pytest.raises(ValueError, match="too long"):                 # ... and keeps its refusals, before the vocoder runs
            getattr(e, decode)(codes, eq=Eq.notch(50.0, 100.0), **kw)
        with pytest.raises(ValueError, match="f0"):
            getattr(e, decode)(codes, eq=Eq.highpass(13000.0).carried(), **kw)
        assert e.calls == []
    e = _StageEngine()
    assert e._equalised(["rows"], None) == ["rows"] and e.calls == []


class _GenEngine:
    """stands in for model.engine under utils.generation / utils.prompt_making: records the stages, refuses like the real one"""

    def __init__(self):
        self.calls = []

    def eq_plan(self, eq, rate=24000):
        self.calls.append(("eq_plan", rate))
        return Engine.eq_plan(eq, rate)

    def eq_carry_plan(self, eq, rate=24000):
        self.calls.append(("eq_carry_plan", rate))
        return Engine.eq_carry_plan(eq, rate)

    def _equalised(self, rows, eq, rate=24000):
        self.calls.append(("eq", rate, type(eq).__name__))
        return rows

    def resample(self, rows, a, b):
        self.calls.append(("resample", a, b))
        return rows

    def vocos_decode(self, codes, bw, **kw):
        self.calls.append(("vocos_decode", kw.get("eq")))
        return [np.zeros(320 * len(c), np.float32) for c in codes]


class _GenModel:
    def __init__(self):
        self.engine, self.calls = _GenEngine(), 0

    def inference(self, x, x_lens, y, enroll_x_lens=0, **kw):
        self.calls += 1
        return np.zeros((1, 3, 8), np.int64)

    def inference_batch(self, rows, **kw):
        self.calls += 1
        return [np.zeros((3, 8), np.int64) for _ in rows]


class _GenVocos:
    def codes_to_features(self, frames):
        return np.asarray(frames)

    def decode(self, features, bandwidth_id=None):
        return np.zeros((1, 320 * features.shape[-1]), np.float32)


@pytest.fixture
def gen(monkeypatch):
    m = _GenModel()
    monkeypatch.setattr(G, "model", m)
    monkeypatch.setattr(G, "vocos", _GenVocos())
    monkeypatch.setattr(G, "rng", None)
    monkeypatch.setattr(G, "language_detector", lambda t: "en")
    monkeypatch.setattr(G, "sentence_splitter", lambda t: t.split("|"))
    monkeypatch.setattr(G, "text_tokenizer", lambda t: ([7] * 4, ["en"] * 4))
    return m


def test_generation_layer_checks_and_dispatches_a_carried_eq(gen):
    e, hum = gen.engine, Eq.hum()
    G.generate_audio("hello", language="en", eq=hum, sample_rate=8000)
    assert e.calls == [("eq_carry_plan", 24000), ("eq", 24000, "CarriedEq"), ("resample", 24000, 8000)]
    e.calls.clear()
    G.generate_audio_from_long_text("one|two", language="en", eq=hum)
    assert e.calls == [("eq_carry_plan", 24000), ("eq", 24000, "CarriedEq")]
    e.calls.clear()
    G.generate_audio_batch(["a", "b"], language="en", eq=hum)
    assert e.calls == [("eq_carry_plan", 24000), ("vocos_decode", hum)]
    e.calls.clear()
    G.generate_audio("hello", language="en", eq=Eq.rumble())              # a plain Eq is checked and run as before
    assert e.calls == [("eq_plan", 24000), ("eq", 24000, "Eq")]
    e.calls.clear()
    good = gen.calls
    for bad, why in ((Eq.highpass(13000.0).carried(), "f0"), (CarriedEq(), "no section")):
        for call in (lambda: G.generate_audio("hello", language="en", eq=bad), lambda: G.generate_audio_batch(["a"], language="en", eq=bad),
                     lambda: G.generate_audio_from_long_text("one|two", language="en", eq=bad), lambda: G.AudioServer(eq=bad)):
            with pytest.raises(ValueError, match=why):
                call()
    assert gen.calls == good and all(c[0] == "eq_carry_plan" for c in e.calls)   # refused before any model work


def test_enrolment_hands_a_carried_eq_to_the_engine(gen):
    class Tok:
        sample_rate = 16000

        def encode(self, wav):
            return [(np.zeros((1, 8, 2), np.int64), None)]

    wav = E.noise_row(1600, dc=0.2)
    PM.tokenize_audio(Tok(), (wav, 16000), eq=Eq.hum(60.0))
    assert gen.engine.calls == [("eq", 16000, "CarriedEq")]              # at the tokenizer's rate, first of all


# ---- priming -------------------------------------------------------------------------------------------------------------------------

def _db(v):
    return 10.0 * np.log10(np.mean(np.asarray(v, np.float64) ** 2))


@pytest.mark.parametrize("q", [35.0, 100.0])
def test_priming_takes_the_hum_out_from_the_first_sample(q):
    """hum at -27 dBFS, six harmonics, over noise that alone filters to about -46 dBFS: the first 0.25 s of the primed output lie
    within 1 dB of the filtered noise alone; from rest they lie more than 10 dB above it (the notches ring in)"""
    sc = Engine.eq_carry_plan(E.IDENTITY)[1]
    hum = Eq.hum(50.0, 6, q)
    s = hum.sections(24000)
    x, noise = R.hum_row(72000, seed=36)
    assert abs(_db(x.astype(np.float64) - noise) + 27.0) < 0.1
    lead = G.hum_lead(x, s, 24000, hum.prime_hz)
    want = R.prime_lead(x, s, 24000, 50.0)
    assert lead.dtype == np.float32 and len(lead) % 480 == 0 and len(lead) <= 240000
    np.testing.assert_array_equal(lead.view(np.uint32), want.view(np.uint32))                # the host code is the restatement's
    alone = _db(R.eq_carry(noise, s, sc)[0][:6000])
    primed = _db(R.primed(x, s, sc, 24000, 50.0)[0][:6000])
    rest = _db(R.eq_carry(x, s, sc)[0][:6000])
    print(f"Q {q}: filtered noise alone {alone:.1f} dBFS, primed {primed:.1f} dBFS, from rest {rest:.1f} dBFS")
    assert abs(alone + 46.0) < 1.0 and abs(primed - alone) < 1.0 and rest > alone + 10.0
    assert G.hum_lead(x[:4799], s, 24000, 50.0) is None and R.prime_lead(x[:4799], s, 24000, 50.0) is None      # below ten periods: from rest
    assert G.hum_lead(x, E.IDENTITY, 24000, 50.0) is None                  # no pole to ring
