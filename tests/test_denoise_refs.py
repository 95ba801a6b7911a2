"""CPU: the numpy restatement of vx_denoise's contract (tests/_denoise_refs.py) alone -- that the arithmetic the header fixes is a
Fourier transform, that it leaves a clip alone at alpha = 0, and that at the defaults it does what the feature is for: on six gated
vowels in white noise the signal-to-noise ratio over the spoken samples rises and the pauses get quieter.  The thresholds are the
issue's (1 dB and 12 dB); measured with this restatement: SNR +1.68 .. +7.26 dB, pauses -14.05 .. -14.45 dB.  Plus the host-only
facts of the binding: the tables the library reports, the option checks of the Python layer, the `denoise=` keywords."""
import inspect
import re
import os

import numpy as np
import pytest

import vallex_amd
from tests import _denoise_refs as R
from vallex_amd import _capi
from vallex_amd.utils import generation as G
from vallex_amd.utils import prompt_making as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def tab():
    return R.tables()


@pytest.fixture(scope="module")
def claims(tab):
    """the six rows and their restatement at the defaults, computed once"""
    return [(tag, cl, noisy, gate, R.denoise(noisy, R.DEFAULTS, tab)) for tag, cl, noisy, gate in R.claim_rows()]


def test_the_network_is_a_fourier_transform(tab):
    """against numpy.fft.fft on random complex frames: |error| <= 1 x N eps max|X| (factor 1; a radix-2 transform's error grows with
    log2 N eps rms|X|, a prototype measured 4.5e-14 at unit variance against a bound of 1e-11).  The inverse network undoes it."""
    rng = np.random.default_rng(0)
    z = rng.normal(size=(16, R.N)) + 1j * rng.normal(size=(16, R.N))
    re, im = R.fft(z.real, z.imag, tab)
    X = np.fft.fft(z)
    err = np.abs(re + 1j * im - X).max()
    print(f"fft error {err:.3e}, bound {R.N * EPS * np.abs(X).max():.3e}")
    assert err <= 1.0 * R.N * EPS * np.abs(X).max()
    ri, ii = R.fft(re, im, tab, inverse=True)
    assert np.abs((ri + 1j * ii) / R.N - z).max() <= R.N * EPS * np.abs(z).max()


def test_an_impulse_and_a_constant_have_their_textbook_spectra(tab):
    x = np.zeros((2, R.N))
    x[0, 1], x[1, :] = 1.0, 1.0
    re, im = R.fft(x, np.zeros_like(x), tab)
    k = np.arange(R.N)
    assert np.abs(re[0] - np.cos(2 * np.pi * k / R.N)).max() <= 16 * EPS and np.abs(im[0] + np.sin(2 * np.pi * k / R.N)).max() <= 16 * EPS
    assert re[1, 0] == R.N and np.abs(re[1, 1:]).max() == 0 and np.abs(im[1]).max() == 0


def test_alpha_zero_returns_the_input_within_one_ulp(tab, claims):
    """|out - x| <= one fp32 ulp of x, plus the double transform's own error N eps max|x| (the bound of the test above: 5.7e-14 at a peak
    of 0.5, a 500 000th of the ulp of a sample of 1e-6).  The second term matters only where x passes through zero, where the ulp of x
    shrinks below what 512 double additions leave: on the 3 000-sample vowel 3 samples differ at all (0, 1200, 2400: x = 0, -5.7e-15,
    -7.5e-15), by at most 1.4e-17; every other sample comes back bit for bit."""
    tag, _, noisy, _, _ = claims[1]
    vow = R.vowel(110.0, 700.0, R.RATE, 3000)
    for x in (vow, noisy):
        got = R.denoise(x, (0.0,) + R.DEFAULTS[1:], tab)
        d = np.abs(got["out"].astype(np.float64) - x.astype(np.float64))
        off = got["out"].view(np.uint32) != x.view(np.uint32)
        print(f"alpha = 0: {int(off.sum())} of {len(x)} samples off, by at most {d.max():.3e}")
        assert (d <= np.spacing(np.abs(x)).astype(np.float64) + R.N * EPS * float(np.abs(x).max())).all()
        assert off.sum() <= len(x) // 1000
        assert (got["gain"] == 1.0).all()


def test_every_sample_lies_in_four_frames_and_the_window_sums_to_two(tab):
    """w^2 summed over the four frames of a sample is 2: the 0.5 of the synthesis"""
    w2 = (tab[:R.N] ** 2).reshape(4, R.H).sum(0)
    assert np.abs(w2 - 2.0).max() <= 4 * EPS
    for L in R.LENGTHS:
        T = R.frames(L)
        cover = np.zeros(L + 4 * R.N, int)
        for t in range(T):
            cover[(t - 3) * R.H + 2 * R.N: (t - 3) * R.H + 3 * R.N] += 1
        assert (cover[2 * R.N: 2 * R.N + L] == 4).all(), L
        assert R.full(L) == sum(1 for t in range(T) if (t - 3) * R.H >= 0 and (t - 3) * R.H + R.N <= L), L


def test_the_row_builder_is_the_issues(claims):
    assert [c[0] for c in claims] == ["110Hz_0.003", "110Hz_0.01", "110Hz_0.03", "220Hz_0.003", "220Hz_0.01", "220Hz_0.03"]
    for tag, cl, noisy, gate, _ in claims:
        assert len(cl) == 2 * R.RATE and not gate[: R.RATE // 2].any() and not gate[-R.RATE // 4:].any()
        assert (cl[~gate] == 0).all() and 0.3 < gate.mean() < 0.6
        sigma = float(tag.split("_")[1])
        assert abs(np.std(noisy.astype(np.float64) - cl) / sigma - 1) < 0.02


def test_the_audible_claims_at_the_defaults(claims):
    """SNR over the gated-on samples up by at least 1 dB; power more than 1024 samples from any gated-on sample down by at least 12 dB"""
    for tag, cl, noisy, gate, d in claims:
        far = R.far_from(gate)
        gain = R.snr_db(cl, d["out"], gate) - R.snr_db(cl, noisy, gate)
        drop = R.power_db(d["out"], far) - R.power_db(noisy, far)
        print(f"{tag}: SNR {gain:+.2f} dB, pauses {drop:+.2f} dB, K = {d['info']['k']} of {d['info']['full_frames']}")
        assert far.sum() > 10000
        assert gain >= 1.0, (tag, gain)
        assert drop <= -12.0, (tag, drop)
        assert d["info"]["k"] == 37 and d["info"]["frames"] == 378 and d["info"]["full_frames"] == 372


def test_a_given_profile_is_used_as_is(tab, claims):
    for tag, _, noisy, _, d in claims[:2]:
        again = R.denoise(noisy, R.DEFAULTS, tab, psd=d["psd"])
        R.same(again["out"], d["out"], tag)
        R.same(again["gain"], d["gain"], tag)
        assert again["info"]["k"] == 0 and len(again["sel"]) == 0
    other = R.denoise(claims[0][2], R.DEFAULTS, tab, psd=claims[2][4]["psd"])          # the profile of the loudest noise on the quietest row
    assert np.abs(other["out"].astype(np.float64)).mean() < np.abs(claims[0][4]["out"].astype(np.float64)).mean()


def test_the_three_profile_paths_and_the_selection(tab):
    rows = dict(zip(R.LENGTHS, R.length_rows()))
    for L, x in rows.items():
        d = R.denoise(x, R.DEFAULTS, tab)
        F = R.full(L)
        assert d["info"] == dict(frames=-(-L // 128) + 3, full_frames=F, k=min(8, F), nonfinite=0), L
        assert len(d["out"]) == L and np.isfinite(d["out"]).all()
        if F == 0:
            fl = float(np.float32(R.DEFAULTS[1]))                                       # the zero profile: 1 - 0 / S, or the floor at S = 0
            assert (d["psd"] == 0).all() and ((d["gain"] == 1.0) | (d["gain"] == fl)).all()
        elif F < 8:
            assert list(d["sel"]) == list(range(3, 3 + F))
        else:
            assert len(d["sel"]) == 8 and (np.diff(d["sel"]) > 0).all()
            rest = [t for t in range(3, 3 + F) if t not in set(d["sel"])]
            assert d["E"][d["sel"]].max() <= d["E"][rest].min()
    E = np.array([9, 9, 9, 5.0, 1.0, 5.0, 1.0, 5.0, 9, 9, 9])                           # ties go to the lower t
    L = 8 * 128
    assert R.frames(L) == 11 and R.full(L) == 5
    assert list(R.select(E, L, 1)) == [4] and list(R.select(E, L, 3)) == [3, 4, 6] and list(R.select(E, L, 0)) == []
    assert [R.k_of((2, .1, f, k), F) for f, k, F in ((0.1, 8, 372), (0.1, 8, 7), (0.1, 8, 0), (1.0, 0, 20), (0.0, 0, 20), (0.5, 3, 5))] == \
        [37, 7, 0, 20, 0, 3]


def test_odd_inputs(tab):
    x = R.odd_row()
    d = R.denoise(x, R.DEFAULTS, tab)
    assert d["info"]["nonfinite"] == 6 and np.isfinite(d["out"]).all()
    R.same(d["out"], R.denoise(R.clean(x)[0], R.DEFAULTS, tab)["out"])
    z = R.denoise(np.zeros(1300, np.float32), R.DEFAULTS, tab)
    assert (z["out"] == 0).all() and (z["P"] == 0).all() and (z["gain"] == np.float32(R.DEFAULTS[1]).astype(np.float64)).all()


def test_the_library_reports_its_tables_and_they_are_numpys_to_one_ulp(tab):
    vallex_amd.load_library()
    t = _capi.Engine.denoise_tables()
    assert t.shape == (1024,) and t.dtype == np.float64
    w, c, s = t[:512], t[512:768], t[768:]
    for got, want in ((w, tab[:512]), (c, tab[512:768]), (s, tab[768:])):
        assert (np.abs(got - want) <= np.spacing(np.abs(want))).all()
    assert w[0] == 0 and w[256] == 1 and c[0] == 1 and s[0] == 0 and np.signbit(s[0]) and c[128] < 1e-16 and s[128] == -1
    assert vallex_amd.load_library().vx_denoise_tables(None) == _capi.VX_EINVAL


def test_binding_header_and_keywords_agree():
    hdr = open(os.path.join(ROOT, "include", "vallex_hip.h")).read()
    for st in (_capi.vx_denoise_opts, _capi.vx_denoise_info):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (st.__name__, st.__name__), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in re.findall(r"\w+\s+([^;]+);", body) for n in re.findall(r"\w+", decl)]
        assert names == [f[0] for f in st._fields_], (st.__name__, names)
    dev = open(os.path.join(ROOT, "include", "vallex_hip_dev.h")).read()
    assert int(re.search(r"#define VX_DENOISE_WINDOW \(1 << (\d+)\)", hdr).group(1)) == 22 and _capi.DENOISE_WINDOW == 1 << 22
    assert int(re.search(r"#define VX_DEV_DENOISE_WINDOW_MIN (\d+)", dev).group(1)) == _capi.DEV_DENOISE_WINDOW_MIN >= max(R.LENGTHS)
    assert (_capi.DENOISE_N, _capi.DENOISE_HOP, _capi.DENOISE_BINS) == (R.N, R.H, R.B)
    assert {"vx_denoise", "vx_denoise_tables"} <= set(_capi.SYMBOLS)
    assert {"vx_dev_denoise_fft", "vx_dev_denoise_table", "vx_dev_denoise_window", "vx_dev_denoise_div"} <= set(_capi.DEV_SYMBOLS)
    sig = inspect.signature(_capi.Engine.denoise).parameters
    assert list(sig)[1:6] == ["wavs", "strength_db", "floor_db", "frac", "kmin"] and "profile" in sig
    assert (sig["floor_db"].default, sig["frac"].default, sig["kmin"].default, sig["profile"].default) == (-18.0, 0.1, 8, None)
    for fn in (G.generate_audio, G.generate_audio_batch, G.generate_audio_from_long_text, G.AudioServer.__init__, PM.tokenize_audio,
               PM.make_prompt, _capi.Engine.vocos_decode, _capi.Engine.encodec_decode):
        assert inspect.signature(fn).parameters["denoise"].default is None, fn


def test_the_python_layer_converts_db_and_refuses_before_any_launch():
    o, psd = _capi.Engine._denoise_opts()
    assert psd is None and o.alpha == 2.0 and o.floor == np.float32(10.0 ** (-18.0 / 20.0)) and o.frac == np.float32(0.1) and o.kmin == 8
    assert (o.alpha, o.floor, o.frac, o.kmin) == tuple(np.float32(v) for v in R.DEFAULTS[:3]) + (R.DEFAULTS[3],)
    assert _capi.Engine._denoise_opts(strength_db=0.0)[0].alpha == 1.0 and _capi.Engine._denoise_opts(floor_db=0.0)[0].floor == 1.0
    assert abs(_capi.Engine._denoise_opts(strength_db=6.0)[0].alpha - 3.981) < 1e-3
    for bad in (dict(strength_db=float("nan")), dict(strength_db=4000.0), dict(floor_db=0.1), dict(floor_db=-2000.0), dict(frac=-0.1),
                dict(frac=1.5), dict(frac=float("nan")), dict(kmin=-1), dict(profile=np.zeros(256)), dict(profile=-np.ones(257)),
                dict(profile=np.full(257, np.inf))):
        with pytest.raises(ValueError, match="denoise"):
            _capi.Engine._denoise_opts(**bad)
        with pytest.raises(ValueError, match="denoise"):
            G.Denoise(**bad)
    d = G.Denoise(strength_db=3.0, floor_db=-12.0, frac=0.2, kmin=4, profile=np.ones(257))
    assert _capi.Engine._denoise_parts(d) == dict(strength_db=3.0, floor_db=-12.0, frac=0.2, kmin=4, profile=d.profile)
    assert _capi.Engine._denoise_parts(True) == {}
    for bad in (False, 1.0, "yes"):
        with pytest.raises(ValueError, match="denoise"):
            _capi.Engine._denoise_parts(bad)
