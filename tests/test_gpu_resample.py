"""GPU: the device resampler (vx_resample, csrc/resample.hip) against tests/_resample_refs.py.

Every bound here is derived (tests/_resample_refs.py): K fp32 fmas are within (K + 1) 2^-24 sum |k_j| |x_j| of the exact sum over the
SAME fp32 taps, so the float64 reference runs on the taps read back from the device; exact statements (impulse responses, windows,
batching, composition) are compared word for word.  One un-finalized context serves the kernel tests: the entry needs no weights."""
import ctypes as C

import numpy as np
import pytest

from tests import _resample_refs as R
from vallex_amd import _capi
from vallex_amd._capi import VX_EINVAL, Engine, VallexHipError, _ptr

pytestmark = pytest.mark.gpu

PAIRS = sorted(R.PAIRS)
SENT = np.float32(-1.0e30)


@pytest.fixture(scope="module")
def eng():
    e = Engine(num_layers=2, max_batch=1, max_text=8, max_prompt=8, max_new=8, with_vocos=False)      # created, never finalized
    yield e
    e.close()


@pytest.fixture(scope="module")
def dev_taps(eng):
    return {pr: eng.dev_resample_taps(*pr) for pr in PAIRS}


def _raw(eng, rows, orig, new, out_stride=None, wav_stride=None, lens=None):
    """vx_resample on a sentinel-filled out: (rc, message, out (n, out_stride), out_lens)"""
    n = len(rows)
    ln = np.array([len(r) for r in rows] if lens is None else lens, np.int32)
    ws = max(1, max(len(r) for r in rows)) if wav_stride is None else wav_stride
    buf = np.zeros((n, max(1, ws)), np.float32)
    for i, r in enumerate(rows):
        buf[i, : len(r)] = r
    if out_stride is None:
        out_stride = max(1, max(R.out_len(orig, new, len(r)) for r in rows)) + 5
    out = np.full((n, max(1, out_stride)), SENT, np.float32)
    ol = np.full(n, -7, np.int32)
    rc = eng.lib.vx_resample(eng.ctx, _ptr(buf, C.c_float), ws, _ptr(ln, C.c_int32), n, orig, new, _ptr(out, C.c_float), out_stride,
                             _ptr(ol, C.c_int32))
    return rc, eng.lib.vx_last_error(eng.ctx).decode(), out, ol


def test_taps_and_geometry(eng, dev_taps):
    total = 0
    for pr in PAIRS:
        geom, tp = dev_taps[pr]
        assert geom == R.PAIRS[pr], pr
        assert eng.dev_resample_taps(*pr, taps=False) == (geom, None)
        d = R.ulp_diff(tp, R.taps(*pr))
        total += int((d != 0).sum())
        print(f"{pr[0]} -> {pr[1]}: {int((d != 0).sum())} of {d.size} device taps differ from the torch table, at most {int(d.max())} ulp")
        assert d.max() <= 1, (pr, int(d.max()))
    print(f"device taps: {total} differing words in the fifteen tables")


@pytest.mark.parametrize("orig,new", PAIRS)
def test_float64_and_ragged_batch(eng, dev_taps, orig, new):
    (o, n, width, K), tp = dev_taps[(orig, new)]
    rows = [R.noise(L, 2000 + i) for i, L in enumerate(R.lengths(orig, new))]
    both = eng.resample(rows, orig, new)
    worst = 0.0
    for i, x in enumerate(rows):
        alone = eng.resample([x], orig, new)[0]
        y, a = R.resample_ref64(x, tp, o, n, width)
        assert both[i].shape == alone.shape == y.shape == (R.out_len(orig, new, len(x)),)
        np.testing.assert_array_equal(both[i].view(np.uint32), alone.view(np.uint32))        # a row does not see its launch
        err, bd = np.abs(alone.astype(np.float64) - y), R.bound(a, K)
        worst = max(worst, float((err / np.maximum(bd, 1e-300)).max()))
        assert (err <= bd).all(), (len(x), float(err.max()))
    print(f"{orig} -> {new}: worst error {worst:.2f} of the bound")


@pytest.mark.parametrize("orig,new", PAIRS)
def test_several_tiles(eng, dev_taps, orig, new):
    """13001 samples: at least three workgroup tiles of one row for every pair (a tile is ~2048 outputs or 32 KiB of input span)"""
    (o, n, width, K), tp = dev_taps[(orig, new)]
    x = R.noise(13001, 77)
    got = eng.resample([x], orig, new)[0]
    y, a = R.resample_ref64(x, tp, o, n, width)
    assert got.shape == y.shape
    assert (np.abs(got.astype(np.float64) - y) <= R.bound(a, K)).all()


def _impulse_want(tp, o, n, width, K, L, s, orig, new):
    q = np.arange(R.out_len(orig, new, L))
    j = s + width - (q // n) * o
    ok = (j >= 0) & (j < K)
    # 0 + k: the word of the tap, except that a tap of -0.0 (the clamped ends of a kernel) comes out of fmaf(-0.0, 1.0, +0.0) as +0.0
    return np.float32(0) + np.where(ok, tp[q % n, np.clip(j, 0, K - 1)], np.float32(0)), (q % n)[ok], j[ok]


@pytest.mark.parametrize("orig,new", PAIRS)
def test_impulses_read_back_the_table(eng, dev_taps, orig, new):
    """one launch of o rows, row m a single 1.0: every output is one tap times 1.0 plus zeros -- the device table word for word, 0
    where no tap applies.  At sample m (length 2 K) the taps j <= m + width answer; at sample m + o ceil(K / o) (length 3 K + o) all
    taps of the residue m + width do, and over the o rows that is every word of the table (counted)."""
    (o, n, width, K), tp = dev_taps[(orig, new)]
    for L, shift in ((2 * K, 0), (3 * K + o, o * -(-K // o))):
        rows = np.zeros((o, L), np.float32)
        rows[np.arange(o), np.arange(o) + shift] = 1.0
        got = eng.resample(list(rows), orig, new)
        seen = np.zeros((n, K), bool)
        for m in range(o):
            want, ps, js = _impulse_want(tp, o, n, width, K, L, m + shift, orig, new)
            np.testing.assert_array_equal(got[m].view(np.uint32), want.view(np.uint32), err_msg=f"row {m}, impulse at {m + shift}")
            seen[ps, js] = True
        if shift:
            assert seen.all(), f"{int((~seen).sum())} words of the table were not read"


def test_sentinels_lengths_identity_and_repeat(eng):
    rows = [R.noise(1007, 1), np.zeros(0, np.float32), R.noise(5, 2), R.noise(300, 3)]
    for orig, new in ((24000, 16000), (24000, 44100), (48000, 24000)):
        rc, msg, out, ol = _raw(eng, rows, orig, new)
        assert rc == 0, msg
        assert ol.tolist() == [R.out_len(orig, new, len(r)) for r in rows] and ol[1] == 0
        for b in range(len(rows)):
            assert (out[b, ol[b]:] == SENT).all(), (orig, new, b)              # nothing behind out_lens[b]; row 1 untouched
            assert np.isfinite(out[b, : ol[b]]).all() and (np.abs(out[b, : ol[b]]) < 100).all()
        rc2, _, out2, ol2 = _raw(eng, rows, orig, new)
        assert rc2 == 0
        np.testing.assert_array_equal(out.view(np.uint32), out2.view(np.uint32))            # two calls, the same bits
        for b, got in enumerate(eng.resample(rows, orig, new)):
            np.testing.assert_array_equal(got, out[b, : ol[b]])
    # equal rates (also after the gcd): the input bits, NaN payloads and signed zeros included
    x = R.noise(100, 4)
    x[3], x[4] = np.float32(-0.0), np.float32(np.nan)
    rc, msg, out, ol = _raw(eng, [x, x[:7]], 16000, 16000)
    assert rc == 0 and ol.tolist() == [100, 7]
    np.testing.assert_array_equal(out[0, :100].view(np.uint32), x.view(np.uint32))
    np.testing.assert_array_equal(out[1, :7].view(np.uint32), x[:7].view(np.uint32))
    assert (out[0, 100:] == SENT).all() and (out[1, 7:] == SENT).all()
    assert eng.resample([], 24000, 16000) == []


def test_windows_are_bit_identical(eng):
    """rows of 1007 and 2015 samples through a window of the documented minimum and of an odd size above it: several windows and
    launches per row, the same words as the default single pass; 0 restores the default"""
    assert _capi.DEV_RESAMPLE_WINDOW_MIN == 512
    rows = [R.noise(1007, 11), R.noise(2 * 1007 + 1, 12)]
    pairs = [(24000, 44100), (44100, 24000), (24000, 16000), (24000, 11025)]
    eng.dev_resample_window(0)
    ref = {pr: [r.copy() for r in eng.resample(rows, *pr)] for pr in pairs}
    try:
        for win in (_capi.DEV_RESAMPLE_WINDOW_MIN, 777):
            eng.dev_resample_window(win)
            for pr in pairs:
                for got, want in zip(eng.resample(rows, *pr), ref[pr]):
                    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=f"window {win}, {pr}")
        # a window below a pair's K cannot hold one block: refused while it is set (700 -> 1: K = 9186), accepted at the default
        eng.dev_resample_window(_capi.DEV_RESAMPLE_WINDOW_MIN)
        with pytest.raises(VallexHipError) as ei:
            eng.resample([R.noise(20000, 13)], 700, 1)
        assert ei.value.code == VX_EINVAL and "window" in str(ei.value)
        for bad in (1, _capi.DEV_RESAMPLE_WINDOW_MIN - 1, -5, _capi.RESAMPLE_WINDOW + 1):
            with pytest.raises(VallexHipError) as ei:
                eng.dev_resample_window(bad)
            assert ei.value.code == VX_EINVAL and "input_samples" in str(ei.value)
    finally:
        eng.dev_resample_window(0)
    assert eng.resample([R.noise(20000, 13)], 700, 1)[0].shape == (29,)
    for got, want in zip(eng.resample(rows, 24000, 44100), ref[(24000, 44100)]):
        np.testing.assert_array_equal(got, want)


def test_long_kernels_run_from_global_memory(eng):
    """700 -> 1: K = 9186 taps do not fit the staged span, the kernel reads its samples from global memory -- same taps, same order"""
    (o, n, width, K), tp = eng.dev_resample_taps(700, 1)
    assert (o, n, width, K) == R.geometry(700, 1) == (700, 1, 4243, 9186)
    rows = [R.noise(20000, 21), R.noise(699, 22), R.noise(1, 23)]
    both = eng.resample(rows, 700, 1)
    for x, got in zip(rows, both):
        y, a = R.resample_ref64(x, tp, o, n, width)
        assert got.shape == y.shape
        assert (np.abs(got.astype(np.float64) - y) <= R.bound(a, K)).all()
        np.testing.assert_array_equal(eng.resample([x], 700, 1)[0].view(np.uint32), got.view(np.uint32))


@pytest.mark.parametrize("orig,new", PAIRS)
def test_against_the_python_path(eng, dev_taps, orig, new):
    """resample_sinc_hann (torch fp32 conv) and the device are each within the fma bound of the exact sum over their own taps; where
    a device tap differs from the torch one, sum |dk_j| |x_j| is added"""
    from vallex_amd.utils import prompt_making as PM
    (o, n, width, K), tp = dev_taps[(orig, new)]
    x = R.noise(1007, 31)
    got = eng.resample([x], orig, new)[0]
    ref = PM.resample_sinc_hann(x[None], orig, new)[0]
    _, a = R.resample_ref64(x, tp, o, n, width)
    _, a_t = R.resample_ref64(x, R.taps(orig, new), o, n, width)
    _, extra = R.resample_ref64(x, tp.astype(np.float64) - R.taps(orig, new).astype(np.float64), o, n, width)
    assert got.shape == ref.shape
    assert (np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= R.bound(a, K) + R.bound(a_t, K) + extra).all()


def _sine(freq, sr, n, phase=0.3):
    return np.sin(2 * np.pi * freq * np.arange(n) / sr + phase).astype(np.float32)


def test_resampler_properties_on_the_device(eng):
    """tests/test_resample.py's properties of a band-limited resampler, on the device"""
    edge = 200
    for sr in (8000, 16000, 22050, 44100, 48000):
        n = sr // 4 + 17
        dc, sine = eng.resample([np.ones(n, np.float32), _sine(440.0, sr, n)], sr, 24000)
        assert dc.shape == (R.out_len(sr, 24000, n),) and dc.dtype == np.float32
        np.testing.assert_allclose(dc[edge:-edge], 1.0, atol=2e-3)
        np.testing.assert_allclose(sine[edge:-edge], _sine(440.0, 24000, len(sine))[edge:-edge], atol=3e-3)
    for new in (8000, 16000, 44100, 48000):                         # and out of 24 kHz
        dc, sine = eng.resample([np.ones(6017, np.float32), _sine(440.0, 24000, 6017)], 24000, new)
        np.testing.assert_allclose(dc[edge:-edge], 1.0, atol=2e-3)
        np.testing.assert_allclose(sine[edge:-edge], _sine(440.0, new, len(sine))[edge:-edge], atol=3e-3)
    hi = eng.resample([_sine(18000.0, 48000, 24000)], 48000, 24000)[0]
    assert float(np.abs(hi[edge:-edge]).max()) < 2e-2                # above the new Nyquist


def _golden_codes12():
    from tests._util import golden
    codes = golden("nl2_bestof3")["codes"][0].astype(np.int64)
    assert codes.shape == (12, 8)
    return codes


def test_vocos_decode_at_another_rate():
    from tests._util import get_model
    m = get_model(2, 0, 2.5, vocos=True)
    e = m.engine
    codes = [_golden_codes12(), _golden_codes12()[:5]]
    w24 = [w.copy() for w in e.vocos_decode(codes, 2)]
    # without the argument: the bits of the plain vx_vocos_decode call
    buf = np.zeros((2, 12, 8), np.int64)
    buf[0], buf[1, :5] = codes[0], codes[1]
    lens = np.array([12, 5], np.int32)
    audio = np.zeros((2, 12 * 320), np.float32)
    assert e.lib.vx_vocos_decode(e.ctx, _ptr(buf, C.c_int64), 12, _ptr(lens, C.c_int32), 2, 2, _ptr(audio, C.c_float), 12 * 320) == 0
    np.testing.assert_array_equal(w24[0], audio[0])
    np.testing.assert_array_equal(w24[1], audio[1, : 5 * 320])
    for a, b in zip(e.vocos_decode(codes, 2, sample_rate=24000), w24):
        np.testing.assert_array_equal(a, b)
    w16 = e.vocos_decode(codes, 2, sample_rate=16000)
    for a, b in zip(w16, e.resample(w24, 24000, 16000)):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    assert [len(w) for w in w16] == [2560, -(-2 * 1600 // 3)]


def test_encodec_at_other_rates():
    from oracle.encodec_oracle import encodec_encoder_state_dict, encodec_state_dict
    from tests._util import get_model
    m = get_model(2, 0, 2.5, max_new=64, max_batch=4)
    sd = dict(encodec_state_dict(3))
    sd.update(encodec_encoder_state_dict(4))
    m.load_encodec_state_dict(sd)
    e = m.engine
    codes = [_golden_codes12()]
    w24 = e.encodec_decode(codes)
    np.testing.assert_array_equal(e.encodec_decode(codes, sample_rate=24000)[0], w24[0])
    w48 = e.encodec_decode(codes, sample_rate=48000)[0]
    np.testing.assert_array_equal(w48.view(np.uint32), e.resample(w24, 24000, 48000)[0].view(np.uint32))
    assert w48.shape == (2 * 12 * 320,)
    wav48k = (0.1 * R.noise(9000, 41)).astype(np.float32)
    got = e.encodec_encode([wav48k], sample_rate=48000)[0]
    want = e.encodec_encode(e.resample([wav48k], 48000, 24000))[0]
    assert got.shape == want.shape == (-(-4500 // 320), 8)
    np.testing.assert_array_equal(got, want)


def test_generate_audio_and_the_enrolment_hook():
    from oracle import synth
    from vallex_amd.utils import generation as G
    from vallex_amd.utils import prompt_making as PM
    G.preload_models(state_dict=synth.vallex_state_dict(2, 11), vocos_state_dict=synth.vocos_state_dict(2), num_layers=2, max_new=64,
                     max_prompt=128, max_text=64, max_batch=2)
    ids = synth.synth_text(6, 1)
    us = synth.uniforms(32, 1, 5)[:, 0]
    w24 = G.generate_audio(ids, language="en", uniforms=us, force_eos_at=12)
    w16 = G.generate_audio(ids, language="en", uniforms=us, force_eos_at=12, sample_rate=16000)
    assert w24.shape == (12 * 320,) and w16.shape == (-(-2 * len(w24) // 3),) and w16.dtype == np.float32
    np.testing.assert_array_equal(w16.view(np.uint32), G.model.engine.resample([w24], 24000, 16000)[0].view(np.uint32))
    np.testing.assert_array_equal(G.generate_audio(ids, language="en", uniforms=us, force_eos_at=12, sample_rate=24000), w24)
    b16 = G.generate_audio_batch([ids], language="en", uniforms=us[:, None], force_eos_at=12, sample_rate=16000)[0]
    np.testing.assert_array_equal(b16, w16)
    l16 = G.generate_audio_from_long_text([ids], language="en", uniforms=us, force_eos_at=12, sample_rate=16000)
    np.testing.assert_array_equal(l16, w16)
    with G.AudioServer(sample_rate=16000, force_eos_at=12) as srv:
        s16 = srv.submit(ids, language="en", seed=9).result()
    with G.AudioServer(force_eos_at=12) as srv:
        s24 = srv.submit(ids, language="en", seed=9).result()
    np.testing.assert_array_equal(s16, G.model.engine.resample([s24], 24000, 16000)[0])

    # PM.resampler = PM.device_resampler is what tokenize_audio calls; a stub tokenizer sees the device's samples
    seen = []

    class Tok:
        sample_rate = 24000

        def encode(self, w):
            seen.append(np.array(w))
            return [(np.zeros((1, 8, 1), np.int64), None)]

    w = (0.1 * np.stack([R.noise(1600, 51), R.noise(1600, 52)])).astype(np.float32)
    PM.resampler = PM.device_resampler
    try:
        PM.tokenize_audio(Tok(), (w, 16000))
    finally:
        PM.resampler = None
    assert seen[0].shape == (1, 1, 2400)
    want = G.model.engine.resample([w.mean(0)], 16000, 24000)[0]
    np.testing.assert_array_equal(seen[0][0, 0].view(np.uint32), want.view(np.uint32))
    two = PM.device_resampler(w, 16000, 24000)                       # (C, L) in, (C, L') out, channels independent
    assert two.shape == (2, 2400)
    np.testing.assert_array_equal(two[1], G.model.engine.resample([w[1]], 16000, 24000)[0])
    PM.tokenize_audio(Tok(), (w, 16000))                            # the default stays the torch path
    np.testing.assert_array_equal(seen[1][0], PM.resample_sinc_hann(w.mean(0, keepdims=True), 16000, 24000))


def test_nothing_else_moves():
    """greedy ids of nl2_greedy_eos before and after interleaved resample calls; a resample call while a serving session is open
    succeeds and the session's result is what it is without the call; no fallback is counted"""
    from tests._util import case_row, get_model, golden
    c, row, _ = case_row("nl2_greedy_eos")
    m = get_model(c["num_layers"], c["seed"], c["eos_gain"], vocos=True)
    e = m.engine
    x = R.noise(3001, 61)
    before = m.inference_batch([row], top_k=1, force_eos_at=c["force_eos_at"])[0]
    r1 = e.resample([x], 24000, 44100)[0].copy()
    after = m.inference_batch([row], top_k=1, force_eos_at=c["force_eos_at"])[0]
    np.testing.assert_array_equal(before, golden("nl2_greedy_eos")["codes"][0])
    np.testing.assert_array_equal(after, before)
    fb = e.last_fallbacks()
    e.resample([x], 24000, 16000)
    assert e.last_fallbacks() == fb

    def session(interleave):
        got = {}
        with e.serve(top_k=10, force_eos_at=30) as sess:
            ids = sess.submit(m.make_batch([row, row]), [dict(seed=5), dict(seed=6, best_of=2)])
            sess.run(3, lambda rid, cd: got.__setitem__(rid, cd))
            if interleave:
                np.testing.assert_array_equal(e.resample([x], 24000, 44100)[0].view(np.uint32), r1.view(np.uint32))
            sess.run(0, lambda rid, cd: got.__setitem__(rid, cd))
        return [got[i] for i in ids]

    for a, b in zip(session(False), session(True)):
        np.testing.assert_array_equal(a, b)


def test_refusals(eng):
    x = R.noise(100, 71)
    ok = eng.resample([x], 24000, 16000)[0].copy()
    lib, ctx = eng.lib, eng.ctx
    buf = np.zeros((1, 100), np.float32)
    buf[0] = x
    ln = np.array([100], np.int32)
    out = np.full((1, 80), SENT, np.float32)
    ol = np.full(1, -7, np.int32)
    fp, ip = lambda a: _ptr(a, C.c_float), lambda a: _ptr(a, C.c_int32)

    def refused(field, *args):
        rc = lib.vx_resample(ctx, *args)
        msg = lib.vx_last_error(ctx).decode()
        assert rc == VX_EINVAL and field in msg, (field, rc, msg)
        assert (out == SENT).all() and ol[0] == -7, field                 # nothing launched, nothing written

    refused("wav", None, 100, ip(ln), 1, 24000, 16000, fp(out), 80, ip(ol))
    refused("lens", fp(buf), 100, None, 1, 24000, 16000, fp(out), 80, ip(ol))
    refused("out", fp(buf), 100, ip(ln), 1, 24000, 16000, None, 80, ip(ol))
    refused("out_lens", fp(buf), 100, ip(ln), 1, 24000, 16000, fp(out), 80, None)
    assert lib.vx_resample(None, fp(buf), 100, ip(ln), 1, 24000, 16000, fp(out), 80, ip(ol)) == VX_EINVAL
    refused("batch", fp(buf), 100, ip(ln), 0, 24000, 16000, fp(out), 80, ip(ol))
    refused("batch", fp(buf), 100, ip(ln), -1, 24000, 16000, fp(out), 80, ip(ol))
    refused("orig_rate", fp(buf), 100, ip(ln), 1, 0, 16000, fp(out), 80, ip(ol))
    refused("new_rate", fp(buf), 100, ip(ln), 1, 24000, -16000, fp(out), 80, ip(ol))
    refused("lens[0]", fp(buf), 100, ip(np.array([-1], np.int32)), 1, 24000, 16000, fp(out), 80, ip(ol))
    refused("wav_stride", fp(buf), 100, ip(np.array([101], np.int32)), 1, 24000, 16000, fp(out), 80, ip(ol))
    refused("out_stride", fp(buf), 100, ip(ln), 1, 24000, 16000, fp(out), 66, ip(ol))            # ceil(200 / 3) = 67
    refused("taps", fp(buf), 100, ip(ln), 1, 44101, 24000, fp(out), 80, ip(ol))
    refused("taps", fp(buf), 100, ip(ln), 1, 24000, 44101, fp(out), 80, ip(ol))
    with pytest.raises(VallexHipError) as ei:
        eng.dev_resample_taps(44101, 24000)
    assert ei.value.code == VX_EINVAL and "taps" in str(ei.value)
    # the context still resamples, to the same bits
    assert lib.vx_resample(ctx, fp(buf), 100, ip(ln), 1, 24000, 16000, fp(out), 80, ip(ol)) == 0
    assert ol[0] == 67 and (out[0, 67:] == SENT).all()
    np.testing.assert_array_equal(out[0, :67].view(np.uint32), ok.view(np.uint32))
