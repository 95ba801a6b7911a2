"""EnCodec SEANet decoder.  CPU: oracle vs the committed output of the installed transformers port,
and the state-dict normalisation; GPU: the HIP decoder vs the same goldens."""
import os

import numpy as np
import pytest

import vallex_amd  # noqa: F401
from oracle.encodec_oracle import (EncodecDecoderOracle, EncodecEncoderOracle, encodec_encoder_state_dict,
                                   encodec_state_dict)
from oracle.make_golden_encodec import CASES, ENC_CASES, GOLD, case_codes, case_wav
from vallex_amd.data.tokenizer import AudioTokenizer, canonical_encodec_state_dict


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_matches_transformers_port(name):
    g = np.load(os.path.join(GOLD, name + ".npz"))["audio"]
    out = EncodecDecoderOracle(encodec_state_dict(3)).decode(case_codes(name))
    assert out.shape == g.shape
    np.testing.assert_allclose(out, g, atol=1e-6, rtol=0)


@pytest.mark.parametrize("name", list(ENC_CASES))
def test_encoder_oracle_matches_transformers_port(name):
    """SEANet encoder + RVQ encode (prompt enrolment, data/tokenizer.py:92-111): the oracle's codes are
    bit-exact against `transformers.EncodecModel.encode(bandwidth=6.0)`, its embeddings agree to fp32 rounding."""
    g = np.load(os.path.join(GOLD, name + ".npz"))
    orc = EncodecEncoderOracle(encodec_encoder_state_dict(4), encodec_state_dict(3))
    wav = case_wav(name)
    emb = orc.embeddings(wav)
    assert emb.shape[-1] == -(-wav.shape[-1] // 320)                   # T = ceil(L / hop)
    np.testing.assert_allclose(emb[:, :, :4].numpy(), g["emb"], atol=1e-6, rtol=0)
    codes = orc.quantize(emb)
    assert codes.shape == g["codes"].shape
    np.testing.assert_array_equal(codes, g["codes"])


def test_rvq_codes_are_nearest_neighbours():
    """Domain property of the RVQ (size independent): code q of every frame is the codeword nearest to the residual left
    by codebooks 0..q-1 (checked in float64 against the brute-force distance), i.e. encode is greedy residual quantisation."""
    dec_sd = encodec_state_dict(3)
    orc = EncodecEncoderOracle(encodec_encoder_state_dict(4), dec_sd)
    emb = orc.embeddings(case_wav("encodec_enc_7777"))
    codes = orc.quantize(emb)                                           # (B, T, 8)
    residual = emb.numpy().astype(np.float64)[0].T                      # (T, 128)
    for q in range(8):
        e = dec_sd[f"quantizer.{q}.embed"].astype(np.float64)           # (1024, 128)
        d = ((residual[:, None, :] - e[None]) ** 2).sum(-1)             # (T, 1024)
        chosen = d[np.arange(d.shape[0]), codes[0, :, q]]
        assert np.all(chosen <= d.min(1) + 1e-4)                        # fp32 distance ties within rounding
        residual = residual - e[codes[0, :, q]]


def test_state_dict_normalisation_folds_weight_norm():
    sd = encodec_state_dict(3)
    rng = np.random.default_rng(0)
    pkg = {}                                        # the `encodec` package's naming, weight_g / weight_v form
    for k, v in sd.items():
        if k.startswith("quantizer."):
            pkg[f"quantizer.vq.layers.{k.split('.')[1]}._codebook.embed"] = v
        elif ".lstm." in k:
            pkg["decoder.model." + k[len("decoder."):]] = v
        else:
            i, rest = k[len("decoder."):].split(".", 1)
            sub, leaf = ("", rest) if rest in ("weight", "bias") else rest.rsplit(".", 1)
            sub = {"": "", "block1": "block.1.", "block3": "block.3.", "shortcut": "shortcut."}[sub]
            inner = "convtr.convtr." if (int(i) in (3, 6, 9, 12) and sub == "") else "conv.conv."
            if leaf == "bias":
                pkg[f"decoder.model.{i}.{sub}{inner}bias"] = v
            else:
                g = rng.uniform(0.5, 2.0, size=(v.shape[0],) + (1,) * (v.ndim - 1)).astype(np.float32)
                n = np.sqrt((v.astype(np.float64) ** 2).reshape(v.shape[0], -1).sum(1)).reshape(g.shape)
                pkg[f"decoder.model.{i}.{sub}{inner}weight_g"] = (n * 1.0).astype(np.float32)      # g = ||v||  ->  w = v
                pkg[f"decoder.model.{i}.{sub}{inner}weight_v"] = v
    pkg["encoder.model.0.conv.conv.weight_v"] = np.zeros((4, 4, 4), np.float32)                 # ignored
    same = canonical_encodec_state_dict(sd)                          # canonical names pass through unchanged
    assert set(same) == set(sd) and all(np.array_equal(same[k], sd[k]) for k in sd)
    canon = canonical_encodec_state_dict(pkg)
    assert set(canon) == set(sd)
    for k in sd:
        np.testing.assert_allclose(canon[k], sd[k], atol=1e-6, rtol=1e-6)


@pytest.mark.gpu
def test_hip_decoder_matches_transformers_port():
    from tests._util import get_model
    m = get_model(2, 0, 2.5, max_new=64, max_batch=4)
    m.load_encodec_state_dict(encodec_state_dict(3))
    tok = AudioTokenizer(device="cuda:0", valle=m)
    for name in CASES:
        codes = case_codes(name)                                        # (B, T, 8)
        g = np.load(os.path.join(GOLD, name + ".npz"))["audio"]
        import torch
        out = tok.decode([(torch.from_numpy(codes).permute(0, 2, 1), None)]).numpy()[:, 0]
        assert out.shape == g.shape
        err = np.abs(out - g)
        assert err.max() <= 2e-5, (name, err.max())                      # audio amplitude ~0.15: fp32 reassociation only
        assert float(np.sqrt(np.mean(err ** 2))) <= 1e-5
    # ragged batch: two sequences of different length decoded together == decoded alone
    c0, c1 = case_codes("encodec_T37")[0], case_codes("encodec_T5")[0]
    both = m.engine.encodec_decode([c0, c1])
    np.testing.assert_allclose(both[1], np.load(os.path.join(GOLD, "encodec_T5.npz"))["audio"][0], atol=2e-5, rtol=0)
    np.testing.assert_allclose(both[0], np.load(os.path.join(GOLD, "encodec_T37.npz"))["audio"][0], atol=2e-5, rtol=0)


def test_canonical_state_dict_covers_the_encoder():
    """transformers-port names (parametrised weight-norm) of encoder + decoder -> the canonical folded names the C ABI loads."""
    from oracle.make_golden_encodec import load_into_transformers
    dec, enc = encodec_state_dict(3), encodec_encoder_state_dict(4)
    tsd = load_into_transformers(dec, enc).state_dict()
    canon = canonical_encodec_state_dict(tsd)
    want = dict(dec)
    want.update(enc)
    assert set(canon) == set(want)
    for k in want:
        np.testing.assert_allclose(canon[k], want[k], atol=1e-6, rtol=1e-6)


def _codes_agree_up_to_ties(got, gold, emb, dec_sd, tol=1e-4):
    """RVQ codes can legitimately differ from another fp32 implementation where two codewords are (nearly) equidistant
    (the GEMM summation order decides).  Accept a frame if its codes are equal, or if at the FIRST differing codebook both
    candidates are within `tol` (relative) of the minimum distance in float64; later codebooks of that frame then differ
    by construction and are not compared.  Returns the number of frames that used the tie rule."""
    ties = 0
    T = gold.shape[0]
    for t in range(T):
        if (got[t] == gold[t]).all():
            continue
        q = int(np.argmax(got[t] != gold[t]))
        r = emb[:, t].astype(np.float64)
        for j in range(q):
            r = r - dec_sd[f"quantizer.{j}.embed"][gold[t, j]].astype(np.float64)
        e = dec_sd[f"quantizer.{q}.embed"].astype(np.float64)
        d = ((r[None] - e) ** 2).sum(1)
        assert d[got[t, q]] <= d.min() * (1 + tol) + 1e-9, (t, q, d[got[t, q]], d.min())
        ties += 1
    return ties


@pytest.mark.gpu
def test_hip_encoder_matches_transformers_port():
    from tests._util import get_model
    m = get_model(2, 0, 2.5, max_new=64, max_batch=4)
    dec = encodec_state_dict(3)
    sd = dict(dec)
    sd.update(encodec_encoder_state_dict(4))
    m.load_encodec_state_dict(sd)
    tok = AudioTokenizer(device="cuda:0", valle=m)
    orc = EncodecEncoderOracle(encodec_encoder_state_dict(4), dec)
    for name in ENC_CASES:
        wav = case_wav(name)                                            # (B, L)
        gold = np.load(os.path.join(GOLD, name + ".npz"))["codes"]      # (B, T, 8)
        frames = tok.encode(wav[:, None, :])
        assert len(frames) == 1 and frames[0][1] is None
        got = np.transpose(np.asarray(frames[0][0]), (0, 2, 1))         # (B, 8, T) -> (B, T, 8)
        assert got.shape == gold.shape
        emb = orc.embeddings(wav).numpy()
        # integer output: the bar is equality.  Measured on MI355X (profiles/r03_rvq_ties.log): all 101 frames x 8 codebooks of
        # both fixtures bit-identical, 0 frames decided by a near-tie.  The tie analysis stays as the failure diagnosis: it
        # tells a legitimate fp32 near-tie of the nearest-codeword search (both candidates within 1e-4 relative of the float64
        # minimum distance) from a real defect.
        ties = sum(_codes_agree_up_to_ties(got[b], gold[b], emb[b], dec) for b in range(got.shape[0]))
        frames = gold.shape[0] * gold.shape[1]
        print(f"{name}: {frames - ties} of {frames} frames bit-identical on all 8 codebooks, {ties} decided by a near-tie")
        assert ties == 0, f"{ties} of {frames} frames differ from the port at a near-tie of the codeword search"
        np.testing.assert_array_equal(got, gold)


@pytest.mark.gpu
def test_hip_encoder_matches_the_oracle_on_short_prompts():
    """waveforms at which the host geometry of the strided convs enters its short-input branch (an input not longer than a conv's
    pad is zero-extended before the reflect: 1, 2 samples; one frame and the lengths around it: 319, 320, 321; two frames and one
    sample: 641), batched two at a time with unequal lengths, against the CPU oracle on every waveform alone.  Integer output: the
    bar is equality wherever the float64 gap between the two nearest codewords allows it (_codes_agree_up_to_ties)."""
    from tests._util import get_model
    m = get_model(2, 0, 2.5, max_new=64, max_batch=4)
    dec = encodec_state_dict(3)
    sd = dict(dec)
    sd.update(encodec_encoder_state_dict(4))
    m.load_encodec_state_dict(sd)
    orc = EncodecEncoderOracle(encodec_encoder_state_dict(4), dec)
    rng = np.random.default_rng(9)
    wavs = {L: (0.1 * rng.standard_normal(L)).astype(np.float32) for L in (1, 2, 100, 319, 320, 321, 641)}
    ties = frames = 0
    for pair in ((1, 641), (321, 2), (100, 320), (319, 1)):
        got = m.engine.encodec_encode([wavs[L] for L in pair])
        for L, codes in zip(pair, got):
            emb = orc.embeddings(wavs[L][None])
            gold = orc.quantize(emb)[0]
            assert codes.shape == gold.shape == (-(-L // 320), 8), (L, codes.shape)
            assert codes.min() >= 0 and codes.max() < 1024
            ties += _codes_agree_up_to_ties(codes, gold, emb.numpy()[0], dec)
            frames += len(gold)
    print(f"short prompts: {frames - ties} of {frames} frames bit-identical on all 8 codebooks, {ties} decided by a near-tie")


@pytest.mark.gpu
def test_hip_encoder_keeps_codes_in_range_for_a_non_finite_sample():
    """one NaN sample in a prompt waveform leaves frames without any comparable codeword distance: every code the encoder returns
    must still be a table index (rvq_select_kernel: such a frame gets code 0), for the row with the NaN and for its batch neighbour"""
    from tests._util import get_model
    m = get_model(2, 0, 2.5, max_new=64, max_batch=4)
    dec = encodec_state_dict(3)
    sd = dict(dec)
    sd.update(encodec_encoder_state_dict(4))
    m.load_encodec_state_dict(sd)
    rng = np.random.default_rng(10)
    wav = (0.1 * rng.standard_normal(1000)).astype(np.float32)
    clean = m.engine.encodec_encode([wav])[0]
    wav_nan = wav.copy()
    wav_nan[500] = np.nan
    bad, other = m.engine.encodec_encode([wav_nan, wav])
    assert bad.shape == other.shape == (4, 8)
    assert bad.min() >= 0 and bad.max() < 1024, bad
    np.testing.assert_array_equal(other, clean)                        # the neighbour of the batch is not affected
    assert m.engine.encodec_decode([bad])[0].shape == (4 * 320,)       # and the codes can be gathered by


@pytest.mark.gpu
def test_make_prompt_writes_a_reference_format_preset(tmp_path):
    """prompt enrolment end to end (utils/prompt_making.py:57-84): waveform -> EnCodec encoder + RVQ on the GPU -> .npz in the
    reference's wire format -> usable as `prompt=` of generate_audio."""
    from scipy.io import wavfile
    from oracle import synth
    from vallex_amd.utils import generation as G
    from vallex_amd.utils import prompt_making as PM
    dec = encodec_state_dict(3)
    sd = dict(dec)
    sd.update(encodec_encoder_state_dict(4))
    G.preload_models(state_dict=synth.vallex_state_dict(2, 11), vocos_state_dict=synth.vocos_state_dict(2), num_layers=2, max_new=64,
                     max_prompt=128, max_text=64, max_batch=2)
    G.model.load_encodec_state_dict(sd)
    PM.codec = None
    G.language_detector = lambda text: "en"
    G.text_tokenizer = lambda text: ([5 + (ord(ch) % 60) for ch in text], ["en"] * len(text))
    try:
        rng = np.random.default_rng(3)
        wav = (0.1 * rng.standard_normal((2, 7777))).astype(np.float32)                    # stereo, not a multiple of the hop
        path = PM.make_prompt("unit", (wav, 24000), transcript="hello there", save_dir=str(tmp_path))
        d = np.load(path)
        T = -(-7777 // 320)
        assert d["audio_tokens"].shape == (1, T, 8) and d["audio_tokens"].min() >= 0 and d["audio_tokens"].max() < 1024
        assert d["text_tokens"].shape == (1, len("[EN]hello there[EN]")) and int(d["lang_code"]) == 2
        # the same codes as encoding the mono mix directly
        tok = AudioTokenizer(device="cuda:0", valle=G.model)
        direct = np.asarray(tok.encode(wav.mean(0, keepdims=True)[None])[0][0])
        np.testing.assert_array_equal(np.transpose(direct, (0, 2, 1)), d["audio_tokens"])
        # a WAV file on disk gives the same preset (16-bit PCM round trip aside: use float WAV)
        wavfile.write(str(tmp_path / "p.wav"), 24000, wav.T)
        d2 = np.load(PM.make_prompt("unit2", str(tmp_path / "p.wav"), transcript="hello there", save_dir=str(tmp_path)))
        np.testing.assert_array_equal(d2["audio_tokens"], d["audio_tokens"])
        # and it drops into generate_audio
        out = G.generate_audio(synth.synth_text(6, 1), prompt=path, language="en", uniforms=synth.uniforms(32, 1, 5)[:, 0], force_eos_at=8)
        assert out.shape == (8 * 320,) and np.isfinite(out).all()
        with pytest.raises(ValueError, match="too long"):
            PM.make_prompt("long", (np.zeros((1, 24000 * 16), np.float32), 24000), transcript="x", save_dir=str(tmp_path))
        # another sample rate is resampled to 24 kHz first (data/tokenizer.py:105): 8000 samples at 16 kHz -> 12000 -> 38 frames
        # (this engine's arena holds max_new = 64 frames)
        w16 = (0.1 * rng.standard_normal((1, 8000))).astype(np.float32)
        d3 = np.load(PM.make_prompt("sr", (w16, 16000), transcript="x", save_dir=str(tmp_path)))
        assert d3["audio_tokens"].shape == (1, 38, 8)
        direct = np.asarray(tok.encode(PM.resample_sinc_hann(w16, 16000, 24000)[None])[0][0])
        np.testing.assert_array_equal(np.transpose(direct, (0, 2, 1)), d3["audio_tokens"])
    finally:
        G.language_detector = None
        G.text_tokenizer = None
