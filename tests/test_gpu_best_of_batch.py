"""GPU: best_of = N > 1 for every row of a multi-row call (vx_infer decodes R = min(max_batch, 32) // N rows x N beams per
micro-batch, one prefill per row fanned out to its beams).  Row r must return exactly what a batch-1 best_of call on that row alone
returns with the same draws (uniforms column r*N + j = beam j of row r), and a row taken from a live-reference golden must come back
bit for bit wherever it sits in the batch."""
import os

import numpy as np
import pytest

from oracle import synth
from oracle.make_golden import CASES, UI_CASES, case_inputs, load_preset
from tests import _util
from tests._util import case_model, case_row, golden

pytestmark = pytest.mark.gpu


def _filler(preset, n_text, seed, lang, frames=None):
    """a row from a committed preset prompt (its first `frames` frames) with synthetic text of its own length"""
    a, t, pl = load_preset(preset)
    return dict(text=np.concatenate([t[0], synth.synth_text(n_text, seed)]), prompt=a[0, :frames], enroll=t.shape[-1],
                prompt_language=pl, text_language=lang)


def _ui_row(c):
    a, t, text, pl, langs = case_inputs(c)
    return dict(text=text[0], prompt=a[0], enroll=t.shape[-1], prompt_language=pl, text_language=langs)


def _run(m, rows, c, us, n, **kw):
    return m.inference_batch(rows, top_k=c["top_k"], temperature=c.get("temperature", 1.0), uniforms=us,
                             force_eos_at=c["force_eos_at"], best_of=n, length_penalty=c.get("length_penalty", 1.0),
                             return_worst=c.get("return_worst", False), **kw)


def _check_rows(m, rows, c, us, n, outs, skip=()):
    """every row of a batched call equals the batch-1 best_of call on that row with its own uniform columns"""
    for i, r in enumerate(rows):
        if i in skip:
            continue
        alone = _run(m, [r], c, us[:, i * n:(i + 1) * n], n)[0]
        np.testing.assert_array_equal(outs[i], alone, err_msg=f"row {i} of {len(rows)}")


UI_FILLERS = [("paimon", 25, 71, "en"), ("librispeech_1", 60, 72, "zh"), ("cafe", 12, 73, "ja", 200), ("librispeech_1", 90, 74, "en", 150),
              ("paimon", 40, 75, "zh", 120)]


@pytest.mark.parametrize("arith", ["default", "f32"])
@pytest.mark.parametrize("name", ["nl12_ui_bestof5_ja", "nl12_ui_bestof5_ja_worst"])
def test_ui_call_batched_six_rows_of_five_beams(name, arith):
    """the reference UI's call (top_k=-100, temperature 1, best_of=5) for 6 requests at once: 30 decode rows in one micro-batch,
    the live-reference golden as row 2, five preset-prompt rows of different lengths around it"""
    c = UI_CASES[name]
    n = c["best_of"]
    m = case_model(c, arith=arith, max_new=128, max_prompt=700, max_text=256, max_batch=32)
    rows = [_filler(*f) for f in UI_FILLERS]
    rows.insert(2, _ui_row(c))
    us = np.concatenate([synth.uniforms(4096, n, 9_100 + i) if i != 2 else synth.uniforms(4096, n, c["useed"])
                         for i in range(len(rows))], axis=1)
    outs = _run(m, rows, c, us, n)
    np.testing.assert_array_equal(outs[2], golden(name)["codes"][0])
    _check_rows(m, rows, c, us, n, outs, skip=(2,))


@pytest.mark.parametrize("name", ["nl2_bestof3", "nl2_bestof3_worst"])
def test_micro_batch_boundaries(name):
    """max_batch = 6 with best_of = 3: two rows (six decode rows) per micro-batch.  The golden is row 3 = the second row of the second
    micro-batch (uniform column slice 9 .. 11, slot map with unequal contexts); the last micro-batch holds one row"""
    c, row, gus = case_row(name)
    n = c["best_of"]
    m = case_model(c, max_batch=6)
    rows = [_filler("librispeech_1", 14, 81, "en", 90), _filler("paimon", 6, 82, "zh"), _filler("cafe", 22, 83, "ja", 140), row,
            _filler("librispeech_1", 9, 84, "en", 60)]
    us = np.concatenate([gus if i == 3 else synth.uniforms(4096, n, 9_200 + i) for i in range(len(rows))], axis=1)
    outs = _run(m, rows, c, us, n)
    st = m.engine.last_stats()
    np.testing.assert_array_equal(outs[3], golden(name)["codes"][0])
    assert st["ar_ms"] > 0 and st["nar_ms"] > 0, st
    assert st["frames"] == sum(len(o) for o in outs), st
    _check_rows(m, rows, c, us, n, outs, skip=(3,))


def test_range_fallback_redoes_the_fan_out():
    """weights whose FFN activations leave the fp16 range: the prefill of the micro-batch is re-run on the exact-fp32 kernels, and
    the fan-out behind it must run again (row 1 of 3, nine decode rows)"""
    name = "nl2_bestof3"
    c, row, gus = case_row(name)
    n = c["best_of"]
    sd = synth.out_of_range_state_dict(synth.vallex_state_dict(c["num_layers"], c["seed"], c["eos_gain"]), c["num_layers"], "ffn")
    m = _util.VALLE(1024, 16, c["num_layers"], norm_first=True, add_prenet=False, prefix_mode=1, share_embedding=True,
                    nar_scale_factor=1.0, prepend_bos=True, num_quantizers=8, engine_max_new=320, engine_max_prompt=400,
                    engine_max_text=256, engine_max_batch=12)
    m.to("cuda:0").load_state_dict(sd, strict=True)
    rows = [_filler("librispeech_1", 18, 91, "en", 100), row, _filler("cafe", 5, 92, "ja", 70)]
    us = np.concatenate([gus if i == 1 else synth.uniforms(4096, n, 9_300 + i) for i in range(len(rows))], axis=1)
    outs = _run(m, rows, c, us, n)
    assert m.engine.last_fallbacks()["prefill"] >= 1, m.engine.last_fallbacks()
    np.testing.assert_array_equal(outs[1], golden(name)["codes"][0])


def test_seeded_micro_batches_draw_their_own_streams():
    """no uniforms: two identical rows in different micro-batches (max_batch = 3, best_of = 3: one row per micro-batch) must not
    draw the same beams; the first micro-batch keeps the caller's seed, so a batch-1 call is unchanged by the feature"""
    c = CASES["nl2_full_multinomial"]
    _, row, _ = case_row("nl2_full_multinomial")
    m = case_model(c, max_batch=3)
    kw = dict(top_k=-100, temperature=1.0, force_eos_at=32, best_of=3, seed=20_261_016)
    before = m.inference_batch([row], **kw)[0]
    outs = m.inference_batch([row, row], **kw)
    after = m.inference_batch([row], **kw)[0]
    np.testing.assert_array_equal(before, after)
    np.testing.assert_array_equal(outs[0], before)
    assert outs[0].shape != outs[1].shape or not np.array_equal(outs[0], outs[1]), "both micro-batches drew the same beams"


def test_python_api_best_of_batch():
    """generate_audio_batch(..., best_of=3) returns one waveform of 320 x frames samples per utterance, each equal to
    generate_audio on that utterance with its three uniform columns; VALLE.inference_batch row i equals VALLE.inference(row i)"""
    from vallex_amd.utils import generation as G
    n = 3
    G.preload_models(state_dict=synth.vallex_state_dict(2, 11), vocos_state_dict=synth.vocos_state_dict(2), num_layers=2, max_new=320,
                     max_prompt=400, max_text=256, max_batch=8)
    pdir = os.path.join(os.path.dirname(__file__), "golden", "presets")
    texts = [synth.synth_text(12, 41), synth.synth_text(7, 42), synth.synth_text(15, 43)]
    prompts = [os.path.join(pdir, "paimon.npz"), None, os.path.join(pdir, "cafe.npz")]
    langs = ["en", "zh", "ja"]
    us = synth.uniforms(64, 3 * n, 321)
    wavs = G.generate_audio_batch(texts, prompts=prompts, language=langs, uniforms=us, force_eos_at=20, best_of=n)
    assert len(wavs) == 3
    for i in range(3):
        assert len(wavs[i]) % 320 == 0 and len(wavs[i]) <= 20 * 320, len(wavs[i])
        alone = G.generate_audio(texts[i], prompt=prompts[i], language=langs[i], uniforms=us[:, n * i:n * i + n], force_eos_at=20,
                                 best_of=n)
        np.testing.assert_array_equal(wavs[i], alone)
    m = G.model
    rows = [_filler("librispeech_1", 10, 51, "en", 80), _filler("paimon", 16, 52, "zh"), _filler("cafe", 4, 53, "ja", 50)]
    outs = m.inference_batch(rows, top_k=10, uniforms=us, force_eos_at=24, best_of=n)
    for i, r in enumerate(rows):
        one = m.inference(r["text"][None], np.array([len(r["text"])]), r["prompt"][None], r["enroll"], top_k=10,
                          prompt_language=r["prompt_language"], text_language=r["text_language"], uniforms=us[:, n * i:n * i + n],
                          force_eos_at=24, best_of=n)
        np.testing.assert_array_equal(outs[i], one.numpy()[0])
