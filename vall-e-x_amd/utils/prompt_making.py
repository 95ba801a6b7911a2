"""Prompt enrolment on MI355X: mirror of the reference's `utils/prompt_making.make_prompt` (utils/prompt_making.py:57-84) and
`data/tokenizer.tokenize_audio` (data/tokenizer.py:99-111) -- waveform in, `.npz` voice preset out, in the reference's wire format
(`audio_tokens (1, T, 8)`, `text_tokens (1, S)`, `lang_code`), so the file drops into `generate_audio(prompt=...)` of either
implementation.  The audio side (EnCodec SEANet encoder + RVQ, 6 kbps) runs in libvallex_hip.so (`vx_encodec_encode`).

What is NOT here (third-party CPU code outside the hot path): Whisper transcription (pass `transcript=`), the G2P /
BPE tokenizer and langid (same pluggable hooks as `utils.generation`).  Audio at another sample rate is resampled to 24 kHz like the
reference does (data/tokenizer.py:105 `convert_audio` = `torchaudio.transforms.Resample(sr, 24000)`): `resample_sinc_hann` below restates
torchaudio's published default (Hann-windowed sinc, lowpass_filter_width 6, rolloff 0.99) -- torchaudio is not installed here, so this
one piece is NOT pinned to the package; assign `resampler = lambda wav, sr, target_sr: ...` to plug in the real one.
`device_resampler` is the same (unpinned) algorithm on the GPU (`vx_resample`): `resampler = device_resampler` plugs it in, and it is
what a process WITHOUT torch gets on its own (the built-in needs torch).  Stereo is averaged like the reference does
(utils/prompt_making.py:63-64).
"""
from __future__ import annotations

import logging
import math
import os
from typing import Callable, Optional, Tuple, Union

import numpy as np

from ..data.tokenizer import AudioTokenizer
from ..macros import lang2code, lang2token
from . import generation as G

codec: Optional[AudioTokenizer] = None        # module global like the reference's (utils/prompt_making.py:27)
CUSTOMS_DIR = "./customs/"
resampler: Optional[Callable[[np.ndarray, int, int], np.ndarray]] = None      # (wav (C, L), sr, target_sr) -> (C, L'); None = built-in


def resample_sinc_hann(wav: np.ndarray, orig_freq: int, new_freq: int, lowpass_filter_width: int = 6,
                       rolloff: float = 0.99) -> np.ndarray:
    """Band-limited resampling of (C, L) fp32 audio: the algorithm torchaudio documents for `transforms.Resample` with its defaults
    (resampling_method "sinc_interp_hann").  With o, n = the two rates over their gcd: n phase kernels of 2*width + o taps,
    k_i[j] = sinc(t) * cos^2(pi t / (2 lpw)) * base / o with t = clamp((-i / n + (j - width) / o) * base, +-lpw), base =
    min(o, n) * rolloff, width = ceil(lpw * o / base) (built in fp64, applied in fp32); the zero-padded signal is correlated at
    stride o, the n phases interleave to the output, cut to ceil(n * L / o) samples."""
    import torch
    import torch.nn.functional as F
    wav = np.asarray(wav, np.float32)
    g = math.gcd(int(orig_freq), int(new_freq))
    o, n = int(orig_freq) // g, int(new_freq) // g
    if o == n:
        return wav
    base = min(o, n) * rolloff
    width = math.ceil(lowpass_filter_width * o / base)
    idx = torch.arange(-width, width + o, dtype=torch.float64)[None, None] / o
    # torchaudio's _get_sinc_resample_kernel with dtype=None: the phase term is an int64 arange divided in fp32 and promoted to
    # fp64 when idx is added -- reproduced so that the fp32 taps are the package's bit for bit
    t = ((torch.arange(0, -n, -1).to(torch.float32) / n).to(torch.float64)[:, None, None] + idx) * base
    t = t.clamp_(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    kernels = (torch.where(t == 0, torch.ones_like(t), t.sin() / t) * window * (base / o)).to(torch.float32)    # (n, 1, 2*width + o)
    x = torch.from_numpy(np.ascontiguousarray(wav.reshape(-1, wav.shape[-1])))
    length = x.shape[-1]
    x = F.pad(x, (width, width + o))
    y = F.conv1d(x[:, None], kernels, stride=o).transpose(1, 2).reshape(x.shape[0], -1)
    y = y[:, : math.ceil(n * length / o)]
    return y.reshape(wav.shape[:-1] + (y.shape[-1],)).numpy()


def device_resampler(wav: np.ndarray, sr: int, target_sr: int) -> np.ndarray:
    """`resampler` hook on the device: (C, L) fp32 at sr -> (C, ceil(n L / o)) at target_sr through the loaded model's engine
    (Engine.resample, vx_resample) -- resample_sinc_hann's taps and sums, K fmaf per sample, every channel a row of one launch."""
    if G.model is None:
        raise RuntimeError("call preload_models() first: the device resampler runs on the loaded model's engine")
    wav = np.asarray(wav, np.float32)
    rows = G.model.engine.resample(list(wav.reshape(-1, wav.shape[-1])), int(sr), int(target_sr))
    return np.stack(rows).reshape(wav.shape[:-1] + (rows[0].shape[-1],))


def _builtin_resampler() -> Callable[[np.ndarray, int, int], np.ndarray]:
    """`resampler is None`: the torch restatement -- enrolment results do not change -- and, only where torch cannot be imported
    (that case used to raise), the device path."""
    try:
        import torch  # noqa: F401
    except ImportError:
        return device_resampler
    return resample_sinc_hann


def _load_wav(path: str) -> Tuple[np.ndarray, int]:
    from scipy.io import wavfile                     # PCM / float WAV; the reference uses torchaudio.load
    sr, data = wavfile.read(path)
    if data.dtype.kind == "i":
        data = data.astype(np.float32) / float(np.iinfo(data.dtype).max + 1)
    elif data.dtype.kind == "u":
        data = (data.astype(np.float32) - 128.0) / 128.0
    data = np.asarray(data, np.float32)
    wav = data[None, :] if data.ndim == 1 else data.T            # (channels, samples) like torchaudio
    return wav, int(sr)


TRIM_FRAME, TRIM_KEEP = 240, 2400      # trim_db: 10 ms analysis frames at 24 kHz, 100 ms kept on both sides of the spoken span


def trim_silence(wav: np.ndarray, trim_db: float) -> np.ndarray:
    """(1, L) mono fp32 at 24 kHz -> (1, L') without the leading and trailing frames whose mean square is below 10^(trim_db / 10), on the
    loaded model's engine (Engine.finish, vx_finish: trim both sides, keep TRIM_KEEP samples; level and format untouched).  Silence in
    front of a prompt costs prompt frames of the KV arena on every request that uses it."""
    if G.model is None:
        raise RuntimeError("call preload_models() first: trim_db runs on the loaded model's engine")
    rows, infos = G.model.engine.finish([wav.reshape(-1)], TRIM_FRAME, silence_db=float(trim_db), trim=3, keep=TRIM_KEEP)
    if infos[0]["active_frames"] == 0:
        raise ValueError(f"no 10 ms frame of the prompt is above trim_db = {trim_db} dB: the clip is silent")
    return np.array(rows[0], np.float32)[None]


PROMPT_CEILING_DB = -1.0               # lufs: the sample peak of a levelled clip stays below this


def level_loudness(wav: np.ndarray, lufs: float, sample_rate: int) -> np.ndarray:
    """(1, L) mono fp32 at sample_rate -> the clip at `lufs` LUFS (BS.1770), on the loaded model's engine (Engine.finish_loud,
    vx_finish_loud: no trim, fp32 out, sample peak at most PROMPT_CEILING_DB dBFS).  The loudness of a cloned voice follows the
    loudness of its enrolment clip."""
    if G.model is None:
        raise RuntimeError("call preload_models() first: lufs runs on the loaded model's engine")
    rows, _ = G.model.engine.finish_loud([wav.reshape(-1)], int(sample_rate), float(lufs), PROMPT_CEILING_DB)
    return np.array(rows[0], np.float32)[None]


def shift_pitch(wav: np.ndarray, pitch) -> np.ndarray:
    """(1, L) mono fp32 at 24 kHz -> the clip at `pitch` (semitones, or the ratio as a Fraction or a (num, den) pair) with the same
    length, on the loaded model's engine (Engine.shift: vx_stretch, then vx_resample).  The pitch of a cloned voice follows the pitch
    of its enrolment clip; the formants move along, so this is meant for a few semitones -- a utils.generation.Pitch as `pitch` keeps
    them (vx_f0, then vx_psola)."""
    if G.model is None:
        raise RuntimeError("call preload_models() first: pitch runs on the loaded model's engine")
    return np.array(G.model.engine.shift([wav.reshape(-1)], pitch)[0], np.float32)[None]


def suppress_noise(wav: np.ndarray, denoise) -> np.ndarray:
    """(1, L) mono fp32 -> the clip with its steady noise (hiss, a fan) suppressed, same length, on the loaded model's engine
    (Engine.denoise: vx_denoise).  A zero-shot model clones the recording, not only the voice: the noise of an enrolment clip would be
    in every utterance.  denoise: True for the defaults, or a utils.generation.Denoise (chosen values, or a stored noise profile -- what
    a clip of continuous speech needs, which has no quiet frames to take one from)."""
    if G.model is None:
        raise RuntimeError("call preload_models() first: denoise runs on the loaded model's engine")
    return np.array(G.model.engine._denoised([wav.reshape(-1)], denoise)[0], np.float32)[None]


def equalise(wav: np.ndarray, eq, sample_rate: int) -> np.ndarray:
    """(1, L) mono fp32 at sample_rate -> the clip through `eq` (a utils.generation.Eq, resolved at sample_rate, or (n, 5) sections),
    same length, on the loaded model's engine (Engine.eq: vx_eq).  A zero-shot model clones the recording: a DC offset, desk rumble
    or the boom of a close microphone would be in every utterance, and would decide which frames `suppress_noise` takes for noise --
    Eq.rumble() in front of it is what a studio chain does first."""
    if G.model is None:
        raise RuntimeError("call preload_models() first: eq runs on the loaded model's engine")
    return np.array(G.model.engine._equalised([wav.reshape(-1)], eq, int(sample_rate))[0], np.float32)[None]


def shorten_pauses(wav: np.ndarray, max_pause_ms: float, sample_rate: int) -> np.ndarray:
    """(1, L) mono fp32 at sample_rate -> the clip with every pause inside the speech held to max_pause_ms, on the loaded model's
    engine (Engine.pauses and Engine.retime: vx_pauses, vx_retime; utils.generation.Pauses' defaults otherwise).  The speech keeps
    its bits.  A long gap in an enrolment clip costs prompt frames of the KV arena on every request that uses it, as silence in
    front of it does."""
    if G.model is None:
        raise RuntimeError("call preload_models() first: max_pause_ms runs on the loaded model's engine")
    return np.array(G.model.engine._paused([wav.reshape(-1)], G.Pauses(max_ms=float(max_pause_ms)), int(sample_rate))[0], np.float32)[None]


def tokenize_audio(tokenizer: AudioTokenizer, audio: Union[str, Tuple[np.ndarray, int]], trim_db: Optional[float] = None,
                   lufs: Optional[float] = None, pitch=None, denoise=None, max_pause_ms: Optional[float] = None, eq=None):
    """data/tokenizer.py:99-111: (path | (wav (C, L), sr)) -> `tokenizer.encode(wav[None])` = [(codes (1, 8, T), None)].
    trim_db (no reference counterpart; None = the clip as it is): `trim_silence` on the 24 kHz mono clip before the encoder sees it.
    lufs (no reference counterpart; None = the clip's own level): `level_loudness` on that clip, after the trim.
    pitch (no reference counterpart; None = the clip's own pitch): `shift_pitch` on the 24 kHz mono clip, before the trim.
    eq (no reference counterpart; None = the clip's own spectrum): `equalise` on the mono clip at the tokenizer's rate, first of all,
    so that a DC offset or rumble does not choose the noise frames of `denoise`.
    denoise (no reference counterpart; None = the clip as recorded): `suppress_noise` on the mono clip, behind eq and in front of
    everything else.
    max_pause_ms (no reference counterpart; None = the clip's own pauses): `shorten_pauses` on the mono clip, behind denoise and
    pitch and in front of the trim."""
    wav, sr = _load_wav(audio) if isinstance(audio, str) else audio
    wav = np.asarray(wav.detach().cpu().numpy() if hasattr(wav, "detach") else wav, np.float32)
    if wav.ndim == 1:
        wav = wav[None]
    if wav.shape[0] > 1:                                          # convert_audio(..., target_channels=1): channel mean, then resample
        wav = wav.mean(0, keepdims=True)
    if sr != tokenizer.sample_rate:
        wav = np.asarray((resampler or _builtin_resampler())(wav, int(sr), tokenizer.sample_rate), np.float32)
    if eq is not None:
        wav = equalise(wav, eq, tokenizer.sample_rate)
    if denoise is not None:
        wav = suppress_noise(wav, denoise)
    if pitch is not None:
        if tokenizer.sample_rate != 24000:
            raise ValueError(f"pitch: Engine.shift works at 24 kHz, the tokenizer at {tokenizer.sample_rate}")
        wav = shift_pitch(wav, pitch)
    if max_pause_ms is not None:
        wav = shorten_pauses(wav, max_pause_ms, tokenizer.sample_rate)
    if trim_db is not None:
        wav = trim_silence(wav, trim_db)
    if lufs is not None:
        wav = level_loudness(wav, lufs, tokenizer.sample_rate)
    return tokenizer.encode(wav[None])                            # (1, 1, L)


def make_transcript(name, wav, sr, transcript: Optional[str] = None):
    """utils/prompt_making.py:87-120 without Whisper: the transcript must be given; language from the detector hook.
    Like the reference (:91-92, `wav /= wav.abs().max()` on the caller's FloatTensor) a waveform whose peak exceeds 1 is
    normalised IN PLACE, so the audio that `tokenize_audio` encodes afterwards is the normalised one."""
    if isinstance(wav, np.ndarray) and wav.size and float(np.abs(wav).max()) > 1:
        wav /= np.abs(wav).max()
    if transcript is None or transcript == "":
        raise RuntimeError("no transcript given: the reference transcribes with Whisper here (utils/prompt_making.py:99-110), which "
                           "is outside this package; pass transcript=")
    if G.language_detector is None:
        raise RuntimeError("set vallex_amd.utils.generation.language_detector (the reference uses langid.classify, "
                           "utils/prompt_making.py:113)")
    lang = G.language_detector(transcript)
    lang_token = lang2token[lang]
    return lang_token + transcript + lang_token, lang


def make_prompt(name: str, audio_prompt_path: Union[str, Tuple[np.ndarray, int]], transcript: Optional[str] = None,
                save_dir: Optional[str] = None, trim_db: Optional[float] = None, lufs: Optional[float] = None, pitch=None,
                denoise=None, max_pause_ms: Optional[float] = None, eq=None) -> str:
    """utils/prompt_making.py:57-84.  `audio_prompt_path`: a WAV path or `(wav (C, L), sr)`.  Returns the path of the written .npz.
    trim_db: as `tokenize_audio` (leading and trailing silence of the clip is cut before it is encoded); lufs: as `tokenize_audio`
    (the clip is brought to that loudness, after the trim, before it is encoded); pitch: as `tokenize_audio` (the clip is shifted by
    that many semitones, or that ratio, before the trim: the cloned voice follows its prompt); denoise: as `tokenize_audio` (the
    clip's steady noise is suppressed in front of everything but eq, so that it is not cloned with the voice); max_pause_ms: as
    `tokenize_audio` (every pause inside the speech is held to that length, behind denoise and pitch and in front of the trim); eq: as
    `tokenize_audio` (the clip goes through the equaliser first of all: Eq.rumble() takes a DC offset and rumble out before the noise
    estimate sees them)."""
    global codec
    if G.model is None:
        raise RuntimeError("call preload_models() first (with EnCodec weights: model.load_encodec_state_dict)")
    if codec is None:
        codec = AudioTokenizer(device=G.device, valle=G.model)
    wav_pr, sr = _load_wav(audio_prompt_path) if isinstance(audio_prompt_path, str) else audio_prompt_path
    wav_pr = np.array(wav_pr, np.float32)                         # own copy: make_transcript may normalise it in place
    if wav_pr.ndim == 1:
        wav_pr = wav_pr[None]
    if wav_pr.shape[-1] / sr > 15:                                # :60-61
        raise ValueError(f"Prompt too long, expect length below 15 seconds, got {wav_pr.shape[-1] / sr} seconds.")
    if wav_pr.shape[0] == 2:                                      # :62-63
        wav_pr = wav_pr.mean(0, keepdims=True)
    text_pr, lang_pr = make_transcript(name, wav_pr, sr, transcript)
    encoded_frames = tokenize_audio(codec, (wav_pr, sr), trim_db=trim_db, lufs=lufs, pitch=pitch, denoise=denoise,
                                    max_pause_ms=max_pause_ms, eq=eq)    # :67
    codes = encoded_frames[0][0]
    codes = codes.numpy() if hasattr(codes, "numpy") else np.asarray(codes)
    audio_tokens = np.transpose(codes, (0, 2, 1))                 # (1, T, 8)   (:68)
    if G.text_tokenizer is None:
        raise RuntimeError("set vallex_amd.utils.generation.text_tokenizer (the reference's PhonemeBpeTokenizer.tokenize)")
    phonemes, _langs = G.text_tokenizer(f"{text_pr}".strip())     # :71
    text_tokens = np.asarray(phonemes, np.int64)[None]            # text_collater([phonemes])  (:72-76)
    d = save_dir if save_dir is not None else CUSTOMS_DIR
    os.makedirs(d, exist_ok=True)
    save_path = os.path.join(d, f"{name}.npz")
    np.savez(save_path, audio_tokens=audio_tokens, text_tokens=text_tokens, lang_code=lang2code[lang_pr])      # :81-82
    logging.info(f"Successful. Prompt saved to {save_path}")
    return save_path
