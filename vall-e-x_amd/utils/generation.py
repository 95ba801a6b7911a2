"""Drop-in for the reference's `utils/generation.py` API on MI355X:

    preload_models()                                                     utils/generation.py:50-89
    generate_audio(text, prompt=None, language='auto', accent='no-accent')        :92-152
    generate_audio_from_long_text(text, prompt=None, language='auto', accent='no-accent', mode='sliding-window')  :155-276

Same signatures, same `.npz` prompt format (keys audio_tokens/text_tokens/lang_code), same return type
(np.float32 (n,)), same exceptions for the same misuse.  Bodies are host glue around the C ABI; AR+NAR and the Vocos
head run in libvallex_hip.so.  The CPU text front-end (G2P cleaners, langid, sentence splitting) is NOT part of the hot
path: it is pluggable through `text_tokenizer` / `sentence_splitter`, exactly like the reference's module
globals, and already-tokenised phoneme ids may be passed in place of `text`.
"""
from __future__ import annotations

import logging
import math
import os
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple, Union

import numpy as np

from ..macros import (NUM_LAYERS, NUM_HEAD, N_DIM, NUM_QUANTIZERS, PREFIX_MODE, SAMPLE_RATE, code2lang,  # noqa: F401
                      lang2token, langdropdown2token, token2lang)
from ..models.vallex import VALLE

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

# module globals, as in the reference (utils/generation.py:30-48)
device = "cuda:0"
model: Optional[VALLE] = None
vocos = None
text_tokenizer: Optional[Callable[[str], Tuple[List[int], List[str]]]] = None   # text -> (phone ids, per-id langs)
sentence_splitter: Optional[Callable[[str], List[str]]] = None
language_detector: Optional[Callable[[str], str]] = None
rng = None      # test hook: an object with .random() replaces the sliding-window coin; None = the reference's own draw,
#                `torch.rand(1) < 0.5` (utils/generation.py:264), which follows torch.manual_seed like the reference does

checkpoints_dir = "./checkpoints/"
model_checkpoint_name = "vallex-checkpoint.pt"
PRESET_DIRS = ["./presets/", "./customs/"]


class VocosHIP:
    """Stand-in for the pip `vocos` object the reference holds (utils/generation.py:89,148-150): the two calls the
    reference makes, fused on the GPU."""

    def __init__(self, valle: VALLE):
        self._m = valle

    def codes_to_features(self, codes):
        c = codes.detach().cpu().numpy() if torch is not None and isinstance(codes, torch.Tensor) else np.asarray(codes)
        assert c.ndim == 3 and c.shape[0] == NUM_QUANTIZERS, c.shape            # (8, B, T)
        return ("codes", np.ascontiguousarray(np.transpose(c, (1, 2, 0))).astype(np.int64))   # (B, T, 8)

    def decode(self, features, bandwidth_id=None):
        tag, codes = features
        assert tag == "codes"
        bid = 2 if bandwidth_id is None else int(np.asarray(
            bandwidth_id.detach().cpu().numpy() if torch is not None and isinstance(bandwidth_id, torch.Tensor)
            else bandwidth_id).reshape(-1)[0])
        audio = self._m.engine.vocos_decode([codes[i] for i in range(codes.shape[0])], bid)
        out = np.stack(audio) if len({a.shape[0] for a in audio}) == 1 else audio
        return torch.from_numpy(out) if torch is not None and isinstance(out, np.ndarray) else out


def _torch_load(path, allow_unsafe_pickle: Optional[bool] = None):
    """torch.load(path, map_location='cpu') as the reference does (utils/generation.py:79), under torch >= 2.6's
    weights_only=True: a checkpoint of plain tensors -- what `["model"]` is -- needs nothing else.  Published training
    checkpoints carry harmless bookkeeping objects next to "model"; the ones known from the reference's trainer
    (argparse.Namespace, pathlib paths, OrderedDict) are allow-listed for this one load.  Anything else is REFUSED: the
    permissive unpickler executes code from the file, so it runs only on an explicit opt-in --
    `allow_unsafe_pickle=True` (preload_models(..., allow_unsafe_pickle=True)) or VALLEX_ALLOW_UNSAFE_PICKLE=1 -- for a
    file whose origin the caller trusts, like the reference's torch 2.0 `torch.load` did for every file."""
    import argparse
    import collections
    import pathlib
    if allow_unsafe_pickle is None:
        allow_unsafe_pickle = os.environ.get("VALLEX_ALLOW_UNSAFE_PICKLE", "") == "1"
    if allow_unsafe_pickle:
        logging.warning(f"{path}: loading with weights_only=False (explicit opt-in): the file can execute arbitrary code")
        return torch.load(path, map_location="cpu", weights_only=False)
    if not hasattr(torch.serialization, "safe_globals"):
        raise RuntimeError(f"torch {torch.__version__} has no torch.serialization.safe_globals (needs torch >= 2.5): the allow-listed "
                           "weights-only load of a training checkpoint is not available; pass allow_unsafe_pickle=True for a file you trust")
    paths = [pathlib.PosixPath, pathlib.PurePosixPath, pathlib.Path]
    # Python >= 3.13 moved the classes to pathlib._local, so `cls.__module__` no longer matches the "pathlib.PosixPath" a checkpoint
    # written by an older interpreter names: register them under the historical name as well (torch accepts (obj, "qualified.name"))
    safe = [argparse.Namespace, collections.OrderedDict] + paths
    safe += [(cls, f"pathlib.{cls.__name__}") for cls in paths if cls.__module__ != "pathlib"]
    try:
        with torch.serialization.safe_globals(safe):
            return torch.load(path, map_location="cpu", weights_only=True)
    except Exception as e:                                   # pickle.UnpicklingError: weights-only refused a global
        if "weights_only" not in str(e) and "Weights only" not in str(e):
            raise
        raise RuntimeError(
            f"{path}: torch refused to load it with weights_only=True ({type(e).__name__}: it pickles objects outside the "
            f"allow-list). Loading such a file executes code from it. If you trust its origin, pass allow_unsafe_pickle=True "
            f"(preload_models / tools/verify_checkpoint.py --allow-unsafe-pickle) or set VALLEX_ALLOW_UNSAFE_PICKLE=1.") from e


def preload_models(checkpoint: Optional[str] = None, vocos_checkpoint: Optional[str] = None, state_dict=None,
                   vocos_state_dict=None, num_layers: int = NUM_LAYERS, allow_unsafe_pickle: Optional[bool] = None,
                   **engine_opts):
    """Build the engine and load weights.  With no arguments behaves like the reference (expects
    ./checkpoints/vallex-checkpoint.pt; there is no network here, so a missing file raises instead of downloading).
    Checkpoint files are read with torch's weights-only unpickler; allow_unsafe_pickle=True is the explicit opt-in to the
    permissive one (see _torch_load)."""
    global model, vocos
    if state_dict is None:
        path = checkpoint or os.path.join(checkpoints_dir, model_checkpoint_name)
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} not found (the reference downloads it, utils/generation.py:53-65; "
                                    "no network here): pass checkpoint= or state_dict=")
        state_dict = _torch_load(path, allow_unsafe_pickle)["model"]                                  # :79-83
    m = VALLE(N_DIM, NUM_HEAD, num_layers, norm_first=True, add_prenet=False, prefix_mode=PREFIX_MODE,
              share_embedding=True, nar_scale_factor=1.0, prepend_bos=True, num_quantizers=NUM_QUANTIZERS,
              **{"engine_" + k: v for k, v in engine_opts.items()})
    m.to(device).load_state_dict(state_dict, strict=True)
    m.eval()
    if vocos_state_dict is None and vocos_checkpoint is not None:
        vocos_state_dict = _torch_load(vocos_checkpoint, allow_unsafe_pickle)
    if vocos_state_dict is not None:
        m.load_vocos_state_dict(vocos_state_dict)
    model = m
    vocos = VocosHIP(m) if vocos_state_dict is not None else None
    return None


def _load_prompt(prompt):
    """utils/generation.py:103-119: path, preset name or custom name -> (audio (1,Tp,8), text (1,Sp), lang str)."""
    prompt_path = prompt
    for d in [""] + PRESET_DIRS:
        cand = prompt if d == "" else d + prompt + ".npz"
        if os.path.exists(cand):
            prompt_path = cand
            break
    else:
        raise ValueError(f"Cannot find prompt {prompt}")
    data = np.load(prompt_path)
    return (np.asarray(data["audio_tokens"]).astype(np.int32), np.asarray(data["text_tokens"]).astype(np.int32),
            code2lang[int(data["lang_code"])])


def _tokenize(text, lang_token) -> Tuple[np.ndarray, Union[List[str], None]]:
    """utils/generation.py:127-132 (`text_tokenizer.tokenize(f"_{text}")` + collater).  A sequence of ints is taken
    as already-tokenised phoneme ids."""
    if not isinstance(text, str):
        ids = np.asarray(text, np.int32).reshape(-1)
        if ids.size == 0:
            raise ValueError("Empty text is given")                    # utils/g2p/__init__.py:23-24
        return ids, None
    if text_tokenizer is None:
        raise RuntimeError("no text front-end configured: set vallex_amd.utils.generation.text_tokenizer to a callable "
                           "text -> (phoneme ids, languages) (the reference's PhonemeBpeTokenizer), or pass phoneme ids")
    ids, langs = text_tokenizer(f"_{lang_token}{text}{lang_token}".strip())
    if len(ids) == 0:
        raise ValueError("Empty text is given")
    return np.asarray(ids, np.int32), list(langs)


def _carry_coin() -> bool:
    """utils/generation.py:264: `if torch.rand(1) < 0.5` -- drawn from torch's global generator, so a script that calls
    torch.manual_seed flips the same coins as it does with the reference."""
    if rng is not None:
        return rng.random() < 0.5
    if torch is not None:
        return bool(torch.rand(1) < 0.5)
    return float(np.random.random()) < 0.5


def _detect(text, language):
    if language != "auto":
        return language
    if not isinstance(text, str):
        raise ValueError("language='auto' needs a text string")
    if language_detector is None:
        raise RuntimeError("language='auto' needs a language detector (the reference uses langid, "
                           "utils/generation.py:96): set vallex_amd.utils.generation.language_detector")
    return language_detector(text)


@dataclass(frozen=True)
class Finish:
    """The output stage of a waveform (Engine.finish, vx_finish), accepted as `finish=` wherever a waveform leaves: it is applied after
    the resampler, at the output rate.  frame None = 10 ms at that rate (sample_rate // 100).  A frame is active iff its mean square
    exceeds 10^(silence_db / 10); trim bit 0 / bit 1 cut before the first / behind the last active frame, `keep` samples stay;
    level_mode 1 / 2 brings the peak / the RMS over the active frames to level_db dBFS with at most max_gain_db of gain; fade_in /
    fade_out are samples of smoothstep; pcm16: int16 instead of float32.  The measurements of the last call stay in
    `model.engine.last_finish_info`.  lufs (None: the level is level_mode's): the kept span is brought to that BS.1770 loudness instead
    (Engine.finish_loud, vx_finish_loud) under max_gain_db and a sample peak of ceiling_db dBFS; level_mode must then be 0.  The
    loudness measurements stay in `model.engine.last_loudness_info`."""
    frame: Optional[int] = None
    silence_db: float = -40.0
    trim: int = 0
    keep: int = 0
    level_mode: int = 0
    level_db: float = -1.0
    max_gain_db: float = 20.0
    fade_in: int = 0
    fade_out: int = 0
    pcm16: bool = False
    lufs: Optional[float] = None
    ceiling_db: float = -1.0

    def __post_init__(self):
        if self.lufs is not None and self.level_mode != 0:
            raise ValueError("Finish: lufs and level_mode != 0 both set a level; give one")


@dataclass(frozen=True)
class LimitedFinish(Finish):
    """A `Finish` whose loudness target is held under ceiling_db dBTP by a true-peak look-ahead limiter (Engine.finish_limited,
    vx_finish_limited) instead of by a smaller gain: the gain is set by lufs and max_gain_db alone, so a loud sample no longer makes
    the whole utterance quieter than the target.  lufs must be set.  lookahead None = 5 ms at the output rate (sample_rate // 200),
    1 .. 1024 samples; oversample 1, 2, 4 or 8: the detector's interpolation.  The limiter's measurements stay in
    `model.engine.last_limit_info`."""
    lookahead: Optional[int] = None
    oversample: int = 4

    def __post_init__(self):
        super().__post_init__()
        if self.lufs is None:
            raise ValueError("LimitedFinish: lufs must be set (the limiter sits behind the loudness target)")


def _finished(wavs, finish, sample_rate):
    """the waveforms of a call, already at their output rate, through `finish` (None: as they are): one vx_finish call for the list"""
    if finish is None:
        return wavs
    return model.engine._finished(wavs, finish, SAMPLE_RATE if sample_rate is None else int(sample_rate))


class Pitch:
    """A pitch request with its method, accepted wherever `pitch=` is: `pitch` as there (a float in semitones, or the ratio as a
    Fraction or a (num, den) pair).  formants=True keeps the spectral envelope, and with it the speaker: Engine.shift runs the pitch
    tracker and the PSOLA shift (vx_f0, then vx_psola) in place of the stretch-and-resample shift; the ratio must lie in 2/3 .. 2.
    formants=False is the plain `pitch=`.  range (None: as spoken; needs formants=True): the intonation is scaled around its median by
    that factor (utils.alignment.range_contour): 0 flattens it, above 1 widens it, 0 .. 4.  Every ValueError is raised here."""

    def __init__(self, pitch, formants: bool = True, range=None):
        self.pitch, self.formants, self.range = pitch, bool(formants), range
        from .._capi import Engine
        Engine._shift_plan(self, None)

    def __repr__(self):
        return f"Pitch({self.pitch!r}, formants={self.formants}, range={self.range!r})"


@dataclass(eq=False)
class Denoise:
    """A noise-suppression request with chosen values, accepted wherever `denoise=` is (True there means these defaults):
    strength_db, the over-subtraction in dB of power (None: a factor of 2); floor_db, the smallest gain; frac and kmin, the share and
    the least count of a clip's quietest full frames its noise profile is taken from; profile, a stored profile (257 powers,
    Engine.noise_profile) used in place of the clip's own -- what continuous speech needs, which has no quiet frames.  Every
    ValueError is raised here."""

    strength_db: Optional[float] = None
    floor_db: float = -18.0
    frac: float = 0.1
    kmin: int = 8
    profile: Optional[np.ndarray] = None

    def __post_init__(self):
        if self.profile is not None:
            self.profile = np.array(self.profile, np.float64).reshape(-1)
        from .._capi import Engine
        Engine._denoise_opts(self.strength_db, self.floor_db, self.frac, self.kmin, self.profile)


@dataclass(frozen=True)
class Pauses:
    """A request to change the pauses inside the speech, accepted wherever `pauses=` is: a pause is a stretch of at least at_least_ms
    at or below silence_db (the rule of Finish(trim=...), Engine.pauses) between the first and the last sound; keep_ms of it stay
    untouched at either end.  Each pause is scaled by `scale` (None: kept), then held to min_ms .. max_ms (None: no bound), and walked
    to that length by WSOLA (Engine.retime, vx_retime); everything else keeps its bits.  A pause can change by a factor of 4 at the
    most and never falls below two hops (20 ms).  Leading and trailing silence are Finish's."""
    max_ms: Optional[float] = None
    min_ms: Optional[float] = None
    scale: Optional[float] = None
    silence_db: float = -50.0
    at_least_ms: float = 150.0
    keep_ms: float = 20.0

    def __post_init__(self):
        for name in ("max_ms", "min_ms", "scale"):
            v = getattr(self, name)
            if v is not None and not (np.isfinite(v) and v > 0):
                raise ValueError(f"Pauses: {name} {v!r} is not a positive number")
        if self.max_ms is not None and self.min_ms is not None and self.min_ms > self.max_ms:
            raise ValueError(f"Pauses: min_ms {self.min_ms} above max_ms {self.max_ms}")
        if not (np.isfinite(self.silence_db) and self.silence_db <= 0):
            raise ValueError(f"Pauses: silence_db {self.silence_db!r} is not a finite value <= 0")
        if not (np.isfinite(self.at_least_ms) and self.at_least_ms > 0 and np.isfinite(self.keep_ms) and self.keep_ms >= 0):
            raise ValueError(f"Pauses: at_least_ms {self.at_least_ms!r} must be positive and keep_ms {self.keep_ms!r} not negative")


class Eq(tuple):
    """An equaliser request, accepted wherever `eq=` is: an immutable tuple of specs (kind, f0_hz, q, gain_db), at most 8, one biquad
    each (Engine.eq, vx_eq).  The specs are resolved to coefficients at the sample rate of the call (`sections`), so one object serves
    the enrolment end (at the tokenizer's rate) and the output end (at 24 kHz).  `a + b` is the cascade of both.  A filter whose
    memory is longer than vx_eq's warm-up carries (a narrow hum notch: 50 Hz at Q 100) is refused by the call that would run a plain
    Eq; the same specs as a `CarriedEq` (`carried()`, `Eq.hum()`) run on the stage that carries its state and has no such limit."""

    __slots__ = ()
    KINDS = ("highpass", "lowpass", "bandpass", "notch", "peak", "low_shelf", "high_shelf")
    MAX_SECTIONS = 8

    def __new__(cls, specs=()):
        out = []
        for sp in specs:
            if len(sp) != 4:
                raise ValueError(f"Eq: a spec is (kind, f0_hz, q, gain_db), got {sp!r}")
            kind, f0, q, gain = sp[0], float(sp[1]), float(sp[2]), float(sp[3])
            if kind not in cls.KINDS:
                raise ValueError(f"Eq: kind {kind!r} is none of {cls.KINDS}")
            if not (np.isfinite(f0) and f0 > 0):
                raise ValueError(f"Eq: f0 {sp[1]!r} is not a positive frequency")
            if not (np.isfinite(q) and q > 0):
                raise ValueError(f"Eq: q {sp[2]!r} is not a finite value above 0")
            if not abs(gain) <= 24.0:
                raise ValueError(f"Eq: gain_db {sp[3]!r} outside -24 .. 24")
            out.append((kind, f0, q, gain))
        if len(out) > cls.MAX_SECTIONS:
            raise ValueError(f"Eq: {len(out)} sections, at most {cls.MAX_SECTIONS}")
        return super().__new__(cls, out)

    def __add__(self, other):
        if not isinstance(other, Eq):
            return NotImplemented
        if isinstance(self, CarriedEq) or isinstance(other, CarriedEq):   # either side carried: carried, primed as the first that is
            hz = [e.prime_hz for e in (self, other) if getattr(e, "prime_hz", None) is not None]
            opt = tuple(getattr(self, "optional", (False,) * len(self))) + tuple(getattr(other, "optional", (False,) * len(other)))
            return CarriedEq(tuple(self) + tuple(other), prime_hz=hz[0] if hz else None, optional=opt)
        return Eq(tuple(self) + tuple(other))

    def carried(self, prime_hz=None):
        """the same specs on the stage that carries its state (Engine.eq_carry): no limit on the filter's memory"""
        return CarriedEq(tuple(self), prime_hz=prime_hz)

    @classmethod
    def hum(cls, f0=50.0, harmonics=6, q=35.0):
        """mains hum: notches at f0 k, k = 1 .. harmonics (those at or above the Nyquist of the call's rate are dropped when the specs
        are resolved), carried, and primed at f0 so that the notches do not ring in over the start of the clip (`CarriedEq`)"""
        if not (isinstance(harmonics, (int, np.integer)) and 1 <= harmonics <= cls.MAX_SECTIONS):
            raise ValueError(f"Eq.hum: harmonics {harmonics!r} outside 1 .. {cls.MAX_SECTIONS}")
        return CarriedEq([("notch", float(f0) * k, q, 0.0) for k in range(1, int(harmonics) + 1)], prime_hz=float(f0),
                         optional=(True,) * int(harmonics))

    def __repr__(self):
        return f"Eq({list(self)!r})"

    @classmethod
    def highpass(cls, f, q=0.7071):
        return cls([("highpass", f, q, 0.0)])

    @classmethod
    def lowpass(cls, f, q=0.7071):
        return cls([("lowpass", f, q, 0.0)])

    @classmethod
    def bandpass(cls, f, q=0.7071):
        return cls([("bandpass", f, q, 0.0)])

    @classmethod
    def notch(cls, f, q=0.7071):
        return cls([("notch", f, q, 0.0)])

    @classmethod
    def peak(cls, f, gain_db, q=1.0):
        return cls([("peak", f, q, gain_db)])

    @classmethod
    def low_shelf(cls, f, gain_db, q=0.7071):
        return cls([("low_shelf", f, q, gain_db)])

    @classmethod
    def high_shelf(cls, f, gain_db, q=0.7071):
        return cls([("high_shelf", f, q, gain_db)])

    @classmethod
    def rumble(cls):
        """a high-pass at 80 Hz, Q 0.7071: DC offset, desk rumble and the boom of a close microphone"""
        return cls.highpass(80.0, 0.7071)

    @classmethod
    def telephone(cls):
        """the telephone band, fourth-order Butterworth 300 .. 3400 Hz: in front of an 8 kHz delivery"""
        return cls.highpass(300.0, 0.5412) + cls.highpass(300.0, 1.3066) + cls.lowpass(3400.0, 0.5412) + cls.lowpass(3400.0, 1.3066)

    @classmethod
    def presence(cls):
        """a peak at 3 kHz, +4 dB, Q 1 and a high shelf at 8 kHz, +3 dB: for small speakers"""
        return cls.peak(3000.0, 4.0, 1.0) + cls.high_shelf(8000.0, 3.0)

    def sections(self, sample_rate=SAMPLE_RATE) -> np.ndarray:
        """(n, 5) float64, b0 b1 b2 a1 a2 per section at sample_rate (vx_eq_design).  ValueError: no section, or a spec the rate does
        not allow (f0 at or above sample_rate / 2)."""
        from .._capi import Engine
        if not len(self):
            raise ValueError("Eq: no section")
        return np.stack([Engine.eq_design(kind, f0, q, gain, int(sample_rate)) for kind, f0, q, gain in self])

    def response(self, freqs, sample_rate=SAMPLE_RATE) -> np.ndarray:
        """|H| of the cascade at freqs (Hz), from the designed coefficients"""
        z = np.exp(-2j * np.pi * np.asarray(freqs, np.float64) / float(sample_rate))
        h = np.ones(z.shape, np.complex128)
        for b0, b1, b2, a1, a2 in self.sections(sample_rate):
            h = h * (b0 + b1 * z + b2 * z * z) / (1.0 + a1 * z + a2 * z * z)
        return np.abs(h)


PRIME_PERIODS, PRIME_CAP_S = 10, 10


def hum_lead(x, sections, sample_rate, prime_hz):
    """the lead a primed filter runs in front of a row (integers and numpy; None: the row starts from rest): the mean of the row's
    first 10 periods of P = round(sample_rate / prime_hz) samples -- the row's own periodic component, everything else averaged down
    -- tiled to the smallest multiple of P that is at least ln(1000) / -ln(r) samples (r = max sqrt(a2) over the sections with
    a2 > 0, the slowest pole radius: the ring-in has fallen by 60 dB), at most 10 s.  A non-finite sample counts as 0, as in the
    stage.  A row below 10 periods has no lead."""
    x = np.asarray(x, np.float32).reshape(-1)
    P = int(round(float(sample_rate) / float(prime_hz)))
    a2 = [float(c[4]) for c in np.asarray(sections, np.float64).reshape(-1, 5) if c[4] > 0]
    if P < 1 or len(x) < PRIME_PERIODS * P or not a2:
        return None
    need = math.log(1000.0) / -math.log(max(math.sqrt(v) for v in a2))
    reps = max(1, min(int(math.ceil(need / P)), PRIME_CAP_S * int(sample_rate) // P))
    head = x[: PRIME_PERIODS * P]
    head = np.where(np.isfinite(head), head, np.float32(0)).astype(np.float64)
    return np.tile(head.reshape(PRIME_PERIODS, P).mean(axis=0).astype(np.float32), reps)


class CarriedEq(Eq):
    """An `Eq` that runs on the carried-state stage (Engine.eq_carry, vx_eq_carry) wherever `eq=` is accepted: the same specs and
    limits, no limit on the filter's memory.  `a + b` with either side carried is carried.  prime_hz (None: every row starts from
    rest): the rows start from the state the filter is in after a lead built from the row's own component of that period
    (`hum_lead`), so a hum notch takes the hum out from the first sample instead of ringing in over the first second.  optional:
    one flag per spec; a flagged spec at or above the Nyquist of the call's rate is dropped by `sections` (Eq.hum's harmonics)."""

    is_carried = True

    def __new__(cls, specs=(), prime_hz=None, optional=None):
        self = super().__new__(cls, specs)
        if prime_hz is not None and not (np.isfinite(float(prime_hz)) and float(prime_hz) > 0):
            raise ValueError(f"CarriedEq: prime_hz {prime_hz!r} is not a positive frequency")
        opt = (False,) * len(self) if optional is None else tuple(bool(v) for v in optional)
        if len(opt) != len(self):
            raise ValueError(f"CarriedEq: {len(opt)} optional flags for {len(self)} specs")
        self.__dict__.update(prime_hz=None if prime_hz is None else float(prime_hz), optional=opt)
        return self

    def __setattr__(self, name, value):
        raise AttributeError("a CarriedEq is immutable")

    def __repr__(self):
        opt = f", optional={self.optional!r}" if any(self.optional) else ""
        return f"CarriedEq({list(self)!r}, prime_hz={self.prime_hz!r}{opt})"

    def carried(self, prime_hz=None):
        return self if prime_hz is None else CarriedEq(tuple(self), prime_hz=prime_hz, optional=self.optional)

    def sections(self, sample_rate=SAMPLE_RATE) -> np.ndarray:
        kept = Eq([sp for sp, opt in zip(self, self.optional) if not (opt and sp[1] >= 0.5 * float(sample_rate))])
        return kept.sections(sample_rate)

    def prime(self, engine, wavs, sections, sample_rate):
        """the start states (rows, 2 n) float64 of `wavs` under this filter: every lead through one Engine.eq_carry call of its own,
        from rest; a row without a lead starts from rest.  None: no row has one."""
        leads = [hum_lead(w, sections, sample_rate, self.prime_hz) for w in wavs]
        have = [i for i, ld in enumerate(leads) if ld is not None]
        if not have:
            return None
        state = np.zeros((len(wavs), 2 * len(sections)), np.float64)
        state[have] = engine.eq_carry([leads[i] for i in have], np.asarray(sections, np.float64), sample_rate, return_state=True)[1]
        return state


def _equalised(wavs, eq):
    """the 24 kHz waveforms of a vocoder call through `eq` (None: as they are), behind denoise, pauses and speed / pitch and directly
    in front of the resampler"""
    if eq is None:
        return wavs
    return model.engine._equalised(wavs, eq, SAMPLE_RATE)


def _check_eq(eq):
    """the ValueError of an `eq` argument that Engine.eq (a CarriedEq: Engine.eq_carry) would refuse at 24 kHz, before anything is
    synthesised"""
    if eq is not None and getattr(eq, "is_carried", False):
        model.engine.eq_carry_plan(eq, SAMPLE_RATE)
    elif eq is not None:
        model.engine.eq_plan(eq, SAMPLE_RATE)


def _paused(wavs, pauses):
    """the 24 kHz waveforms of a vocoder call through `pauses` (None: as they are), behind `denoise` and in front of speed and pitch"""
    if pauses is None:
        return wavs
    return model.engine._paused(wavs, pauses, SAMPLE_RATE)


def _denoised(wavs, denoise):
    """the 24 kHz waveforms of a vocoder call through `denoise` (None: as they are), directly behind the vocoder"""
    if denoise is None:
        return wavs
    return model.engine._denoised(wavs, denoise)


def _check_denoise(denoise):
    """the ValueError of a `denoise` argument that Engine.denoise would refuse, before anything is synthesised"""
    if denoise is not None:
        model.engine._denoise_opts(**model.engine._denoise_parts(denoise))


def _at_speed(wavs, speed, pitch=None):
    """the 24 kHz waveforms of a vocoder call at `speed` (None: as they are): one vx_stretch call for the list, before the resampler;
    with `pitch` (None: as they are): Engine.shift, the stretch at the combined speed and the p -> q resample, for the list"""
    if pitch is not None:
        return model.engine.shift(wavs, pitch, speed)
    if speed is None:
        return wavs
    return model.engine.stretch(wavs, speed)


def _check_pitch(pitch, speed):
    """the ValueError of a `pitch` / `speed` pair that Engine.shift would refuse, before anything is synthesised"""
    if pitch is not None:
        model.engine._shift_plan(pitch, speed)


def _to_rate(wavs, sample_rate):
    """the 24 kHz waveforms of a vocoder call at `sample_rate` (None / 24000: as they are): one vx_resample launch for the list"""
    if sample_rate is None or int(sample_rate) == SAMPLE_RATE:
        return wavs
    if int(sample_rate) <= 0:
        raise ValueError(f"sample_rate must be positive, got {sample_rate}")
    return model.engine.resample(wavs, SAMPLE_RATE, int(sample_rate))


def _infer_one(text, audio_prompts, text_prompts, lang_pr, language, accent, **kw):
    lang_token = lang2token[language]                                  # KeyError on unknown language (macros.py:8-13)
    lang = token2lang[lang_token]
    phone_tokens, langs = _tokenize(text, lang_token)
    enroll_x_lens = text_prompts.shape[-1]
    text_tokens = np.concatenate([text_prompts.reshape(-1), phone_tokens])[None]          # :133
    lens = np.array([text_tokens.shape[-1]], np.int32)
    if lang_pr is None:
        lang_pr = lang if lang != "mix" else "en"                      # :123
    lang_eff = lang if accent == "no-accent" else token2lang[langdropdown2token[accent]]   # :136
    text_language = (langs if langs is not None else lang_eff) if accent == "no-accent" else lang_eff
    if text_language == "mix":
        raise KeyError("mix")                                          # language_ID has no 'mix' (models/vallex.py:439-443)
    out = model.inference(text_tokens, lens, audio_prompts, enroll_x_lens=enroll_x_lens, top_k=-100, temperature=1,
                          prompt_language=lang_pr, text_language=text_language, **kw)
    return out, phone_tokens


def generate_audio(text, prompt=None, language="auto", accent="no-accent", sample_rate=None, finish=None, speed=None, pitch=None,
                   denoise=None, pauses=None, eq=None, **kw):
    """utils/generation.py:92-152.  sample_rate (no reference counterpart; None = 24 kHz, the reference's): the waveform is resampled
    on the device (Engine.resample, vx_resample) to that rate.  finish (a `Finish`; None = the raw fp32 of the reference): the output
    stage behind it -- trim, level, fades, int16 with pcm16=True.  speed (a float, a Fraction or a (num, den) pair in 1/2 .. 2; None =
    the pace the model produced): the speaking rate, a pitch-preserving time-stretch on the device (Engine.stretch, vx_stretch) at
    24 kHz, before the resampler.  pitch (a float in semitones, -12 .. 12, or the ratio as a Fraction or a (num, den) pair in
    1/2 .. 2; None = the pitch the model produced): a pitch shift that keeps the duration (Engine.shift: the stretch at speed / ratio,
    then a resample by the ratio), in place of the stretch.  It moves the formants with the pitch: meant for a few semitones.  A
    `Pitch` (pitch, formants=True, range=None) keeps the formants instead (the pitch tracker, then the PSOLA shift: vx_f0, vx_psola)
    and can scale the intonation's range; it is accepted wherever `pitch=` is.  denoise (None = the waveform as the vocoder gave it;
    True or a `Denoise`): spectral noise suppression on the device (Engine.denoise, vx_denoise) directly behind the vocoder, before
    speed, pitch, resample and finish -- for a preset that was enrolled from a noisy clip.  pauses (None = the pauses the model
    sampled; a `Pauses`): the pauses inside the speech are found (Engine.pauses, vx_pauses) and shortened, lengthened or scaled by a
    piecewise time map (Engine.retime, vx_retime) at 24 kHz, behind denoise and in front of speed and pitch; the speech between them
    keeps its bits.  eq (None = the spectrum the vocoder gave; an `Eq`): a cascade of biquads on the device (Engine.eq, vx_eq) at
    24 kHz, behind denoise, pauses and speed / pitch and directly in front of the resample -- a telephone band precedes the decimation,
    and loudness, limiter and trim of `finish` measure what is delivered."""
    if model is None or vocos is None:
        raise RuntimeError("call preload_models() first")
    _check_eq(eq)
    _check_pitch(pitch, speed)
    _check_denoise(denoise)
    if isinstance(text, str):
        text = text.replace("\n", "").strip(" ")
    language = _detect(text, language)
    if prompt is not None:
        audio_prompts, text_prompts, lang_pr = _load_prompt(prompt)
    else:
        audio_prompts = np.zeros([1, 0, NUM_QUANTIZERS], np.int32)     # :121-123
        text_prompts = np.zeros([1, 0], np.int32)
        lang_pr = None
    logging.info(f"synthesize text: {text}")
    encoded_frames, _ = _infer_one(text, audio_prompts, text_prompts, lang_pr, language, accent, **kw)
    frames = (encoded_frames.permute(2, 0, 1) if torch is not None and isinstance(encoded_frames, torch.Tensor)
              else np.transpose(np.asarray(encoded_frames), (2, 0, 1)))                                         # :148
    features = vocos.codes_to_features(frames)
    samples = vocos.decode(features, bandwidth_id=np.array([2]))
    s = samples.squeeze()
    s = s.cpu().numpy() if torch is not None and isinstance(s, torch.Tensor) else np.asarray(s)
    if denoise is not None:
        s = _denoised([s.reshape(-1)], denoise)[0]
    if pauses is not None:
        s = _paused([s.reshape(-1)], pauses)[0]
    if speed is not None or pitch is not None or eq is not None:
        return _finished(_to_rate(_equalised(_at_speed([s.reshape(-1)], speed, pitch), eq), sample_rate), finish, sample_rate)[0]
    if finish is not None:
        return _finished(_to_rate([s.reshape(-1)], sample_rate), finish, sample_rate)[0]
    return s if sample_rate is None else _to_rate([s.reshape(-1)], sample_rate)[0]


def generate_audio_batch(texts, prompts=None, language="auto", accent="no-accent", text_languages=None, sample_rate=None, finish=None,
                         speed=None, pitch=None, denoise=None, pauses=None, eq=None, **kw):
    """Batch form of `generate_audio` (no reference equivalent: the reference synthesises one utterance per call,
    utils/generation.py:92-152): utterance i of the batch equals `generate_audio(texts[i], prompts[i], language[i], accent)`.
    `texts`: strings (need the tokenizer hook) or phoneme-id arrays; `prompts`: one preset name / path / None per utterance (or
    one for all); `language`: one string or one per utterance; `text_languages`: optional per-utterance per-id language lists
    (what the tokenizer returned, `TextFrontendService`).  All utterances go through ONE `VALLE.inference_batch` call and ONE
    Vocos call.  `**kw` goes to `inference_batch`: `best_of`, `length_penalty` and `return_worst` apply to every utterance (best_of
    = N: N beams per utterance), injected `uniforms` are (steps, len(texts) x max(1, N)) with column i*N + j for beam j of
    utterance i.  `sample_rate` (None = 24 kHz): the waveforms are resampled on the device in one more launch.  `finish` (a
    `Finish`): the output stage behind it, one more call for the list.  `speed` (None = as produced): the speaking rate, one vx_stretch
    call for the list before both.  `pitch` (None = as produced): the pitch shift of `generate_audio`, Engine.shift for the list in
    place of the stretch.  `denoise` (None = as produced): the noise suppression of `generate_audio`, one Engine.denoise call for the
    list directly behind Vocos.  `pauses` (None = as produced): the pause control of `generate_audio`, one Engine.pauses and one
    Engine.retime call for the list behind that.  `eq` (None = as produced): the equaliser of `generate_audio`, one Engine.eq call for
    the list directly in front of the resample.  Returns a list of float32 waveforms (int16 with pcm16=True)."""
    if model is None or vocos is None:
        raise RuntimeError("call preload_models() first")
    _check_eq(eq)
    _check_pitch(pitch, speed)
    _check_denoise(denoise)
    n = len(texts)
    prompts = list(prompts) if isinstance(prompts, (list, tuple)) else [prompts] * n
    langs_in = list(language) if isinstance(language, (list, tuple)) else [language] * n
    text_languages = list(text_languages) if text_languages is not None else [None] * n
    rows = [_utterance_row(text, prompt, lang_in, accent, tl)
            for text, prompt, lang_in, tl in zip(texts, prompts, langs_in, text_languages)]
    codes = model.inference_batch(rows, top_k=-100, temperature=1, **kw)
    return model.engine.vocos_decode(codes, 2, sample_rate=SAMPLE_RATE if sample_rate is None else int(sample_rate), finish=finish,
                                     speed=speed, pitch=pitch, denoise=denoise, pauses=pauses, eq=eq)


def _utterance_row(text, prompt, lang_in, accent, tl=None) -> dict:
    """the inference_batch row of one utterance of generate_audio_batch / AudioServer (front-end work on the calling thread)"""
    if isinstance(text, str):
        text = text.replace("\n", "").strip(" ")
    lang_in = _detect(text, lang_in)
    if prompt is not None:
        audio_prompts, text_prompts, lang_pr = _load_prompt(prompt)
    else:
        audio_prompts = np.zeros([1, 0, NUM_QUANTIZERS], np.int32)
        text_prompts = np.zeros([1, 0], np.int32)
        lang_pr = None
    lang_token = lang2token[lang_in]
    lang = token2lang[lang_token]
    phone_tokens, langs = _tokenize(text, lang_token)
    if tl is not None:
        langs = list(tl)
    if lang_pr is None:
        lang_pr = lang if lang != "mix" else "en"
    lang_eff = lang if accent == "no-accent" else token2lang[langdropdown2token[accent]]
    text_language = (langs if langs is not None else lang_eff) if accent == "no-accent" else lang_eff
    if text_language == "mix":
        raise KeyError("mix")
    return dict(text=np.concatenate([text_prompts.reshape(-1), phone_tokens]), prompt=audio_prompts[0],
                enroll=text_prompts.shape[-1], prompt_language=lang_pr, text_language=text_language)


class AudioServer:
    """Audio-level counterpart of `generate_audio` / `generate_audio_batch` on a serving session (VALLE.serve): `submit` may be
    called from any thread at any time -- a UI can hand in its best_of=5 calls (launch-ui.py) concurrently -- and returns a
    Future of the float32 waveform.  Front-end work (tokenizer, prompt lookup, language detection) runs on the submitting thread;
    the codes of every group of completed requests go through Vocos on the server's worker thread.  Utterance i equals
    `generate_audio_batch([text], [prompt], language, accent, best_of=..., seed=...)[0]`.  `**serve_kw` goes to VALLE.serve
    (sync_every, force_eos_at, max_steps).  `sample_rate` (None = 24 kHz): ONE output rate for the server, applied to every delivered
    waveform behind Vocos (vx_resample is allowed while the session is open).  `finish` (a `Finish`): ONE output stage for the server,
    applied behind that (vx_finish is allowed as well).  `speed` (None = as produced): ONE speaking rate for the server, applied to
    every delivered waveform between Vocos and the resampler (vx_stretch is allowed as well).  `pitch` (None = as produced): ONE pitch
    shift for the server (generate_audio's `pitch`), applied there in place of the stretch.  `denoise` (None = as produced): ONE noise
    suppression for the server (generate_audio's `denoise`), applied directly behind Vocos (vx_denoise is allowed as well).  `pauses` (None = as produced): ONE pause
    control for the server (generate_audio's `pauses`), applied behind that (vx_pauses and vx_retime are allowed as well).
    `eq` (None = as produced): ONE equaliser for the server (generate_audio's `eq`), applied directly in front of the resampler (vx_eq
    is allowed as well)."""

    def __init__(self, sample_rate=None, finish=None, speed=None, pitch=None, denoise=None, pauses=None, eq=None, **serve_kw):
        if model is None or vocos is None:
            raise RuntimeError("call preload_models() first")
        rate = SAMPLE_RATE if sample_rate is None else int(sample_rate)
        if rate <= 0:
            raise ValueError(f"sample_rate must be positive, got {sample_rate}")
        self.sample_rate = rate
        self.finish = finish
        self.speed = speed
        _check_pitch(pitch, speed)
        self.pitch = pitch
        _check_denoise(denoise)
        self.denoise = denoise
        self.pauses = pauses
        _check_eq(eq)
        self.eq = eq
        self._server = model.serve(top_k=-100, temperature=1.0,
                                   post=lambda codes: model.engine.vocos_decode(codes, 2, sample_rate=rate, finish=finish, speed=speed,
                                                                                pitch=pitch, denoise=denoise, pauses=pauses, eq=eq),
                                   **serve_kw)

    def submit(self, text, prompt=None, language="auto", accent="no-accent", best_of=1, seed=None, uniforms=None,
               length_penalty=1.0, return_worst=False, text_language=None, top_k=-100, temperature=1.0, top_p=1.0,
               repetition_penalty=1.0, repetition_window=0, min_frames=0):
        """top_k / temperature: generate_audio's defaults, per request.  top_p / repetition_penalty / repetition_window / min_frames:
        the request's logit filters (Server.submit); the defaults are neutral.  The Future can be cancelled until it is delivered."""
        row = _utterance_row(text, prompt, language, accent, text_language)
        return self._server.submit(row, best_of=best_of, seed=seed, uniforms=uniforms, length_penalty=length_penalty,
                                   return_worst=return_worst, top_k=top_k, temperature=temperature, top_p=top_p,
                                   repetition_penalty=repetition_penalty, repetition_window=repetition_window,
                                   min_frames=min_frames)

    def close(self):
        self._server.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def generate_audio_from_long_text(text, prompt=None, language="auto", accent="no-accent", mode="sliding-window", sample_rate=None,
                                  finish=None, speed=None, pitch=None, denoise=None, pauses=None, eq=None, **kw):
    """utils/generation.py:155-276.  `text` may also be a list of sentences / id arrays (pre-split).  sample_rate, finish, speed,
    pitch, denoise, pauses, eq: as generate_audio (the noise suppression, the pause control, the stretch or the shift, the equaliser
    and the output stage see the concatenated waveform once)."""
    if model is None or vocos is None:
        raise RuntimeError("call preload_models() first")
    _check_eq(eq)
    _check_pitch(pitch, speed)
    _check_denoise(denoise)
    if prompt is None or prompt == "":
        prompt = None
        mode = "sliding-window"                                        # :162-163: overrides ANY mode, also an unknown one
    if isinstance(text, str):
        if sentence_splitter is None:
            raise RuntimeError("no sentence splitter configured (the reference uses utils/sentence_cutter.py): set "
                               "vallex_amd.utils.generation.sentence_splitter or pass a list of sentences")
        sentences = sentence_splitter(text)
    else:
        sentences = list(text)
    if language == "auto":                                             # :166-167: langid.classify(text) on the WHOLE input
        language = _detect(text if isinstance(text, str) else (sentences[0] if sentences else ""), language)
    if prompt is not None:
        audio_prompts, text_prompts, lang_pr = _load_prompt(prompt)
    else:
        audio_prompts = np.zeros([1, 0, NUM_QUANTIZERS], np.int32)
        text_prompts = np.zeros([1, 0], np.int32)
        lang_pr = None
    # the reference only looks at `mode` here, after the override, the sentence split, the language detection and the prompt
    # lookup (its if / elif / else ends in the raise, utils/generation.py:197,229,275-276) -- same order of errors
    if mode not in ("fixed-prompt", "sliding-window"):
        raise ValueError(f"No such mode {mode}")                       # :276
    original = (audio_prompts, text_prompts)
    chunks = []
    for sent in sentences:
        if isinstance(sent, str):
            sent = sent.replace("\n", "").strip(" ")
            if sent == "":
                continue                                               # :198-199,236-237
        frames, phone_tokens = _infer_one(sent, audio_prompts, text_prompts, lang_pr, language, accent, **kw)
        f = frames.numpy() if torch is not None and isinstance(frames, torch.Tensor) else np.asarray(frames)
        chunks.append(f)
        if mode == "sliding-window":
            if _carry_coin():                                          # torch.rand(1) < 0.5  (:264)
                # encoded_frames[:, :, -NUM_QUANTIZERS:] slices the codebook axis, i.e. keeps ALL frames (:265)
                audio_prompts = f[:, :, -NUM_QUANTIZERS:].astype(np.int32)
                text_prompts = np.asarray(phone_tokens, np.int32)[None]             # text_tokens[:, enroll_x_lens:] (:266)
            else:
                audio_prompts, text_prompts = original                 # :268-269
    if not chunks:
        return np.zeros(0, np.int16 if finish is not None and finish.pcm16 else np.float32)
    complete = np.concatenate(chunks, axis=1)                          # (1, sum T, 8)
    features = vocos.codes_to_features(np.transpose(complete, (2, 0, 1)))
    samples = vocos.decode(features, bandwidth_id=np.array([2]))
    s = samples.squeeze()
    s = s.cpu().numpy() if torch is not None and isinstance(s, torch.Tensor) else np.asarray(s)
    if denoise is not None:
        s = _denoised([s.reshape(-1)], denoise)[0]
    if pauses is not None:
        s = _paused([s.reshape(-1)], pauses)[0]
    if speed is not None or pitch is not None or eq is not None:
        return _finished(_to_rate(_equalised(_at_speed([s.reshape(-1)], speed, pitch), eq), sample_rate), finish, sample_rate)[0]
    if finish is not None:
        return _finished(_to_rate([s.reshape(-1)], sample_rate), finish, sample_rate)[0]
    return s if sample_rate is None else _to_rate([s.reshape(-1)], sample_rate)[0]
