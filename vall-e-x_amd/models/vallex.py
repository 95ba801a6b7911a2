"""`VALLE` with the reference's constructor / load_state_dict / inference signatures (models/vallex.py:405-686),
implemented as a thin host shim over the C ABI (include/vallex_hip.h).  No torch modules, no CPU math: weights go
straight to the GPU engine, tokens come back.

Differences a caller can observe (all documented in DESIGN.md):
  * `inference` accepts the same arguments and returns the same LongTensor (1, T, 8), including `best_of` /
    `length_penalty` / `return_worst` (beams = rows of the micro-batch, selection on the device-accumulated log-probs);
  * extra, reference-less entry points for what BASELINE.json measures: `inference_batch` (distinct utterances in one
    call; the reference can only batch beams of ONE utterance, models/vallex.py:491,525-527) and the reproducibility
    hooks `uniforms=` / `force_eos_at=` (the reference needs monkey-patching for the same effect).
"""
from __future__ import annotations

import math
import threading
from concurrent.futures import Future, InvalidStateError
from typing import Dict, List, Optional, Sequence, Union

import numpy as np

from .. import macros
from .._capi import ARITH, VX_EINVAL, Batch, Engine, ServeSession, VallexHipError

try:  # torch is plumbing only: the reference API hands tensors in and out
    import torch
except Exception:  # pragma: no cover
    torch = None

NUM_AUDIO_TOKENS = macros.NUM_AUDIO_TOKENS


def _np(a, dtype=None):
    if torch is not None and isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    return a.astype(dtype) if dtype is not None else a


def fresh_seed() -> int:
    """Seed of the device sampler for ONE call.  The reference samples from torch's global generator (torch.multinomial,
    models/vallex.py:850): repeated calls differ, `torch.manual_seed` makes a script reproducible.  Same contract here:
    every call that is not given an explicit `seed=` draws a new 62-bit seed from that generator."""
    if torch is not None:
        return int(torch.randint(0, 2 ** 62, (1,)).item())
    return int(np.random.default_rng().integers(0, 2 ** 62))


def vocos_expected_keys() -> List[str]:
    """The tensors of `charactr/vocos-encodec-24khz` the Vocos head computes with: codebook table, embed conv,
    AdaLayerNorm tables, 8 ConvNeXt blocks, final LayerNorm, ISTFT head projection."""
    k = ["feature_extractor.codebook_weights", "backbone.embed.weight", "backbone.embed.bias", "backbone.norm.scale.weight",
         "backbone.norm.shift.weight"]
    for i in range(8):
        k += [f"backbone.convnext.{i}." + s for s in ("dwconv.weight", "dwconv.bias", "norm.scale.weight", "norm.shift.weight",
                                                      "pwconv1.weight", "pwconv1.bias", "pwconv2.weight", "pwconv2.bias", "gamma")]
    return k + ["backbone.final_layer_norm.weight", "backbone.final_layer_norm.bias", "head.out.weight", "head.out.bias"]


def expected_keys(num_layers: int) -> List[str]:
    """State-dict layout of the reference (models/vallex.py:55-264,405-445)."""
    k = ["ar_text_embedding.word_embeddings.weight", "nar_text_embedding.word_embeddings.weight",
         "ar_audio_embedding.word_embeddings.weight", "ar_text_position.alpha", "ar_audio_position.alpha"]

    def layer(p, adaptive):
        out = [p + s for s in ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight",
                               "self_attn.out_proj.bias", "linear1.weight", "linear1.bias", "linear2.weight",
                               "linear2.bias")]
        for n in ("norm1", "norm2"):
            if adaptive:
                out += [p + n + s for s in (".project_layer.weight", ".project_layer.bias", ".norm.weight", ".norm.bias")]
            else:
                out += [p + n + ".weight", p + n + ".bias"]
        return out

    for i in range(num_layers):
        k += layer(f"ar_decoder.layers.{i}.", False)
    k += ["ar_decoder.norm.weight", "ar_decoder.norm.bias", "ar_predict_layer.weight"]
    k += [f"nar_audio_embeddings.{j}.word_embeddings.weight" for j in range(8)]
    k += ["nar_text_position.alpha", "nar_audio_position.alpha"]
    for i in range(num_layers):
        k += layer(f"nar_decoder.layers.{i}.", True)
    k += ["nar_decoder.norm.project_layer.weight", "nar_decoder.norm.project_layer.bias", "nar_decoder.norm.norm.weight",
          "nar_decoder.norm.norm.bias"]
    k += [f"nar_predict_layers.{j}.weight" for j in range(7)]
    k += [f"nar_stage_embeddings.{j}.word_embeddings.weight" for j in range(7)]
    k += ["ar_language_embedding.word_embeddings.weight", "nar_language_embedding.word_embeddings.weight"]
    return k


def sine_pe_table(rows: int, d: int = 1024) -> np.ndarray:
    """SinePositionalEmbedding.extend_pe (modules/embedding.py:75-91), built with the same torch fp32 ops on the host
    and uploaded -- never recomputed with device sin/cos."""
    if torch is not None:
        pe = torch.zeros(rows, d)
        position = torch.arange(0, rows, dtype=torch.float32).unsqueeze(1)
        div_term = torch.exp(torch.arange(0, d, 2, dtype=torch.float32) * -(math.log(10000.0) / d))
        pe[:, 0::2] = torch.sin(position * div_term)
        pe[:, 1::2] = torch.cos(position * div_term)
        return pe.numpy()
    pos = np.arange(rows, dtype=np.float32)[:, None]
    div = np.exp(np.arange(0, d, 2, dtype=np.float32) * np.float32(-(math.log(10000.0) / d)))
    pe = np.zeros((rows, d), np.float32)
    pe[:, 0::2] = np.sin(pos * div)
    pe[:, 1::2] = np.cos(pos * div)
    return pe


class VALLE:
    """Drop-in for models.vallex.VALLE on the inference path."""

    def __init__(self, d_model: int, nhead: int, num_layers: int, norm_first: bool = True, add_prenet: bool = False,
                 prefix_mode: int = 0, share_embedding: bool = True, nar_scale_factor: float = 1.0, **kwargs):
        # the shipped checkpoint's configuration (utils/generation.py:67-78) is what the kernels implement
        if (d_model, nhead) != (1024, 16) or not norm_first or add_prenet or prefix_mode != 1 or nar_scale_factor != 1.0:
            raise NotImplementedError("the gfx950 engine implements the shipped VALL-E X configuration only: "
                                      "d_model=1024, nhead=16, norm_first, no prenet, prefix_mode=1")
        if kwargs.get("num_quantizers", 8) != 8 or not kwargs.get("prepend_bos", True):
            raise NotImplementedError("num_quantizers=8 and prepend_bos=True only")
        self.num_layers = num_layers
        self.language_ID = {"en": 0, "zh": 1, "ja": 2}          # models/vallex.py:439-443
        self._sd: Optional[Dict[str, np.ndarray]] = None
        self._vocos_sd: Optional[Dict[str, np.ndarray]] = None
        self._encodec_sd: Optional[Dict[str, np.ndarray]] = None
        self._engine: Optional[Engine] = None
        self._device_id = 0
        self.engine_opts = dict(max_batch=int(kwargs.get("engine_max_batch", 32)),
                                max_text=int(kwargs.get("engine_max_text", 512)),
                                max_prompt=int(kwargs.get("engine_max_prompt", 2048)),   # >= max_new: sliding-window carry-over
                                max_new=int(kwargs.get("engine_max_new", 2048)),
                                use_graph=bool(kwargs.get("engine_use_graph", True)),
                                debug_taps=bool(kwargs.get("engine_debug_taps", False)),
                                cu_mask=int(kwargs.get("engine_cu_mask", 0)),
                                arith=kwargs.get("engine_arith", "default"))

    # ---- nn.Module-ish surface used by the reference's callers --------------------------------------------------
    def to(self, device):
        s = str(device)
        if not s.startswith("cuda"):
            raise RuntimeError("vall-e-x_amd runs on MI355X only (device 'cuda[:N]'); there is no CPU path")
        self._device_id = int(s.split(":")[1]) if ":" in s else 0
        return self

    def eval(self):
        return self

    def load_state_dict(self, state_dict, strict: bool = True):
        """VALLE.load_state_dict(checkpoint["model"], strict=True) (utils/generation.py:79-83)."""
        want = expected_keys(self.num_layers)
        missing = [k for k in want if k not in state_dict]
        unexpected = [k for k in state_dict if k not in set(want)]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for VALLE: missing {missing[:4]}... "
                               f"unexpected {unexpected[:4]}...")
        self._sd = {k: _np(state_dict[k], np.float32) for k in want if k in state_dict}
        self._engine = None
        return self

    def load_vocos_state_dict(self, state_dict):
        """Weights of `Vocos.from_pretrained('charactr/vocos-encodec-24khz')` (utils/generation.py:89), vocos key names.  The
        published checkpoint also carries the whole EnCodec model under `feature_extractor.encodec.*` and the ISTFT window
        buffer; only the tensors the head computes with (`vocos_expected_keys`) are uploaded, the rest is ignored."""
        want = vocos_expected_keys()
        missing = [k for k in want if k not in state_dict]
        if missing:
            raise RuntimeError(f"Error(s) in loading the Vocos state_dict: missing {missing[:4]}{'...' if len(missing) > 4 else ''}")
        self._vocos_sd = {k: _np(state_dict[k], np.float32) for k in want}
        self._engine = None
        return self

    def load_encodec_state_dict(self, state_dict):
        """Weights of `EncodecModel.encodec_model_24khz()` (data/tokenizer.py:71-73): encodec-package, transformers-port or
        canonical key names.  The RVQ codebooks and the SEANet decoder are required; if the SEANet encoder is in the dict too,
        `AudioTokenizer.encode` (prompt enrolment) is available as well."""
        from ..data.tokenizer import canonical_encodec_state_dict
        self._encodec_sd = canonical_encodec_state_dict(state_dict)
        self._engine = None
        return self

    # ---- engine ------------------------------------------------------------------------------------------------
    @property
    def engine(self) -> Engine:
        if self._engine is None:
            if self._sd is None:
                raise RuntimeError("load_state_dict() first")
            o = self.engine_opts
            eng = Engine(self._device_id, self.num_layers, o["max_batch"], o["max_text"], o["max_prompt"], o["max_new"],
                         o["use_graph"], self._vocos_sd is not None, o["debug_taps"], self._encodec_sd is not None,
                         o["cu_mask"], ARITH[o["arith"]] if isinstance(o["arith"], str) else int(o["arith"]))
            for k, v in self._sd.items():
                eng.load_tensor(k, v)
            tmax = o["max_text"] + o["max_prompt"] + o["max_new"] + 16
            eng.load_tensor("pe_table", sine_pe_table(max(4000, tmax)))
            if self._vocos_sd is not None:
                for k, v in self._vocos_sd.items():
                    eng.load_tensor("vocos." + k, v)
            if self._encodec_sd is not None:
                for k, v in self._encodec_sd.items():
                    eng.load_tensor("encodec." + k, v)
            eng.finalize()
            self._engine = eng
        return self._engine

    def _lang_row(self, S: int, enroll: int, prompt_language, text_language) -> np.ndarray:
        out = np.empty(S, np.int32)
        out[:enroll] = self.language_ID[prompt_language]              # KeyError on unknown language, like the reference
        if isinstance(text_language, str):
            out[enroll:] = self.language_ID[text_language]
        else:
            ids = [self.language_ID[t] for t in text_language]
            if len(ids) != S - enroll:
                raise RuntimeError(f"text_language list has {len(ids)} entries for {S - enroll} text tokens")
            out[enroll:] = ids
        return out

    # ---- the reference entry point ---------------------------------------------------------------------------------
    def inference(self, x, x_lens, y, enroll_x_lens, top_k: int = -100, temperature: float = 1.0,
                  prompt_language: str = None, text_language: Union[str, List[str]] = None, best_of: int = 1,
                  length_penalty: float = 1.0, return_worst: bool = False, *, uniforms=None, force_eos_at=None,
                  seed: Optional[int] = None):
        xa, xl, ya = _np(x), _np(x_lens), _np(y)
        assert xa.ndim == 2, xa.shape                      # models/vallex.py:488-493
        assert xl.ndim == 1, xl.shape
        assert ya.ndim == 3, ya.shape
        assert ya.shape[0] == 1, ya.shape
        assert np.all(xl > 0)
        S = int(xl.max())
        row = dict(text=xa[0, :S], prompt=ya[0], enroll=int(_np(enroll_x_lens)), prompt_language=prompt_language,
                   text_language=text_language)
        u = None
        if uniforms is not None:
            u = np.asarray(uniforms, np.float32)
            u = u.reshape(-1, max(1, int(best_of))) if u.ndim == 1 else u
        codes = self.inference_batch([row], top_k=top_k, temperature=temperature, uniforms=u, force_eos_at=force_eos_at,
                                     seed=seed, best_of=best_of, length_penalty=length_penalty,
                                     return_worst=return_worst)[0]
        out = codes[None]
        return torch.from_numpy(out) if torch is not None else out

    def continual(self, x, x_lens, y):
        """`VALLE.continual` (models/vallex.py:688-787): NAR-only continuation.  The first half of `y` (1, T, 8) -- at most
        3 s = 225 frames -- is the acoustic prompt, the first codebook of the remaining frames is taken as given and
        codebooks 2..8 of those frames are predicted; the text gets NO language embedding on this path.
        Returns (1, T - prefix_len, 8) like the reference."""
        xa, xl, ya = _np(x), _np(x_lens), _np(y)
        assert xa.ndim == 2, xa.shape                      # models/vallex.py:706-712
        assert xl.ndim == 1, xl.shape
        assert ya.ndim == 3, ya.shape
        assert ya.shape[0] == 1, ya.shape
        assert np.all(xl > 0)
        S = int(xl.max())
        prefix_len = min(int(ya.shape[1] * 0.5), 3 * 75)   # :722
        text = _np(xa[0, :S], np.int32)
        batch = Batch([text], [np.full(S, -1, np.int32)], [_np(ya[0, :prefix_len], np.int32).reshape(-1, 8)])
        codes = self.engine.nar(batch, [_np(ya[0, prefix_len:, 0], np.int32)])[0]
        out = codes[None]
        return torch.from_numpy(out) if torch is not None else out

    def inference_batch(self, rows: Sequence[dict], top_k: int = -100, temperature: float = 1.0, uniforms=None,
                        force_eos_at=None, seed: Optional[int] = None, sync_every: int = 8, best_of: int = 1,
                        length_penalty: float = 1.0, return_worst: bool = False, continuous: bool = False,
                        on_row=None) -> List[np.ndarray]:
        """rows[i] = dict(text ids (S,), prompt codes (Tp,8), enroll, prompt_language, text_language).
        Row i equals `inference` run alone on that row.  Returns one (T_i, 8) int64 array per row.
        `best_of` = N > 1 decodes every row as N beams (the UI's call, launch-ui.py:285-295, for a whole batch); `length_penalty`
        and `return_worst` select per row.  Injected `uniforms` are (steps, len(rows) x max(1, N)): column i*N + j feeds beam j of
        row i, so row i equals `inference(row i, best_of=N, uniforms=uniforms[:, i*N:(i+1)*N])`.
        `continuous=True` runs the continuous schedule (vx_infer_continuous): a finished row's decode row is refilled with the next
        waiting row at the next host poll; `on_row(i, codes)` (continuous only) receives every row as soon as its NAR stages are
        done.  Without injected uniforms row i >= 32 then draws a stream of its own (include/vallex_hip.h)."""
        Engine.check_continuous(best_of, continuous, on_row)
        if seed is None:
            seed = fresh_seed()
        texts, langs, prompts = [], [], []
        for r in rows:
            t = _np(r["text"], np.int32).reshape(-1)
            p = _np(r["prompt"], np.int32).reshape(-1, 8)
            texts.append(t)
            prompts.append(p)
            langs.append(self._lang_row(len(t), int(r["enroll"]), r["prompt_language"], r["text_language"]))
        return self.engine.infer(Batch(texts, langs, prompts), top_k=top_k, temperature=temperature, uniforms=uniforms,
                                 seed=seed, force_eos_at=force_eos_at, sync_every=sync_every, best_of=best_of,
                                 length_penalty=length_penalty, return_worst=return_worst, continuous=continuous,
                                 on_row=on_row)

    # ---- teacher-forced scoring (vx_score) ---------------------------------------------------------------------
    def score(self, x, x_lens, y, enroll_x_lens, codes, prompt_language: str = None,
              text_language: Union[str, List[str]] = None, parts: str = "both"):
        """How likely the model finds `codes` (1, T, 8), as `inference` returns them, for the same x / y / languages: the quantity
        `VALLE.forward` feeds to F.cross_entropy and `inference` selects its best_of beam on (models/vallex.py:572, :583-594).
        Returns a dict: logp (T, 8) float32 and rank (T, 8) int32 -- column 0 from the AR stack given the earlier frames' first
        codebook, column q from NAR stage q - 1 given codebooks 0 .. q-1; rank = number of strictly larger logits -- and eos_logp,
        eos_rank: the stop decision behind the last frame.  sum(logp[:, 0]) + eos_logp is the beam's sum(logp).
        parts: "ar", "nar" or "both"; what is left out is NaN / -1."""
        xa, xl, ya, ca = _np(x), _np(x_lens), _np(y), _np(codes)
        assert xa.ndim == 2, xa.shape                      # the checks of inference (models/vallex.py:488-493)
        assert xl.ndim == 1, xl.shape
        assert ya.ndim == 3, ya.shape
        assert ya.shape[0] == 1, ya.shape
        assert np.all(xl > 0)
        assert ca.ndim == 3 and ca.shape[0] == 1 and ca.shape[2] == 8, ca.shape
        S = int(xl.max())
        row = dict(text=xa[0, :S], prompt=ya[0], enroll=int(_np(enroll_x_lens)), prompt_language=prompt_language,
                   text_language=text_language)
        return self.score_batch([row], [ca[0]], parts=parts)[0]

    def score_batch(self, rows: Sequence[dict], codes_list: Sequence[np.ndarray], parts: str = "both") -> List[dict]:
        """`score` for the row dicts of `inference_batch`: codes_list[i] (T_i, 8) is scored for rows[i], one call for all rows."""
        if parts not in ("ar", "nar", "both"):
            raise ValueError(f"parts must be 'ar', 'nar' or 'both', got {parts!r}")
        if len(rows) != len(codes_list):
            raise ValueError(f"{len(codes_list)} code arrays for {len(rows)} rows")
        res = self.engine.score(self.make_batch(rows), [_np(c, np.int64).reshape(-1, 8) for c in codes_list], parts)
        return [dict(logp=lp, rank=rk, eos_logp=el, eos_rank=er) for lp, rk, el, er in res]

    # ---- text alignment (vx_align) -------------------------------------------------------------------------------
    def align(self, x, x_lens, y, enroll_x_lens, codes, prompt_language: str = None,
              text_language: Union[str, List[str]] = None, head_weights=None):
        """Where in the text every frame of `codes` (1, T, 8), as `inference` returns them, came from: the attention of the AR row
        that predicts frame t over the S text positions (the prompt's text included), summed over layers and heads with
        head_weights (num_layers, 16); None: 1 / (16 num_layers) each.  Returns a dict: attn (T, S) float32; text_mass (T,), its row
        sums (with uniform weights the text's share of the attention, at most 1); segments (S - enroll, 2) int32, first and last frame
        of every token of the text that was synthesised (utils.alignment.monotonic_segments), or None when T < S - enroll.
        The segments follow the documented rule whatever the weights are; how well they track the speech depends on which heads of a
        trained checkpoint align -- that calibration is the caller's, through head_weights."""
        xa, xl, ya, ca = _np(x), _np(x_lens), _np(y), _np(codes)
        assert xa.ndim == 2, xa.shape                      # the checks of inference (models/vallex.py:488-493)
        assert xl.ndim == 1, xl.shape
        assert ya.ndim == 3, ya.shape
        assert ya.shape[0] == 1, ya.shape
        assert np.all(xl > 0)
        assert ca.ndim == 3 and ca.shape[0] == 1 and ca.shape[2] == 8, ca.shape
        S = int(xl.max())
        row = dict(text=xa[0, :S], prompt=ya[0], enroll=int(_np(enroll_x_lens)), prompt_language=prompt_language,
                   text_language=text_language)
        return self.align_batch([row], [ca[0]], head_weights=head_weights)[0]

    def align_batch(self, rows: Sequence[dict], codes_list: Sequence[np.ndarray], head_weights=None) -> List[dict]:
        """`align` for the row dicts of `inference_batch`: codes_list[i] (T_i, 8) is aligned with the text of rows[i], one call."""
        from ..utils.alignment import monotonic_segments
        if len(rows) != len(codes_list):
            raise ValueError(f"{len(codes_list)} code arrays for {len(rows)} rows")
        res = self.engine.align(self.make_batch(rows), [_np(c, np.int64).reshape(-1, 8) for c in codes_list], head_weights)
        out = []
        for r, a in zip(rows, res):
            enroll = int(r["enroll"])
            seg = monotonic_segments(a, enroll) if a.shape[0] >= a.shape[1] - enroll else None
            out.append(dict(attn=a, text_mass=a.sum(1), segments=seg))
        return out

    def serve(self, top_k: int = -100, temperature: float = 1.0, sync_every: int = 8, force_eos_at=None, max_steps: int = 32,
              post=None, **kw) -> "Server":
        """A threaded serving front end (include/vallex_hip.h vx_serve_*): `Server.submit(row, best_of=..., seed=...)` may be called
        from any thread at any time and returns a Future of the row's (T, 8) int64 codes -- exactly what `inference_batch([row],
        best_of=..., seed=...)` returns.  sync_every applies to the whole session; top_k / temperature / force_eos_at given here
        are the defaults of the requests that do not set their own; best_of, length_penalty, return_worst, seed, uniforms, top_k,
        temperature and force_eos_at are per request (Server.submit).  A request's Future can be cancelled until it is delivered.  `max_steps`: decode steps per
        vx_serve_run, i.e. how long a new submission waits at most for the worker to pick it up.  `post(codes list) -> results`
        (optional) runs on the worker thread for every group of completed requests (AudioServer: Vocos)."""
        if kw:
            bad = sorted(kw)
            raise ValueError(f"{', '.join(bad)}: per request in a serving session (Server.submit), not session-wide"
                             if set(bad) <= {"best_of", "length_penalty", "return_worst", "seed", "uniforms"}
                             else f"unexpected arguments {bad}")
        return Server(self, top_k=top_k, temperature=temperature, sync_every=sync_every, force_eos_at=force_eos_at,
                      max_steps=max_steps, post=post)

    def make_batch(self, rows: Sequence[dict]) -> Batch:
        texts = [_np(r["text"], np.int32).reshape(-1) for r in rows]
        prompts = [_np(r["prompt"], np.int32).reshape(-1, 8) for r in rows]
        langs = [self._lang_row(len(t), int(r["enroll"]), r["prompt_language"], r["text_language"])
                 for t, r in zip(texts, rows)]
        return Batch(texts, langs, prompts)


class Server:
    """Threaded front end of a serving session (VALLE.serve).  One worker thread owns every C call on the model's engine: it opens the
    session, moves queued submissions into it between two vx_serve_run calls, runs the session while anything is decoding or
    waiting, and resolves every request's Future as soon as its NAR stages are done.  submit() is thread-safe and does the host
    work of a row (ids, languages, prompt) on the submitting thread.  close() (or leaving a `with` block) finishes everything that
    was submitted, then closes the session.  A C error fails every outstanding Future with the VallexHipError and closes the session;
    a request the library refuses (VX_EINVAL at submit: oversized row, too few uniforms) fails its own Future only.  A Future stays
    PENDING until it is delivered, so `fut.cancel()` succeeds while its request waits or decodes: a done-callback wakes the worker,
    which cancels the request in the session (vx_serve_cancel) before its next vx_serve_run -- the request's decode rows go to the
    next admission -- and a cancelled Future never receives a result."""

    def __init__(self, model: "VALLE", top_k=-100, temperature=1.0, sync_every=8, force_eos_at=None, max_steps=32, post=None):
        self._model = model
        self._opts = dict(top_k=top_k, temperature=temperature, sync_every=sync_every, force_eos_at=force_eos_at)
        self._max_steps = int(max_steps)
        self._post = post
        self._cv = threading.Condition()
        self._queue: List[tuple] = []           # (Batch, request dict, Future) not yet handed to the library
        self._futs: Dict[int, Future] = {}     # request id -> Future (worker thread only)
        self._closing = False
        self._error: Optional[BaseException] = None
        engine = model.engine                   # built here: a weight error surfaces on the caller's thread
        self.rows = min(engine.max_batch, 32)
        self._ready = threading.Event()
        self._thread = threading.Thread(target=self._loop, name="vallex-serve", daemon=True)
        self._thread.start()
        self._ready.wait()
        if self._error is not None:
            raise self._error

    def submit(self, row: dict, best_of: int = 1, seed: Optional[int] = None, uniforms=None, length_penalty: float = 1.0,
               return_worst: bool = False, top_k: Optional[int] = None, temperature: Optional[float] = None,
               force_eos_at: Optional[int] = None, top_p: Optional[float] = None, repetition_penalty: Optional[float] = None,
               repetition_window: Optional[int] = None, min_frames: Optional[int] = None) -> Future:
        """row: the dict of inference_batch (text, prompt, enroll, prompt_language, text_language).  Returns a Future of the
        (T, 8) int64 codes (or of post's result).  seed=None draws a fresh seed, like inference; top_k / temperature /
        force_eos_at None: the session's value.  top_p (nucleus sampling after top_k), repetition_penalty over the last
        repetition_window generated frames (0: all of them) and min_frames (no EOS before that many frames); None: off."""
        u = ServeSession.check_request(best_of, uniforms, self.rows, top_k, temperature, force_eos_at, top_p=top_p,
                                       repetition_penalty=repetition_penalty, repetition_window=repetition_window,
                                       min_frames=min_frames)
        if seed is None:
            seed = fresh_seed()
        batch = self._model.make_batch([row])
        req = dict(best_of=int(best_of), seed=int(seed), uniforms=u, length_penalty=float(length_penalty),
                   return_worst=bool(return_worst))
        for k, v in (("top_k", top_k), ("temperature", temperature), ("force_eos_at", force_eos_at), ("top_p", top_p),
                     ("repetition_penalty", repetition_penalty), ("repetition_window", repetition_window),
                     ("min_frames", min_frames)):
            if v is not None:
                req[k] = v
        fut: Future = Future()
        with self._cv:
            if self._closing or self._error is not None:
                raise RuntimeError("the server is closed" if self._error is None else f"the server failed: {self._error}")
            self._queue.append((batch, req, fut))
            self._cv.notify()
        fut.add_done_callback(self._wake)
        return fut

    def _wake(self, fut: Future):
        """done-callback of every Future: a cancellation wakes the worker (it cancels the request before its next run)"""
        if fut.cancelled():
            with self._cv:
                self._cv.notify()

    def close(self):
        """finish every submitted request, then close the session (idempotent)"""
        with self._cv:
            self._closing = True
            self._cv.notify()
        if self._thread.is_alive() and threading.current_thread() is not self._thread:
            self._thread.join()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- worker thread ----
    def _loop(self):
        try:
            session = self._model.engine.serve(**self._opts)
        except BaseException as e:
            self._error = e
            self._ready.set()
            return
        self._ready.set()
        try:
            while True:
                # Futures cancelled since the last run: out of the session before the next one
                for rid in [r for r, f in self._futs.items() if f.cancelled()]:
                    session.cancel(rid)
                    del self._futs[rid]
                with self._cv:
                    while not self._queue and not self._futs and not self._closing:
                        self._cv.wait()
                    # the exit test reads the live queue under the lock: a submit() that got in before close() is served
                    if not self._queue and not self._futs and self._closing:
                        break
                    items, self._queue = self._queue, []
                for batch, req, fut in items:
                    if fut.cancelled():
                        continue
                    try:
                        rid = session.submit(batch, [req])[0]
                    except VallexHipError as e:
                        if e.code != VX_EINVAL:
                            raise
                        self._settle(fut, exc=e)         # refused: this request only, the session goes on
                        continue
                    self._futs[rid] = fut
                if self._futs:
                    done = []
                    session.run(self._max_steps, lambda rid, codes: done.append((rid, codes)))
                    self._deliver(done)
        except BaseException as e:
            self._fail(e)
        finally:
            try:
                session.close()
            except BaseException:
                pass

    def _deliver(self, done):
        if not done:
            return
        futs = [self._futs.pop(rid) for rid, _ in done]
        codes = [c for _, c in done]
        try:
            res = self._post(codes) if self._post is not None else codes
        except BaseException as e:
            for f in futs:
                self._settle(f, exc=e)
            return
        for f, r in zip(futs, res):
            self._settle(f, res=r)

    @staticmethod
    def _settle(f: Future, res=None, exc=None):
        """a Future cancelled after its request was delivered (between run() and here) keeps its cancellation"""
        try:
            if exc is not None:
                f.set_exception(exc)
            else:
                f.set_result(res)
        except InvalidStateError:
            pass

    def _fail(self, e: BaseException):
        with self._cv:
            self._error = e
            self._closing = True
            items, self._queue = self._queue, []
        for f in list(self._futs.values()) + [it[2] for it in items]:
            if not f.done():
                self._settle(f, exc=e)
        self._futs.clear()
