/* vallex_hip.h -- C ABI of the MI355X-native VALL-E X inference hot path (libvallex_hip.so).
 *
 * The reference (Plachtaa/VALL-E-X) has no FFI or plugin interface: its drop-in boundary is the Python API
 * (utils/generation.py:50,92,155 and models/vallex.py:458).  The package `vall-e-x_amd/` keeps those Python
 * signatures and binds THIS header through ctypes; each entry point below cites the reference code it replaces
 * (paths relative to the reference repository root).
 *
 * Conventions
 *   - plain pointers and sizes only; host pointers unless stated; the library owns all device memory inside an
 *     opaque context (weights, KV arena, activations) and one HIP stream per context;
 *   - every function returns 0 on success or a negative VX_E* code; vx_last_error() gives the message;
 *   - a context is not thread-safe; different contexts (one per GPU / per host thread) are independent;
 *   - token ids are int32 on the way in (max id 2047) and int64 on the way out, like the reference's LongTensor.
 */
#ifndef VALLEX_HIP_H
#define VALLEX_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VX_OK 0
#define VX_EINVAL (-1)   /* bad argument / shape (reference: AssertionError, models/vallex.py:488-493) */
#define VX_EHIP (-2)     /* HIP runtime failure (no GPU, OOM, launch error) */
#define VX_ESTATE (-3)   /* call order violated (e.g. infer before vx_finalize_weights) */
#define VX_ENOTFOUND (-4)/* unknown tensor name (reference: load_state_dict(strict=True) unexpected key) */

typedef struct vx_ctx vx_ctx;

/* ABI guard.  Every descriptor struct starts with `struct_size` = sizeof(that struct) as the CALLER compiled it; the library
 * rejects a mismatch with VX_EINVAL instead of reading past the end of a shorter (older) struct.  vx_abi_version() returns
 * VX_ABI_VERSION of the library that was actually loaded, so a binding can check it before the first call. */
#define VX_ABI_VERSION 6      /* 6: best_of > 1 with batch > 1 (vx_sampling layout unchanged since 5) */
int32_t vx_abi_version(void);

/* Model/arena geometry.  d_model=1024, 16 heads, FFN 4096, 8 codebooks are fixed by the kernels
 * (macros.py:1-6, utils/generation.py:67-78); the layer count is configurable so tests can run reduced stacks. */
typedef struct vx_config {
  uint32_t struct_size;    /* = sizeof(vx_config) */
  int32_t num_layers;      /* 12 for the shipped checkpoint */
  int32_t max_batch;       /* rows per vx_infer call; AR runs in micro-batches of <= 32 rows */
  int32_t max_text;        /* max text ids per row (prompt text + text), S */
  int32_t max_prompt;      /* max prompt frames per row, Tp */
  int32_t max_new;         /* max generated frames per row (the reference cap is 16*S, models/vallex.py:577) */
  int32_t use_graph;       /* 1: replay the AR step as a hipGraph */
  int32_t with_vocos;      /* 1: allocate the Vocos head */
  int32_t debug_taps;      /* 1: keep per-layer activations for vx_read_tap */
  int32_t with_encodec;    /* 1: allocate the EnCodec SEANet decoder arena (needs the "encodec.*" tensors) */
  uint32_t cu_mask[8];     /* all zero: the context's stream may use every CU.  Otherwise bit i of word i/32 enables CU i
                              (hipExtStreamCreateWithCUMask): contexts that SHARE one GPU get disjoint CU sets, so the
                              latency-bound decode of one batch runs beside the matrix-bound NAR stages of another */
  int32_t arith;           /* arithmetic of the full-sequence projections and attention (AR prefill, NAR stages; the cached decode
                              step is exact fp32 always): 0 = default (f16x2 unless the environment says otherwise:
                              VX_GEMM_X3 / VX_GEMM_F32 / VX_ATTN_X3 / VX_ATTN_F32 = 1), VX_ARITH_F16X2, VX_ARITH_BF16X3,
                              VX_ARITH_F32 (the reference's own arithmetic).  See vx_arith_mode / vx_last_fallbacks. */
} vx_config;
#define VX_ARITH_DEFAULT 0
#define VX_ARITH_F16X2 1   /* operands split into fp16 head + tail (22 significant bits), fp32 accumulate, f16 MFMA */
#define VX_ARITH_BF16X3 2  /* operands split into three bf16 terms (24 bits), fp32 accumulate, bf16 MFMA */
#define VX_ARITH_F32 3     /* fp32 operands, fp32 MFMA */

/* ---- lifetime -------------------------------------------------------------------------------------------
 * replaces: model construction + .to(device) in preload_models(), utils/generation.py:67-89 */
int vx_create(int device_id, const vx_config* cfg, vx_ctx** out);
void vx_destroy(vx_ctx* ctx);
const char* vx_last_error(const vx_ctx* ctx);   /* ctx may be NULL: last error of a failed vx_create */
int vx_synchronize(vx_ctx* ctx);

/* ---- weights --------------------------------------------------------------------------------------------
 * replaces: VALLE.load_state_dict(checkpoint["model"], strict=True), utils/generation.py:79-83, and
 * Vocos.from_pretrained, utils/generation.py:89.  `name` is the reference state-dict key,
 * Vocos tensors are prefixed "vocos." + their key in the vocos package.  fp32, C-contiguous, copied. */
int vx_load_tensor(vx_ctx* ctx, const char* name, const float* data, const int64_t* shape, int32_t ndim);
/* checks that all 374 (for 12 layers) keys arrived, builds packed decode images, the positional table
 * (modules/embedding.py:75-91) and the per-stage AdaLN projections (modules/transformer.py:96-100). */
int vx_finalize_weights(vx_ctx* ctx);

/* ---- batch descriptor -------------------------------------------------------------------------------------
 * One row = one utterance = one reference `VALLE.inference(x, x_lens, y, enroll_x_lens, ...)` call. */
typedef struct vx_batch {
  uint32_t struct_size;         /* = sizeof(vx_batch) */
  int32_t batch;
  const int32_t* text_ids;      /* [batch][text_stride]   x: prompt text ids ++ text ids (utils/generation.py:133) */
  const int32_t* text_lang;     /* [batch][text_stride]   per-token MODEL language id en0/zh1/ja2 (models/vallex.py:439-443,
                                   499-505): first enroll_len entries = prompt_language, rest = text_language;
                                   -1 = add no language embedding to that token (VALLE.continual, models/vallex.py:716-729) */
  int32_t text_stride;
  const int32_t* text_lens;     /* [batch]  x_lens */
  const int32_t* prompt_codes;  /* [batch][prompt_stride][8]   y (audio prompt), values 0..1023 */
  int32_t prompt_stride;
  const int32_t* prompt_lens;   /* [batch]  y.shape[1] */
} vx_batch;

/* topk_sampling arguments (models/vallex.py:836-853) + reproducibility hooks */
typedef struct vx_sampling {
  uint32_t struct_size;         /* = sizeof(vx_sampling) */
  int32_t top_k;                /* <= 0: no filtering (API default -100); 1: greedy */
  float temperature;            /* > 0 */
  const float* uniforms;        /* optional [uniforms_steps][batch x max(1, best_of)] in [0,1): inverse-CDF draws replacing
                                   torch.multinomial (models/vallex.py:850); column r*best_of + j feeds beam j of row r (without
                                   best_of: column r feeds row r).  NULL -> counter-based RNG from `seed` */
  int32_t uniforms_steps;
  uint64_t seed;
  int32_t force_eos_at;         /* >= 0: the (n+1)-th sample is forced to EOS (benchmark stand-in for a trained
                                   model's termination; -1 = off) */
  int32_t sync_every;           /* host polls the device EOS flags every n steps (reference: every step,
                                   models/vallex.py:574-578); <= 0 -> 8 */
  int32_t best_of;              /* <= 1: off.  N > 1: every row of the batch is decoded as N beams sampled independently, and per
                                   row the beam with the best sum(logp)/len^length_penalty goes on to the NAR stages
                                   (models/vallex.py:525-527,572,583-594).  Row r returns what a batch-1 call on row r alone
                                   returns with the same draws.  N must not exceed min(max_batch, 32); the engine decodes
                                   floor(min(max_batch, 32) / N) rows x N beams at a time.  top_k, temperature, best_of,
                                   length_penalty, return_worst, force_eos_at and seed apply to every row. */
  float length_penalty;         /* models/vallex.py:584 */
  int32_t return_worst;         /* models/vallex.py:590-591 */
} vx_sampling;

/* ---- the hot path ---------------------------------------------------------------------------------------- */
/* replaces: VALLE.inference AR loop + 7 NAR stages, models/vallex.py:458-686.
 * out_codes [batch][out_stride][8] int64 (row b valid for out_lens[b] frames), out_lens [batch]. */
int vx_infer(vx_ctx* ctx, const vx_batch* b, const vx_sampling* s, int64_t* out_codes, int32_t out_stride,
             int32_t* out_lens);

/* Continuous batching (additive: VX_ABI_VERSION stays 6; a binding detects this entry point by its symbol).
 * vx_infer decodes a batch in micro-batches of min(max_batch, 32) rows and runs each until its LONGEST row has stopped.  This entry
 * decodes on one decode batch of min(max_batch, 32, batch) rows for the whole call: when a row stops (EOS, 16 x text length,
 * max_new or force_eos_at), the next waiting caller row, in caller order, takes its place at the next host poll (sync_every).
 * batch may exceed max_batch: the call holds device memory for its decode rows and one NAR group only.
 *   - out_codes / out_lens: filled exactly as vx_infer fills them.
 *   - on_row: may be NULL.  Otherwise it is called once per caller row, on the calling thread, from inside this call, in the order
 *     rows complete (their NAR stages run in groups of up to 32 finished rows): codes [frames][8] is valid only during the
 *     callback (it points into out_codes).  The callback must not call into the same context.
 *   - injected uniforms keep vx_infer's layout [uniforms_steps][batch]: column r feeds caller row r, indexed by that row's own step.
 *   - without uniforms, row r draws u = (splitmix64(splitmix64(splitmix64(seed) + r) + step) >> 40) x 2^-24: vx_infer's counter
 *     formula keyed on the CALLER row r.  Rows r < min(max_batch, 32) therefore equal vx_infer's rows with the same seed; later
 *     rows get streams of their own (in vx_infer, row r draws the stream of row r mod min(max_batch, 32)).
 *   - best_of > 1 is refused with VX_EINVAL.
 *   - vx_last_stats: AR steps = decode steps run, AR ms includes the admission prefills, NAR ms covers the NAR groups;
 *     vx_last_truncated and vx_last_fallbacks report the call as they do for vx_infer. */
typedef void (*vx_row_done_fn)(void* user, int32_t row, const int64_t* codes /* [frames][8] */, int32_t frames);
int vx_infer_continuous(vx_ctx* ctx, const vx_batch* b, const vx_sampling* s, vx_row_done_fn on_row, void* user,
                        int64_t* out_codes, int32_t out_stride, int32_t* out_lens);

/* Serving session (additive: VX_ABI_VERSION stays 6).  vx_infer and vx_infer_continuous take a closed batch; a session takes
 * requests at any time and admits each into the running decode batch as soon as enough decode rows are free.  Contract: a request
 * returns exactly what a batch-1 vx_infer call on it returns (same seed or same draws, same best_of / length_penalty /
 * return_worst, same top_k / temperature / force_eos_at), whatever else is in the session.  With per-request filters
 * (vx_request_filters, vx_serve_submit_filtered) the same holds: a request returns the same result whatever else is in the session,
 * and with the neutral filters (top_p 1, repetition_penalty 1, min_frames 0) it returns what that batch-1 vx_infer call returns.
 *   - Per request: best_of, length_penalty, return_worst, seed or injected uniforms (vx_request), and top_k, temperature and
 *     force_eos_at (vx_request_sampling, vx_serve_submit_ex).  Session-wide: sync_every only.  The session samples every decode row
 *     with its own request's top_k / temperature / force_eos_at; vx_serve_open's values are the defaults of vx_serve_submit.
 *   - vx_serve_open reads the session-wide fields of vx_sampling only: top_k, temperature, force_eos_at (the defaults), sync_every.  best_of (<= 1),
 *     seed (0), uniforms (NULL), length_penalty (0 or 1) and return_worst (0) must keep their defaults: they are per request.  The
 *     decode batch is nd = min(max_batch, 32) rows, all free.  One session per context: while it is open, vx_infer,
 *     vx_infer_continuous, vx_ar_prefill, vx_ar_step and vx_nar return VX_EINVAL (they would overwrite the decode state);
 *     vx_vocos_decode and vx_encodec_* stay allowed.
 *   - vx_serve_submit copies everything it needs (the caller's buffers may be freed on return), does no GPU work and writes
 *     increasing request ids.  Every row is checked as vx_infer checks it, plus best_of <= nd and, with injected uniforms,
 *     uniforms_steps >= min(16 x text length, max_new, the request's force_eos_at) + 1.  On any failure nothing of the call is
 *     enqueued.  vx_serve_submit_ex takes one vx_request_sampling per request as well (smp NULL: the session's values, exactly
 *     vx_serve_submit); it checks struct_size, temperature > 0 and finite, force_eos_at >= -1.
 *   - vx_serve_run admits waiting requests first come first served: the head request waits until best_of decode rows are free, a
 *     later request does not overtake it.  It runs up to max_steps decode steps (<= 0: until no request is decoding or waiting), with
 *     host polls every sync_every steps and at the step where a row reaches its cap; requests whose beams have all stopped go through
 *     the NAR stages in groups of up to 32, and before it returns every request that finished during the call has been delivered:
 *     on_done (may be NULL) is called once per request on the calling thread, codes [frames][8] valid during the callback only; the
 *     callback must not call into the same context.  live / waiting (may be NULL): requests decoding / not admitted yet.
 *     vx_last_stats, vx_last_truncated and vx_last_fallbacks describe the last vx_serve_run; vx_last_truncated judges every request
 *     by its own force_eos_at.
 *   - vx_serve_cancel, between two vx_serve_run calls, drops a request; state (may be NULL) = 0: unknown id, already delivered or
 *     already cancelled (not an error); 1: it was waiting and is removed; 2: it was decoding (some of its beams may have stopped
 *     already): its beam rows stop before the next decode step and are free for the next admission.  A cancelled request never
 *     reaches on_done, and cancelling never changes what another request returns.  Called from inside vx_serve_run (on_done) it
 *     returns VX_EINVAL and changes nothing.
 *   - vx_serve_close drops waiting requests and requests still decoding; the context is usable for vx_infer again.  vx_destroy closes
 *     an open session.
 *   - Beams.  A request with best_of = N is prefilled once and decoded as N beams on N free decode rows (any slots).  It is harvested
 *     when all N have stopped (EOS, 16 x text length, max_new or force_eos_at: models/vallex.py:572-578) and its winner is selected
 *     as vx_infer selects it: sum(logp) / (1 + Tp + frames)^length_penalty, first index wins ties, or the worst with return_worst.
 *   - RNG.  Beam j of a request with seed s draws u_t = (splitmix64(splitmix64(splitmix64(s) + j) + t) >> 40) x 2^-24 at its own step
 *     t: vx_infer's formula for decode row j of a batch-1 call.  Injected uniforms are [uniforms_steps][max(1, best_of)]: column j
 *     feeds beam j.
 *   - Arithmetic.  The f16x2 range guard works per admission round: a raised flag re-runs the round (prefill, beam fan-out, first
 *     sample) on the fp32 kernels and counts in vx_last_fallbacks and towards sticky mode. */
typedef struct vx_serve vx_serve;
typedef struct vx_request {
  uint32_t struct_size;         /* = sizeof(vx_request) */
  int32_t best_of;              /* <= 1: one beam; N: N beams, N <= min(max_batch, 32) */
  float length_penalty;
  int32_t return_worst;
  uint64_t seed;                /* counter RNG key of this request (ignored with uniforms) */
  const float* uniforms;        /* optional [uniforms_steps][max(1, best_of)]: column j feeds beam j */
  int32_t uniforms_steps;
} vx_request;
typedef void (*vx_serve_done_fn)(void* user, int64_t request_id, const int64_t* codes /* [frames][8] */, int32_t frames);
int vx_serve_open(vx_ctx* ctx, const vx_sampling* s, vx_serve** out);
/* rows->batch requests, req [rows->batch]; ids_out [rows->batch] (may be NULL) */
int vx_serve_submit(vx_serve* srv, const vx_batch* rows, const vx_request* req, int64_t* ids_out);
int vx_serve_run(vx_serve* srv, int32_t max_steps, vx_serve_done_fn on_done, void* user, int32_t* live_requests,
                 int32_t* waiting_requests);
int vx_serve_close(vx_serve* srv);
/* per-request topk_sampling arguments (models/vallex.py:836-853) of a serving session */
typedef struct vx_request_sampling {
  uint32_t struct_size;         /* = sizeof(vx_request_sampling) */
  int32_t top_k;                /* as vx_sampling.top_k */
  float temperature;            /* > 0, finite */
  int32_t force_eos_at;         /* as vx_sampling.force_eos_at: -1 off, n >= 0: the (n+1)-th sample is EOS (at most n frames) */
} vx_request_sampling;
int vx_serve_submit_ex(vx_serve* srv, const vx_batch* rows, const vx_request* req,
                       const vx_request_sampling* smp /* [rows->batch] or NULL */, int64_t* ids_out);
int vx_serve_cancel(vx_serve* srv, int64_t request_id, int32_t* state /* may be NULL */);
/* Per-request logit filters of a serving session, applied per decode row to the row's fp32 logits in this order: repetition
 * penalty, min_frames, temperature, top_k, top_p, then the draw.
 *   - repetition_penalty r over the request's own generated frames (per beam; the prompt does not count), the last
 *     repetition_window of them (0: all): every token that occurs there, once however often, gets l > 0 ? l / r : l * r.
 *   - min_frames m: EOS cannot be sampled while fewer than m frames are generated.  The stop rules still end the request
 *     (16 x text length, max_new, force_eos_at, which overrides the sample as before).
 *   - top_p: nucleus sampling over the tokens top_k left (top_k_top_p_filtering, models/vallex.py:811-832): a token stays iff the
 *     probability mass of the strictly larger logits is <= top_p.  Every token tied with the last kept value is kept (the reference's
 *     unstable sort splits such a tie arbitrarily).  sum(logp) of best_of is taken under the filtered distribution.
 * flt NULL: exactly vx_serve_submit_ex.  Checked (VX_EINVAL, nothing enqueued, the message names the field): struct_size; top_p finite,
 * > 0 and <= 1; repetition_penalty finite and > 0; repetition_window >= 0; min_frames >= 0. */
typedef struct vx_request_filters {
  uint32_t struct_size;         /* = sizeof(vx_request_filters) */
  float top_p;                  /* (0, 1]; 1: off */
  float repetition_penalty;     /* > 0; 1: off */
  int32_t repetition_window;    /* frames looked back; 0: every generated frame */
  int32_t min_frames;           /* 0: off */
} vx_request_filters;
int vx_serve_submit_filtered(vx_serve* srv, const vx_batch* rows, const vx_request* req,
                             const vx_request_sampling* smp /* [rows->batch] or NULL */,
                             const vx_request_filters* flt /* [rows->batch] or NULL */, int64_t* ids_out);

/* replaces: vocos.codes_to_features + vocos.decode(features, bandwidth_id), utils/generation.py:148-150.
 * codes [batch][codes_stride][8] int64, lens [batch] frames; audio [batch][audio_stride] fp32, 320*len samples each. */
int vx_vocos_decode(vx_ctx* ctx, const int64_t* codes, int32_t codes_stride, const int32_t* lens, int32_t batch,
                    int32_t bandwidth_id, float* audio, int64_t audio_stride);

/* replaces: AudioTokenizer.decode(frames) -> codec.decode (EnCodec 24 kHz SEANet decoder: RVQ sum, Conv1d, 2-layer LSTM,
 * 4 x [ELU, ConvTranspose1d, ResnetBlock], ELU, Conv1d), data/tokenizer.py:95-96 -- the legacy vocoder the reference keeps
 * beside Vocos (README.md:29-30).  Tensors are loaded as "encodec." + {quantizer.{q}.embed, decoder.{i}.weight|bias,
 * decoder.{i}.block1|block3|shortcut.weight|bias, decoder.1.lstm.*} with weight-norm already folded.
 * codes [batch][codes_stride][8] int64, lens [batch]; audio [batch][audio_stride] fp32, 320*len samples each. */
int vx_encodec_decode(vx_ctx* ctx, const int64_t* codes, int32_t codes_stride, const int32_t* lens, int32_t batch,
                      float* audio, int64_t audio_stride);

/* replaces: AudioTokenizer.encode(wav) -> codec.encode (EnCodec 24 kHz SEANet encoder + residual vector quantiser at 6 kbps,
 * 8 codebooks), data/tokenizer.py:92-111 -- the prompt-enrolment path (tokenize_audio, utils/prompt_making.py:57-84).
 * Needs the decoder tensors plus "encodec.encoder." + {0,3,6,9,12,15}.{weight,bias}, {1,4,7,10}.{block1,block3,shortcut}.{weight,
 * bias}, 13.lstm.* (weight-norm folded).  wav [batch][wav_stride] fp32 mono 24 kHz, lens [batch] samples;
 * codes [batch][codes_stride][8] int64, out_lens [batch] = ceil(len / 320) frames. */
int vx_encodec_encode(vx_ctx* ctx, const float* wav, int64_t wav_stride, const int32_t* lens, int32_t batch, int64_t* codes,
                      int32_t codes_stride, int32_t* out_lens);

/* Sample-rate conversion of mono fp32 rows on the device: the other rates at both audio ends (everything above takes and gives
 * 24 kHz).  replaces: convert_audio -> torchaudio.transforms.Resample(sr, 24000) with its defaults, data/tokenizer.py:105 -- restated
 * from the package's published algorithm, unpinned (the package is not installed where this was written).
 * With o, n = orig_rate, new_rate over their gcd: base = min(o, n) * 0.99, width = ceil(6 o / base), K = 2 width + o; n phase kernels
 * of K Hann-windowed sinc taps, built on the host in double (the phase -p / n in fp32), rounded once to fp32 and cached per (o, n);
 *   out[b][i n + p] = sum_j k_p[j] * x_b[i o + j - width],  x_b = 0 outside [0, lens[b]),  out_lens[b] = ceil(n lens[b] / o).
 * Every element is one zero-initialised accumulator and K fmaf in tap order: its bits do not depend on the batch or on the windows.
 *   wav [batch][wav_stride] fp32, lens [batch] samples (0 allowed: the row writes nothing); out [batch][out_stride] fp32; elements
 *   behind out_lens[b] are not written.  orig_rate == new_rate copies the input bits.
 * Needs no weights: it works on any created context, before vx_finalize_weights too, and while a serving session is open; it touches
 * no decode state, no KV arena and no fallback counter.  The first call allocates its device buffers (vx_destroy frees them): one
 * launch holds VX_RESAMPLE_WINDOW input samples (and twice as many output samples); the rows of a call are packed into launches in
 * order and a row that does not fit is cut into windows, each with the real samples its taps reach on both sides -- by the rule above
 * the result is bit-identical to a single pass.
 * VX_EINVAL, nothing launched, the message naming the field: a NULL pointer; batch <= 0; a rate <= 0; a length negative or above
 * wav_stride; out_stride below an output length; n K above 2^18 taps (1 MiB; e.g. 44101 -> 24000 -- every pair of the usual audio
 * rates is below 52 000). */
#define VX_RESAMPLE_WINDOW (1 << 23)
int vx_resample(vx_ctx* ctx, const float* wav, int64_t wav_stride, const int32_t* lens, int32_t batch, int32_t orig_rate,
                int32_t new_rate, float* out, int64_t out_stride, int32_t* out_lens);

/* The output stage between a vocoder (or the resampler) and a sound device or file: trim, level, fade and 16-bit PCM of mono fp32
 * rows on the device, with the measurements it rests on.  No reference counterpart: the reference hands back raw fp32.
 * vx_finish measures every row (frame table -> vx_wave_info) and, when `out` is given, writes the kept span of every row, scaled,
 * faded and in the asked format.  Every quantity is defined so that a plain numpy restatement reproduces it bit for bit:
 *
 * - Samples.  y[i] = isfinite(x[i]) ? x[i] : 0.  A non-finite sample never reaches an output.  It is counted in `nonfinite` (whole
 *   row).
 * - Frames.  Frame f covers samples [f F, min((f+1) F, L)); n_f is its count.  e_f is ONE LANE's sum in double of
 *   (double)y * (double)y, taken in sample order from 0.0.  The square is exact in double, so contraction to an fma cannot change a
 *   bit.  This equals np.cumsum(y.astype(f64) ** 2)[-1].  p_f = max |y|.  A frame's bits do not depend on the row, batch, tile or
 *   window it lands in.
 * - Active.  A frame is active iff e_f > thr2 * n_f, evaluated in double.  thr2 = pow(10.0, silence_db / 10.0) is computed once on
 *   the host.  mean_square = (sum e_f) / (sum n_f) over the active frames, in frame order in double.
 * - Span.  No active frame: begin = end = 0 on any trimmed side.  An untrimmed call keeps [0, L).  The gain is 1.  Otherwise, with
 *   first and last active frames a and z: begin = (trim & 1) ? max(0, a F - keep) : 0 and
 *   end = (trim & 2) ? min(L, (z + 1) F + keep) : L.
 * - Gain.  The gain is computed on the host in double and rounded once to fp32.  t = pow(10, level_db / 20).  Peak mode:
 *   g = t / peak.  RMS mode: g = t / sqrt(mean_square).  The result is min(g, pow(10, max_gain_db / 20)) (and at most FLT_MAX, so
 *   that the fp32 gain is finite).  The gain is 1 when the denominator is 0.
 * - Fades.  Two host-built fp32 tables use the smoothstep w(u) = u u (3 - 2u) with u = (j + 0.5) / n, evaluated in double with
 *   + - * / only and rounded once.  No transcendental is used, so numpy reproduces every word.  Output sample i of n gets tab_in[i]
 *   if i < fade_in, and tab_out[n - 1 - i] if n - 1 - i < fade_out.  It gets both where they overlap.  Rows shorter than a fade use
 *   the part of the table they reach.
 * - Apply.  The order is: v = y * g, then v *= tab_in[..] if it applies, then v *= tab_out[..] if it applies.  These are three
 *   separately rounded fp32 multiplies.  VX_PCM_F32: out = v.  `clipped` counts |v| > 1.  VX_PCM_S16: r = rintf(v * 32768.0f)
 *   (round half to even), stored as int16 clamped to [-32768, 32767].  `clipped` counts the samples the clamp changed.  Elements
 *   behind out_lens[b] are not written.  A row of length 0 writes nothing.
 * - Exactness and atomics.  The integer counts use integer atomics.  There are no floating-point atomics anywhere.  Two calls give
 *   the same bits.
 * - State.  As vx_resample: it needs no weights; it works on any created context, before vx_finalize_weights and while a serving
 *   session is open; it touches no decode state, KV arena or fallback counter; the first call allocates its device buffers, which it
 *   shares with the resampler's, since a context is single-threaded; vx_destroy frees them; all transfers go through the context's
 *   pinned ring.
 * - Windows.  One launch holds VX_FINISH_WINDOW (2^23) input samples.  Rows are packed into launches in order.  A longer row is cut at
 *   frame multiples for the measure pass and anywhere for the apply pass.  By the rules above the result is bit-identical to a single
 *   pass.
 * - Refusals.  These return VX_EINVAL, launch nothing and write nothing, and the message names the field: NULL wav / lens / o / info;
 *   out given without out_lens; batch <= 0; a wrong struct_size; every range above; a length negative or above wav_stride; out_stride
 *   below a row's UNTRIMMED length, so that refusal never depends on the data.
 *
 *   wav [batch][wav_stride] fp32, lens [batch] samples; out [batch][out_stride] elements of `format` (float or int16_t), NULL:
 *   measure only (info[b].clipped = 0); out_lens [batch] = end - begin (written when given); info [batch].  With `out` NULL the
 *   fields trim .. format are still checked. */
#define VX_PCM_F32 0
#define VX_PCM_S16 1
#define VX_LEVEL_NONE 0
#define VX_LEVEL_PEAK 1
#define VX_LEVEL_RMS  2
#define VX_FINISH_WINDOW (1 << 23)
typedef struct vx_finish_opts {
  uint32_t struct_size;   /* = sizeof(vx_finish_opts) */
  int32_t frame;          /* analysis frame in samples, 16 .. 4096 (10 ms = rate / 100) */
  float silence_db;       /* finite, <= 0: a frame is ACTIVE iff its mean square exceeds 10^(silence_db / 10) */
  int32_t trim;           /* bit 0: cut before the first active frame, bit 1: cut behind the last one */
  int32_t keep;           /* >= 0: samples kept outside the active span on a trimmed side */
  int32_t level_mode;     /* VX_LEVEL_* */
  float level_db;         /* finite, <= 0: target dBFS of the peak / of the RMS over the active frames */
  float max_gain_db;      /* finite, >= 0: cap of the gain */
  int32_t fade_in, fade_out; /* >= 0 samples, <= 2^20 */
  int32_t format;         /* VX_PCM_* : element type of out */
} vx_finish_opts;
typedef struct vx_wave_info {
  int32_t begin, end;     /* the kept span [begin, end) in input samples; out_len = end - begin */
  int32_t active_frames, nonfinite, clipped;
  float peak;             /* max |y| over the frames that intersect [begin, end) */
  float gain;             /* the linear gain that was applied (1 with VX_LEVEL_NONE) */
  double mean_square;     /* over the active frames; 0 if there is none */
} vx_wave_info;
int vx_finish(vx_ctx* ctx, const float* wav, int64_t wav_stride, const int32_t* lens, int32_t batch, const vx_finish_opts* o,
              void* out /* may be NULL: measure only */, int64_t out_stride /* in elements */, int32_t* out_lens, vx_wave_info* info);

/* The speaking rate: a pitch-preserving time-stretch of mono fp32 rows on the device by WSOLA (waveform-similarity overlap-add).  No
 * reference counterpart: the reference's pace is whatever the checkpoint and the prompt produce.  Each output hop is a crossfade
 * between the continuation of the previous input segment and a new input segment, which is searched near its nominal position for the
 * best match with that continuation.  The chosen positions are the exact map from output time to input time.  Inputs are a row x of
 * length L and the options speed_num / speed_den, hop (H) and search (D).  The speed is reduced by its gcd and written num / den
 * below.  Every quantity is defined so that a plain numpy restatement reproduces it bit for bit:
 *
 * - Samples.  y[i] = isfinite(x[i]) ? x[i] : 0.  Outside [0, L), y = 0.
 * - Lengths.  Lout = ceil(L * den / num) in 64-bit integers.  The row has M = ceil(Lout / H) frames.  Frame k writes output samples
 *   [k H, min((k + 1) H, Lout)).
 * - Nominal positions.  n_k = floor(k * H * num / den) in 64-bit integers.
 * - Frame 0.  p_0 = 0 and out[j] = y[j].
 * - Search, for k >= 1.  The template is t[j] = y[p_{k-1} + H + j] for j in [0, H).  For every d in [-D, D], ONE LANE computes two
 *   double sums from 0.0 in order j = 0 .. H-1: c_d = sum (double)y[n_k + d + j] * (double)t[j] and e_d = sum (double)y[n_k + d + j]^2.
 *   Every product of two fp32 values is exact in double, so contraction to an fma cannot change a bit.  These sums equal
 *   np.cumsum(...)[-1] in float64.  D_d = e_d - 2.0 * c_d in double: the squared distance to the template minus the template's own
 *   energy.  2 c is exact, so it is again contraction-proof.  p_k = n_k + d*, where d* has the smallest D_d.  Ties go to the smallest
 *   |d|, then to the negative d.  Consequence: an all-zero row keeps its nominal positions.
 * - Crossfade.  w = the smoothstep table of H entries, w[j] = u u (3 - 2u) at u = (j + 0.5) / H, built in double and rounded once to
 *   fp32 (the fade table of vx_finish).  For k >= 1: out[k H + j] = (float)((double)y[p_k + j] * (double)w[j] + (double)t[j] *
 *   (double)w[H-1-j]).  That is two exact products, one double addition and one rounding to fp32.
 * - Positions.  pos[b][k] = p_k (int32) is returned when `pos` is given.
 * - Speed 1.  With num == den the input bits are copied and pos[k] = k H, as vx_resample does at equal rates.
 * - Exactness.  No floating-point atomics.  Two calls give the same bits.  A row's bits do not depend on the batch or on the launch
 *   windows.
 * - State.  As vx_resample: it needs no weights and works before vx_finalize_weights; it works while a serving session is open; it
 *   touches no decode state, KV arena or fallback counter; it runs in the resampler's launch buffers, with a small positions / cost
 *   buffer of its own; transfers go through the pinned ring.
 * - Windows.  One launch holds VX_STRETCH_WINDOW (2^23) input samples.  Rows are packed into launches in order.  A longer row is cut
 *   at frame boundaries; its next window goes into the next launch and starts from the position found for the frame before it.
 * - Refusals.  These return VX_EINVAL, launch nothing and write nothing, and the message names the field: hop outside 16 .. 2048;
 *   search outside 0 .. 1024; speed_num or speed_den outside 1 .. 32767, or num / den outside 1/2 .. 2 (the output then fits the
 *   resampler's two-to-one output buffer); a wrong struct_size; NULL wav / lens / o / out / out_lens; batch <= 0; a length negative
 *   or above wav_stride; out_stride below a row's Lout; pos_stride below a row's M when pos is given.
 *
 *   wav [batch][wav_stride] fp32, lens [batch] samples (0 allowed: the row writes nothing); out [batch][out_stride] fp32, out_lens
 *   [batch] = Lout; pos [batch][pos_stride] int32 or NULL.  Elements behind out_lens[b] and behind pos[b][M] are not written. */
#define VX_STRETCH_WINDOW (1 << 23)
typedef struct vx_stretch_opts {
  uint32_t struct_size;   /* = sizeof(vx_stretch_opts) */
  int32_t speed_num, speed_den; /* 1 .. 32767 each, 1/2 <= speed_num / speed_den <= 2: above 1 is faster (shorter) */
  int32_t hop;            /* H, 16 .. 2048 samples (10 ms = rate / 100) */
  int32_t search;         /* D, 0 .. 1024 samples on either side of the nominal position */
} vx_stretch_opts;
int vx_stretch(vx_ctx* ctx, const float* wav, int64_t wav_stride, const int32_t* lens, int32_t batch, const vx_stretch_opts* o,
               float* out, int64_t out_stride, int32_t* out_lens, int32_t* pos /* may be NULL */, int64_t pos_stride);

/* Where the pauses of a row are: the frames pass of vx_finish (frames of o->frame = F samples, the same kernel and the same frame
 * table) reduced on the host to the quiet stretches INSIDE the speech.  No reference counterpart.
 *
 * - Frames.  Frame f covers the samples [f F, min((f + 1) F, L)), n_f of them; e_f is the double sum of the exact squares of y in
 *   sample order, y[i] = isfinite(x[i]) ? x[i] : 0, as vx_finish states it.
 * - Quiet.  Frame f is quiet iff e_f <= 10^(silence_db / 10) * n_f -- the negation of vx_finish's active rule with the same
 *   operands, so the detector and `trim` agree to the bit on every frame.
 * - Pauses.  Let f_first and f_last be the first and the last frame that is not quiet.  A pause is a maximal run [f_a, f_b) of quiet
 *   frames with f_first < f_a and f_b <= f_last, of at least min_frames frames.  Leading and trailing silence are no pauses (they
 *   are vx_finish's trim); a row without an active frame has none.
 * - Spans.  A pause is reported as the sample span [f_a F + keep, f_b F - keep) and dropped when that span is empty.  Spans come in
 *   order: spans[b][2 i], spans[b][2 i + 1] = begin, end of pause i; counts[b] = the number reported.
 * - Refusals.  VX_EINVAL, nothing launched or written behind the frames pass, the message names the field: a wrong struct_size; NULL
 *   wav / lens / o / spans / counts; batch <= 0; a length negative or above wav_stride; frame outside 16 .. 4096; silence_db not
 *   finite or above 0; min_frames below 1; keep below 0; a span_stride below 2 * counts[b] -- the message names the row and the
 *   count needed, and no row's spans are written.
 * - Limits.  The detector assumes a steady noise floor, as `trim` does: one threshold for the whole row.
 * - State.  As vx_finish: no weights, no decode state, the resampler's launch buffers; the launch window of the frames pass is
 *   vx_finish's. */
typedef struct vx_pause_opts {
  uint32_t struct_size;   /* = sizeof(vx_pause_opts) */
  int32_t frame;          /* F, 16 .. 4096 samples (10 ms = rate / 100) */
  float silence_db;       /* finite, <= 0: a frame at or below this mean square (dBFS) is quiet */
  int32_t min_frames;     /* >= 1: the shortest run of quiet frames that is a pause */
  int32_t keep;           /* >= 0: samples of a pause left out of its span at either end */
} vx_pause_opts;
int vx_pauses(vx_ctx* ctx, const float* wav, int64_t wav_stride, const int32_t* lens, int32_t batch, const vx_pause_opts* o,
              int32_t* spans, int64_t span_stride /* in int32 elements */, int32_t* counts);

/* A piecewise time map applied by WSOLA: where vx_stretch has one speed for the row, vx_retime takes anchors (input sample, output
 * sample) and maps every segment between two anchors at its own rate.  Segments of equal input and output length are copied, the
 * others are walked by WSOLA under vx_stretch's arithmetic with both ends pinned, so that every segment starts and ends at a known
 * input sample and the segments of a row do not depend on each other.  No reference counterpart.  Inputs are a row x of length L,
 * its anchors and the options hop (H) and search (D).
 *
 * - Anchors.  Row b has n_anchors[b] = m + 1 anchors (a_i, b_i), i = 0 .. m, at anchors[b][2 i], anchors[b][2 i + 1]; both
 *   coordinates strictly increase, (a_0, b_0) = (0, 0) and a_m = L.  Lout = b_m.  A row of length 0 has the single anchor (0, 0)
 *   and writes nothing.
 * - Segments.  Segment i maps the input [a_i, a_{i+1}), la samples, onto the output [b_i, b_{i+1}), lb samples.
 * - Samples.  y[i] = isfinite(x[i]) ? x[i] : 0.  Outside [0, L), y = 0.
 * - Copy segment, la == lb.  out[b_i + j] has the bits of x[a_i + j], non-finite values included, as vx_stretch at speed 1.
 * - Walked segment, la != lb.  It needs la >= 2H, lb >= 2H and 1/4 <= la / lb <= 4.  It has M = floor(lb / H) frames and rem =
 *   lb - M H; frame k writes the output samples [b_i + k H, b_i + (k + 1) H), the last one rem more.
 *   - Start pin.  p_0 = a_i and out[b_i + j] = y[a_i + j] for j in [0, H); cost 0.  The segment before ended at a_i exactly.
 *   - Nominal positions, 1 <= k <= M - 1.  n_k = a_i + floor(k * (la - lb + (M - 1) H) / (M - 1)) in 64-bit integers: the straight
 *     line from p_0 to the end pin.
 *   - Template.  t[j] = y[p_{k-1} + H + j], j in [0, H).  It may read past a_{i+1}: the row's own samples, 0 past its end.
 *   - Search, 1 <= k <= M - 2.  d in [-D, D] with a_i <= n_k + d <= a_{i+1} - H; d = 0 always qualifies.  For every such d ONE LANE
 *     computes two double sums from 0.0 in order j = 0 .. H-1: c_d = sum (double)y[n_k + d + j] * (double)t[j] and e_d = sum
 *     (double)y[n_k + d + j]^2; D_d = e_d - 2.0 * c_d.  p_k = n_k + d* with the smallest D_d, ties to the smallest |d|, then to the
 *     negative d.  Every product is exact in double: contraction changes no bit.
 *   - End pin, k = M - 1.  p_{M-1} = n_{M-1} = a_{i+1} - (H + rem) without a search; its cost is D_0, the D of that one offset.
 *   - Crossfade, 1 <= k <= M - 1.  out[b_i + k H + j] = (float)((double)y[p_k + j] * (double)w[j] + (double)t[j] * (double)w[H-1-j])
 *     with the smoothstep table w of H entries (vx_stretch's).  Frame M - 1 then continues plainly: out[b_i + M H + j] =
 *     y[p_{M-1} + H + j] for j in [0, rem).  The segment therefore ends with y[a_{i+1} - 1] and the next one goes on from a_{i+1}.
 * - Tables.  pos[b] and cost[b] (either may be NULL) hold p_k and the winning D_d of the frames of the row's walked segments, in
 *   segment order, frame order inside a segment; their count is the sum of M over the walked segments.
 * - Exactness.  A sample's bits depend on its row, its anchors and the options only: not on the batch, the launch windows or the
 *   workgroup a segment lands on.  No atomics.  Two calls give the same bits.
 * - Windows.  One launch holds VX_RETIME_WINDOW input samples.  A walked segment is one job and is never cut: it needs its samples
 *   [a_i - D, a_{i+1} + D + H), cut to the row, inside one launch.  Copy segments are cut anywhere.
 * - Refusals.  VX_EINVAL, nothing launched, nothing written, the message names the field: a wrong struct_size; NULL wav / lens /
 *   anchors / n_anchors / o / out / out_lens; batch <= 0; a length negative or above wav_stride; hop outside 16 .. 2048; search
 *   outside 0 .. 1024; n_anchors[b] below 1 or 2 n_anchors[b] above anchor_stride; anchors that do not start at (0, 0), do not
 *   increase or do not end at a_m = L; a walked segment with la or lb below 2H, or la / lb outside 1/4 .. 4; a walked segment longer
 *   than a launch window; out_stride below a row's Lout; pos_stride below a row's frame count when pos or cost is given.
 * - Limits.  The end pin is a forced offset: an anchor in the middle of voiced speech can cost a phase step across one hop, and
 *   `cost` shows it -- put anchors into pauses and between words.  A walked segment is not cut across launches.
 * - State.  As vx_stretch.
 *
 *   wav [batch][wav_stride] fp32; anchors [batch][anchor_stride] int32; out [batch][out_stride] fp32, out_lens [batch] = Lout; pos
 *   [batch][pos_stride] int32, cost [batch][pos_stride] double.  Elements behind out_lens[b] and behind the last record are not
 *   written. */
#define VX_RETIME_WINDOW (1 << 23)
typedef struct vx_retime_opts {
  uint32_t struct_size;   /* = sizeof(vx_retime_opts) */
  int32_t hop;            /* H, 16 .. 2048 samples */
  int32_t search;         /* D, 0 .. 1024 samples on either side of the nominal position */
} vx_retime_opts;
int vx_retime(vx_ctx* ctx, const float* wav, int64_t wav_stride, const int32_t* lens, int32_t batch, const int32_t* anchors,
              int64_t anchor_stride /* in int32 elements */, const int32_t* n_anchors, const vx_retime_opts* o, float* out,
              int64_t out_stride, int32_t* out_lens, int32_t* pos /* may be NULL */, double* cost /* may be NULL */, int64_t pos_stride);

/* Programme loudness after ITU-R BS.1770 (the quantity of EBU R 128 and of every delivery specification in LUFS) of mono fp32 rows on
 * the device, and vx_finish with its level step replaced by a loudness target.  No reference counterpart.  All arithmetic is double
 * unless stated.  Every operation named is separately rounded.  A plain numpy restatement reproduces every quantity bit for bit, given
 * the ten coefficients the library reports.
 *
 * - Samples.  y[i] = isfinite(x[i]) ? x[i] : 0, counted in `nonfinite` (over the measured span).
 * - Rate and steps.  sample_rate is in 8000 .. 192000.  Step S = sample_rate / 10 by integer division (100 ms).  A block is 4 steps.
 *   The block hop is 1 step.  This is the standard's 75 % overlap.  The warm-up is W = 2 S.
 * - Coefficients.  vx_loudness_coeffs(rate, double c[10]) is a pure host function and needs no context.  It fills
 *   c = {b0, b1, b2, a1, a2} of the shelf, then the same five of the high-pass.  Shelf: K = tan(pi * 1681.974450955533 / fs),
 *   Vh = 10^(3.999843853973347 / 20), Vb = Vh^0.4996667741545416, Q = 0.7071752369554196, a0 = 1 + K/Q + K K,
 *   b = {(Vh + Vb K/Q + K K)/a0, 2 (K K - Vh)/a0, (Vh - Vb K/Q + K K)/a0}, a1 = 2 (K K - 1)/a0, a2 = (1 - K/Q + K K)/a0.  High-pass:
 *   K = tan(pi * 38.13547087602444 / fs), Q = 0.5003270373238773, b = {1, -2, 1}, a1 and a2 formed as for the shelf.  At 48 kHz this
 *   is the standard's table.  tan and pow may differ by an ulp between libraries.  Everything downstream is therefore defined on the
 *   coefficients the call reports.
 * - Filter.  Each stage is transposed direct form II, in exactly this order and association.  Shelf: u = b0 x + s1,
 *   s1 = (b1 x - a1 u) + s2, s2 = b2 x - a2 u.  High-pass, on u with t1, t2, giving v: the same three lines.  No step is contracted
 *   to an fma.
 * - Step energies.  z_j covers samples [j S, min((j+1) S, n)) of the measured span.  ONE lane starts both stages from rest
 *   (s1 = s2 = t1 = t2 = 0) at sample j S - W.  Samples before the span count as 0.  It runs to the end of the step.  Over the step's
 *   own samples it accumulates z = z + v v from 0.0 in sample order.  The largest pole radius is sqrt(a2) of the high-pass, between
 *   0.9705 at 8 kHz and 0.99875 at 192 kHz, so W rho^W is 2.5e-18 .. 6.1e-17: starting from rest instead of from the true history is
 *   below one rounding error.  In exchange a step's bits depend on nothing but the W + S samples it reads: not the row, batch, job,
 *   tile or window.
 * - Blocks.  For a span of n >= 4 S samples the blocks are k = 0 .. (n - 4 S) / S, complete blocks only, and
 *   m_k = (((z_k + z_{k+1}) + z_{k+2}) + z_{k+3}) / (4 S).  For 1 <= n < 4 S there is one block over the whole span:
 *   m_0 = (sum of z_j in order) / n.  This departs from the standard: an utterance shorter than 400 ms must still be levelled.
 *   n = 0: no block.
 * - Gates.  They run on the host, in energy, in block order.  Absolute gate: m_k > A, with A = pow(10, (-70 + 0.691) / 10) computed
 *   once (`above_abs` blocks).  Relative gate: among those, m_k > 0.1 * (sum m_k / count) (`gated` blocks).  mean_square is the mean of
 *   m_k over the blocks passing both gates, summed in block order.  loudness = -0.691 + 10 log10(mean_square).  max_momentary is the
 *   same formula on the largest m_k of all blocks.  No block at all gives loudness = max_momentary = -HUGE_VAL.  Blocks of which none
 *   passes the gates give loudness = -HUGE_VAL and mean_square = 0.  In either case the gain is 1.
 * - Gain of vx_finish_loud.  t = pow(10, (target_lufs - loudness) / 20).
 *   g = min(t, pow(10, max_gain_db / 20), pow(10, ceiling_db / 20) / peak, FLT_MAX), rounded once to fp32.  peak is vx_wave_info.peak
 *   over the kept span.  The ceiling term is dropped when peak is 0.  max_gain_db comes from the vx_finish_opts.
 * - Span.  vx_finish_loud measures loudness over the kept span [begin, end), with step 0 starting at begin.  The loudness it reports
 *   is therefore bit-equal to vx_loudness on the slice, and the delivered audio has the target loudness, not the untrimmed row.
 * - vx_finish_loud is vx_finish with the level step replaced: o->level_mode must be VX_LEVEL_NONE.  Trim, keep, fades, format,
 *   refusals, sentinels and out == NULL (measure only) are as in vx_finish.  The order is: frames pass, span, steps pass over the
 *   span, gates and gain, apply.  A call that fits one launch uploads its samples once.
 * - State.  As vx_finish: no weights, no decode state, allowed while a serving session is open; it runs in the resampler's launch
 *   buffers plus a step table; transfers go through the pinned ring.
 * - Windows.  One launch holds VX_LOUDNESS_WINDOW (2^23) samples.  Rows are packed into launches in order.  A longer row is cut at
 *   step multiples, and a later part carries the W samples in front of its first step.  By the rules above no cut changes a bit.
 * - Refusals.  These return VX_EINVAL, launch nothing and write nothing, and the message names the field: NULL wav / lens / info
 *   (vx_finish_loud: o / lo / linfo as well); batch <= 0; a length negative or above wav_stride; sample_rate outside 8000 .. 192000;
 *   vx_finish_loud: everything vx_finish refuses, a wrong struct_size of either struct, level_mode other than VX_LEVEL_NONE,
 *   target_lufs not finite or outside -70 .. 0, ceiling_db not finite or above 0.  vx_loudness_coeffs returns VX_EINVAL for a NULL c
 *   or a rate out of range.
 * Not covered: loudness range, short-term loudness, channel weights of more than one channel.  True peak: vx_limit below. */
#define VX_LOUDNESS_WINDOW (1 << 23)
typedef struct vx_loudness_opts {
  uint32_t struct_size;   /* = sizeof(vx_loudness_opts) */
  int32_t sample_rate;    /* 8000 .. 192000 */
  float target_lufs;      /* finite, -70 .. 0 */
  float ceiling_db;       /* finite, <= 0: dBFS the sample peak may reach after the gain */
} vx_loudness_opts;
typedef struct vx_loudness_info {
  double loudness;        /* LUFS of the gated blocks; -HUGE_VAL when none passes */
  double mean_square;     /* mean K-weighted energy of the gated blocks; 0 when none passes */
  double max_momentary;   /* LUFS of the loudest block; -HUGE_VAL without a block */
  int32_t blocks, above_abs, gated, nonfinite;
} vx_loudness_info;
int vx_loudness_coeffs(int32_t sample_rate, double c[10]);
int vx_loudness(vx_ctx* ctx, const float* wav, int64_t wav_stride, const int32_t* lens, int32_t batch, int32_t sample_rate,
                vx_loudness_info* info);
int vx_finish_loud(vx_ctx* ctx, const float* wav, int64_t wav_stride, const int32_t* lens, int32_t batch, const vx_finish_opts* o,
                   const vx_loudness_opts* lo, void* out /* may be NULL: measure only */, int64_t out_stride, int32_t* out_lens,
                   vx_wave_info* info, vx_loudness_info* linfo);

/* A true-peak look-ahead limiter of mono fp32 rows on the device (vx_limit), and vx_finish_loud with its sample-peak ceiling term
 * replaced by that limiter (vx_finish_limited): the gain is set by the loudness target alone and the limiter holds the ceiling.  No
 * reference counterpart.  A plain numpy restatement reproduces every quantity bit for bit, given the taps and the ceiling the library
 * reports, independent of the batch and of the windows.
 *
 * Inputs: a row x of length L; pre_gain gs (fp32, finite, > 0); ceiling_db (finite, <= 0); lookahead Wn (1 .. 1024 samples), with
 * N = 2 Wn + 1; oversample n in {1, 2, 4, 8}.
 *
 * - Samples.  y[i] = isfinite(x[i]) ? x[i] : 0.  Non-finite samples are counted in `nonfinite`.  y = 0 outside [0, L).
 * - Taps.  These are the resampler's own table for the pair (o, n) = (1, n): width 7 and K = 15, k_p[j] for p < n, j < 15, in fp32.
 *   vx_limit_taps(oversample, float* taps) is a pure host function (taps is [n][15]).  It needs no context and reports the taps.
 *   Everything downstream is defined on the reported taps, as vx_loudness_coeffs does for its coefficients.  n = 1 has no taps.
 * - Detector.  For n > 1: d_p[i] = sum_j (double)k_p[j] * (double)y[i + j - 7].  The sum runs in tap order j = 0 .. 14 from 0.0 in
 *   double.  The product of two fp32 values is exact in double.  Contraction to an fma therefore changes no bit.
 *   P[i] = (float) max(|y[i]|, |d_0[i]|, .., |d_{n-1}[i]|).  A max is exact in any order.  For n = 1: P[i] = |y[i]|.
 * - Demand.  c = (float) pow(10, ceiling_db / 20).  It is computed once on the host and reported in the info.
 *   den = (double)P[i] * (double)gs.  This product is exact.  r = den > (double)c ? (double)c / den : 1.0.  This is one correctly
 *   rounded double division.  q[i] = (int64) floor(r * 16777216.0), an integer in [0, 2^24].  q = 2^24 outside [0, L).
 * - Hold and smooth.  Both are defined for every integer i, and both are integer arithmetic.  m[i] = min_{|k - i| <= Wn} q[k].
 *   s[i] = sum_{|k - i| <= Wn} m[k], which is below 2^36.  Being integers, they are exact in any order, so no decomposition and no
 *   cut can change a bit.
 * - Gain and output.  g[i] = (float)((double)s[i] / (double)(N * 16777216)).  This is one double division and one rounding.
 *   out[i] = (y[i] * gs) * g[i].  These are two separately rounded fp32 multiplies, so nothing can be contracted.
 * - Consequences.  m[k] <= q[i] whenever |k - i| <= Wn.  Hence s[i] <= N q[i], and g[i] <= q[i] / 2^24, which is exact in fp32, and
 *   that is <= r.  So |out[i]| <= c (1 + 2^-22).  Where nothing within 2 Wn exceeds the ceiling, g = 1.0 exactly.  With gs = 1 the
 *   output then has the bits of y.  An isolated over-ceiling sample at k0 with demand q0 gives the trapezoid
 *   s[i] = N 2^24 - max(0, N - |i - k0|) (2^24 - q0).
 * - Info per row.  peak = max_i P[i].  This is the true peak of the input at n-times oversampling, linear, before pre_gain.  It is 0
 *   for an empty row.  min_gain = min_i g[i].  It is 1 for an empty row.  reduced = #{i : g[i] < 1}.  nonfinite.  ceiling = c.
 *   With out == NULL (measure only) peak, nonfinite and ceiling are measured; min_gain is 1 and reduced is 0.
 * - Exactness.  No floating-point atomics, and no atomics at all in the kernel.  Two calls give the same bits.  A row's bits depend
 *   on neither the batch nor the windows.
 * - State.  As vx_finish: no weights; works before vx_finalize_weights and while a serving session is open; touches no decode state,
 *   KV arena or fallback counter; runs in the resampler's launch buffers plus what it allocates at first use, which vx_destroy
 *   frees; transfers go through the pinned ring.
 * - Windows.  One launch holds VX_LIMIT_WINDOW (2^23) samples.  Rows are packed in order.  A longer row is cut anywhere.  A part
 *   carries the 2 Wn + 7 real samples its outputs reach on either side.  Zeros exist only outside the row.
 * - vx_finish_limited is vx_finish_loud with two changes.  The gain: the ceiling term is dropped,
 *   g = min(10^((target - loudness) / 20), 10^(max_gain_db / 20), FLT_MAX), rounded once; it is 1 when nothing passes the gates.  The
 *   limiter runs between the gain and the fades: it limits the kept span [begin, end) as a row of its own, with zeros outside, with
 *   pre_gain = g and ceiling_db = lo->ceiling_db.  The existing apply pass then runs over the limited samples at gain 1, which is
 *   exact: fades and format as before.  The output is therefore bit-equal to vx_finish(vx_limit(x[begin:end], g, ceiling),
 *   VX_LEVEL_NONE, no trim, same fades and format).  level_mode must be VX_LEVEL_NONE.  out == NULL measures only, giving
 *   liminfo.peak of the span.  vx_wave_info.gain reports g.  A call that fits one launch uploads its samples once.
 * - Refusals.  These return VX_EINVAL, launch nothing and write nothing, and the message names the field: NULL wav, lens, o or info;
 *   batch <= 0; a wrong struct_size; a length negative or above wav_stride; out_stride below a length when out is given; pre_gain
 *   not finite or <= 0; ceiling_db not finite or > 0; lookahead outside 1 .. 1024; oversample not one of 1, 2, 4, 8.
 *   vx_finish_limited: every refusal of vx_finish_loud and of vx_limit (lim and liminfo NULL as well).  vx_limit_taps returns
 *   VX_EINVAL for a NULL taps or an oversample that is not one of 1, 2, 4, 8.
 * Not covered: the true peak after the time-varying gain is close to the ceiling but not bounded by it; the loudness after limiting
 * is slightly below the target; loudness range and short-term loudness remain unbuilt. */
#define VX_LIMIT_WINDOW (1 << 23)
typedef struct vx_limit_opts {
  uint32_t struct_size;   /* = sizeof(vx_limit_opts) */
  int32_t lookahead;      /* Wn, 1 .. 1024 samples */
  int32_t oversample;     /* n: 1, 2, 4 or 8 */
} vx_limit_opts;
typedef struct vx_limit_info {
  float peak;             /* max P: the true peak of the input, linear, before pre_gain */
  float min_gain;         /* min g; 1 for an empty row */
  float ceiling;          /* c */
  int32_t reduced;        /* samples with g < 1 */
  int32_t nonfinite;
} vx_limit_info;
int vx_limit_taps(int32_t oversample, float* taps /* [oversample][15]; untouched for oversample 1 */);
int vx_limit(vx_ctx* ctx, const float* wav, int64_t wav_stride, const int32_t* lens, int32_t batch, float pre_gain, float ceiling_db,
             const vx_limit_opts* o, float* out /* NULL: measure only -> peak, nonfinite */, int64_t out_stride, vx_limit_info* info);
int vx_finish_limited(vx_ctx* ctx, const float* wav, int64_t wav_stride, const int32_t* lens, int32_t batch, const vx_finish_opts* o,
                      const vx_loudness_opts* lo, const vx_limit_opts* lim, void* out /* may be NULL: measure only */, int64_t out_stride,
                      int32_t* out_lens, vx_wave_info* info, vx_loudness_info* linfo, vx_limit_info* liminfo);

/* The fundamental frequency: F0 per frame of mono fp32 rows on the device by YIN (de Cheveigne & Kawahara 2002: the difference
 * function, its cumulative-mean normalisation, the absolute threshold, parabolic refinement).  No reference counterpart.  It is the
 * measurement behind the pitch control: a pitch shift by p / q is vx_stretch at speed q / p followed by vx_resample with orig_rate = p,
 * new_rate = q, and vx_f0 is what shows that the result moved by p / q.  Inputs are a row x of length L and the
 * options sample_rate, hop (H), window (W), lag_min, lag_max and threshold.  All arithmetic is double and every named operation is
 * rounded on its own (no contraction), so that a plain numpy restatement reproduces every output word for word:
 *
 * - Samples.  y[i] = isfinite(x[i]) ? x[i] : 0.  Outside [0, L), y = 0.  `nonfinite` counts the non-finite samples of the row.
 * - Frames.  M = ceil(L / H); a row with L = 0 has no frame.  Frame k is centred on k H + H/2: its first sample is
 *   s_k = k H + H/2 - (W + lag_max)/2 in 64-bit integers with integer division (it may be negative), and it reads
 *   y[s_k .. s_k + W + lag_max).
 * - Difference.  For every t in [0, lag_max] ONE LANE computes d(t) = the sum from 0.0, in order j = 0 .. W-1, of e * e with
 *   e = (double)y[s_k + j] - (double)y[s_k + j + t].  The subtraction, the product and the addition are three roundings: an fma of
 *   e * e + acc would change bits.  This equals np.cumsum(e * e)[-1] in float64.
 * - Normalisation.  c(t) = d(1) + .. + d(t), added in lag order (a serial prefix: double addition is not associative).  d'(0) = 1 and
 *   d'(t) = c(t) > 0 ? (d(t) * (double)t) / c(t) : 1.
 * - Pick.  The first u in [lag_min, lag_max] with d'(u) < (double)threshold, then t = u stepped upward while t + 1 <= lag_max and
 *   d'(t + 1) < d'(t): the frame is voiced.  Without such a u, t = the arg-min of d' over [lag_min, lag_max], ties to the smallest lag:
 *   the frame is unvoiced.
 * - Refinement.  With a, b, c = d'(t - 1), d'(t), d'(t + 1): if t + 1 <= lag_max, b <= a, b <= c and den = (a - 2.0 * b) + c > 0, then
 *   off = (0.5 * (a - c)) / den, else off = 0.  f0 = (float)((double)sample_rate / ((double)t + off)).
 * - Outputs per frame.  f0[b][k] = that candidate, always written; lag[b][k] = +t of a voiced and -t of an unvoiced frame;
 *   ap[b][k] = (float)d'(t), the aperiodicity.  An all-zero frame gives lag = -lag_min, ap = 1, f0 = sample_rate / lag_min.
 * - Info.  Plain host code over the voiced frames of the row: f0_median = the lower median of the fp32 values (element (n - 1) / 2 of
 *   the n sorted values), f0_min and f0_max over the same frames; all three 0 without a voiced frame.
 * - Exactness.  No floating-point atomics.  Two calls give the same bits.  A row's bits depend neither on the batch nor on the launch
 *   windows: frames are independent.
 * - State.  As vx_stretch: it needs no weights, works while a serving session is open, touches no decode state, and runs in the
 *   resampler's launch buffers; transfers go through the pinned ring.
 * - Windows.  One launch holds VX_F0_WINDOW (2^23) samples.  Rows are packed into launches in order.  A longer row is cut at frame
 *   boundaries, and every part is staged with all the samples its frames reach.
 * - Refusals.  These return VX_EINVAL, launch nothing and write nothing, and the message names the field: sample_rate outside
 *   8000 .. 192000; hop outside 16 .. 4096; window outside 16 .. 2048; lag_min or lag_max outside 2 <= lag_min < lag_max <= 1024;
 *   threshold not finite or outside (0, 1]; a wrong struct_size; NULL wav / lens / o / f0 / lag / info; batch <= 0; a length negative
 *   or above wav_stride; frame_stride below a row's M.
 *
 *   wav [batch][wav_stride] fp32, lens [batch] samples (0 allowed: the row writes nothing but its info); f0, lag and ap (when given)
 *   [batch][frame_stride]; info [batch].  Elements behind M of a row are not written. */
#define VX_F0_WINDOW (1 << 23)
typedef struct vx_f0_opts {
  uint32_t struct_size;     /* = sizeof(vx_f0_opts) */
  int32_t sample_rate;      /* 8000 .. 192000: only turns lags into Hz */
  int32_t hop;              /* H, 16 .. 4096 */
  int32_t window;           /* W, 16 .. 2048: samples summed per lag */
  int32_t lag_min, lag_max; /* 2 <= lag_min < lag_max <= 1024 */
  float threshold;          /* finite, in (0, 1] */
} vx_f0_opts;
typedef struct vx_f0_info {
  int32_t frames, voiced_frames, nonfinite;
  float f0_median, f0_min, f0_max;
} vx_f0_info;
int vx_f0(vx_ctx* ctx, const float* wav, int64_t wav_stride, const int32_t* lens, int32_t batch, const vx_f0_opts* o, float* f0,
          int32_t* lag, float* ap /* may be NULL */, int64_t frame_stride, vx_f0_info* info);

/* The formant-preserving pitch shift: time-domain PSOLA of mono fp32 rows on the device, from the lags vx_f0 gives.  No reference
 * counterpart.  Pitch marks are walked along the waveform one period apart, and two-period grains around them are laid down again
 * at a new spacing: every grain keeps its shape, and with it the spectral envelope, while the spacing sets the pitch.  Inputs are a
 * row x of length L, the signed lags lag[0 .. Mf) of that row at hop Hf (Mf = ceil(L / Hf); lag > 0 is voiced), the options
 * period_min, period_max, unvoiced_period (U) and the pitch ratio ratio_q16 (Q16), and optionally a per-frame array ratio[b][k]
 * (Q16) that replaces ratio_q16 frame by frame.  All floating-point arithmetic is double and every named operation is rounded on
 * its own, so that a plain numpy restatement reproduces marks, grain table and output word for word:
 *
 * - Samples.  y[i] = isfinite(x[i]) ? x[i] : 0, and 0 outside [0, L).  `nonfinite` counts the non-finite samples of the row.
 * - Period at a position.  For a sample index a, k = min(a / Hf, Mf - 1) by integer division.  The position is VOICED iff
 *   period_min <= lag[k] <= period_max; P = lag[k] where voiced, else U.  A lag outside the bounds is unvoiced, not an error.
 * - Analysis marks, a serial walk per row.  a_0 = 0.  Given a_i with its P and voicing: unvoiced, a_{i+1} = a_i + U.  Voiced:
 *   D = P / 8 by integer division and the template is t[j] = y[a_i + j], j in [0, P).  For every d in [-D, D] ONE LANE computes two
 *   double sums from 0.0 in order j = 0 .. P-1: c_d = sum (double)y[a_i + P + d + j] * (double)t[j] and
 *   e_d = sum (double)y[a_i + P + d + j]^2 (products of two fp32 values are exact in double: contraction-proof, the rule of
 *   vx_stretch).  cost_d = e_d - 2.0 * c_d; d* has the smallest cost, ties go to the smallest |d|, then to the negative d;
 *   a_{i+1} = a_i + P + d*.  N is the number of marks below L; the first mark at or above L is kept as a_N, it closes the last
 *   period.  An all-zero row steps by exactly P.
 * - Synthesis marks, serial integer arithmetic.  Time is an int64 in units of 2^-16 sample: S_0 = 0, s_j = (S_j + 32768) >> 16.
 *   While s_j < L: i(j) is the index in [0, N-1] of the analysis mark nearest to s_j, ties to the lower index; g = a_{i+1} - a_i at
 *   i = i(j); r is the ratio of frame min(a_i / Hf, Mf - 1) if mark i is voiced, else 65536; S_{j+1} = S_j + floor((g << 32) / r).
 *   J is the number of grains.  The duration is kept: the output has L samples; unvoiced stretches are re-laid at their own spacing.
 *   Grains stop at s_j < L: at a ratio below 1 the last grain may end up to half an output period before L, and those samples
 *   are gaps.
 * - Grain j.  Centre s_j, source centre a = a_{i(j)}, right width Wr = a_{i+1} - a_i, left width Wl = a_i - a_{i-1} (for i = 0,
 *   a_1 - a_0).  For rr in [-Wl, Wr): u = ((double)(rr + Wl) + 0.5) / (double)Wl if rr < 0, else
 *   u = ((double)(Wr - rr) - 0.5) / (double)Wr; w = (float)((u * u) * (3.0 - 2.0 * u)), every operation rounded on its own, no fma:
 *   the smoothstep of vx_finish and vx_stretch.  Every weight is positive.
 * - Output.  For every n in [0, L) ONE LANE walks the grains that cover n in order of j: num += (double)y[a + (n - s_j)] * (double)w
 *   (an exact product and one addition), den += (double)w; out[n] = den > 0 ? (float)(num / den) : 0.  `gaps` counts the samples
 *   with den == 0.  With every ratio at 65536 the output equals y bit for bit (a -0.0 comes out as +0.0: num starts from +0.0).
 * - Info.  marks = N, voiced_marks = the voiced ones of a_0 .. a_{N-1}, grains = J, gaps, nonfinite.
 * - Exactness.  No floating-point atomics.  Two calls give the same bits.  A row's bits depend neither on the batch nor on the launch
 *   windows.
 * - State.  As vx_f0 / vx_stretch: it needs no weights, works while a serving session is open, touches no decode state, and runs in
 *   the resampler's launch buffers, whose upper half holds the lags, the marks and the grain table; transfers go through the pinned
 *   ring.
 * - Windows.  One launch holds VX_PSOLA_WINDOW (2^23) samples.  Rows are packed into launches in order.  A row is not cut across
 *   launches: a longer row is refused (349 s at 24 kHz).
 * - Refusals.  These return VX_EINVAL, launch nothing (the mark walk aside, where marks_stride is judged) and write nothing, and the
 *   message names the field: hop outside 16 .. 4096; period_min / period_max outside 16 <= period_min <= period_max <= 1024;
 *   unvoiced_period outside [period_min, period_max]; ratio_q16, or any element of ratio within a row's Mf, outside 43691 .. 131072
 *   (2/3 .. 2: below 2/3 the grains no longer overlap); a wrong struct_size; NULL wav / lens / lag / o / out / info; batch <= 0; a
 *   length negative, above wav_stride or above VX_PSOLA_WINDOW; lag_stride below a row's Mf; out_stride below L; marks_stride below
 *   N + 1 when marks is given (the library knows N after the walk and before anything is written to the caller).
 *
 *   wav [batch][wav_stride] fp32, lens [batch]; lag and ratio (when given) [batch][lag_stride] int32; out [batch][out_stride] fp32,
 *   L samples per row; marks (when given) [batch][marks_stride] int32 = a_0 .. a_N; info [batch].  Elements behind a row's end are
 *   not written. */
#define VX_PSOLA_WINDOW (1 << 23)
typedef struct vx_psola_opts {
  uint32_t struct_size;     /* = sizeof(vx_psola_opts) */
  int32_t hop;              /* Hf, 16 .. 4096: the hop the lags were measured at */
  int32_t period_min, period_max; /* 16 <= period_min <= period_max <= 1024 */
  int32_t unvoiced_period;  /* U, period_min .. period_max */
  int32_t ratio_q16;        /* 43691 .. 131072: the pitch ratio, 65536 = 1 */
} vx_psola_opts;
typedef struct vx_psola_info {
  int32_t marks, voiced_marks, grains, gaps, nonfinite;
} vx_psola_info;
int vx_psola(vx_ctx* ctx, const float* wav, int64_t wav_stride, const int32_t* lens, int32_t batch, const int32_t* lag, int64_t lag_stride,
             const int32_t* ratio /* may be NULL */, const vx_psola_opts* o, float* out, int64_t out_stride,
             int32_t* marks /* may be NULL */, int64_t marks_stride, vx_psola_info* info);

/* Spectral noise suppression of mono fp32 rows on the device: an enrolment clip with hiss or fan noise is cleaned before it is
 * cloned.  No reference counterpart.  A short-time Fourier analysis (frame N = 512, hop H = 128, B = 257 bins, square-root Hann
 * window on both sides), a noise profile taken from the quietest frames of the row (or given by the caller), a floored spectral
 * subtraction gain on a five-frame power average, and overlap-add.  All arithmetic is IEEE double and every named operation is
 * rounded on its own (no fma), so that a plain numpy restatement reproduces every word:
 *
 * - Tables, built once on the host in double.  Window w[n] = sqrt(0.5 - 0.5 cos(2 pi n / N)), n = 0 .. 511.  Twiddles
 *   c[k] = cos(2 pi k / N), s[k] = -sin(2 pi k / N), k = 0 .. 255.  vx_denoise_tables(double t[1024]) is a pure host function, needs
 *   no context and reports the words the library uses: w [512], c [256], s [256].  Everything downstream is defined on these words.
 * - Samples.  y[i] = isfinite(x[i]) ? x[i] : 0, and 0 outside [0, L).  `nonfinite` counts the non-finite samples of the row.
 * - Frames.  A row of L samples has T = ceil(L / H) + 3 frames.  Frame t covers samples [(t - 3) H, (t - 3) H + N); every sample
 *   lies in exactly four frames.  A frame is FULL if it lies wholly inside the row: t = 3 .. floor(L / H) - 1, F of them.
 * - FFT.  Radix-2 decimation in time over 512 complex doubles, in place.  The input (double)y[(t - 3) H + n] * w[n], imaginary part
 *   +0.0, is loaded in bit-reversed order.  Stages m = 2, 4 .. 512 with h = m / 2; butterfly j = 0 .. 255 has g = j / h, p = j % h,
 *   i0 = g m + p, i1 = i0 + h, q = p (N / m), and computes tr = c[q] re[i1] - s[q] im[i1], ti = c[q] im[i1] + s[q] re[i1],
 *   (re, im)[i0] = a + t, (re, im)[i1] = a - t, a the old value at i0: two products and one sum per component, each rounded.  The
 *   inverse is the same network with s negated, then the real part times 1 / N.
 * - Power and energy.  P[t][k] = re re + im im for k = 0 .. 256; E[t] is ONE LANE's sum of P[t][0 .. 256] from 0.0 in bin order.
 * - Noise profile Nz [257].  noise_psd given: Nz = noise_psd, and K = 0 is reported.  Otherwise
 *   K = min(max(kmin, floor((double)frac * (double)F)), F); the host chooses the K full frames smallest in the total order
 *   (E[t], t); Nz[k] = (sum of P[t][k] over the chosen frames from 0.0 in ascending t) / (double)K.  With K = 0 (no full frame, or
 *   kmin = 0 under a small frac) the profile is all zero.
 * - Gain.  S[t][k] = ((((P[a][k] + P[b][k]) + P[t][k]) + P[d][k]) + P[e][k]) / 5.0 with a, b, d, e = t - 2, t - 1, t + 1, t + 2 clamped
 *   to [0, T - 1].  g = S > 0 ? 1.0 - ((double)alpha * Nz[k]) / S : (double)floor; then g = g > floor ? g : floor.  Bin k > 256 takes
 *   g[N - k]; both components of the spectrum are multiplied by g.
 * - Synthesis.  y_t[n] = (re'[n] * (1.0 / N)) * w[n], re' the inverse network's real part.  For output sample i, acc = 0.0 and its
 *   four frames are added in ascending t; out[i] = (float)(0.5 * acc).  With alpha = 0 the output is the input within one fp32 ulp.
 * - Exactness.  No atomics.  Two calls give the same bits.  A row's bits depend neither on the batch nor on the launch windows.
 *   Double division on the device is correctly rounded (vx_dev_denoise_div probes it); sqrt runs on the host alone.
 * - State.  As vx_psola: it needs no weights, works while a serving session is open and touches no decode state.  Samples go
 *   through the resampler's launch buffers and the pinned ring; the power table of one window (about 68 MB) is the stage's own
 *   allocation, made by the first call and freed by vx_destroy.
 * - Windows.  One launch holds VX_DENOISE_WINDOW (2^22) samples and at most 256 rows.  Rows are packed into launches in order.  A row
 *   is not cut across launches: a longer row is refused (174 s at 24 kHz).
 * - Refusals.  These return VX_EINVAL, launch nothing and write nothing, and the message names the field: a wrong struct_size;
 *   alpha not finite or below 0; floor outside (0, 1]; frac outside [0, 1]; kmin below 0; NULL wav / lens / o / out / info;
 *   batch <= 0; a length negative, above wav_stride, above out_stride or above VX_DENOISE_WINDOW; a noise_psd word that is not finite
 *   or below 0.
 *
 *   wav [batch][wav_stride] fp32, lens [batch]; noise_psd (when given) [257] doubles, one profile for every row; out
 *   [batch][out_stride] fp32, L samples per row; psd_out (when given) [batch][257] doubles, the profile every row was cleaned with;
 *   info [batch].  Elements behind a row's end are not written. */
#define VX_DENOISE_WINDOW (1 << 22)
#define VX_DENOISE_N 512
#define VX_DENOISE_HOP 128
#define VX_DENOISE_BINS 257
typedef struct vx_denoise_opts {
  uint32_t struct_size;     /* = sizeof(vx_denoise_opts) */
  float alpha;              /* over-subtraction factor, finite and >= 0 (0: the identity) */
  float floor;              /* smallest gain, in (0, 1] */
  float frac;               /* share of the full frames taken as noise, in [0, 1] */
  int32_t kmin;             /* ... and at least this many of them, >= 0 */
} vx_denoise_opts;
typedef struct vx_denoise_info {
  int32_t frames, full_frames, k, nonfinite;
} vx_denoise_info;
int vx_denoise_tables(double t[1024]);
int vx_denoise(vx_ctx* ctx, const float* wav, int64_t wav_stride, const int32_t* lens, int32_t batch, const vx_denoise_opts* o,
               const double* noise_psd /* may be NULL */, float* out, int64_t out_stride, double* psd_out /* may be NULL */,
               vx_denoise_info* info);

/* A biquad equaliser of mono fp32 rows on the device: the one stage that changes the spectrum on purpose -- a high-pass in front of an
 * enrolment clip's noise estimate, a telephone band in front of the 8 kHz resample, a presence lift.  No reference counterpart.
 *
 * - Sections.  A filter is 1 .. VX_EQ_MAX_SECTIONS (8) second-order sections in series, each five doubles b0 b1 b2 a1 a2 with a0
 *   normalised to 1: sections [nsections][5].  vx_eq_design(kind, sample_rate, f0, q, gain_db, c) is a pure host function that writes
 *   the audio-EQ-cookbook section of a kind (VX_EQ_HIGHPASS .. VX_EQ_HIGHSHELF; the band-pass has a 0 dB peak; gain_db is read by the
 *   peak and the two shelves), divided by a0, in double, with w0 = 2 pi f0 / sample_rate, alpha = sin w0 / (2 q), A = 10^(gain_db / 40),
 *   1 - cos w0 = 2 sin^2(w0 / 2) and 1 + cos w0 = 2 cos^2(w0 / 2).  Any stable section of the caller's own is as good.
 * - Per-sample arithmetic.  Section after section, each in transposed direct form II, all in IEEE double with contraction off and
 *   every operation rounded on its own (the recursion of vx_loudness):
 *       u  = b0 * x + s1
 *       s1 = (b1 * x - a1 * u) + s2
 *       s2 = b2 * x - a2 * u          x of the next section = u
 *   The input is widened from fp32; a non-finite input sample is 0 and is counted (nonfinite).  The output is ONE rounding of the last
 *   u to fp32; a result that is not finite after that rounding is written as 0 and counted (nonfinite_out), so a NaN or an Inf never
 *   reaches an output.  (The identity section 1 0 0 0 0 returns the input bits; a -0 comes back as +0.)
 * - Bounded memory.  Output sample n of a row belongs to step j = n / S, S = VX_EQ_STEP.  Its value is the recursion above started
 *   from rest (every s1, s2 = +0) at sample j S - W and run to n; samples before the row are 0.  An output is therefore a function of
 *   at most W + S input samples and the coefficients: its bits do not depend on the row, the batch, the job, the tile, the window or
 *   the launch.  No atomics, no inline assembly.
 * - W is a function of the filter alone, computed on the host in double: a unit impulse runs through the cascade with the recursion
 *   above for 2 VX_EQ_WARM_MAX samples, h[k]; T(k) = |h[k]| + T(k + 1), summed from the far end with one addition per sample; W is the
 *   smallest multiple of 32 with T(W) <= 2^-24.  vx_eq_plan(sections, n, &warm, &step) is a pure host function that reports W and S.
 *   Starting from rest at p is filtering the row with everything before p zeroed, so the distance to the unbounded recursion at any
 *   sample is at most peak(x) T(W) <= 2^-24 peak(x): below half an fp32 ulp of a full-scale output.
 * - The limit.  A filter whose T does not fall to 2^-24 within VX_EQ_WARM_MAX samples is refused: narrow hum notches (50 Hz, Q 100 at
 *   24 kHz) need a carried state, which this stage does not have.
 * - info [batch]: warm = W; nonfinite, nonfinite_out as above; peak = the largest |out| of the row (a maximum: order-free, exact).
 * - State.  As vx_denoise: it needs no weights, works while a serving session is open and touches no decode state.  Samples go
 *   through the resampler's launch buffers and the pinned ring.
 * - Windows.  One launch holds VX_EQ_WINDOW (2^23) staged samples, warm-ups included.  Rows are packed into launches in order.  A
 *   longer row is cut at step multiples, and a later part carries the W samples in front of its first step.  By the rules above no
 *   cut changes a bit.
 * - Refusals.  These return VX_EINVAL, launch nothing and write nothing, and the message names the section or the field: NULL wav /
 *   lens / sections / out / info (vx_eq_design: c; vx_eq_plan: sections, warm or step); batch <= 0; a length negative, above wav_stride
 *   or above out_stride; nsections outside 1 .. 8; a coefficient that is not finite; an unstable section (|a2| >= 1 or
 *   |a1| >= 1 + a2); no W up to VX_EQ_WARM_MAX.  vx_eq_design: kind out of range, sample_rate outside 8000 .. 192000, f0 outside
 *   (0, sample_rate / 2), q not above 0, |gain_db| above 24.  The two host functions have no context: vx_eq_last_error() returns the
 *   message of the last one of them that refused on the calling thread ("" before the first).
 *
 *   wav [batch][wav_stride] fp32, lens [batch] (a row of length 0 is legal and writes nothing); out [batch][out_stride] fp32, L samples
 *   per row.  Elements behind a row's end are not written. */
#define VX_EQ_MAX_SECTIONS 8
#define VX_EQ_WARM_MAX 65536
#ifndef VX_EQ_STEP        /* a constant of the contract; tools/eq_bench.py builds the library at others to measure them */
#define VX_EQ_STEP 128
#endif
#define VX_EQ_WINDOW (1 << 23)
#define VX_EQ_HIGHPASS 0
#define VX_EQ_LOWPASS 1
#define VX_EQ_BANDPASS 2
#define VX_EQ_NOTCH 3
#define VX_EQ_PEAK 4
#define VX_EQ_LOWSHELF 5
#define VX_EQ_HIGHSHELF 6
typedef struct vx_eq_info {
  int32_t warm, nonfinite, nonfinite_out;
  float peak;
} vx_eq_info;
int vx_eq_design(int32_t kind, int32_t sample_rate, double f0, double q, double gain_db, double c[5]);
int vx_eq_plan(const double* sections, int32_t nsections, int32_t* warm, int32_t* step);
const char* vx_eq_last_error(void);
int vx_eq(vx_ctx* ctx, const float* wav, int64_t wav_stride, const int32_t* lens, int32_t batch, const double* sections,
          int32_t nsections, float* out, int64_t out_stride, vx_eq_info* info);

/* The equaliser with a carried state: the same cascade as vx_eq without its bounded memory, for the filters vx_eq refuses or pays a
 * long warm-up for (mains-hum notches, a 5 Hz high-pass), and with a state input and output, which gives a caller chunked filtering
 * and a start from something other than rest.  No reference counterpart.
 *
 * - Sections, per-sample arithmetic, the sanitising of the input, the single rounding of the output, nonfinite, nonfinite_out and
 *   peak are exactly vx_eq's (above).
 * - State and step.  The state of a cascade of ns sections is z = (s1[0], s2[0], .., s1[ns - 1], s2[ns - 1]), D = 2 ns doubles.  A row
 *   is walked in steps of Sc = VX_EQ_CARRY_STEP samples.
 * - M [D][D], row-major: column k is the state the cascade reaches from the unit state e_k (every other component +0) over Sc zero
 *   inputs, run by the recursion above.  vx_eq_carry_plan(sections, nsections, m, &step) is a pure host function that reports M and
 *   Sc; it refuses what vx_eq's section checks refuse and an M with an entry that is not finite.
 * - A row of n samples has J = ceil(n / Sc) steps; the last one is padded with zeros.  Three passes:
 *     ends   f_j = the state after the Sc samples of step j, started from rest.
 *     chain  z_0 = state_in of the row (rest when state_in is NULL), then for every component i
 *                acc = M[i][0] * z_j[0];   acc = acc + M[i][k] * z_j[k]  for k = 1 .. D - 1 in this order;   z_{j+1}[i] = f_j[i] + acc
 *            in double, every operation rounded on its own (no fma).  Structural zeros of M are multiplied and added like any other
 *            entry: the rule has no cases.
 *     rows   step j runs the cascade from z_j over its own samples; each value of the last section is rounded once to fp32.
 *   The cascade is linear in (state, input), so this is mathematically the unbounded recursion from state_in; the distance to it is
 *   rounding in double alone.  There is no W and no limit on a filter's memory.
 * - Consequence.  The bits of a row are a function of the row, the coefficients and its state_in.  They do not depend on the batch,
 *   the job, the tile, the window or the launch.  No atomics, no inline assembly.
 * - state_in [batch][D] (may be NULL: every row from rest); state_out [batch][D] (may be NULL): the state the rows pass holds behind
 *   the row's last sample; for a row of length 0 it is the row's state_in.  A row filtered in two calls, state_out of the first as
 *   state_in of the second, equals the one call within rounding in double (far below half an fp32 ulp of the peak), but not bit for
 *   bit: at a cut the second call starts from the state the rows pass ran to, the one call from f + M z, and the two differ in
 *   rounding.  Cut at multiples of Sc if the second call's steps are to be the one call's.
 * - info [batch]: a vx_eq_info with warm = 0.
 * - Windows.  As vx_eq, on the same field (vx_dev_eq_window): rows are packed into launches of VX_EQ_WINDOW staged samples in order;
 *   a longer row is cut at step multiples and the chain's z is carried into the next launch on the device.  No cut changes a bit.
 *   Every window runs three launches (ends, chain, rows) on the context's stream; the step tables lie in the launch buffers.
 * - Refusals.  VX_EINVAL, nothing launched, nothing written, the message names the section or the field: NULL wav / lens / sections /
 *   out / info (vx_eq_carry_plan: sections, m or step); batch <= 0; a length negative, above
 *   wav_stride or above out_stride; nsections outside 1 .. 8; a coefficient that is not finite; an unstable section; a state_in
 *   entry that is not finite.  vx_eq_carry_plan has no context: its message is vx_eq_last_error()'s, and it is vx_eq_plan's own text
 *   for the same sections -- it starts "vx_eq_plan:", and a NULL m or step reads "sections, warm or step is NULL". */
#ifndef VX_EQ_CARRY_STEP  /* a constant of the contract; tools/eq_carry_bench.py builds the library at others to measure them */
#define VX_EQ_CARRY_STEP 512
#endif
int vx_eq_carry_plan(const double* sections, int32_t nsections, double* m /* [2 ns][2 ns] */, int32_t* step);
int vx_eq_carry(vx_ctx* ctx, const float* wav, int64_t wav_stride, const int32_t* lens, int32_t batch, const double* sections,
                int32_t nsections, const double* state_in /* [batch][2 ns] or NULL */, float* out, int64_t out_stride,
                double* state_out /* [batch][2 ns] or NULL */, vx_eq_info* info);

/* ---- step-level entries (kernel-level parity tests; same kernels as vx_infer) ---------------------------- */
/* first ar_decoder.infer call (models/vallex.py:528-562): embeds, runs the prefix-LM prefill, fills the KV arena,
 * leaves the logits of the last row available.  batch <= 32. */
int vx_ar_prefill(vx_ctx* ctx, const vx_batch* b);
/* logits of the newest position, [batch][1025] (ar_predict_layer, models/vallex.py:568) */
int vx_ar_logits(vx_ctx* ctx, float* out);
/* teacher-forced decode step: append tokens[b] (as if sampled) and run one cached step (models/vallex.py:552-562) */
int vx_ar_step(vx_ctx* ctx, const int32_t* tokens);
/* NAR stages only (models/vallex.py:600-686): codes0 [batch][codes0_stride] first-codebook ids, lens [batch] */
int vx_nar(vx_ctx* ctx, const vx_batch* b, const int32_t* codes0, int32_t codes0_stride, const int32_t* lens,
           int64_t* out_codes, int32_t out_stride);
/* Teacher-forced scoring: the log-probability the model gives codes that already exist -- the argument of F.cross_entropy in
 * VALLE.forward (the AR stack on the first codebook, the NAR stages on codebooks 2 .. 8) and the quantity best_of selects on,
 * sum(logp) / len^penalty (models/vallex.py:572, :583-594).  One full-sequence pass per part instead of one cached step per frame.
 *   codes [batch][codes_stride][8] int64: vx_infer's output layout, a result can be passed straight back; lens [batch],
 *   0 <= T_b <= max_new; batch <= max_batch (groups of min(max_batch, 32) rows).  logp, rank [batch][out_stride][8]; eos_logp,
 *   eos_rank [batch].
 *   - Column 0 (VX_SCORE_AR): log-softmax over the 1025 AR logits of the row that predicts frame t, given the text, the prompt's first
 *     codebook and codes[b][:t][0]; no temperature, no filter (the sampler's logp at top_k <= 0, temperature 1).  eos_logp[b],
 *     eos_rank[b]: the same for id 1024 at the row behind the last frame, so sum_t logp[b][t][0] + eos_logp[b] is sum(logp) of
 *     models/vallex.py:572 for that beam.  T_b = 0 is allowed: only the EOS pair is written.
 *   - Columns q = 1 .. 7 (VX_SCORE_NAR): log-softmax over the 1024 logits of NAR stage q - 1 at frame t, given the text, the whole
 *     prompt and codes[b][:][0 .. q-1].  The stages run the kernels of vx_nar on the same shapes: scoring what vx_infer generated
 *     scores bit-identical logits.
 *   - rank = number of logits STRICTLY greater than the target's (0: the target is an arg-max, ties included).
 *   - Columns of a part that was not asked for and frames behind T_b are not written; an output pointer only that part needs may be NULL.
 * Nothing is written to the KV arena and no decode state is touched.  Both passes sit behind the f16x2 range guard (a raised flag
 * re-runs the pass in fp32 and counts in vx_last_fallbacks: the AR pass as a prefill phase, the NAR pass as a NAR phase).  The first
 * call allocates its device buffers (vx_destroy frees them).  vx_last_stats then reports 0 AR steps, the scored frames and the
 * AR-pass / NAR-pass milliseconds.
 * VX_EINVAL, nothing launched, the message naming the field: everything vx_infer refuses in the batch; parts outside 1 .. 3; a length
 * outside 0 .. max_new; codes_stride or out_stride below a length; a code outside 0 .. 1023 in a part that reads it (AR: codebook 0;
 * NAR: all eight); while a serving session is open.  VX_ESTATE before vx_finalize_weights. */
#define VX_SCORE_AR 1
#define VX_SCORE_NAR 2
int vx_score(vx_ctx* ctx, const vx_batch* b, const int64_t* codes, int32_t codes_stride, const int32_t* lens, int32_t parts,
             float* logp, int32_t* rank, int32_t out_stride, float* eos_logp, int32_t* eos_rank);
/* Text alignment: where in the text a frame came from.  attn[b][t][s], t < lens[b], s < text_lens[b], is the weighted sum over the
 * layers l and heads h of the probability that the AR row predicting frame t (sequence-local row S + Tp + t of
 * text ++ BOS ++ prompt ++ frames, models/vallex.py:535-549) puts on text position s -- the prompt's text included: the caller
 * knows `enroll`.  One teacher-forced full-sequence AR pass over the given codes (vx_score's), with one more launch per weighted
 * layer; exact fp32 softmax of that layer's q and k, whatever arithmetic the pass runs in.
 *   codes [batch][codes_stride][8] int64, vx_infer's output layout; only codebook 0 of codes and of the prompt is read.  lens [batch],
 *   0 <= T_b <= max_new (T_b = 0: the row writes nothing); batch <= max_batch (groups of min(max_batch, 32) rows).
 *   head_weights [num_layers][16], finite, >= 0, not all zero -- or NULL: 1 / (16 num_layers) each, and every row of attn then sums
 *   to the text's share of the attention, at most 1.  Which heads of a trained checkpoint follow the speech is the caller's
 *   calibration.  Nothing behind the last weighted layer's in_proj runs.
 *   attn [batch][out_stride][text_out_stride]: elements outside t < lens[b], s < text_lens[b] are not written.
 * Nothing is written to the KV arena and no decode state is touched.  The pass sits behind the f16x2 range guard (a raised flag
 * re-runs it in fp32 from a zeroed sum and counts in vx_last_fallbacks as a prefill phase).  The first call allocates its device
 * buffer, min(max_batch, 32) * max_new rows of max_text floats (vx_destroy frees it).  vx_last_stats then reports 0 AR steps, the
 * aligned frames, the pass's milliseconds as AR ms and 0 NAR ms.
 * VX_EINVAL, nothing launched, the message naming the field: everything vx_infer refuses in the batch; a length outside
 * 0 .. max_new; codes_stride or out_stride below a length; text_out_stride below a text length; a codebook-0 id outside 0 .. 1023;
 * head_weights non-finite, negative or all zero; while a serving session is open.  VX_ESTATE before vx_finalize_weights. */
int vx_align(vx_ctx* ctx, const vx_batch* b, const int64_t* codes, int32_t codes_stride, const int32_t* lens,
             const float* head_weights, float* attn, int32_t out_stride, int32_t text_out_stride);
/* copy a named debug buffer (needs cfg.debug_taps) -- or, when no tap has that name, a tensor exactly as vx_load_tensor stored it
 * (read-back check of an upload) -- to the host; returns the number of floats copied or < 0 */
int64_t vx_read_tap(vx_ctx* ctx, const char* name, float* dst, int64_t max_floats);

/* counters of the last vx_infer: AR steps run, generated frames, AR / NAR wall milliseconds (stream-synchronised) */
int vx_last_stats(vx_ctx* ctx, int64_t* ar_steps, int64_t* frames, double* ar_ms, double* nar_ms);

/* number of rows of the last vx_infer whose generation was cut by the ARENA (cfg.max_new frames) before the reference's own stop
 * rule -- EOS, or more than 16 * text_len frames (models/vallex.py:575-578) -- would have ended it.  0 = every row is what the
 * reference would have produced; > 0: create the context with a larger max_new. */
int vx_last_truncated(vx_ctx* ctx, int32_t* rows);

/* The f16x2 kernels need |activation|, |q|/8, |k|, |v| < 2047 (fp16 range at their fixed scale); the reference's fp32 path has
 * no such bound (modules/transformer.py:371-373, modules/activation.py:144-166).  A phase (AR prefill of a micro-batch / the 7
 * NAR stages of a micro-batch) whose operands leave that range is detected on the device and RE-RUN on the exact-fp32 kernels
 * automatically; the call succeeds with the fp32 result.  This reports how many phases of the last vx_infer / vx_ar_prefill /
 * vx_nar took that path, and the count since vx_create (any pointer may be NULL). */
int vx_last_fallbacks(vx_ctx* ctx, int32_t* prefill_phases, int32_t* nar_phases, int64_t* lifetime_phases);

/* Sticky fallback (ABI 5).  After two CONSECUTIVE raises of a phase kind (a clean f16x2 pass of the kind resets the count) the
 * context runs that kind on the exact-fp32 kernels directly instead of paying an f16x2 pass and an fp32 pass per call; every 32nd
 * phase of the kind is tried on f16x2 again and a clean pass leaves sticky mode.  vx_fallback_state reports whether the AR prefill /
 * the NAR stages are in sticky mode right now and how many times the context entered it since vx_create (any pointer may be NULL);
 * vx_fallback_reset leaves it at once (e.g. after a batch of known outlier inputs).  No reference counterpart: the reference is
 * fp32 throughout. */
int vx_fallback_state(vx_ctx* ctx, int32_t* sticky_prefill, int32_t* sticky_nar, int64_t* times_engaged);
int vx_fallback_reset(vx_ctx* ctx);

/* the arithmetic the context actually runs (after vx_finalize_weights): gemm_mode / attn_mode = 0 f16x2, 1 bf16x3, 2 fp32 */
int vx_arith_mode(vx_ctx* ctx, int32_t* gemm_mode, int32_t* attn_mode);

#ifdef __cplusplus
}
#endif
#endif /* VALLEX_HIP_H */
