// Internal declarations shared by the engine's translation units (engine.hip: context, prefill / decode step / NAR and their seams;
// schedule.hip: the three host schedulers -- vx_infer, vx_infer_continuous, the serving session -- and their ABI entries;
// weights.hip: ingest of the reference state-dict; vocoders.hip: Vocos head, EnCodec decoder / encoder drivers;
// beams.hip: the best_of fan-out; admit.hip / serve.hip: admission kernels of the continuous schedule / the serving session;
// serve_sample.hip: the serving session's per-row sampler;
// bench_harness.hip: the measurement entries of include/vallex_hip_dev.h; score.hip: teacher-forced scoring, vx_score;
// dev_wave.hip: vx_dev_wave_op, the correctness entry of the Vocos / EnCodec glue kernels; dev_seam.hip: vx_dev_seam_op, the one of the
// embedding / argmax / KV / admission kernels; resample.hip: vx_resample, kernel and driver; finish.hip: vx_finish, the output stage).
// Not part of the public C ABI.
#pragma once

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <functional>
#include <map>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/vallex_hip.h"
#include "vx_common.h"

using namespace vx;

namespace vxe {

struct Tensor {
  float* d = nullptr;
  std::vector<int64_t> shape;
  size_t n = 0;
};

struct LayerW {
  const float *in_w, *in_b, *out_w, *out_b, *l1_w, *l1_b, *l2_w, *l2_b, *n1_w, *n1_b, *n2_w, *n2_b;
  float *in_wp = nullptr, *out_wp = nullptr, *l1_wp = nullptr, *l2_wp = nullptr;   // packed decode images (AR only)
  float* out_wh = nullptr;                                                         // head-major W_o (fused out_proj in dec_attn)
  unsigned short *in_w3 = nullptr, *out_w3 = nullptr, *l1_w3 = nullptr, *l2_w3 = nullptr;   // 3 bf16 planes [3][N][K]
};

// Host <-> device transfers.  Every byte that crosses the boundary goes through a context-owned PINNED ring (hipHostMalloc, one per
// context = per GPU = per rank): a host source is copied into the ring and DMA'd from there, a host destination is filled from the
// ring behind the next stream sync.  No call of the library hands a caller's (or its own) pageable pages to the runtime, so nothing
// depends on the driver pinning user memory on the fly (the userptr path -- the one a box-level fault of round 5 died in, inside the
// first weight upload, replacing load_state_dict + .to(device) of utils/generation.py:79-83).  Transfers larger than a chunk are cut
// into chunks, so the CPU copy of chunk i + 1 overlaps the DMA of chunk i; the ring wraps by synchronising the stream.
struct PinRing {
  char* base = nullptr;
  size_t cap = 0, head = 0;
  struct Pend { void* dst; const char* src; size_t n; };
  std::vector<Pend> pend;          // device -> host copies in flight: ring slot -> caller memory at the next xfer_sync
};
constexpr size_t XFER_CHUNK = 8u << 20;

struct ProfClass {
  std::vector<hipEvent_t> ev;   // pairs
  size_t used = 0;
  double bytes = 0;
};

constexpr int SK_QKV = 4, SK_OUT = 4, SK_L2 = 8, SK_PRED = 4;
constexpr int PRED_NPAD = 1056;
constexpr int FB_STICKY_AFTER = 2;
constexpr int FB_STICKY_PROBE_EVERY = 32;

}  // namespace vxe
using namespace vxe;

struct vx_ctx {
  vx_config cfg{};
  int dev = 0;
  hipStream_t stream = nullptr;
  PinRing ring;                    // pinned staging of every host transfer (xfer_h2d / xfer_d2h / xfer_sync)
  hipEvent_t ev_t[3] = {nullptr, nullptr, nullptr};   // AR / NAR phase timing of vx_infer (created once, vx_create)
  std::string err;
  const char* launch_fail = nullptr;   // a launcher refused a configuration that is not compiled in (set by LAUNCH, read by the ABI call)
  std::map<std::string, Tensor> w;
  bool finalized = false;
  std::vector<void*> allocs;

  // derived weights
  int NL = 0;
  float* pe = nullptr;
  int pe_rows = 0;
  std::vector<LayerW> ar, nar;
  float* ada = nullptr;            // [7][2NL+1][2048]
  float* pred_wp = nullptr;        // packed ar_predict_layer
  const float** nar_tabs_dev = nullptr;
  bool has_vocos = false;
  float *vc_embed_w = nullptr, *vc_head_w = nullptr, *vc_head_b = nullptr, *vc_dft = nullptr, *vc_win2 = nullptr;

  // geometry
  int mbr = 0;                     // rows per micro-batch (<= 32)
  int Tmax = 0;                    // KV rows per (row, head)
  long Mmax = 0;                   // packed rows of a micro-batch on the full-sequence paths

  // arithmetic of the transformer projections of prefill / NAR: 0 = f16x2 (default; gemm_f16x2.hip), 1 = bf16x3
  // (VX_GEMM_X3=1; gemm_bf16x3*.hip), 2 = exact fp32 MFMA (VX_GEMM_F32=1; gemm_f32.hip).  All three keep every golden's ids.
  int gemm_mode = 0;
  bool attn_x3 = true;                        // 16-bit-plane attention (h2 or x3); VX_ATTN_F32=1 keeps the fp32 MFMA kernel
  bool attn_h2 = true;                        // f16x2 attention (attn_full_h2.hip); VX_ATTN_X3=1: bf16x3 (attn_full_x3.hip)
  int* range_flag = nullptr;       // device flag: an operand of an f16x2 GEMM / attention did not fit fp16 (read at the phase's
                                   // existing host sync; a raised flag re-runs the phase on the exact-fp32 kernels)
  unsigned long long* seed_dev = nullptr;   // seed of the counter-based sampler (device word: not part of the captured graph)
  int st_fb_prefill = 0, st_fb_nar = 0;     // phases of the last call that were re-run in fp32 (vx_last_fallbacks)
  long fb_total = 0;                        // ... since the context was created
  // sticky fallback: a checkpoint whose operands leave the fp16 range on (nearly) every call would pay an f16x2 pass AND an fp32
  // pass each time.  After FB_STICKY_AFTER CONSECUTIVE raises of a phase kind (a clean f16x2 pass of that kind resets the count: two
  // outlier inputs days apart in a long-running server never add up) that kind runs on the exact-fp32 kernels directly (still
  // counted by vx_last_fallbacks); while the count is non-zero the NAR phase polls the flag right behind stage 0 instead of behind
  // stage 6.  Sticky mode is not for ever: every FB_STICKY_PROBE_EVERY-th phase of the kind is tried on f16x2 again and a clean pass
  // leaves it (a burst of outlier inputs costs at most that many fp32 phases).  vx_fallback_state reports it, vx_fallback_reset
  // clears it.
  int fb_prefill_raises = 0, fb_nar_raises = 0;
  bool sticky_prefill_f32 = false, sticky_nar_f32 = false;
  int sticky_prefill_age = 0, sticky_nar_age = 0;     // fp32-direct phases since sticky mode engaged / since the last probe
  long sticky_engaged = 0;                            // how many times either kind ENTERED sticky mode since vx_create
  unsigned short* fa3b = nullptr;  // second plane buffer: linear1 writes linear2's A planes straight from its epilogue (f16x2 mode)
  unsigned short* fa3 = nullptr;   // activation planes [2 or 3][M][K<=4096]
  unsigned short* pred_w3[N_Q - 1] = {};
  // full-sequence arena
  float *fx = nullptr, *fxn = nullptr, *fqkv = nullptr, *fatt = nullptr, *fffn = nullptr, *fyemb = nullptr,
        *flogits = nullptr;
  int* imeta = nullptr;            // device int scratch for row metadata
  long imeta_cap = 0;
  std::vector<int> hmeta;          // host staging for imeta

  // decode arena
  float *kc = nullptr, *vc = nullptr;      // [NL][mbr*16][Tmax][64]
  float *dh = nullptr, *dh2 = nullptr, *xp = nullptr, *xp_att = nullptr, *xp4 = nullptr;
  bool sb_qkv = false;             // ... on the small-batch chain with norm1 + QKV folded into the attention launch
  int sb_qkv_rows = 4, sb_qkv_nsplit = 0;   // sb_qkv up to this many rows (VX_SB_QKV=n, 0 = off), forced split count (VX_SB_QKV_NSPLIT)
  bool sb_chain = false;           // the current micro-batch decodes on the small-batch chain (set by ar_prefill)
  bool sb_fuse = true;             // <= SB_ROWS rows: reduce+LN / combine folded into the consuming GEMM (VX_SB_FUSE=0: the general chain)
  bool qkv_bal = true;             // the decode in_proj GEMM on 512 workgroups (8 K slices of q, 4 of k / v; VX_QKV_BALANCED=0: 384 x 4 slices)
  bool l2_kmap = true;             // linear2 of the 5 .. 32-row chain: one K slice per XCD (decode.hip skinny_gemm_kernel; VX_L2_KMAP=0: column tile fastest)
  bool l1_interleave = true;       // linear1 requests w[u], x0[u], x1[u] per k-block (VX_L1_INTERLEAVE=0: all of x, then the weights)
  float* qk_new = nullptr;         // [MB][16][2][64]: q / 8 and k_new of the step's new token (dec_attn_qkv_kernel -> out_proj prologue)
  float *p_qkv = nullptr, *p_o = nullptr, *p_oh = nullptr, *p_logits = nullptr, *part_o = nullptr, *part_ml = nullptr;
  std::map<const unsigned short*, int> w_shift;   // f16x2: power-of-two scale exponent of every weight's planes
  bool nar_trim = true;            // last NAR layer computes only the generated rows (VX_NAR_TRIM=1; engine.hip struct Trim)
  bool balance_rows = true;        // dec_attn launch order pairs long with short contexts per CU (VX_BALANCE_ROWS=0: batch order)
  bool fuse_out = true;            // out_proj folded into dec_attn when nsplit == 1 (VX_FUSE_OUT=0: separate skinny GEMM)
  int fuse_split = 1;              // ... and, 8 .. 16 rows, with 2 .. 4 context splits: slabs per (head, split) weighed by the consumer (VX_FUSE_SPLIT=0: dec_attn | combine | out_proj; any non-zero value also fuses, above 4 rows, whenever VX_ATT_NSPLIT forces 2 .. 4 splits -- the 8 .. 16-row rule itself asks for 1)
  bool split_fused = false;        // decided per micro-batch by the prefill
  float *d_logits = nullptr, *d_uniforms = nullptr, *sum_logp = nullptr;
  long uniforms_cap = 0;
  int *cur_tok = nullptr, *cur_pos = nullptr, *ctx_len = nullptr, *n_gen = nullptr, *active = nullptr,
      *text_len = nullptr, *gen = nullptr, *force_tok = nullptr, *n_active = nullptr, *slot_meta = nullptr, *slot_of = nullptr;
  int gen_stride = 0;
  int cur_batch = 0;
  int nsplit = 1;
  int att_nsplit_force = 0;        // VX_ATT_NSPLIT=n: context splits of dec_attn on the general chain (0 = 512 / (rows x 16) workgroups rule)
  std::vector<int> h_L;            // prefill lengths of the current micro-batch
  vx_serve* serve = nullptr;       // the open serving session (vx_serve_open); it owns the decode state while it is open
  int* row_smp = nullptr;          // [MB][4] per-row sampling record of the session's sampler (first vx_serve_open allocates it)
  int* row_flt = nullptr;          // [MB][4] per-row filter record {top_p bits, penalty bits, window, min_frames}, allocated with row_smp

  // teacher-forced scoring (score.hip): allocated by the first vx_score, a context that never scores holds none of it
  float* sc_predw = nullptr;       // ar_predict_layer.weight zero-padded to [1028][1024] (the full-sequence GEMMs need N % 4 == 0)
  float* sc_logits = nullptr;      // AR logits of the scored rows [sum (T_b + 1)][1028] when flogits is too small for them
  float* sc_logp = nullptr;        // [8 mbr (max_new + 1)] log-probabilities of the targets, as the kernel wrote them
  int* sc_rank = nullptr;          // ... and their ranks
  // text alignment (vx_align, score.hip): allocated by the first vx_align
  float* al_out = nullptr;         // [mbr max_new][roundup(max_text, 4)] attention of the aligned frames over the text, summed over layers
  float* al_w = nullptr;           // [NL][16] head weights of the call
  // sample-rate conversion (vx_resample, resample.hip): allocated by the first vx_resample; needs no weights
  float *rs_in = nullptr, *rs_out = nullptr;      // input / output samples of one launch
  int* rs_meta = nullptr;          // job records of one launch
  long rs_window = 0;              // input samples per launch set by vx_dev_resample_window (0: the default, VX_RESAMPLE_WINDOW)
  std::map<std::pair<int, int>, float*> rs_taps;  // (o, n) -> device tap table [K][n]
  // output stage (vx_finish, finish.hip): runs in the resampler's launch buffers (rs_buffers); needs no weights
  float* fn_fade = nullptr;        // [2][2^20] the fade-in / fade-out tables, allocated by the first call with a fade
  int fn_fade_n[2] = {0, 0};       // the lengths the two device tables were last built for
  long fn_window = 0;              // input samples per launch set by vx_dev_finish_window (0: the default, VX_FINISH_WINDOW)
  // time-stretch (vx_stretch, stretch.hip): runs in the resampler's launch buffers (rs_buffers); needs no weights.  The three tables
  // are the time map's too (vx_retime: ws_tables, wave_stage.h)
  float* st_fade = nullptr;        // [2048] the crossfade table of the hop it was last built for (st_fade_n)
  int st_fade_n = 0;
  int* st_pos = nullptr;           // [ST_FRAME_CAP] positions of one launch's frames
  double* st_cost = nullptr;       // [ST_FRAME_CAP] winning costs of one launch's frames
  long st_window = 0;              // input samples per launch set by vx_dev_stretch_window (0: the default, VX_STRETCH_WINDOW)
  // loudness (vx_loudness / vx_finish_loud, loudness.hip): runs in the resampler's launch buffers (rs_buffers); needs no weights
  double* ln_z = nullptr;          // [LN_Z_CAP] step energies of one launch
  int* ln_nonf = nullptr;          // [LN_Z_CAP] non-finite samples of one launch's steps
  long ln_window = 0;              // samples per launch set by vx_dev_loudness_window (0: the default, VX_LOUDNESS_WINDOW)
  // limiter (vx_limit / vx_finish_limited, limit.hip): runs in the resampler's launch buffers (rs_buffers); needs no weights
  double* lm_taps = nullptr;       // [8][15] the detector's taps, widened, of the oversampling they were last built for (lm_taps_n)
  int lm_taps_n = 0;
  float* lm_rec = nullptr;         // [LM_REC_CAP][4] tile records of one launch: {peak, min gain, reduced, non-finite}
  long lm_window = 0;              // samples per launch set by vx_dev_limit_window (0: the default, VX_LIMIT_WINDOW)
  // pitch tracker (vx_f0, f0.hip): runs in the resampler's launch buffers (rs_buffers) alone; needs no weights
  long f0_window = 0;              // samples per launch set by vx_dev_f0_window (0: the default, VX_F0_WINDOW)
  // formant-preserving pitch shift (vx_psola, psola.hip): runs in the resampler's launch buffers (rs_buffers) alone; needs no weights
  long ps_window = 0;              // samples per launch set by vx_dev_psola_window (0: the default, VX_PSOLA_WINDOW)
  // noise suppression (vx_denoise, denoise.hip): samples in the resampler's launch buffers (rs_buffers); needs no weights
  double* dn_buf = nullptr;        // the stage's own tables, allocated by the first call: w, stage twiddles, P, E, profiles, chosen frames
  long dn_window = 0;              // samples per launch set by vx_dev_denoise_window (0: the default, VX_DENOISE_WINDOW)

  // graph
  hipGraphExec_t graph_exec = nullptr, graph_exec_n = nullptr;   // one decode step / GRAPH_STEPS steps per launch
  bool graph_multi = true;         // several steps per graph launch (VX_GRAPH_MULTI=0: one)
  std::string graph_sig;

  // taps
  std::map<std::string, Tensor> taps;

  // profiling / stats
  int prof_on = 0;                 // 0 off, 1 every class (AR step runs eagerly), 2 full-sequence classes only
  ProfClass prof[6];             // 0 dec_attn, 1 skinny GEMMs, 2 projections, 3 full-seq attention, 4 vocoder GEMMs, 5 LSTM recurrences
  int64_t st_steps = 0, st_frames = 0;
  int st_truncated = 0;            // rows of the last vx_infer cut by the arena (max_new) before the reference's stop rule
  double st_ar_ms = 0, st_nar_ms = 0;

  // EnCodec decoder (optional)
  bool has_encodec = false;
  float *ec_codebook = nullptr, *ec_w0 = nullptr, *ec_lstm_b[2] = {nullptr, nullptr}, *ec_whh_p[2] = {nullptr, nullptr};
  float *ec_wT[4] = {}, *ec_bT[4] = {}, *ec_w1[4] = {}, *ec_w3[4] = {};
  float *ec_e0 = nullptr, *ec_x0 = nullptr, *ec_y1 = nullptr, *ec_y2 = nullptr, *ec_xg = nullptr, *ec_col = nullptr,
        *ec_a = nullptr, *ec_sc = nullptr, *ec_out = nullptr, *ec_h = nullptr, *ec_audio = nullptr, *ec_hp = nullptr,
        *ec_c = nullptr, *ec_pg = nullptr;
  long ec_frames_cap = 0;
  // EnCodec SEANet encoder + RVQ encode (prompt enrolment; shares the decoder's arena)
  bool has_encodec_enc = false;
  float *en_w1[4] = {}, *en_w3[4] = {}, *en_wd[4] = {}, *en_w15 = nullptr, *en_lstm_b[2] = {nullptr, nullptr},
        *en_whh_p[2] = {nullptr, nullptr}, *en_e2 = nullptr, *en_scores = nullptr;
  long long* en_codes = nullptr;

  // vocos arena
  float *vfeat = nullptr, *vcol = nullptr, *vx0 = nullptr, *vx1 = nullptr, *vhid = nullptr, *vo = nullptr,
        *vreim = nullptr, *vframes = nullptr, *vaudio = nullptr;
  long v_rows_cap = 0;

  // time map (vx_retime, retime.hip): runs in the resampler's launch buffers (rs_buffers) and the stretch's tables; needs no weights.
  // Behind everything else: the fields in front of it keep the places they had
  long rt_window = 0;              // input samples per launch set by vx_dev_retime_window (0: the default, VX_RETIME_WINDOW)
  // equaliser (vx_eq, eq.hip): runs in the resampler's launch buffers (rs_buffers) alone; needs no weights.  Behind everything else too
  long eq_window = 0;              // staged samples per launch set by vx_dev_eq_window (0: the default, VX_EQ_WINDOW)
};

#define HIPCHK(expr)                                                                                   \
  do {                                                                                                 \
    hipError_t _e = (expr);                                                                            \
    if (_e != hipSuccess) {                                                                            \
      char _buf[512];                                                                                  \
      snprintf(_buf, sizeof _buf, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      c->err = _buf;                                                                                   \
      return VX_EHIP;                                                                                  \
    }                                                                                                  \
  } while (0)

#define FAIL(code, ...)                         \
  do {                                          \
    char _buf[512];                             \
    snprintf(_buf, sizeof _buf, __VA_ARGS__);   \
    c->err = _buf;                              \
    return (code);                              \
  } while (0)

// every struct that crosses the C ABI carries its size: a caller built against another header is refused, not misread
#define CHECK_STRUCT(v, T)                                                                                                          \
  do {                                                                                                                              \
    if ((v).struct_size != sizeof(T))                                                                                               \
      FAIL(VX_EINVAL, #T ".struct_size is %u, this library expects %zu (ABI version %d)", (v).struct_size, sizeof(T), VX_ABI_VERSION); \
  } while (0)

// launchers that compile a split count in return false instead of launching an uninstantiated configuration
#define LAUNCH(call)                                      \
  do {                                                    \
    if (!(call) && !c->launch_fail) c->launch_fail = #call; \
  } while (0)

namespace vxe {

int xfer_h2d(vx_ctx* c, void* dst_dev, const void* src_host, size_t bytes);    // asynchronous on c->stream; src is free on return
int xfer_d2h(vx_ctx* c, void* dst_host, const void* src_dev, size_t bytes);    // dst is valid after the next xfer_sync
int xfer_sync(vx_ctx* c);                                                      // stream sync + delivery of pending d2h + ring reset
#define H2D(dst, src, bytes) do { if (int _e = xfer_h2d(c, (dst), (src), (bytes))) return _e; } while (0)
#define D2H(dst, src, bytes) do { if (int _e = xfer_d2h(c, (dst), (src), (bytes))) return _e; } while (0)
#define SYNC() do { if (int _e = xfer_sync(c)) return _e; } while (0)

// geometry of the padded copy launch_enc_pad_elu writes in front of a causal Conv1d(k = 2r, stride r) on Lc input rows (EncodecConv1d):
// n_out = ceil(Lc / r) output frames; rows = (n_out + 1) r rows of the copy (left pad r + Lc + the right pad that completes the last
// frame); Le = the length the input is zero-extended to before reflecting (Le > Lc only for inputs not longer than the larger pad,
// _pad1d).  One rule for the encoder (vocoders.hip) and the correctness entry (dev_wave.hip).
struct EncPadGeom { long n_out, rows, Le; };
inline EncPadGeom enc_pad_geom(long Lc, int r) {
  const long n_out = (Lc + r - 1) / r;
  const long rows = (n_out + 1) * r, extra = n_out * r - Lc;       // extra: the right pad
  const long max_pad = std::max<long>(r, extra);
  const long Le = Lc <= max_pad ? Lc + (max_pad - Lc + 1) : Lc;    // EncodecConv1d._pad1d: short inputs are zero-extended
  return {n_out, rows, Le};
}

// host side of the packed-x image (decode.hip) for the correctness entries: float4 column c4 of row b at
// ((c4 >> 1) * 64 + b + 32 * (c4 & 1)) * 4, for any K; rows [MB][kk] row-major
inline void dev_pack_image(float* img, const float* rows, int kk) {
  for (int b = 0; b < MB; ++b)
    for (int c4 = 0; c4 < kk / 4; ++c4) memcpy(img + (((size_t)(c4 >> 1) * 64) + b + 32 * (c4 & 1)) * 4, rows + (size_t)b * kk + 4 * c4, 16);
}
inline void dev_unpack_image(float* rows, const float* img, int kk) {
  for (int b = 0; b < MB; ++b)
    for (int c4 = 0; c4 < kk / 4; ++c4) memcpy(rows + (size_t)b * kk + 4 * c4, img + (((size_t)(c4 >> 1) * 64) + b + 32 * (c4 & 1)) * 4, 16);
}

template <typename T>
int dev_alloc(vx_ctx* c, T** p, size_t count, bool zero = true) {
  void* q = nullptr;
  HIPCHK(hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T)));
  c->allocs.push_back(q);
  if (zero) HIPCHK(hipMemsetAsync(q, 0, std::max<size_t>(count, 1) * sizeof(T), c->stream));
  *p = reinterpret_cast<T*>(q);
  return VX_OK;
}

const float* W(vx_ctx* c, const std::string& name);

// f16x2 weight planes (vx_common.h): the shift of a tensor from its max |w| -- max |w| * 2^shift in [16384, 32768), shift clamped to
// 0 .. 24; a zero or non-finite maximum takes 24.  The loader (weights.hip) and vx_dev_gemm (bench_harness.hip) share it.
inline int h2_weight_shift(float absmax) {
  if (!(absmax > 0.f) || !(absmax < __builtin_inff())) return 24;
  int ex;
  (void)frexpf(absmax, &ex);
  const int shift = 15 - ex;
  return shift < 0 ? 0 : shift > 24 ? 24 : shift;
}

// ---- profiling helpers: an event pair around one launch --------------------------------------------------
struct ProfScope {
  vx_ctx* c;
  int which;
  bool on;
  ProfScope(vx_ctx* c_, int w) : c(c_), which(w), on(c_->prof_on == 1 || (c_->prof_on == 2 && w >= 2)) {
    if (!on) return;
    ProfClass& p = c->prof[which];
    if (p.used + 2 > p.ev.size()) {
      for (int i = 0; i < 2; ++i) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) { on = false; return; }
        p.ev.push_back(e);
      }
    }
    (void)hipEventRecord(p.ev[p.used], c->stream);
  }
  ~ProfScope() {
    if (!on) return;
    ProfClass& p = c->prof[which];
    (void)hipEventRecord(p.ev[p.used + 1], c->stream);
    p.used += 2;
  }
};

int upload_meta(vx_ctx* c);

struct MetaBuilder {
  vx_ctx* c;
  explicit MetaBuilder(vx_ctx* c_) : c(c_) { c->hmeta.clear(); }
  // reserve n ints, return offset
  long add(const std::vector<int>& v) {
    long off = (long)c->hmeta.size();
    c->hmeta.insert(c->hmeta.end(), v.begin(), v.end());
    while (c->hmeta.size() % 4) c->hmeta.push_back(0);
    return off;
  }
  const int* dev(long off) const { return c->imeta + off; }
};

int tap_store(vx_ctx* c, const std::string& name, const float* src, size_t n);
// C = resid + colscale * act(A W^T + bias) on the fp32 MFMA (cls: profiling class, 2 = transformer projections, 4 = vocoders)
void gemm(vx_ctx* c, const float* A, int lda, const float* Wt, int ldw, const float* bias, const float* resid, int ldr,
          const float* colscale, float* C, int ldc, long M, int N, int K, int act, const int* gather = nullptr, int cls = 4,
          const int* resid_rows = nullptr);
bool range_guarded(const vx_ctx* c);
int ensure_f32_buffers(vx_ctx* c);
int take_range_flag(vx_ctx* c, bool* raised);
int check_batch(vx_ctx* c, const vx_batch* b, int max_rows);
SampleArgs make_sample_args(vx_ctx* c, const vx_sampling* s, int commit, float* logits_out);
struct ServeSampleArgs;
// rsa != null (serving session): the step ends in the per-row sampler (serve_sample.hip) instead of dec_sample
void ar_step_launches(vx_ctx* c, const SampleArgs* sa, const ServeSampleArgs* rsa = nullptr);
void read_dec_gemm_levers(vx_ctx* c);      // VX_L2_KMAP / VX_L1_INTERLEAVE -> c->l2_kmap / c->l1_interleave (engine.hip; called at finalize)
// the switched launchers of the decode step's GEMMs (decode.hip, round 35): linear2 with the K slice fastest in the block id, linear1
// with the request order of rounds 2 .. 34
}  // namespace vxe
namespace vx {
void launch_skinny_gemm_kmap(const float* Wp, const float* xp, float* partial, int Npad, int K, int splitk, hipStream_t s, bool wt, bool kmap);
void launch_skinny16_relu_pack_xfirst(const float* W16, const float* xp, const float* bias, float* xp_out, int N, int K, hipStream_t s);
#ifdef VX_DEV_PROBES
void dev_read_wave_stamps(unsigned long long* out);      // decode.hip: lane 0 of every wave of linear1 (tools/step_timeline.py --step)
#endif
}  // namespace vx
namespace vxe {
inline void launch_linear1(const vx_ctx* c, const float* W16, const float* xp, const float* bias, float* xp_out, hipStream_t s) {
  if (c->l1_interleave) launch_skinny16_relu_pack(W16, xp, bias, xp_out, D_FF, D_MODEL, s);
  else launch_skinny16_relu_pack_xfirst(W16, xp, bias, xp_out, D_FF, D_MODEL, s);
}
int launch_status(vx_ctx* c);      // VX_EINVAL (+ message) if a launcher refused since the last check
// decode geometry of a decode batch of nrows rows (engine.hip): sets c->nsplit, c->split_fused, c->sb_chain, c->sb_qkv; `identity`: the
// launch slot order is the identity.  Also called by vx_dev_dec_attn (bench_harness.hip), which restores the four fields.
void decode_geometry(vx_ctx* c, int nrows, bool identity);
// best_of fan-out (beams.hip): one launch per prefill.  pairs [npairs][3] = {source slot, destination slot, cached rows}: that many
// K / V rows of every (layer, head) are copied between the two arena slots; dh[d] = hsrc[hsrc_row[d]] for the nrows decode rows.
// Every slot < mbr, every row count <= Tmax (the caller builds the table from its own slot map).
void launch_beam_fanout(float* kc, float* vc, long cache_layer, int layers, int Tmax, const int* pairs, int npairs,
                        const float* hsrc, const int* hsrc_row, float* dh, int nrows, hipStream_t s);

// sequence tables of one full-sequence AR prefill (engine.hip prefill_tables: ar_prefill's first fill and the continuous schedule's
// admissions); offsets into the MetaBuilder of the prefill
struct PrefillPlan {
  int nb = 0, max_len = 0, n_t = 0, n_a = 0;
  long M = 0;
  std::vector<int> seq_off, seq_len, S_;
  std::vector<int> row_b;          // [M] prefill row of every packed row; the caller maps it to an arena slot and adds it as o_rb
  long o_off = 0, o_len = 0, o_S = 0, o_dt = 0, o_it = 0, o_lt = 0, o_pt = 0, o_da = 0, o_ia = 0, o_pa = 0, o_rt = 0, o_rb = 0,
       o_tq = 0, o_tc = 0, o_tr = 0;
  double trim_flops = 0;
  bool trim = false, trim_h2 = false;
  int hrow(int i) const { return trim ? i : seq_off[i] + seq_len[i] - 1; }   // row of sequence i's last position in prefill_hsrc
};

// continuous schedule (admit.hip).  Admission of waiting caller rows into free decode rows of a running decode batch:
//   tab [n][5] = {decode row d, prompt frames Tp, context S + 1 + Tp, text length S, row of hsrc}: the decode state of row d as
//   ar_prefill sets it (slot_meta context included; the active flag is set by launch_admit_mask) and hres[d] = hsrc[row];
void launch_admit_rows(const int* tab, int n, const float* hsrc, float* hres, int* cur_tok, int* cur_pos, int* ctx_len, int* n_gen,
                       int* text_len, int* slot_meta, const int* slot_of, hipStream_t s);
//   phase 0: saved[d] = admitted[d] ? 0 : active[d], active[d] = admitted[d] (the sampler then commits the admitted rows only);
//   phase 1: active[d] |= saved[d], slot_meta[4 slot_of[d] + 2] = active[d], *n_active = number of active rows.  nrows <= 64.
void launch_admit_mask(int phase, const int* admitted, int* saved, int nrows, int* active, int* slot_meta, const int* slot_of,
                       int* n_active, hipStream_t s);
//   the sampler's draws of decode column d for steps 0 .. steps-1, u[t * ncols + d]: pairs [n][2] = {d, caller row r};
//   staged != null: staged[i * steps + t] (injected uniforms, column r of the caller's [steps][batch]); else the counter-based
//   draw of caller row r, splitmix64(splitmix64(splitmix64(seed) + r) + t) >> 40 x 2^-24 (dec_sample_kernel's formula)
void launch_admit_uniforms(const int* pairs, int n, const float* staged, int steps, unsigned long long seed, float* u, int ncols,
                           hipStream_t s);

// serving session (serve.hip): one launch per admission writes, for every admitted beam row, its draws, a zero sum_logp and its two
// per-row records.  tab [n][SERVE_UTAB], 13 words per beam row:
//   0 decode row d | 1 beam j | 2 offset of beam j's staged draws in `staged` (-1: counter-based, keyed on (seed, j)) | 3 draws to write
//   4, 5 seed low / high word | 6 top_k | 7 temperature bits | 8 force_eos_at   -> row_smp[4 d ..] = {top_k, temperature bits, force_eos_at, 0}
//   9 top_p bits | 10 repetition penalty bits | 11 repetition window | 12 min_frames   -> row_flt[4 d ..] = those four
constexpr int SERVE_UTAB = 13;
void launch_serve_uniforms(const int* tab, int n, int max_steps, const float* staged, float* u, int ncols, float* sum_logp,
                           int* row_smp, int* row_flt, hipStream_t s);
// cancellation of decoding requests (serve.hip): active[d] = 0 for every bit d of `rows`, then, for d < nrows,
// slot_meta[4 slot_of[d] + 2] = active[d] and *n_active = number of active rows (recounted from the flags).  nrows <= 32.
void launch_serve_cancel(unsigned rows, int nrows, int* active, int* slot_meta, const int* slot_of, int* n_active, hipStream_t s);

// the serving session's sampler (serve_sample.hip): dec_sample_kernel's computation with top_k, temperature and force_eos_at read
// per decode row from row_smp (written at admission by launch_serve_uniforms) instead of launch constants.  Always commits, always
// draws from `uniforms` (the session writes every admitted row's column), always accumulates sum_logp.  row_flt (may be null: every
// row neutral) adds the per-row top_p, repetition penalty over the row's generated frames and min_frames.
struct ServeSampleArgs {
  const float* partial; int splitk; int npad;     // logits partials [splitk][MB][npad]
  const int* row_smp;                              // [MB][4] = {top_k, temperature bits, force_eos_at, 0}
  const int* row_flt;                              // [MB][4] = {top_p bits, penalty bits, window, min_frames}; null: neutral
  const float* uniforms; int uniforms_stride;     // [steps][uniforms_stride]
  int* cur_tok; int* cur_pos; int* ctx_len; int* n_gen; int* active; int* n_active; const int* text_len;
  int* slot_meta; const int* slot_of;
  int* gen; int gen_stride;
  float* sum_logp;
  int batch;
  // the fused start of the next step, as SampleArgs (emb_tab == null: off)
  const float* emb_tab; const float* emb_alpha; const float* pe; const float* ln_g; const float* ln_b;
  float* emb_h; float* emb_xp;
  int wt;
};
bool launch_serve_sample(const ServeSampleArgs& a, hipStream_t s);

// Row trimming of the LAST decoder layer of a NAR stage (f16x2 mode, and since round 6 the reference-arithmetic fp32 mode): only the
// generated frames of every sequence reach a predict layer (models/vallex.py:672-679), so behind the K / V projection -- which
// attention needs for ALL rows -- the layer only has to produce those rows: attention queries, out_proj, norm2 and the FFN run on the
// Mc = sum T_b compacted rows.  Every op of the block treats rows independently, so each kept row goes through exactly the arithmetic
// it would see untrimmed: same ids, same logits, bit for bit.  The compacted residual stream lives in c->fxn (f16x2 mode: unused
// otherwise) or in the QKV buffer (fp32 mode).
struct Trim {
  long Mc;               // kept rows
  const int* q_first;    // [batch] first kept sequence-local row (S + Tp)
  const int* c_off;      // [batch] first compacted row of the sequence
  const int* rows;       // [Mc] packed row of every compacted row (residual gather)
  double attn_flops;     // 4 * T_b * L_b * 1024 summed: the queries that are still computed
};
// Attention tap of full_layer (vx_align): behind the in_proj -- the fp32 QKV buffer holds the layer's q and k in every arithmetic
// mode, and the trimmed fp32 path reuses it behind the attention -- ONE launch of align_rows_kernel (align.hip) adds the layer's
// weighted text attention of the rows in `tab` to `out`.  stop: nothing behind the tap is needed, the layer ends there.
struct AlignTap {
  const int* tab;        // [nseq][6] = {seq_off, seq_len, S, q_first, n_rows, out_off}
  int nseq, max_rows;    // max_rows: the largest n_rows
  const float* w;        // [16] the layer's head weights
  float* out;
  int ld_out;
  bool stop;
};
void launch_align_rows(const float* qkv, const int* tab, int nseq, int max_rows, const float* w, float* out, int ld_out, hipStream_t s);
// engine.hip, shared with the scoring passes (score.hip)
constexpr int VX_RETRY_F32 = 1;      // internal: the phase raised the f16x2 range flag, run it again on the fp32 kernels
void proj(vx_ctx* c, const float* A, int lda, const float* Wf, const unsigned short* W3, const float* bias, const float* resid, int ldr,
          float* C, int ldc, long M, int N, int K, int act, const int* gather = nullptr, const unsigned short* a_pre = nullptr,
          unsigned short* out_pl = nullptr, const int* resid_rows = nullptr);
int full_layer(vx_ctx* c, const LayerW& L, long M, const int* seq_off, const int* seq_len, const int* prefix_len, int batch, int max_len,
               const float* ada1, const float* ada2, float* kcl, float* vcl, const int* row_b, const int* row_t, double attn_flops,
               const Trim* tr = nullptr, const AlignTap* tap = nullptr);
int prefill_tables(vx_ctx* c, const vx_batch* b, int r0, int nb, PrefillPlan& p, MetaBuilder& mb);
// engine.hip, shared with the schedulers (schedule.hip)
constexpr int GRAPH_STEPS = 4;       // decode steps per multi-step graph launch (ar_step_run)
int ar_prefill(vx_ctx* c, const vx_batch* b, int r0, int nb, int beams = 1);
void prefill_embed(vx_ctx* c, const PrefillPlan& p, const MetaBuilder& mb);
int prefill_layers(vx_ctx* c, const PrefillPlan& p, const MetaBuilder& mb);
const float* prefill_hsrc(const vx_ctx* c, const PrefillPlan& p);
int reset_decode_state(vx_ctx* c, const MetaBuilder& mb, int nrows, long o_pos, long o_ctx, long o_zero, long o_active, long o_text,
                       long o_meta, long o_slot);
int ar_step_run(vx_ctx* c, const SampleArgs* sa, const std::string& sig, int nsteps = 1, const ServeSampleArgs* rsa = nullptr);
// one NAR pass (engine.hip; the generating pass and the scoring pass of score.hip drive the same tables and the same stage):
// offsets into the pass's MetaBuilder
struct NarPlan {
  int nb = 0, max_len = 0, n_t = 0;
  long M = 0, Y = 0, sumT = 0;     // packed rows, prompt + generated frames, generated frames
  double attn_flops = 0, trim_attn_flops = 0;
  long o_off = 0, o_len = 0, o_dt = 0, o_it = 0, o_lt = 0, o_pt = 0, o_yc = 0, o_nj = 0, o_yd = 0, o_yp = 0, o_gr = 0, o_gy = 0, o_qf = 0,
       o_co = 0;
};
int nar_plan(vx_ctx* c, const vx_batch* b, int r0, int nb, const std::vector<int>& T, const std::function<int(int, int)>& code0,
             MetaBuilder& mb, NarPlan& p);
int nar_stage(vx_ctx* c, const NarPlan& p, const MetaBuilder& mb, int st, bool taps);
int nar_early_flag(vx_ctx* c, int st);
int nar_generate(vx_ctx* c, const vx_batch* b, int r0, int nb, const std::vector<int>& T, const int* codes0, long codes0_stride,
                 std::vector<int>& out_codes /* [7][sumT] */, long& sumT_out);
void interleave_codes(int64_t* dst, const int* codes0_row, const std::vector<int>& oc, long sumT, long off, int T);
inline void reset_call_stats(vx_ctx* c) {      // what vx_last_stats / vx_last_truncated / vx_last_fallbacks report is per call
  c->st_steps = 0; c->st_frames = 0; c->st_ar_ms = 0; c->st_nar_ms = 0; c->st_truncated = 0;
  c->st_fb_prefill = c->st_fb_nar = 0;
}
// schedule.hip: entry points that overwrite the decode state refuse to run while a serving session owns it; vx_destroy frees an open one
int serve_busy(vx_ctx* c, const char* what);
void serve_free(vx_serve* v);
// (the launch buffers of the waveform entries and what else their translation units share: wave_stage.h)
// score.hip: (log-probability, rank) of targets[r] in logits[r][0 .. ncols-1], one wavefront per row
void launch_score_rows(const float* logits, int ld, int rows, int ncols, const int* targets, float* logp, int* rank, hipStream_t s);

// ---- the f16x2 range guard with sticky fp32 fallback: ONE protocol for every guarded phase -------------------------------------
// (what the guard is for: engine.hip, above range_guarded; the sticky rule: vx_ctx, above fb_prefill_raises)
struct F32Scope {            // the full-sequence path on the exact-fp32 kernels for the lifetime of the object
  vx_ctx* c;
  int gm;
  bool ax;
  explicit F32Scope(vx_ctx* c_) : c(c_), gm(c_->gemm_mode), ax(c_->attn_x3) { c->gemm_mode = 2; c->attn_x3 = false; }
  ~F32Scope() { c->gemm_mode = gm; c->attn_x3 = ax; }
};

// the end of every `once` (below): flag = the range flag as it came back on the phase's own host sync.  Raised: cleared on the stream
// (the re-run starts from a clean flag) and VX_RETRY_F32; else VX_OK
int retry_if_raised(vx_ctx* c, int flag);
// ... preceded by that sync, for a `once` that has queued everything else it wants back: the flag rides along, stream sync, verdict
int sync_guarded(vx_ctx* c);

// the two phase kinds count and go sticky separately
struct GuardKind { bool& sticky; int& age; int& raises; int& st_fb; };
inline GuardKind prefill_kind(vx_ctx* c) { return {c->sticky_prefill_f32, c->sticky_prefill_age, c->fb_prefill_raises, c->st_fb_prefill}; }
inline GuardKind nar_kind(vx_ctx* c) { return {c->sticky_nar_f32, c->sticky_nar_age, c->fb_nar_raises, c->st_fb_nar}; }

// One guarded phase.  once() runs the phase up to and including the host sync it has anyway, reads the flag on that sync
// (`if (range_guarded(c)) D2H(&flag, ...)`: false under F32Scope, so the fp32 run reads nothing) and ends in retry_if_raised.
//   probe (not sticky, or every FB_STICKY_PROBE_EVERY-th phase of a sticky kind): once() on f16x2; a clean pass resets the consecutive
//     count and leaves sticky mode, a raise counts towards it (FB_STICKY_AFTER) and the phase runs again on the exact-fp32 kernels;
//   direct (sticky): once() on the fp32 kernels straight away; the counts do not move.
// Either fp32 run counts in vx_last_fallbacks (k.st_fb) and in the lifetime total.
template <typename Once>
int guarded(vx_ctx* c, GuardKind k, Once once) {
  const bool watch = range_guarded(c);
  bool direct = watch && k.sticky;
  if (direct && ++k.age >= FB_STICKY_PROBE_EVERY) { k.age = 0; direct = false; }
  auto fb_outcome = [&](bool raised) {       // outcome of a phase that RAN on f16x2
    if (!watch) return;
    if (!raised) { k.raises = 0; k.sticky = false; k.age = 0; return; }
    if (++k.raises >= FB_STICKY_AFTER && !k.sticky) { k.sticky = true; k.age = 0; ++c->sticky_engaged; }
  };
  if (!direct) {
    const int e = once();
    if (e == VX_OK || e == VX_RETRY_F32) fb_outcome(e == VX_RETRY_F32);
    if (e != VX_RETRY_F32) return e;
  }
  ++k.st_fb; ++c->fb_total;
  if (int e = ensure_f32_buffers(c)) return e;
  F32Scope f32(c);
  return once();
}

}  // namespace vxe
