// Teacher-forced scoring: how likely the model finds codes that already exist (vx_score, include/vallex_hip.h).
// The quantity VALLE.forward feeds to F.cross_entropy (models/vallex.py: the AR stack on the first codebook, the NAR stages on
// codebooks 2 .. 8) and the one best_of selects on (sum(logp) / len^penalty, models/vallex.py:572, :583-594).  Both passes drive the
// full-sequence layers of engine.hip (full_layer + Trim), behind the range guard of engine_ctx.h (guarded), with the GIVEN codes as inputs; the one new kernel turns logit rows into
// (log-probability, rank) of a target id.
// Text alignment (vx_align) is the same AR pass with a tap in every weighted layer: align_rows_kernel (align.hip) turns the layer's q and k
// into the attention of the frames' rows over the text.
#include <cmath>

#include "engine_ctx.h"

#include "../../include/vallex_hip_dev.h"

namespace vxe {

// ---------------------------------------------------------------------------------------------
// (logp, rank) of targets[row] in logits[row][0 .. ncols-1]:  m = max_j l_j, s = sum_j expf(l_j - m), logp = (l_t - m) - logf(s),
// rank = #{j : l_j > l_t} (strictly: rank 0 = the target is an arg-max, ties included).  One wavefront per row, four rows per block;
// the row is read once, as 16-byte loads held in registers (ncols <= 1280), wave-shuffle reductions, no LDS.  Columns ncols .. ld-1
// are padding: a 16-byte group that starts behind ncols is not loaded, the tail of the group that straddles ncols is masked.
// ---------------------------------------------------------------------------------------------
constexpr int SCORE_GROUPS = 5;              // float4 groups per lane: 5 x 64 x 4 = 1280 columns
constexpr int SCORE_MAX_COLS = SCORE_GROUPS * 64 * 4;

__global__ __launch_bounds__(256) void score_rows_kernel(const float* __restrict__ logits, int ld, int rows, int ncols,
                                                         const int* __restrict__ targets, float* __restrict__ logp,
                                                         int* __restrict__ rank) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* xr = logits + (long)row * ld;
  const int t = targets[row];
  float v[SCORE_GROUPS * 4];
  float m = -INFINITY, lt = -INFINITY;
#pragma unroll
  for (int i = 0; i < SCORE_GROUPS; ++i) {
    const int c = (i * 64 + lane) * 4;
    f32x4 q = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    if (c < ncols) q = *reinterpret_cast<const f32x4*>(xr + c);      // c + 3 < ld: ld >= ncols, ld % 4 == 0
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float x = c + e < ncols ? q[e] : -INFINITY;
      v[i * 4 + e] = x;
      m = fmaxf(m, x);
      if (c + e == t) lt = x;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    m = fmaxf(m, __shfl_xor(m, o, 64));
    lt = fmaxf(lt, __shfl_xor(lt, o, 64));                           // one lane holds l_t, the others -inf
  }
  float s = 0.f;
  int above = 0;
#pragma unroll
  for (int i = 0; i < SCORE_GROUPS; ++i) {
    const int c = (i * 64 + lane) * 4;
    float ex[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool in = c + e < ncols;
      ex[e] = in ? expf(v[i * 4 + e] - m) : 0.f;
      above += (in && v[i * 4 + e] > lt) ? 1 : 0;
    }
    s += (ex[0] + ex[1]) + (ex[2] + ex[3]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o, 64);
    above += __shfl_xor(above, o, 64);
  }
  if (lane == 0) {
    logp[row] = (lt - m) - logf(s);
    rank[row] = above;
  }
}

void launch_score_rows(const float* logits, int ld, int rows, int ncols, const int* targets, float* logp, int* rank, hipStream_t s) {
  if (rows <= 0) return;
  hipLaunchKernelGGL(score_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, logits, ld, rows, ncols, targets, logp, rank);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
constexpr int SCORE_LD = 1028;               // AR logits row: 1025 columns padded to the GEMMs' N % 4 == 0

// device memory only a scoring context needs: the padded predict weight, the result buffers, and a logits buffer when the NAR
// stages' one (mbr x max_new rows of 1024) cannot hold mbr x (max_new + 1) rows of 1028
static int score_buffers(vx_ctx* c) {
  if (c->sc_predw) return VX_OK;
  const long rows = (long)c->mbr * (c->cfg.max_new + 1);
  float *logp = nullptr, *pw = nullptr;
  int* rank = nullptr;
  if (int e = dev_alloc(c, &logp, (size_t)rows * N_Q)) return e;
  if (int e = dev_alloc(c, &rank, (size_t)rows * N_Q)) return e;
  if (((long)c->mbr * c->cfg.max_new + 128) * AUDIO_VOCAB < rows * SCORE_LD)
    if (int e = dev_alloc(c, &c->sc_logits, (size_t)rows * SCORE_LD)) return e;
  if (int e = dev_alloc(c, &pw, (size_t)SCORE_LD * D_MODEL)) return e;      // zeroed: rows 1025 .. 1027 stay zero
  HIPCHK(hipMemcpyAsync(pw, W(c, "ar_predict_layer.weight"), (size_t)AR_LOGITS * D_MODEL * sizeof(float), hipMemcpyDeviceToDevice,
                        c->stream));
  c->sc_logp = logp; c->sc_rank = rank; c->sc_predw = pw;
  return VX_OK;
}

// the scored codes of caller rows r0 .. r0+nb-1: codes [batch][stride][8] int64 (vx_infer's output layout)
struct ScoreRows {
  const vx_batch* b;
  const int64_t* codes;
  long stride;
  int r0, nb;
  std::vector<int> T;
  int code(int i, int t, int q) const { return (int)codes[((long)(r0 + i) * stride + t) * N_Q + q]; }
};

// The AR pass over GIVEN frames, shared by the scoring and the alignment pass: the prefill's tables of a batch whose prompts are the
// callers' with the given frames appended (only codebook 0 is read).  q_first[i] = S + Tp: the sequence-local row that predicts frame 0.
static int given_tables(vx_ctx* c, const ScoreRows& R, MetaBuilder& mb, PrefillPlan& p, std::vector<int>& q_first, double& attn_flops) {
  const int nb = R.nb;
  const vx_batch* b = R.b;
  int ps = 1;
  for (int i = 0; i < nb; ++i) ps = std::max(ps, b->prompt_lens[R.r0 + i] + R.T[i]);
  std::vector<int32_t> pc((size_t)nb * ps * N_Q, 0), pl(nb);
  for (int i = 0; i < nb; ++i) {
    const int Tp = b->prompt_lens[R.r0 + i];
    pl[i] = Tp + R.T[i];
    for (int t = 0; t < Tp; ++t) pc[((size_t)i * ps + t) * N_Q] = b->prompt_codes[((long)(R.r0 + i) * b->prompt_stride + t) * N_Q];
    for (int t = 0; t < R.T[i]; ++t) pc[((size_t)i * ps + Tp + t) * N_Q] = R.code(i, t, 0);
  }
  vx_batch bx = *b;
  bx.batch = nb;
  bx.text_ids = b->text_ids + (long)R.r0 * b->text_stride; bx.text_lang = b->text_lang + (long)R.r0 * b->text_stride;
  bx.text_lens = b->text_lens + R.r0;
  bx.prompt_codes = pc.data(); bx.prompt_stride = ps; bx.prompt_lens = pl.data();
  if (int e = prefill_tables(c, &bx, 0, nb, p, mb)) return e;
  q_first.resize(nb);
  attn_flops = 0;
  for (int i = 0; i < nb; ++i) {
    q_first[i] = p.S_[i] + b->prompt_lens[R.r0 + i];
    attn_flops += 4.0 * p.seq_len[i] * (double)p.seq_len[i] * D_MODEL;
  }
  return VX_OK;
}

// layer l of the AR stack on the packed rows of `p` under the prefix-LM mask; nothing goes into the KV arena
static int given_layer(vx_ctx* c, const PrefillPlan& p, const MetaBuilder& mb, int l, double attn_flops, const Trim* tr,
                       const AlignTap* tap = nullptr) {
  return full_layer(c, c->ar[l], p.M, mb.dev(p.o_off), mb.dev(p.o_len), mb.dev(p.o_S), p.nb, p.max_len, nullptr, nullptr, nullptr, nullptr,
                    nullptr, nullptr, attn_flops, tr, tap);
}

// AR pass of one group: text, then BOS ++ prompt codebook 0 ++ codes[:, 0] under the prefix-LM mask of the prefill; nothing goes
// into the KV arena and no decode state is touched.  The last layer computes only the T_b + 1 rows that predict frame 0 .. T_b - 1
// and the stop decision.  logp / rank [sum (T_b + 1)]: row T_b of a sequence scores EOS.
static int score_ar_once(vx_ctx* c, const ScoreRows& R, std::vector<float>& logp, std::vector<int>& rank) {
  const int nb = R.nb, NL = c->NL;
  PrefillPlan p;
  MetaBuilder mb(c);
  std::vector<int> q_first, c_off(nb), rows, tg;
  double trim_flops = 0, attn_flops = 0;
  if (int e = given_tables(c, R, mb, p, q_first, attn_flops)) return e;
  long Mc = 0;
  for (int i = 0; i < nb; ++i) {
    c_off[i] = (int)Mc;
    for (int t = 0; t <= R.T[i]; ++t) {
      rows.push_back(p.seq_off[i] + q_first[i] + t);
      tg.push_back(t < R.T[i] ? R.code(i, t, 0) : EOS_ID);
    }
    Mc += R.T[i] + 1;
    trim_flops += 4.0 * (R.T[i] + 1) * (double)p.seq_len[i] * D_MODEL;
  }
  const long o_qf = mb.add(q_first), o_co = mb.add(c_off), o_rows = mb.add(rows), o_tg = mb.add(tg);
  if (int e = upload_meta(c)) return e;

  prefill_embed(c, p, mb);
  // p.trim: the arithmetic can trim (f16x2 throughout, or fp32 throughout) -- bf16x3, the mixed switches and debug_taps run
  // every row and gather
  const Trim tr{Mc, mb.dev(o_qf), mb.dev(o_co), mb.dev(o_rows), trim_flops};
  for (int l = 0; l < NL; ++l)
    if (int e = given_layer(c, p, mb, l, attn_flops, (p.trim && l == NL - 1) ? &tr : nullptr)) return e;
  // ar_decoder.norm on the kept rows, then ar_predict_layer on the fp32 GEMM (models/vallex.py:568)
  const float *ng = W(c, "ar_decoder.norm.weight"), *nbias = W(c, "ar_decoder.norm.bias");
  float* lg = c->sc_logits ? c->sc_logits : c->flogits;
  const float* A;
  const int* gather = nullptr;
  if (p.trim && p.trim_h2) {             // compacted rows in fxn; fx is free behind the last layer
    launch_layernorm(c->fxn, D_MODEL, c->fx, D_MODEL, (int)Mc, D_MODEL, LN_EPS, ng, nbias, nullptr, nullptr, c->stream);
    A = c->fx;
  } else if (p.trim) {                   // compacted rows in the QKV buffer
    launch_layernorm(c->fqkv, D_MODEL, c->fxn, D_MODEL, (int)Mc, D_MODEL, LN_EPS, ng, nbias, nullptr, nullptr, c->stream);
    A = c->fxn;
  } else {
    launch_layernorm(c->fx, D_MODEL, c->fxn, D_MODEL, (int)p.M, D_MODEL, LN_EPS, ng, nbias, nullptr, nullptr, c->stream);
    A = c->fxn; gather = mb.dev(o_rows);
  }
  gemm(c, A, D_MODEL, c->sc_predw, D_MODEL, nullptr, nullptr, 0, nullptr, lg, SCORE_LD, Mc, SCORE_LD, D_MODEL, ACT_NONE, gather, 2);
  launch_score_rows(lg, SCORE_LD, (int)Mc, AR_LOGITS, mb.dev(o_tg), c->sc_logp, c->sc_rank, c->stream);
  HIPCHK(hipGetLastError());
  logp.resize(Mc); rank.resize(Mc);
  D2H(logp.data(), c->sc_logp, (size_t)Mc * sizeof(float));
  D2H(rank.data(), c->sc_rank, (size_t)Mc * sizeof(int));
  return sync_guarded(c);           // the range flag rides on the sync that brings the results back
}

// NAR pass of one group: the stages of nar_generate_once (engine.hip nar_plan / nar_stage: same tables, same trimming, same final
// AdaLN norm, same pred_w3 projection, the same kernels on the same shapes) with the GIVEN codes[.., st + 1] accumulated behind
// stage st instead of the arg-max, and scored instead of chosen.  logp / rank [7][sum T_b].
static int score_nar_once(vx_ctx* c, const ScoreRows& R, std::vector<float>& logp, std::vector<int>& rank, long& sumT_out) {
  const int nb = R.nb;
  MetaBuilder mb(c);
  NarPlan p;
  if (int e = nar_plan(c, R.b, R.r0, nb, R.T, [&](int i, int t) { return R.code(i, t, 0); }, mb, p)) return e;
  const long sumT = sumT_out = p.sumT;
  logp.assign((size_t)(N_Q - 1) * sumT, 0.f);
  rank.assign((size_t)(N_Q - 1) * sumT, 0);
  if (sumT == 0) return VX_OK;
  std::vector<int> tg((size_t)(N_Q - 1) * sumT);           // [7][sumT]: the targets of stage st = the given codebook st + 1
  for (int st = 0; st < N_Q - 1; ++st) {
    long off = 0;
    for (int i = 0; i < nb; ++i) {
      for (int t = 0; t < R.T[i]; ++t) tg[(size_t)st * sumT + off + t] = R.code(i, t, st + 1);
      off += R.T[i];
    }
  }
  const long o_tg = mb.add(tg);
  if (int e = upload_meta(c)) return e;

  launch_nar_yemb_init(c->fyemb, c->nar_tabs_dev, mb.dev(p.o_yc), mb.dev(p.o_nj), (int)p.Y, c->stream);
  for (int st = 0; st < N_Q - 1; ++st) {
    if (int e = nar_stage(c, p, mb, st, false)) return e;
    const int* given = mb.dev(o_tg) + (long)st * sumT;
    launch_score_rows(c->flogits, AUDIO_VOCAB, (int)sumT, AUDIO_VOCAB, given, c->sc_logp + (long)st * sumT, c->sc_rank + (long)st * sumT,
                      c->stream);
    if (int r = nar_early_flag(c, st)) return r;
    if (st < N_Q - 2) {
      char nm[64];
      snprintf(nm, sizeof nm, "nar_audio_embeddings.%d.word_embeddings.weight", st + 1);
      launch_embed_accum(c->fyemb, mb.dev(p.o_gy), W(c, nm), given, (int)sumT, c->stream);
    }
  }
  HIPCHK(hipGetLastError());
  D2H(logp.data(), c->sc_logp, logp.size() * sizeof(float));
  D2H(rank.data(), c->sc_rank, rank.size() * sizeof(int));
  return sync_guarded(c);
}

// ---------------------------------------------------------------------------------------------
// text alignment (vx_align): the AR pass above with align_rows_kernel (align.hip) tapping every weighted layer's q and k
// ---------------------------------------------------------------------------------------------
static int align_ld(const vx_ctx* c) { return (c->cfg.max_text + 3) / 4 * 4; }

static int align_buffers(vx_ctx* c) {
  if (c->al_out) return VX_OK;
  float *out = nullptr, *w = nullptr;
  if (int e = dev_alloc(c, &out, (size_t)c->mbr * c->cfg.max_new * align_ld(c))) return e;
  if (int e = dev_alloc(c, &w, (size_t)c->NL * N_HEAD)) return e;
  c->al_out = out; c->al_w = w;
  return VX_OK;
}

// One group: attn [sum T_b][align_ld] = sum over the layers l and heads h of hw[l][h] x the probability the row that predicts frame t
// puts on the text columns.  The accumulation buffer is zeroed HERE: a re-run in fp32 starts from zero, not from a half-finished
// sum.  The pass ends behind the in_proj of the last weighted layer: no attention, FFN, final norm or predict layer there, no later layer.
static int align_once(vx_ctx* c, const ScoreRows& R, const float* hw, std::vector<float>& attn) {
  const int nb = R.nb, NL = c->NL, ld = align_ld(c);
  PrefillPlan p;
  MetaBuilder mb(c);
  std::vector<int> q_first, tab;
  double attn_flops = 0;
  if (int e = given_tables(c, R, mb, p, q_first, attn_flops)) return e;
  long sumT = 0;
  int max_rows = 0;
  for (int i = 0; i < nb; ++i) {
    tab.insert(tab.end(), {p.seq_off[i], p.seq_len[i], p.S_[i], q_first[i], R.T[i], (int)sumT});
    sumT += R.T[i];
    max_rows = std::max(max_rows, R.T[i]);
  }
  const long o_tab = mb.add(tab);
  if (int e = upload_meta(c)) return e;
  auto weighted = [&](int l) { for (int h = 0; h < N_HEAD; ++h) if (hw[l * N_HEAD + h] > 0.f) return true; return false; };
  int last = 0;
  for (int l = 0; l < NL; ++l) if (weighted(l)) last = l;
  H2D(c->al_w, hw, (size_t)NL * N_HEAD * sizeof(float));
  HIPCHK(hipMemsetAsync(c->al_out, 0, (size_t)sumT * ld * sizeof(float), c->stream));
  prefill_embed(c, p, mb);
  for (int l = 0; l <= last; ++l) {
    const AlignTap tap{mb.dev(o_tab), nb, max_rows, c->al_w + l * N_HEAD, c->al_out, ld, l == last};
    if (int e = given_layer(c, p, mb, l, attn_flops, nullptr, weighted(l) ? &tap : nullptr)) return e;
  }
  HIPCHK(hipGetLastError());
  attn.resize((size_t)sumT * ld);
  D2H(attn.data(), c->al_out, attn.size() * sizeof(float));
  return sync_guarded(c);           // the range flag rides on the sync that brings the result back
}

}  // namespace vxe

extern "C" {

int vx_align(vx_ctx* c, const vx_batch* b, const int64_t* codes, int32_t codes_stride, const int32_t* lens, const float* head_weights,
             float* attn, int32_t out_stride, int32_t text_out_stride) {
  if (!c) return VX_EINVAL;
  if (c->serve) FAIL(VX_EINVAL, "vx_align: a serving session is open on this context (vx_serve_close it first)");
  HIPCHK(hipSetDevice(c->dev));
  if (int e = check_batch(c, b, c->cfg.max_batch)) return e;
  if (!codes || !lens) FAIL(VX_EINVAL, "vx_align: null codes or lens");
  if (!attn) FAIL(VX_EINVAL, "vx_align: null attn");
  for (int i = 0; i < b->batch; ++i) {
    const int T = lens[i];
    if (T < 0 || T > c->cfg.max_new) FAIL(VX_EINVAL, "vx_align: row %d: lens %d outside 0 .. max_new (%d)", i, T, c->cfg.max_new);
    if (T > codes_stride) FAIL(VX_EINVAL, "vx_align: row %d: codes_stride %d below lens %d", i, codes_stride, T);
    if (T > out_stride) FAIL(VX_EINVAL, "vx_align: row %d: out_stride %d below lens %d", i, out_stride, T);
    if (b->text_lens[i] > text_out_stride)
      FAIL(VX_EINVAL, "vx_align: row %d: text_out_stride %d below the text length %d", i, text_out_stride, b->text_lens[i]);
  }
  for (int i = 0; i < b->batch; ++i)
    for (int t = 0; t < lens[i]; ++t) {
      const int64_t v = codes[((long)i * codes_stride + t) * N_Q];
      if (v < 0 || v >= AUDIO_VOCAB) FAIL(VX_EINVAL, "vx_align: codes: row %d frame %d codebook 0: %lld outside 0 .. 1023", i, t, (long long)v);
    }
  std::vector<float> hw((size_t)c->NL * N_HEAD, 1.0f / (float)(N_HEAD * c->NL));
  if (head_weights) {
    bool any = false;
    for (size_t i = 0; i < hw.size(); ++i) {
      hw[i] = head_weights[i];
      if (!std::isfinite(hw[i]) || hw[i] < 0.f)
        FAIL(VX_EINVAL, "vx_align: head_weights[%d][%d] is negative or not finite", (int)(i / N_HEAD), (int)(i % N_HEAD));
      any |= hw[i] > 0.f;
    }
    if (!any) FAIL(VX_EINVAL, "vx_align: head_weights are all zero");
  }
  if (int e = align_buffers(c)) return e;
  reset_call_stats(c);
  hipEvent_t e0 = c->ev_t[0], e1 = c->ev_t[1];
  const int ld = align_ld(c);
  for (int r0 = 0; r0 < b->batch; r0 += c->mbr) {
    ScoreRows R{b, codes, codes_stride, r0, std::min(c->mbr, b->batch - r0), {}};
    R.T.assign(lens + r0, lens + r0 + R.nb);
    long sumT = 0;
    for (int T : R.T) sumT += T;
    if (sumT == 0) continue;                     // nothing to align in this group
    std::vector<float> a;
    HIPCHK(hipEventRecord(e0, c->stream));
    if (int e = guarded(c, prefill_kind(c), [&] { return align_once(c, R, hw.data(), a); })) return e;
    HIPCHK(hipEventRecord(e1, c->stream));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1)); c->st_ar_ms += ms;
    long off = 0;
    for (int i = 0; i < R.nb; ++i) {
      const int T = R.T[i], S = b->text_lens[r0 + i];
      c->st_frames += T;
      for (int t = 0; t < T; ++t)
        memcpy(attn + ((long)(r0 + i) * out_stride + t) * text_out_stride, a.data() + (off + t) * ld, (size_t)S * sizeof(float));
      off += T;
    }
  }
  return VX_OK;
}

int vx_score(vx_ctx* c, const vx_batch* b, const int64_t* codes, int32_t codes_stride, const int32_t* lens, int32_t parts,
             float* logp, int32_t* rank, int32_t out_stride, float* eos_logp, int32_t* eos_rank) {
  if (!c) return VX_EINVAL;
  if (c->serve) FAIL(VX_EINVAL, "vx_score: a serving session is open on this context (vx_serve_close it first)");
  HIPCHK(hipSetDevice(c->dev));
  if (int e = check_batch(c, b, c->cfg.max_batch)) return e;
  if (parts < 1 || parts > 3) FAIL(VX_EINVAL, "vx_score: parts must be VX_SCORE_AR, VX_SCORE_NAR or both (1 .. 3), got %d", parts);
  const bool do_ar = parts & VX_SCORE_AR, do_nar = parts & VX_SCORE_NAR;
  if (!codes || !lens) FAIL(VX_EINVAL, "vx_score: null codes or lens");
  if (!logp || !rank) FAIL(VX_EINVAL, "vx_score: null logp or rank");
  if (do_ar && (!eos_logp || !eos_rank)) FAIL(VX_EINVAL, "vx_score: VX_SCORE_AR needs eos_logp and eos_rank");
  for (int i = 0; i < b->batch; ++i) {
    const int T = lens[i];
    if (T < 0 || T > c->cfg.max_new) FAIL(VX_EINVAL, "vx_score: row %d: lens %d outside 0 .. max_new (%d)", i, T, c->cfg.max_new);
    if (T > codes_stride) FAIL(VX_EINVAL, "vx_score: row %d: codes_stride %d below lens %d", i, codes_stride, T);
    if (T > out_stride) FAIL(VX_EINVAL, "vx_score: row %d: out_stride %d below lens %d", i, out_stride, T);
  }
  for (int i = 0; i < b->batch; ++i)
    for (int t = 0; t < lens[i]; ++t)
      for (int q = 0; q < (do_nar ? N_Q : 1); ++q) {
        const int64_t v = codes[((long)i * codes_stride + t) * N_Q + q];
        if (v < 0 || v >= AUDIO_VOCAB) FAIL(VX_EINVAL, "vx_score: codes: row %d frame %d codebook %d: %lld outside 0 .. 1023", i, t, q, (long long)v);
      }
  if (int e = score_buffers(c)) return e;
  reset_call_stats(c);
  hipEvent_t e0 = c->ev_t[0], e1 = c->ev_t[1], e2 = c->ev_t[2];
  for (int r0 = 0; r0 < b->batch; r0 += c->mbr) {
    ScoreRows R{b, codes, codes_stride, r0, std::min(c->mbr, b->batch - r0), {}};
    R.T.assign(lens + r0, lens + r0 + R.nb);
    std::vector<float> lp_a, lp_n;
    std::vector<int> rk_a, rk_n;
    long sumT = 0;
    HIPCHK(hipEventRecord(e0, c->stream));
    if (do_ar)
      if (int e = guarded(c, prefill_kind(c), [&] { return score_ar_once(c, R, lp_a, rk_a); })) return e;
    HIPCHK(hipEventRecord(e1, c->stream));
    if (do_nar)
      if (int e = guarded(c, nar_kind(c), [&] { return score_nar_once(c, R, lp_n, rk_n, sumT); })) return e;
    HIPCHK(hipEventRecord(e2, c->stream));
    HIPCHK(hipEventSynchronize(e2));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1)); c->st_ar_ms += ms;
    HIPCHK(hipEventElapsedTime(&ms, e1, e2)); c->st_nar_ms += ms;
    long off_a = 0, off_n = 0;
    for (int i = 0; i < R.nb; ++i) {
      const int T = R.T[i];
      c->st_frames += T;
      for (int t = 0; t < T; ++t) {
        const long o = ((long)(r0 + i) * out_stride + t) * N_Q;
        if (do_ar) { logp[o] = lp_a[off_a + t]; rank[o] = rk_a[off_a + t]; }
        if (do_nar)
          for (int st = 0; st < N_Q - 1; ++st) {
            logp[o + st + 1] = lp_n[(size_t)st * sumT + off_n + t];
            rank[o + st + 1] = rk_n[(size_t)st * sumT + off_n + t];
          }
      }
      if (do_ar) { eos_logp[r0 + i] = lp_a[off_a + T]; eos_rank[r0 + i] = rk_a[off_a + T]; }
      off_a += T + 1; off_n += T;
    }
  }
  return VX_OK;
}

// vx_dev_score_rows: ONE launch of score_rows_kernel on caller rows (private scratch, outputs pre-filled with the sentinels).
int vx_dev_score_rows(vx_ctx* c, int32_t rows, int32_t ncols, int32_t ld, const float* logits, const int32_t* targets, float* logp,
                      int32_t* rank, int32_t rows_out) {
  if (!c) return VX_EINVAL;
  if (c->serve) FAIL(VX_ESTATE, "vx_dev_score_rows: a serving session is open on this context (vx_serve_close it first)");
  if (!logits || !targets || !logp || !rank) FAIL(VX_EINVAL, "vx_dev_score_rows: null logits, targets, logp or rank");
  if (rows < 1 || rows > 4096) FAIL(VX_EINVAL, "vx_dev_score_rows: rows outside 1 .. 4096");
  if (ncols != AUDIO_VOCAB && ncols != AR_LOGITS) FAIL(VX_EINVAL, "vx_dev_score_rows: ncols must be 1024 or 1025");
  if (ld < ncols || ld > 8192 || ld % 4) FAIL(VX_EINVAL, "vx_dev_score_rows: ld outside ncols .. 8192 or ld %% 4 != 0");
  if (rows_out < rows || rows_out > rows + 64) FAIL(VX_EINVAL, "vx_dev_score_rows: rows_out must be rows .. rows + 64");
  for (int i = 0; i < rows; ++i)
    if (targets[i] < 0 || targets[i] >= ncols) FAIL(VX_EINVAL, "vx_dev_score_rows: targets[%d] = %d outside 0 .. ncols - 1", i, targets[i]);
  static_assert(AR_LOGITS <= SCORE_MAX_COLS, "score_rows_kernel holds a row in SCORE_GROUPS float4 per lane");
  HIPCHK(hipSetDevice(c->dev));
  float *dx = nullptr, *dlp = nullptr;
  int *dt = nullptr, *drk = nullptr;
  auto cleanup = [&]() { for (void* p : {(void*)dx, (void*)dlp, (void*)dt, (void*)drk}) if (p) (void)hipFree(p); };
  hipError_t he;
  // an error return drains the ring first: a queued xfer_d2h must not be delivered into host buffers that are gone by then
#define TRY(x) if ((he = (x)) != hipSuccess) { (void)xfer_sync(c); cleanup(); c->err = std::string(#x) + ": " + hipGetErrorString(he); return VX_EHIP; }
#define TRYX(x) do { if (int _e = (x)) { const std::string _m = c->err; (void)xfer_sync(c); c->err = _m; cleanup(); return _e; } } while (0)
  TRY(hipMalloc((void**)&dx, (size_t)rows * ld * 4));
  TRYX(xfer_h2d(c, dx, logits, (size_t)rows * ld * 4));
  TRY(hipMalloc((void**)&dt, (size_t)rows * 4));
  TRYX(xfer_h2d(c, dt, targets, (size_t)rows * 4));
  TRY(hipMalloc((void**)&dlp, (size_t)rows_out * 4));
  TRY(hipMalloc((void**)&drk, (size_t)rows_out * 4));
  {
    const std::vector<float> ff(rows_out, VX_DEV_SENTINEL_F);
    const std::vector<int> fi(rows_out, VX_DEV_SENTINEL_I);
    TRYX(xfer_h2d(c, dlp, ff.data(), ff.size() * 4));
    TRYX(xfer_h2d(c, drk, fi.data(), fi.size() * 4));
  }
  launch_score_rows(dx, ld, rows, ncols, dt, dlp, drk, c->stream);
  TRYX(xfer_d2h(c, logp, dlp, (size_t)rows_out * 4));
  TRYX(xfer_d2h(c, rank, drk, (size_t)rows_out * 4));
  TRYX(xfer_sync(c));
  TRY(hipGetLastError());
#undef TRY
#undef TRYX
  cleanup();
  return VX_OK;
}

}  // extern "C"
