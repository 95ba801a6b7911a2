// Serving session (vx_serve_*, schedule.hip): the sampler of every decode step and of every admission's first sample.
//
// serve_sample_kernel computes exactly what dec_sample_kernel (decode.hip) computes -- split-K reduction of the predict layer's
// logits, temperature, the top-k walk with ties, the inverse-CDF draw, sum(logp), the stop rule and the fused embedding + norm1 of
// the next step -- with the same operations in the same order.  The one difference: top_k, temperature and force_eos_at are read per
// decode row from the session's row record row_smp[4 d ..] (written at admission by serve.hip serve_uniforms_kernel), not from
// launch constants, so requests with different sampling settings share one decode batch and one captured step graph.  A row sampled
// with (k, T, f) here gets the tokens, sum(logp) and next-step dh / xp that dec_sample_kernel gives it with top_k = k,
// temperature = T, force_eos_at = f.  decode.hip is pinned by the counter evidence (bench.py PMC_SOURCES), so the helpers below are
// this file's own copies of decode.hip's: the DPP wave reductions, ln_pack_row's packed-x layout and store_result's write-through
// vector store.  The draws need no splitmix64 here: the session always reads them from the row's d_uniforms column, which
// serve_uniforms_kernel fills at admission with dec_sample_kernel's counter formula (or the request's injected draws).
//
// Per-request filters (vx_request_filters, vx_serve_submit_filtered): a second row record row_flt[4 d ..] = {top_p bits, repetition
// penalty bits, repetition window, min_frames}.  A row with the neutral record (top_p >= 1, penalty == 1, min_frames <= n_gen), or a
// launch without row_flt, takes wave-uniform branches around all of it and runs the sequence above on the same values.  Otherwise, in
// this order, all fp32:
//   1. repetition penalty r over the row's own generated frames gen[max(0, n_gen - w) .. n_gen) (w = 0: all of them; the prompt does
//      not count): every token of that window, once however often it occurs, gets l > 0 ? l / r : l * r.  The window is marked in a
//      1025-bit LDS bitmap (every token range-checked before it indexes the bitmap) and applied to the LDS logit row.
//   2. min_frames m: while n_gen < m, l[EOS] = -inf (no finite logit left: the non-finite guard below samples EOS).
//   3. temperature and 4. top_k as before.
//   5. top_p: with e_i = exp(l_i - max) over the survivors of top_k, total = sum e_i and G(x) = sum of e_j over l_j > x, token i is
//      kept iff G(l_i) <= top_p * total.  On tie-free logits this is top_k_top_p_filtering's rule (models/vallex.py:811-832: sort
//      descending, drop a token when the cumulative probability of the tokens before it exceeds top_p).  DIFFERENCE: the reference's
//      unstable torch.sort splits a tie at the cut arbitrarily; here every token tied with the last kept value is kept -- the rule
//      the reference's own top-k has (`logits < kth`, :808).  The cut is found without a sort: the kept set is {l_i >= x*} for the
//      smallest x* with G(x*) <= top_p * total, and G is monotone, so 32 rounds of bisection over the order-preserving unsigned
//      image of the fp32 values find x* (one 17-value masked sum and one wave sum per round).
// Every new loop has a bound known before it starts (32 rounds; the window is at most gen_stride frames).
#include "engine_ctx.h"

namespace vxe {
namespace {

constexpr int SPL = 17;   // logits per lane: lane l owns the contiguous indices [17 l, 17 l + 17), 64 * 17 = 1088 >= 1025

// write-through vector stores (decode.hip store_result: the 5 .. 32-row chain's consumers find the result in memory)
__device__ __forceinline__ void store_wt(float* p, const f32x4& v, bool wt) {
  if (wt) asm volatile("global_store_dwordx4 %0, %1, off sc1" :: "v"(p), "v"(v) : "memory");
  else *reinterpret_cast<f32x4*>(p) = v;
}

// 64-lane reductions, the same value in every lane: DPP steps inside the 16-lane rows, row_bcast15 / row_bcast31 into row 3, lane 63
// broadcast (decode.hip wave_sum64 / wave_max64f / wave_minmax64i / wave_sum64i_fast)
__device__ __forceinline__ float sum64f(float v) {
  int x = __builtin_bit_cast(int, v);
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, true));
  x = __builtin_bit_cast(int, v);
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, true));
  x = __builtin_bit_cast(int, v);
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, x, 0x141, 0xF, 0xF, true));
  x = __builtin_bit_cast(int, v);
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, x, 0x140, 0xF, 0xF, true));
  x = __builtin_bit_cast(int, v);
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, false));
  x = __builtin_bit_cast(int, v);
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, x, 0x143, 0xC, 0xF, false));
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
__device__ __forceinline__ float max64f(float x) {
  int v = __builtin_bit_cast(int, x);
  x = fmaxf(x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, false)));
  v = __builtin_bit_cast(int, x);
  x = fmaxf(x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, false)));
  v = __builtin_bit_cast(int, x);
  x = fmaxf(x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xF, 0xF, false)));
  v = __builtin_bit_cast(int, x);
  x = fmaxf(x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xF, 0xF, false)));
  v = __builtin_bit_cast(int, x);
  x = fmaxf(x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(v, v, 0x142, 0xA, 0xF, false)));
  v = __builtin_bit_cast(int, x);
  x = fmaxf(x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(v, v, 0x143, 0xC, 0xF, false)));
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 63));
}
template <bool MAX>
__device__ __forceinline__ int minmax64i(int v) {
#define VX_MM(CTRL, RM) { const int t = __builtin_amdgcn_update_dpp(v, v, CTRL, RM, 0xF, false); v = MAX ? max(v, t) : min(v, t); }
  VX_MM(0xB1, 0xF) VX_MM(0x4E, 0xF) VX_MM(0x141, 0xF) VX_MM(0x140, 0xF) VX_MM(0x142, 0xA) VX_MM(0x143, 0xC)
#undef VX_MM
  return __builtin_amdgcn_readlane(v, 63);
}
__device__ __forceinline__ int sum64i(int x) {
  x += __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, true);
  x += __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, true);
  x += __builtin_amdgcn_update_dpp(0, x, 0x141, 0xF, 0xF, true);
  x += __builtin_amdgcn_update_dpp(0, x, 0x140, 0xF, 0xF, true);
  x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, false);
  x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xC, 0xF, false);
  return __builtin_amdgcn_readlane(x, 63);
}

// order-preserving unsigned image of an fp32 value: a < b  <=>  okey(a) < okey(b) (-0 below +0; NaNs at the ends)
__device__ __forceinline__ unsigned okey(float x) {
  const unsigned u = __builtin_bit_cast(unsigned, x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float okey_inv(unsigned k) {
  return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// c + a * b as TWO fp32 operations, the product rounded before the add -- what torch does for `emb + alpha * pe`
// (modules/embedding.py:93-97).  __fmul_rn / __fadd_rn are a plain `*` and `+` in this toolchain and contract into one fma under
// hipcc's default -ffp-contract=fast (found by tests/test_gpu_kernel_sampler.py: v_pk_fma_f32 in the sampler's fused embedding);
// the pragma keeps the two roundings.
__device__ __forceinline__ float mul_add_unfused(float a, float b, float c) {
#pragma clang fp contract(off)
  const float p = a * b;
  return c + p;
}

// LayerNorm of one 1024-wide row held as lane l's float4 columns l + 64 i, written in the packed-x image (decode.hip ln_pack_row)
__device__ __forceinline__ void ln_pack(const f32x4 (&v)[4], int b, const f32x4 (&gg)[4], const f32x4 (&be)[4], float* __restrict__ xp,
                                        bool wt) {
  const int lane = threadIdx.x;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
  const float mean = sum64f(s) * (1.0f / D_MODEL);
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) { const float d = v[i][e] - mean; q += d * d; }
  const float rstd = 1.0f / sqrtf(sum64f(q) * (1.0f / D_MODEL) + LN_EPS);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c4 = lane + 64 * i;
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (v[i][e] - mean) * rstd * gg[i][e] + be[i][e];
    store_wt(xp + (((long)(c4 >> 1) * 64) + b + 32 * (c4 & 1)) * 4, o, wt);
  }
}

// one 64-lane wave per decode row, grid = batch
template <int SK>
__global__ __launch_bounds__(64) void serve_sample_kernel(ServeSampleArgs a) {
  __shared__ float lg[64 * SPL];
  __shared__ unsigned seen[(AR_LOGITS + 31) / 32];                 // tokens of the repetition window, one bit each
  const int b = blockIdx.x, lane = threadIdx.x;
  // row state: every scalar the kernel needs, requested up front (independent loads)
  if (a.active[b] == 0) return;
  const int ngen = a.n_gen[b], pos = a.cur_pos[b], ctx = a.ctx_len[b], tlen = a.text_len[b], slot = a.slot_of[b];
  const int4 smp = *reinterpret_cast<const int4*>(a.row_smp + 4 * b);
  const int top_k = smp.x, force_eos_at = smp.z;
  const float temperature = __builtin_bit_cast(float, smp.y);
  int4 flt = make_int4(0x3F800000, 0x3F800000, 0, 0);              // neutral: top_p 1, penalty 1, window 0, min_frames 0
  if (a.row_flt) flt = *reinterpret_cast<const int4*>(a.row_flt + 4 * b);
  const float top_p = __builtin_bit_cast(float, flt.x), penalty = __builtin_bit_cast(float, flt.y);
  const int rep_window = flt.z, min_frames = flt.w;
  {
    float pp[SPL][SK];
#pragma unroll
    for (int i = 0; i < SPL; ++i) {
      const int n = lane + 64 * i, nc = n < AR_LOGITS ? n : AR_LOGITS - 1;
#pragma unroll
      for (int ks = 0; ks < SK; ++ks) pp[i][ks] = a.partial[((long)ks * MB + b) * a.npad + nc];
    }
#pragma unroll
    for (int i = 0; i < SPL; ++i) {
      const int n = lane + 64 * i;
      float t = pp[i][0];
      if (SK == 2) t = t + pp[i][1];
      if (SK == 4) t = ((t + pp[i][1]) + pp[i][2]) + pp[i][3];
      if (n >= AR_LOGITS) t = -INFINITY;
      lg[n] = t;
    }
  }
  __syncthreads();

  if (penalty != 1.0f) {                                           // wave-uniform: a neutral row reads no history
    if (lane < (AR_LOGITS + 31) / 32) seen[lane] = 0u;
    __syncthreads();
    const int hi = ngen < a.gen_stride ? ngen : a.gen_stride;      // frames this row has written: never past its gen row
    const int lo = (rep_window > 0 && rep_window < hi) ? hi - rep_window : 0;
    for (int i = lo + lane; i < hi; i += 64) {
      const int t = a.gen[(long)b * a.gen_stride + i];
      if ((unsigned)t < (unsigned)AR_LOGITS) atomicOr(&seen[t >> 5], 1u << (t & 31));
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < SPL; ++i) {
      const int n = lane + 64 * i;
      if (n < AR_LOGITS && ((seen[n >> 5] >> (n & 31)) & 1u)) {
        const float x = lg[n];
        lg[n] = x > 0.f ? x / penalty : x * penalty;
      }
    }
    __syncthreads();
  }
  if (ngen < min_frames) {                                         // wave-uniform
    if (lane == 0) lg[EOS_ID] = -INFINITY;
    __syncthreads();
  }

  // the draw and the fixed operands of the fused embedding do not depend on the logits: request them now
  const float u = a.uniforms[(long)ngen * a.uniforms_stride + b];
  f32x4 pe4[4], gg[4], be[4];
  float alpha = 0.f;
  if (a.emb_tab) {
    alpha = a.emb_alpha[0];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = (lane + 64 * i) * 4;
      pe4[i] = *reinterpret_cast<const f32x4*>(a.pe + (long)(pos + 1) * D_MODEL + c);
      gg[i] = *reinterpret_cast<const f32x4*>(a.ln_g + c);
      be[i] = *reinterpret_cast<const f32x4*>(a.ln_b + c);
    }
  }

  float v[SPL];
#pragma unroll
  for (int j = 0; j < SPL; ++j) v[j] = lg[lane * SPL + j];
  if (temperature != 1.0f) {                                       // models/vallex.py:845-846
#pragma unroll
    for (int j = 0; j < SPL; ++j) v[j] = v[j] / temperature;
  }
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < SPL; ++j) mx = fmaxf(mx, v[j]);
  mx = max64f(mx);

  if (top_k > 0 && top_k < AR_LOGITS) {                            // :803-809, ties with the k-th value are kept
    float thr = mx;
    for (int it = 1; it < top_k && thr != -INFINITY; ++it) {
      float cur = -INFINITY;
#pragma unroll
      for (int j = 0; j < SPL; ++j) if (v[j] < thr) cur = fmaxf(cur, v[j]);
      thr = max64f(cur);
    }
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < SPL; ++j) cnt += (v[j] >= thr);
    if (sum64i(cnt) != top_k) {                                    // ties (or fewer than k finite logits): exact walk
      float prev = INFINITY;
      int count = 0;
      thr = mx;
      while (true) {
        float cur = -INFINITY;
#pragma unroll
        for (int j = 0; j < SPL; ++j) if (v[j] < prev) cur = fmaxf(cur, v[j]);
        cur = max64f(cur);
        int c2 = 0;
#pragma unroll
        for (int j = 0; j < SPL; ++j) c2 += (v[j] == cur);
        count += sum64i(c2);
        thr = cur;
        if (count >= top_k || cur == -INFINITY) break;
        prev = cur;
      }
    }
#pragma unroll
    for (int j = 0; j < SPL; ++j) if (v[j] < thr) v[j] = -INFINITY;
  }
  if (top_p < 1.0f) {                                              // wave-uniform; :811-832 without the sort (header comment)
    float ep[SPL], part = 0.f;
#pragma unroll
    for (int j = 0; j < SPL; ++j) { ep[j] = expf(v[j] - mx); part += ep[j]; }
    const float budget = top_p * sum64f(part);
    // invariant: G(klo) > budget or klo is the image of -inf; G(khi) <= budget (G(max) = 0).  khi - klo < 2^32 and every round
    // halves it (rounding up), so after 32 rounds khi - klo <= 1 and khi is the image of the smallest kept value.  Every mid lies
    // between the images of -inf and of the maximum: it is the image of a number, never of a NaN.
    unsigned klo = okey(-INFINITY), khi = okey(mx);
    for (int it = 0; it < 32; ++it) {
      const unsigned mid = klo + ((khi - klo) >> 1);
      const float x = okey_inv(mid);
      float g = 0.f;
#pragma unroll
      for (int j = 0; j < SPL; ++j) g += v[j] > x ? ep[j] : 0.f;
      g = sum64f(g);
      if (g <= budget) khi = mid; else klo = mid;
    }
    const float cut = okey_inv(khi);
#pragma unroll
    for (int j = 0; j < SPL; ++j) if (v[j] < cut) v[j] = -INFINITY;
  }
  // softmax numerators (the common 1 / sum cancels in the inverse CDF)
  float e[SPL], loc = 0.f;
#pragma unroll
  for (int j = 0; j < SPL; ++j) { e[j] = expf(v[j] - mx); loc += e[j]; }
  float incl = loc;                                                // inclusive scan over lanes
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  const float total = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, incl), 63));
  const float thresh = u * total;
  float c = incl - loc;
  int cand = 0x7fffffff, lastnz = -1;
#pragma unroll
  for (int j = 0; j < SPL; ++j) {
    if (e[j] > 0.f) {
      c += e[j];
      lastnz = lane * SPL + j;
      if (c > thresh && cand == 0x7fffffff) cand = lane * SPL + j;
    }
  }
  cand = minmax64i<false>(cand);
  const int last_all = minmax64i<true>(lastnz);
  int tok = cand == 0x7fffffff ? last_all : cand;
  if ((unsigned)tok > (unsigned)EOS_ID) tok = EOS_ID;             // non-finite logits (an f16x2 admission that is re-run in fp32)

  // log-prob of the pick under the filtered distribution (models/vallex.py:851-852), for the beam selection
  if (tok / SPL == lane) {
    float vt = 0.f;
#pragma unroll
    for (int j = 0; j < SPL; ++j) if (tok - lane * SPL == j) vt = v[j];
    a.sum_logp[b] += (vt - mx) - logf(total);
  }

  if (force_eos_at >= 0 && ngen >= force_eos_at) tok = EOS_ID;
  // stop test: EOS, or (y_len - prompt_len) > 16 * text_len (models/vallex.py:575-578), or the arena cap
  const bool stop = tok == EOS_ID || (1 + ngen) > 16 * tlen || ngen >= a.gen_stride;
  if (lane == 0) {
    if (stop) {
      a.active[b] = 0;
      a.slot_meta[4 * slot + 2] = 0;
      atomicSub(a.n_active, 1);
    } else {
      a.gen[(long)b * a.gen_stride + ngen] = tok;
      a.n_gen[b] = ngen + 1;
      a.cur_tok[b] = tok;
      a.cur_pos[b] = pos + 1;
      a.ctx_len[b] = ctx + 1;
      a.slot_meta[4 * slot + 1] = ctx + 1;
    }
  }
  if (stop || !a.emb_tab) return;
  // start of the next step for this row: h = emb[tok] + alpha * pe[pos + 1]; xp = pack(LN(h))
  f32x4 hv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int cc = (lane + 64 * i) * 4;
    hv[i] = *reinterpret_cast<const f32x4*>(a.emb_tab + (long)tok * D_MODEL + cc);
#pragma unroll
    for (int q = 0; q < 4; ++q) hv[i][q] = mul_add_unfused(alpha, pe4[i][q], hv[i][q]);
    store_wt(a.emb_h + (long)b * D_MODEL + cc, hv[i], a.wt != 0);
  }
  ln_pack(hv, b, gg, be, a.emb_xp, a.wt != 0);
}

}  // namespace

bool launch_serve_sample(const ServeSampleArgs& a, hipStream_t s) {
  if (a.splitk == 4) hipLaunchKernelGGL(serve_sample_kernel<4>, dim3(a.batch), dim3(64), 0, s, a);
  else if (a.splitk == 2) hipLaunchKernelGGL(serve_sample_kernel<2>, dim3(a.batch), dim3(64), 0, s, a);
  else if (a.splitk == 1) hipLaunchKernelGGL(serve_sample_kernel<1>, dim3(a.batch), dim3(64), 0, s, a);
  else return false;                       // split-K factor of the predict layer not compiled in
  return true;
}

}  // namespace vxe
