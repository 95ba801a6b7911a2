// A true-peak look-ahead limiter (vx_limit, vx_finish_limited, include/vallex_hip.h) of mono fp32 rows on the device.
//
//   limit    limit_rows_kernel: a tile of LM_T outputs of one part stages y (the sample, 0 if it is not finite, 0 outside the row) over
//            T + 4 Wn + 14 samples into LDS, then, with a barrier between the stages and everything in LDS:
//              detector  P = (float) max(|y|, |d_0|, .., |d_{n-1}|) over T + 4 Wn positions, d_p = the 15-tap sum of the resampler's
//                        (1, n) table in double in tap order; the demand q = floor(min(1, c / (P gs)) 2^24), 2^24 outside the row
//              hold      m = the minimum of q over 2 Wn + 1 positions, over T + 2 Wn positions, by doubling (windows of 1, 2, 4, ..)
//              smooth    s = the sum of m over 2 Wn + 1 positions, from a 64-bit prefix sum
//              output    g = (float)((double)s / (N 2^24)), out = (y gs) g
//            and writes one record per tile {max P, min g, #(g < 1), non-finite samples} over the tile's own outputs.
//
// Arithmetic (the contract the tests rest on): q, m and s are integers, so no decomposition, tile, window or launch can change a bit
// of g; P and out are functions of the 15 samples around an element and of g.  No atomics, no inline assembly.
//
// Work decomposition: a launch covers a ragged list of PARTS (outputs [s, s + cnt) of one row with up to 2 Wn + 7 real samples on
// either side: limit_host.h, lm_plan), grid (tile, part), 256 threads.  Loads and stores are lane-contiguous.  Two instances: Wn up to
// 128 (50 KiB of LDS, three workgroups per CU) and up to 1024 (106 KiB, one); static LDS, so neither needs a launch attribute.
#include "wave_stage.h"
#include "limit_host.h"

#include "../../include/vallex_hip_dev.h"

namespace vxe {

constexpr int LM_T = 2048;                 // outputs of a tile
constexpr int LM_W_SMALL = 128;            // lookahead of the small instance
constexpr long LM_REC_CAP = RS_IN_CAP / LM_T + RS_MAX_JOBS;       // tile records of a launch: one per LM_T outputs plus a cut one per part
static_assert(VX_LIMIT_WINDOW == RS_IN_CAP, "vx_limit runs in the resampler's launch buffers");
static_assert(RS_OUT_CAP >= 2 * RS_IN_CAP, "the limited samples of a resident call sit in the upper half of rs_out");
static_assert(VX_DEV_LIMIT_WINDOW_MIN >= 2 * (2 * LM_LOOKAHEAD_MAX + LM_WIDTH) + 1 && VX_DEV_LIMIT_WINDOW_MIN <= VX_LIMIT_WINDOW,
              "window bounds of the dev header");

struct LmRec { float peak, min_gain; int reduced, nonfinite; };
static_assert(sizeof(LmRec) == 16, "the kernel writes 16-byte tile records");

// tab [nparts][RS_TAB]: {in_off, hl, cnt, hr, out_off, rec_off, pre_gain bits}: the part's outputs are the samples in[in_off + hl .. in_off + hl + cnt),
// the hl samples in front and the hr behind are real samples of the row; whatever lies outside in[in_off .. in_off + hl + cnt + hr) and
// within 2 Wn + 7 of an output lies outside the row.  Output e -> out / Pout / gout [out_off + e] (each may be NULL), tile t ->
// rec[rec_off + t].  measure: detector only, over the tile's own outputs.  kd [n][15]: the taps, widened.
template <int WMAX>
__global__ __launch_bounds__(256) void limit_rows_kernel(const float* __restrict__ in, const int* __restrict__ tab, const double* __restrict__ kd,
                                                         float* __restrict__ out, float* __restrict__ Pout, float* __restrict__ gout,
                                                         LmRec* __restrict__ rec, int n, int Wn, float c, int measure) {
  constexpr int NQ = LM_T + 4 * WMAX, NY = NQ + 2 * LM_WIDTH, NM = LM_T + 2 * WMAX;
  __shared__ float ys[NY];
  __shared__ int qa[NQ], qb[NQ];
  __shared__ long long cs[NM + 1];
  __shared__ long long part[256];
  const int* tb = tab + blockIdx.y * RS_TAB;
  const int cnt = tb[2], e0 = blockIdx.x * LM_T;
  if (e0 >= cnt) return;                                           // block-uniform
  const long in_off = tb[0], out_off = tb[4];
  const int hl = tb[1], have = hl + cnt + tb[3], rec_off = tb[5];
  const float gs = __int_as_float(tb[6]);
  const int tid = threadIdx.x, tc = cnt - e0 < LM_T ? cnt - e0 : LM_T;
  const int H = measure ? 0 : 2 * Wn, N = 2 * Wn + 1;
  const int nq = tc + 2 * H, ny = nq + 2 * LM_WIDTH;
  float peak = 0.f, ming = 1.f;
  int reduced = 0, bad = 0;
  // stage: ys[u] = y of part position e0 + u - H - 7
  for (int u = tid; u < ny; u += 256) {
    const int b = hl + e0 + u - H - LM_WIDTH;
    const float x = b >= 0 && b < have ? in[in_off + b] : 0.f;
    const bool fin = (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u;
    const int own = u - H - LM_WIDTH;
    bad += !fin && own >= 0 && own < tc ? 1 : 0;
    ys[u] = fin ? x : 0.f;
  }
  __syncthreads();
  // detector and demand: qa[v] of part position e0 + v - H
  for (int v = tid; v < nq; v += 256) {
    const int b = hl + e0 + v - H;
    int q = 1 << 24;
    if (b >= 0 && b < have) {
      float yv[LM_K];
#pragma unroll
      for (int j = 0; j < LM_K; ++j) yv[j] = ys[v + j];
      double top = fabs((double)yv[LM_WIDTH]);
      for (int p = 0; p < n; ++p) {
        const double* kp = kd + p * LM_K;
        double d = 0.0;
#pragma unroll
        for (int j = 0; j < LM_K; ++j) d += kp[j] * (double)yv[j];  // the product is exact in double: an fma gives the same bits
        top = fmax(top, fabs(d));
      }
      const float P = (float)top;
      if (!measure) {
        const double den = (double)P * (double)gs;
        const double r = den > (double)c ? (double)c / den : 1.0;
        q = (int)(long long)floor(r * 16777216.0);
      }
      const int own = v - H;
      if (own >= 0 && own < tc) {
        peak = fmaxf(peak, P);
        if (Pout) Pout[out_off + e0 + own] = P;
      }
    }
    qa[v] = q;
  }
  if (!measure) {
    __syncthreads();
    // hold: minima of windows of w = 1, 2, 4, .. positions, then two overlapping windows of the largest w <= N cover N positions
    int* src = qa;
    int* dst = qb;
    int w = 1;
    for (; 2 * w <= N; w *= 2) {
      const int len = nq - 2 * w + 1;
      for (int i = tid; i < len; i += 256) dst[i] = min(src[i], src[i + w]);
      __syncthreads();
      int* t = src; src = dst; dst = t;
    }
    const int nm = tc + 2 * Wn;                                    // dst[i] = m of part position e0 + i - Wn
    for (int i = tid; i < nm; i += 256) dst[i] = min(src[i], src[i + N - w]);
    __syncthreads();
    // smooth: cs[j] = the sum of m over [0, j)
    const int C = (nm + 255) / 256, j0 = tid * C < nm ? tid * C : nm, j1 = j0 + C < nm ? j0 + C : nm;
    long long mine = 0;
    for (int j = j0; j < j1; ++j) mine += dst[j];
    part[tid] = mine;
    __syncthreads();
    for (int d = 1; d < 256; d *= 2) {
      const long long add = tid >= d ? part[tid - d] : 0;
      __syncthreads();
      part[tid] += add;
      __syncthreads();
    }
    long long run = part[tid] - mine;
    for (int j = j0; j < j1; ++j) {
      cs[j] = run;
      run += dst[j];
    }
    if (tid == 255) cs[nm] = part[255];
    __syncthreads();
    const double den = (double)((long long)N << 24);
    for (int e = tid; e < tc; e += 256) {
      const long long s = cs[e + N] - cs[e];
      const float g = (float)((double)s / den);
      const float v = ys[e + H + LM_WIDTH] * gs;
      if (out) out[out_off + e0 + e] = v * g;
      if (gout) gout[out_off + e0 + e] = g;
      ming = fminf(ming, g);
      reduced += g < 1.f ? 1 : 0;
    }
  }
  // the tile's record, reduced in the prefix sums' LDS
  __syncthreads();
  float* red_p = reinterpret_cast<float*>(cs);
  float* red_g = red_p + 256;
  int* red_r = reinterpret_cast<int*>(red_p + 512);
  int* red_z = red_r + 256;
  red_p[tid] = peak; red_g[tid] = ming; red_r[tid] = reduced; red_z[tid] = bad;
  __syncthreads();
  for (int d = 128; d > 0; d /= 2) {
    if (tid < d) {
      red_p[tid] = fmaxf(red_p[tid], red_p[tid + d]);
      red_g[tid] = fminf(red_g[tid], red_g[tid + d]);
      red_r[tid] += red_r[tid + d];
      red_z[tid] += red_z[tid + d];
    }
    __syncthreads();
  }
  if (tid == 0) {
    LmRec r;
    r.peak = red_p[0]; r.min_gain = red_g[0]; r.reduced = red_r[0]; r.nonfinite = red_z[0];
    rec[rec_off + blockIdx.x] = r;
  }
}

// (lm_buffers, lm_run and lm_check: wave_stage.h)
int lm_buffers(vx_ctx* c, int n) {
  if (int e = rs_buffers(c)) return e;
  if (!c->lm_rec) {
    if (int e = dev_alloc(c, &c->lm_rec, (size_t)LM_REC_CAP * 4, false)) return e;
    if (int e = dev_alloc(c, &c->lm_taps, (size_t)LM_OVERSAMPLE_MAX * LM_K, true)) return e;
  }
  if (n > 1 && c->lm_taps_n != n) {
    std::vector<float> t;
    lm_taps(n, t);
    std::vector<double> td(t.begin(), t.end());
    H2D(c->lm_taps, td.data(), td.size() * sizeof(double));
    c->lm_taps_n = n;
  }
  return VX_OK;
}

// The limiter over rows of len[i] samples.  src[i]: the row on the host; resident: the rows already lie in rs_in, row i's sample 0 at
// rs_in + base[i], nothing is uploaded and one launch takes all of them.  dst / dP / dG (each may be NULL): host rows that receive out,
// P and g.  keep (with resident): the limited samples stay on the device, row i's at rs_out + kept[i].  Neither dst, keep nor dG: the
// detector alone runs (peak, nonfinite).
int lm_run(vx_ctx* c, const char* who, const float* const* src, const long* len, int batch, const float* gs, float cc, int Wn, int n, bool resident,
           const std::vector<long>& base, float* const* dst, float* const* dP, float* const* dG, bool keep, std::vector<long>* kept,
           vx_limit_info* info) {
  for (int i = 0; i < batch; ++i) info[i] = {0.f, 1.f, cc, 0, 0};
  if (kept) kept->assign((size_t)batch, 0);
  std::vector<LmJob> jobs;
  const long win = resident ? (long)RS_IN_CAP : wave_window(c->lm_window, VX_LIMIT_WINDOW);
  if (!lm_plan(len, batch, Wn, win, RS_MAX_JOBS, LM_T, &jobs))
    FAIL(VX_EINVAL, "%s: the launch window of %ld samples (vx_dev_limit_window) cannot hold two halos of 2 lookahead + 7 = %ld samples plus one sample",
         who, win, lm_halo(Wn));
  if (resident && !jobs.empty() && jobs.back().launch != 0) FAIL(VX_EINVAL, "%s: resident rows exceed one launch", who);      // the frames pass rules it out
  const bool measure = !(dst || keep || dG);
  float* d_out = keep ? c->rs_out + RS_IN_CAP : dst ? c->rs_out : nullptr;
  float* d_P = dP ? c->rs_out : nullptr;                           // the development entry has no dst: P and g take the two halves
  float* d_g = dG ? c->rs_out + RS_IN_CAP : nullptr;
  LmRec* d_rec = reinterpret_cast<LmRec*>(c->lm_rec);
  std::vector<int> tab;
  std::vector<LmRec> recs;
  return wave_launches(c, jobs, [&](size_t j0, size_t j1) -> int {
    tab.clear();
    long max_cnt = 0, nrec = 0;
    for (size_t q = j0; q < j1; ++q) {
      const LmJob& j = jobs[q];
      const long in_off = resident ? base[(size_t)j.row] + j.s - j.hl : j.off;
      int gbits;
      memcpy(&gbits, &gs[j.row], sizeof gbits);
      for (long v : {in_off, j.hl, j.cnt, j.hr, j.out_off, j.rec_off, (long)gbits, 0L}) tab.push_back((int)v);
      max_cnt = std::max(max_cnt, j.cnt);
      nrec = j.rec_off + (j.cnt + LM_T - 1) / LM_T;
      if (!resident) H2D(c->rs_in + j.off, src[j.row] + j.s - j.hl, (size_t)(j.hl + j.cnt + j.hr) * sizeof(float));
      if (keep && j.s == 0) (*kept)[(size_t)j.row] = RS_IN_CAP + j.out_off;
    }
    if (nrec > LM_REC_CAP) FAIL(VX_EINVAL, "%s: %ld tiles in one launch exceed the record table of %ld", who, nrec, LM_REC_CAP);   // the window rules it out
    H2D(c->rs_meta, tab.data(), tab.size() * sizeof(int));
    const dim3 grid((unsigned)((max_cnt + LM_T - 1) / LM_T), (unsigned)(j1 - j0));
    if (Wn <= LM_W_SMALL)
      hipLaunchKernelGGL(limit_rows_kernel<LM_W_SMALL>, grid, dim3(256), 0, c->stream, c->rs_in, c->rs_meta, c->lm_taps, d_out, d_P, d_g, d_rec,
                         n > 1 ? n : 0, Wn, cc, measure ? 1 : 0);
    else
      hipLaunchKernelGGL(limit_rows_kernel<LM_LOOKAHEAD_MAX>, grid, dim3(256), 0, c->stream, c->rs_in, c->rs_meta, c->lm_taps, d_out, d_P, d_g, d_rec,
                         n > 1 ? n : 0, Wn, cc, measure ? 1 : 0);
    for (size_t q = j0; q < j1; ++q) {
      const LmJob& j = jobs[q];
      if (dst && !keep) D2H(dst[j.row] + j.s, c->rs_out + j.out_off, (size_t)j.cnt * sizeof(float));
      if (dP) D2H(dP[j.row] + j.s, d_P + j.out_off, (size_t)j.cnt * sizeof(float));
      if (dG) D2H(dG[j.row] + j.s, d_g + j.out_off, (size_t)j.cnt * sizeof(float));
    }
    recs.resize((size_t)nrec);
    D2H(recs.data(), d_rec, (size_t)nrec * sizeof(LmRec));
    return VX_OK;
  }, [&](size_t j0, size_t j1) -> int {
    for (size_t q = j0; q < j1; ++q) {
      const LmJob& j = jobs[q];
      vx_limit_info& w = info[j.row];
      for (long t = 0; t < (j.cnt + LM_T - 1) / LM_T; ++t) {
        const LmRec& r = recs[(size_t)(j.rec_off + t)];
        w.peak = std::max(w.peak, r.peak);
        w.min_gain = std::min(w.min_gain, r.min_gain);
        w.reduced += r.reduced;
        w.nonfinite += r.nonfinite;
      }
    }
    return VX_OK;
  });
}

int lm_check(vx_ctx* c, const char* who, const vx_limit_opts* o, float pre_gain, float ceiling_db) {
  if (!o) FAIL(VX_EINVAL, "%s: the vx_limit_opts pointer is NULL", who);
  CHECK_STRUCT_OF(who, *o, vx_limit_opts);
  char why[160];
  if (lm_check_opts(*o, pre_gain, ceiling_db, why, sizeof why)) FAIL(VX_EINVAL, "%s: %s", who, why);
  return VX_OK;
}

}  // namespace vxe

extern "C" {

int vx_limit_taps(int32_t oversample, float* taps) {
  using namespace vxe;
  std::vector<float> t;
  if (!taps || !lm_taps(oversample, t)) return VX_EINVAL;
  for (size_t i = 0; i < t.size(); ++i) taps[i] = t[i];
  return VX_OK;
}

int vx_limit(vx_ctx* c, const float* wav, int64_t wav_stride, const int32_t* lens, int32_t batch, float pre_gain, float ceiling_db,
             const vx_limit_opts* o, float* out, int64_t out_stride, vx_limit_info* info) {
  using namespace vxe;
  if (!c) return VX_EINVAL;
  if (int e = wave_check_rows(c, "vx_limit", wav, wav_stride, lens, batch)) return e;
  if (!o) FAIL(VX_EINVAL, "vx_limit: o is NULL");
  if (!info) FAIL(VX_EINVAL, "vx_limit: info is NULL");
  if (int e = lm_check(c, "vx_limit", o, pre_gain, ceiling_db)) return e;
  if (out)
    if (int e = wave_check_out_stride(c, "vx_limit", lens, batch, out_stride, "")) return e;
  HIPCHK(hipSetDevice(c->dev));
  if (int e = lm_buffers(c, o->oversample)) return e;
  std::vector<const float*> src((size_t)batch);
  std::vector<float*> dst((size_t)batch);
  std::vector<long> len((size_t)batch), base;
  for (int i = 0; i < batch; ++i) {
    src[(size_t)i] = wav + (long)i * wav_stride;
    dst[(size_t)i] = out ? out + (long)i * out_stride : nullptr;
    len[(size_t)i] = lens[i];
  }
  std::vector<vx_limit_info> w((size_t)batch);
  const std::vector<float> gs((size_t)batch, pre_gain);
  if (int e = lm_run(c, "vx_limit", src.data(), len.data(), batch, gs.data(), lm_ceiling(ceiling_db), o->lookahead, o->oversample, false, base,
                     out ? dst.data() : nullptr, nullptr, nullptr, false, nullptr, w.data()))
    return e;
  for (int i = 0; i < batch; ++i) info[i] = w[(size_t)i];
  return VX_OK;
}

int vx_finish_limited(vx_ctx* c, const float* wav, int64_t wav_stride, const int32_t* lens, int32_t batch, const vx_finish_opts* o,
                      const vx_loudness_opts* lo_, const vx_limit_opts* lim, void* out, int64_t out_stride, int32_t* out_lens,
                      vx_wave_info* info, vx_loudness_info* linfo, vx_limit_info* liminfo) {
  using namespace vxe;
  if (!c) return VX_EINVAL;
  if (int e = wave_check_rows(c, "vx_finish_limited", wav, wav_stride, lens, batch)) return e;
  if (!o) FAIL(VX_EINVAL, "vx_finish_limited: o is NULL");
  if (!lo_) FAIL(VX_EINVAL, "vx_finish_limited: lo is NULL");
  if (!lim) FAIL(VX_EINVAL, "vx_finish_limited: lim is NULL");
  if (!info) FAIL(VX_EINVAL, "vx_finish_limited: info is NULL");
  if (!linfo) FAIL(VX_EINVAL, "vx_finish_limited: linfo is NULL");
  if (!liminfo) FAIL(VX_EINVAL, "vx_finish_limited: liminfo is NULL");
  if (out && !out_lens) FAIL(VX_EINVAL, "vx_finish_limited: out is given without out_lens");
  return fn_pipeline(c, "vx_finish_limited", wav, wav_stride, lens, batch, *o, lo_, lim, out, out_stride, out_lens, info, linfo, liminfo);
}

int vx_dev_limit_gain(vx_ctx* c, const float* wav, int32_t len, float pre_gain, float ceiling_db, const vx_limit_opts* o, float* P, float* g) {
  using namespace vxe;
  if (!c) return VX_EINVAL;
  if (!wav) FAIL(VX_EINVAL, "vx_dev_limit_gain: wav is NULL");
  if (!P || !g) FAIL(VX_EINVAL, "vx_dev_limit_gain: P or g is NULL");
  if (len < 0) FAIL(VX_EINVAL, "vx_dev_limit_gain: len %d below 0", len);
  if (int e = lm_check(c, "vx_dev_limit_gain", o, pre_gain, ceiling_db)) return e;
  HIPCHK(hipSetDevice(c->dev));
  if (int e = lm_buffers(c, o->oversample)) return e;
  const long L = len;
  std::vector<long> base;
  vx_limit_info w;
  return lm_run(c, "vx_dev_limit_gain", &wav, &L, 1, &pre_gain, lm_ceiling(ceiling_db), o->lookahead, o->oversample, false, base, nullptr, &P, &g,
                false, nullptr, &w);
}

int vx_dev_limit_window(vx_ctx* c, int32_t samples) {
  return vxe::wave_set_window(c, &vx_ctx::lm_window, "vx_dev_limit_window", "samples", samples, VX_DEV_LIMIT_WINDOW_MIN, VX_LIMIT_WINDOW);
}

}  // extern "C"
