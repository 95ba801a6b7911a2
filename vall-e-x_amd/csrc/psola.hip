// The formant-preserving pitch shift (vx_psola, include/vallex_hip.h): time-domain PSOLA of mono fp32 rows from vx_f0's lags.
//
// Two kernels with plain host code between them.  psola_marks_kernel walks a row's analysis marks: from mark a_i with period P it
// searches the next mark in [a_i + P - D, a_i + P + D], D = P / 8, for the smallest e_d - 2 c_d against the template y[a_i, a_i + P).
// The host (psola_host.h: ps_grains) turns the marks into the synthesis marks and the grain table (s, a, Wl, Wr) in integers.
// psola_synth_kernel writes the output: every sample is the weighted mean of the grains that cover it.  The contract -- sums, tie
// rule, weights, every rounding -- is in the header; psola_host.h has the integers and a sequential reference.
//
// Arithmetic (the contract the tests rest on): candidate d is summed by ONE lane in double in sample order from 0.0, every product of
// two fp32 values is exact in double, the winner is a total order on (cost, |d|, d); an output sample is ONE lane's walk over its
// grains in order of j, an exact product and one addition each, and one division.  Contraction is off for the whole file.  The bits
// therefore depend neither on the lane, the workgroup, the tile, the window nor the launch a row lands in.  No atomics, no inline
// assembly.
//
// Work decomposition.  Marks: mark i + 1 needs mark i, so a row is a serial walk: one 256-thread workgroup per row, the rows of a
// launch side by side on different CUs.  The template and the search region y[a + P - D, a + 2P + D) are widened once to double in
// LDS (zeros outside the row and in place of non-finite samples); candidate c = d + D belongs to lane c mod 256 (at most 257
// candidates), the lanes read reg[c + j] at stride 1 and t[j] as a broadcast; the order and the reduction of the lanes' winners are
// ws_walk.h's.  LDS: 8 + 2 period_max + 2 (period_max / 8) doubles -- 18 496 bytes at the largest options, 7.1 KiB at period_max 400.
// Synthesis: a workgroup writes one tile of PS_TILE outputs of one row, four per lane.  The grains are sorted by s_j and none is
// wider than Wmax = period_max + period_max / 8 on either side, so the tile's grains are the run with s_j in
// (n0 - Wmax, n1 - 1 + Wmax], found by two bisections; they pass through LDS in chunks of 256 records and every lane walks them in
// order.  The source samples are read through L2 (a grain's source lies within 2 Wmax of the tile: the reads of a tile stay in a
// window of a few KiB).
#include "wave_stage.h"
#include "psola_host.h"
#include "ws_walk.h"

#include "../../include/vallex_hip_dev.h"

#pragma clang fp contract(off)

namespace vxe {

constexpr int PS_TAB = 16;                                   // ints of a job record
constexpr int PS_MAX_JOBS = RS_MAX_JOBS * RS_TAB / PS_TAB;   // the records of a launch fill rs_meta
constexpr int PS_TILE = 1024;                                // outputs of a synthesis workgroup
constexpr int PS_CHUNK = 256;                                // grain records in LDS at a time
// rs_out, in words: [0, RS_IN_CAP) the output samples, then the lags, the marks, the mark costs (doubles), the mark counts of the
// jobs and the grain table (four ints a record)
constexpr long PS_LAG_AT = RS_IN_CAP, PS_LAG_CAP = RS_IN_CAP / PS_HOP_MIN + PS_MAX_JOBS;
constexpr long PS_MARK_AT = PS_LAG_AT + PS_LAG_CAP, PS_MARK_CAP = RS_IN_CAP / PS_STEP_MIN + 2 * PS_MAX_JOBS + 2;
constexpr long PS_COST_AT = PS_MARK_AT + PS_MARK_CAP;
constexpr long PS_CNT_AT = PS_COST_AT + 2 * PS_MARK_CAP;
constexpr long PS_GRAIN_AT = PS_CNT_AT + PS_MAX_JOBS, PS_GRAIN_CAP = RS_IN_CAP / PS_GRAIN_STEP_MIN + 2 * PS_MAX_JOBS + 2;
static_assert(VX_PSOLA_WINDOW == RS_IN_CAP, "vx_psola runs in the resampler's launch buffers");
static_assert(VX_DEV_PSOLA_WINDOW_MIN >= 16 && VX_DEV_PSOLA_WINDOW_MIN <= VX_PSOLA_WINDOW, "window bounds of the dev header");
static_assert(PS_COST_AT % 2 == 0 && PS_GRAIN_AT % 4 == 0, "the cost table is 8-byte and the grain table 16-byte aligned");
static_assert(PS_GRAIN_AT + 4 * PS_GRAIN_CAP <= RS_OUT_CAP, "the tables fit behind the output samples");
static_assert(PS_STEP_MIN == 14 && PS_GRAIN_STEP_MIN == 7, "the bounds the dev header promises");
static_assert((8 + 2 * PS_PERIOD_MAX + 2 * (PS_PERIOD_MAX / 8)) * sizeof(double) <= 65536, "LDS of the largest options");
static_assert(sizeof(PsGrain) == 16, "a grain record is four ints");

// tab [njobs][PS_TAB]:
//   0 in_off   first float of the row in `in` (and of its outputs in `out`);  1 L  samples of the row
//   2 lag_off  first lag of the row;  3 Mf  its lags;  4 m_off  first mark (and cost) of the row;  5 m_cap  room for its marks
//   6 g_off    first grain record of the row;  7 J  its grains;  8 b_off  first synthesis workgroup of the row
__global__ __launch_bounds__(256) void psola_marks_kernel(const float* __restrict__ in, const int* __restrict__ tab,
                                                          const int* __restrict__ lag, int* __restrict__ marks, double* __restrict__ cost,
                                                          int* __restrict__ cnt, PsGeom g) {
  extern __shared__ double ps_lds[];
  double* redC = ps_lds;                                         // [4] the wavefronts' winners
  int* redd = reinterpret_cast<int*>(ps_lds + 4);                // [4]
  double* t = ps_lds + 8;                                        // [period_max] the template
  double* reg = t + g.pmax;                                      // [period_max + 2 (period_max / 8)] the search region
  const int* tb = tab + blockIdx.x * PS_TAB;
  const long in_off = tb[0], L = tb[1], Mf = tb[3], m_off = tb[4];
  const int m_cap = tb[5], tid = threadIdx.x;
  const int* lg = lag + tb[2];
  auto y_at = [&](long s) -> double { return s >= 0 && s < L ? (double)ws_clean(in[in_off + s]) : 0.0; };
  long a = 0;
  int i = 0;
  for (;;) {                                                     // a and i are the same in every lane
    if (tid == 0) marks[m_off + i] = (int)a;
    if (a >= L || i + 1 >= m_cap) break;                         // the second never holds (psola_host.h: ps_mark_bound)
    bool voiced;
    const int P = ps_period(g, lg, Mf, a, &voiced);
    if (!voiced) {
      if (tid == 0) cost[m_off + i] = 0.0;
      a += g.U;
      ++i;
      continue;
    }
    const int D = P / 8, R = P + 2 * D, ncand = 2 * D + 1;
    __syncthreads();                                             // nobody reads t, reg or red* of the previous mark any more
    for (int j = tid; j < P; j += 256) t[j] = y_at(a + j);
    for (int j = tid; j < R; j += 256) reg[j] = y_at(a + P - D + j);
    __syncthreads();
    double bC = __builtin_inf();
    int bd = WS_NONE;
    for (int cd = tid; cd < ncand; cd += 256) {
      const double* rp = reg + cd;
      double cs = 0.0, es = 0.0;
#pragma unroll 8
      for (int j = 0; j < P; ++j) {
        const double p = rp[j];
        cs = cs + p * t[j];                                      // both products are exact in double
        es = es + p * p;
      }
      const double Cd = es - 2.0 * cs;                           // 2 c is exact
      if (ws_better(Cd, cd - D, bC, bd)) { bC = Cd; bd = cd - D; }
    }
    const WsWin win = ws_reduce(bC, bd, redC, redd, [] {});
    if (tid == 0) cost[m_off + i] = win.D;
    a += P + win.d;
    ++i;
  }
  if (tid == 0) { cost[m_off + i] = 0.0; cnt[blockIdx.x] = i; }
}

__global__ __launch_bounds__(256) void psola_synth_kernel(const float* __restrict__ in, const int* __restrict__ tab, int njobs,
                                                          const PsGrain* __restrict__ grains, float* __restrict__ out, int Wmax) {
  __shared__ PsGrain gl[PS_CHUNK];
  const int tid = threadIdx.x;
  int jl = 0, jh = njobs - 1;                                    // the row of this workgroup: the last one with b_off <= blockIdx.x
  while (jl < jh) {
    const int m = (jl + jh + 1) >> 1;
    if (tab[m * PS_TAB + 8] <= (int)blockIdx.x) jl = m; else jh = m - 1;
  }
  const int* tb = tab + jl * PS_TAB;
  const long in_off = tb[0], L = tb[1];
  const int J = tb[7];
  const PsGrain* gr = grains + tb[6];
  const long n0 = (long)((int)blockIdx.x - tb[8]) * PS_TILE, n1 = n0 + PS_TILE < L ? n0 + PS_TILE : L;
  auto first_above = [&](long s) {                               // the first grain with s_j > s
    int lo = 0, hi = J;
    while (lo < hi) {
      const int m = (lo + hi) >> 1;
      if (gr[m].s > s) hi = m; else lo = m + 1;
    }
    return lo;
  };
  const int j0 = first_above(n0 - Wmax), j1 = first_above(n1 - 1 + Wmax);
  double num[4] = {0.0, 0.0, 0.0, 0.0}, den[4] = {0.0, 0.0, 0.0, 0.0};
  for (int c0 = j0; c0 < j1; c0 += PS_CHUNK) {                   // block-uniform
    __syncthreads();
    if (c0 + tid < j1) gl[tid] = gr[c0 + tid];
    __syncthreads();
    const int cn = j1 - c0 < PS_CHUNK ? j1 - c0 : PS_CHUNK;
    for (int q = 0; q < cn; ++q) {
      const PsGrain G = gl[q];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long n = n0 + tid + 256 * u;
        const long rr = n - G.s;
        if (n < n1 && rr >= -(long)G.Wl && rr < G.Wr) {
          const float w = ps_weight((int)rr, G.Wl, G.Wr);
          const long src = G.a + rr;
          const float yv = src >= 0 && src < L ? ws_clean(in[in_off + src]) : 0.f;
          num[u] = num[u] + (double)yv * (double)w;
          den[u] = den[u] + (double)w;
        }
      }
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const long n = n0 + tid + 256 * u;
    if (n < n1) out[in_off + n] = den[u] > 0.0 ? (float)(num[u] / den[u]) : 0.f;
  }
}

// every check of vx_psola behind the pointers and before the walk: options, lengths, strides, ratios
static int ps_check(vx_ctx* c, const char* who, const int32_t* lens, int batch, int64_t lag_stride, const int32_t* ratio,
                    const vx_psola_opts* o, int64_t out_stride, PsGeom* g) {
  CHECK_STRUCT(*o, vx_psola_opts);
  char why[160];
  if (ps_check_opts(*o, why, sizeof why)) FAIL(VX_EINVAL, "%s: %s", who, why);
  *g = ps_geometry(*o);
  const long win = wave_window(c->ps_window, VX_PSOLA_WINDOW);
  for (int i = 0; i < batch; ++i) {
    const long L = lens[i];
    if (L > win) FAIL(VX_EINVAL, "%s: lens[%d] = %ld above the window of %ld samples (VX_PSOLA_WINDOW): a row is not cut", who, i, L, win);
    const long Mf = ps_frames(*g, L);
    if (Mf > lag_stride) FAIL(VX_EINVAL, "%s: lag_stride %ld below the %ld frames of row %d", who, (long)lag_stride, Mf, i);
    if (ratio)
      for (long k = 0; k < Mf; ++k) {
        const int r = ratio[(long)i * lag_stride + k];
        if (r < PS_RATIO_MIN || r > PS_RATIO_MAX)
          FAIL(VX_EINVAL, "%s: ratio[%d][%ld] = %d outside %d .. %d", who, i, k, r, PS_RATIO_MIN, PS_RATIO_MAX);
      }
  }
  return wave_check_out_stride(c, who, lens, batch, out_stride, "");
}

// The general path.  First every launch's mark walk, so that N of every row is known before anything reaches the caller; then the
// grain tables on the host; then every launch's synthesis.  With one launch the staged samples stay where they are in between.
// cost / gtab: one row only (vx_dev_psola_table).
static int ps_run(vx_ctx* c, const char* who, const float* wav, int64_t wav_stride, const int32_t* lens, int batch, const int32_t* lag,
                  int64_t lag_stride, const int32_t* ratio, const PsGeom& g, float* out, int64_t out_stride, int32_t* marks,
                  int64_t marks_stride, vx_psola_info* info, double* cost, long cost_cap, int32_t* gtab, long gtab_cap) {
  const long win = wave_window(c->ps_window, VX_PSOLA_WINDOW);
  std::vector<PsJob> jobs;
  if (!ps_plan(g, lens, batch, win, PS_MARK_CAP, PS_GRAIN_CAP, PS_LAG_CAP, PS_MAX_JOBS, &jobs))
    FAIL(VX_EINVAL, "%s: a row in lens is above the window of %ld samples (vx_dev_psola_window)", who, win);
  HIPCHK(hipSetDevice(c->dev));
  if (int e = rs_buffers(c)) return e;
  int* dlag = reinterpret_cast<int*>(c->rs_out + PS_LAG_AT);
  int* dmark = reinterpret_cast<int*>(c->rs_out + PS_MARK_AT);
  double* dcost = reinterpret_cast<double*>(c->rs_out + PS_COST_AT);
  int* dcnt = reinterpret_cast<int*>(c->rs_out + PS_CNT_AT);
  PsGrain* dgrain = reinterpret_cast<PsGrain*>(c->rs_out + PS_GRAIN_AT);
  const size_t lds = (size_t)(8 + 2 * g.pmax + 2 * (g.pmax / 8)) * sizeof(double);
  const bool one_launch = jobs.back().launch == 0;
  std::vector<std::vector<int32_t>> rmarks((size_t)batch);
  std::vector<double> rcost;
  std::vector<int> tab, cnt;
  auto stage = [&](size_t j0, size_t j1) -> int {                // the samples of the launch's rows
    for (size_t k = j0; k < j1; ++k) {
      const PsJob& j = jobs[k];
      if (lens[j.row] > 0) H2D(c->rs_in + j.in_off, wav + (long)j.row * wav_stride, (size_t)lens[j.row] * sizeof(float));
    }
    return VX_OK;
  };
  const int err = wave_launches(c, jobs, [&](size_t j0, size_t j1) -> int {      // the mark walks
    tab.clear();
    cnt.assign(j1 - j0, 0);
    if (int e = stage(j0, j1)) return e;
    for (size_t k = j0; k < j1; ++k) {
      const PsJob& j = jobs[k];
      const long L = lens[j.row], Mf = ps_frames(g, L);
      for (long v : {j.in_off, L, j.lag_off, Mf, j.m_off, ps_mark_bound(L), 0L, 0L, 0L, 0L, 0L, 0L, 0L, 0L, 0L, 0L}) tab.push_back((int)v);
      if (Mf > 0) H2D(dlag + j.lag_off, lag + (long)j.row * lag_stride, (size_t)Mf * sizeof(int));
    }
    H2D(c->rs_meta, tab.data(), tab.size() * sizeof(int));
    hipLaunchKernelGGL(psola_marks_kernel, dim3((unsigned)(j1 - j0)), dim3(256), lds, c->stream, c->rs_in, c->rs_meta, dlag, dmark, dcost,
                       dcnt, g);
    D2H(cnt.data(), dcnt, (j1 - j0) * sizeof(int));
    return VX_OK;
  }, [&](size_t j0, size_t j1) -> int {                            // N marks of every row, then the marks themselves
    for (size_t k = j0; k < j1; ++k) {
      const PsJob& j = jobs[k];
      const long N = cnt[k - j0];
      if (N < 0 || N + 1 > ps_mark_bound(lens[j.row])) FAIL(VX_EHIP, "%s: the mark walk of row %d returned %ld marks", who, j.row, N);
      rmarks[(size_t)j.row].resize((size_t)N + 1);
      D2H(rmarks[(size_t)j.row].data(), dmark + j.m_off, (size_t)(N + 1) * sizeof(int));
      if (cost) {
        rcost.resize((size_t)N + 1);
        D2H(rcost.data(), dcost + j.m_off, (size_t)(N + 1) * sizeof(double));
      }
    }
    SYNC();
    return VX_OK;
  });
  if (err) return err;
  std::vector<std::vector<PsGrain>> rgrains((size_t)batch);
  std::vector<vx_psola_info> rinfo((size_t)batch);
  for (int i = 0; i < batch; ++i) {                              // the synthesis marks; every refusal that needs N
    const long N = (long)rmarks[(size_t)i].size() - 1;
    if (marks && N + 1 > marks_stride)
      FAIL(VX_EINVAL, "%s: marks_stride %ld below the %ld marks of row %d", who, (long)marks_stride, N + 1, i);
    if (cost && N + 1 > cost_cap) FAIL(VX_EINVAL, "%s: cost_cap %ld below the %ld marks of the row", who, cost_cap, N + 1);
    int nv = 0;
    ps_grains(g, lens[i], lag + (long)i * lag_stride, ratio ? ratio + (long)i * lag_stride : nullptr, rmarks[(size_t)i].data(), N,
              &rgrains[(size_t)i], &nv);
    const long J = (long)rgrains[(size_t)i].size();
    if (J > ps_grain_bound(lens[i])) FAIL(VX_EHIP, "%s: row %d has %ld grains, above the bound", who, i, J);
    if (gtab && J > gtab_cap) FAIL(VX_EINVAL, "%s: grain_cap %ld below the %ld grains of the row", who, gtab_cap, J);
    const float* x = wav + (long)i * wav_stride;
    rinfo[(size_t)i] = {(int32_t)N, nv, (int32_t)J, ps_gaps(rgrains[(size_t)i], lens[i]), ps_nonfinite(x, lens[i])};
  }
  std::vector<PsGrain> gall;
  // the synthesis: its own loop, not wave_launches -- a launch group of empty rows alone launches nothing and syncs nothing
  for (size_t j0 = 0, j1; j0 < jobs.size(); j0 = j1) {
    for (j1 = j0 + 1; j1 < jobs.size() && jobs[j1].launch == jobs[j0].launch;) ++j1;
    tab.clear();
    gall.clear();
    long blocks = 0;
    if (!one_launch)
      if (int e = stage(j0, j1)) return e;
    for (size_t k = j0; k < j1; ++k) {
      const PsJob& j = jobs[k];
      const long L = lens[j.row];
      const std::vector<PsGrain>& gr = rgrains[(size_t)j.row];
      for (long v : {j.in_off, L, 0L, 0L, 0L, 0L, (long)gall.size(), (long)gr.size(), blocks, 0L, 0L, 0L, 0L, 0L, 0L, 0L}) tab.push_back((int)v);
      gall.insert(gall.end(), gr.begin(), gr.end());
      blocks += (L + PS_TILE - 1) / PS_TILE;
    }
    if (blocks == 0) continue;
    H2D(c->rs_meta, tab.data(), tab.size() * sizeof(int));
    if (!gall.empty()) H2D(dgrain, gall.data(), gall.size() * sizeof(PsGrain));
    hipLaunchKernelGGL(psola_synth_kernel, dim3((unsigned)blocks), dim3(256), 0, c->stream, c->rs_in, c->rs_meta, (int)(j1 - j0), dgrain,
                       c->rs_out, ps_wmax(g));
    for (size_t k = j0; k < j1; ++k) {
      const PsJob& j = jobs[k];
      if (lens[j.row] > 0) D2H(out + (long)j.row * out_stride, c->rs_out + j.in_off, (size_t)lens[j.row] * sizeof(float));
    }
    if (gtab && !gall.empty()) D2H(gtab, dgrain, gall.size() * sizeof(PsGrain));
    SYNC();
    HIPCHK(hipGetLastError());
  }
  for (int i = 0; i < batch; ++i) {
    if (marks) memcpy(marks + (long)i * marks_stride, rmarks[(size_t)i].data(), rmarks[(size_t)i].size() * sizeof(int32_t));
    info[i] = rinfo[(size_t)i];
  }
  if (cost) memcpy(cost, rcost.data(), rcost.size() * sizeof(double));
  return VX_OK;
}

}  // namespace vxe

extern "C" {

int vx_psola(vx_ctx* c, const float* wav, int64_t wav_stride, const int32_t* lens, int32_t batch, const int32_t* lag, int64_t lag_stride,
             const int32_t* ratio, const vx_psola_opts* o, float* out, int64_t out_stride, int32_t* marks, int64_t marks_stride,
             vx_psola_info* info) {
  using namespace vxe;
  if (!c) return VX_EINVAL;
  if (int e = wave_check_rows(c, "vx_psola", wav, wav_stride, lens, batch)) return e;
  if (!lag) FAIL(VX_EINVAL, "vx_psola: lag is NULL");
  if (!o) FAIL(VX_EINVAL, "vx_psola: o is NULL");
  if (!out) FAIL(VX_EINVAL, "vx_psola: out is NULL");
  if (!info) FAIL(VX_EINVAL, "vx_psola: info is NULL");
  PsGeom g;
  if (int e = ps_check(c, "vx_psola", lens, batch, lag_stride, ratio, o, out_stride, &g)) return e;
  return ps_run(c, "vx_psola", wav, wav_stride, lens, batch, lag, lag_stride, ratio, g, out, out_stride, marks, marks_stride, info, nullptr, 0,
                nullptr, 0);
}

int vx_dev_psola_table(vx_ctx* c, const float* wav, int32_t len, const int32_t* lag, const int32_t* ratio, const vx_psola_opts* o,
                       double* cost, int32_t cost_cap, int32_t* grains, int32_t grain_cap, int32_t* n_marks, int32_t* n_grains) {
  using namespace vxe;
  if (!c) return VX_EINVAL;
  if (!wav) FAIL(VX_EINVAL, "vx_dev_psola_table: wav is NULL");
  if (!lag) FAIL(VX_EINVAL, "vx_dev_psola_table: lag is NULL");
  if (!o) FAIL(VX_EINVAL, "vx_dev_psola_table: o is NULL");
  if (!cost || !grains || !n_marks || !n_grains) FAIL(VX_EINVAL, "vx_dev_psola_table: cost, grains, n_marks or n_grains is NULL");
  if (len < 0) FAIL(VX_EINVAL, "vx_dev_psola_table: len %d below 0", len);
  PsGeom g;
  const int64_t big = 0x7fffffffL;
  if (int e = ps_check(c, "vx_dev_psola_table", &len, 1, big, ratio, o, big, &g)) return e;
  std::vector<float> y((size_t)len + 1);
  vx_psola_info info;
  if (int e = ps_run(c, "vx_dev_psola_table", wav, len, &len, 1, lag, big, ratio, g, y.data(), big, nullptr, 0, &info, cost, cost_cap, grains,
                     grain_cap))
    return e;
  *n_marks = info.marks;
  *n_grains = info.grains;
  return VX_OK;
}

int vx_dev_psola_window(vx_ctx* c, int32_t samples) {
  return vxe::wave_set_window(c, &vx_ctx::ps_window, "vx_dev_psola_window", "samples", samples, VX_DEV_PSOLA_WINDOW_MIN, VX_PSOLA_WINDOW);
}

}  // extern "C"
