// Host side of the formant-preserving pitch shift (psola.hip, vx_psola): option checking, the period lookup, the synthesis-mark walk
// and the grain table (which run between the two launches), the gap count, the launch planner and a sequential reference of the whole
// contract.
// Plain C++17 without the GPU runtime, so a stand-alone program (tools/psola_host_check.cpp) runs exactly this code on a CPU -- against
// the numpy restatement of the contract (tests/_psola_refs.py), through the planner's invariants, under a sanitizer.
// Every position is 64-bit integer arithmetic and every floating-point operation is a separately rounded double operation, as
// include/vallex_hip.h states them: the arithmetic below is compiled with contraction off.
#pragma once

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../include/vallex_hip.h"
#include "ws_walk.h"

namespace vxe {

constexpr int PS_HOP_MIN = 16, PS_HOP_MAX = 4096;
constexpr int PS_PERIOD_MIN = 16, PS_PERIOD_MAX = 1024;
constexpr int PS_RATIO_MIN = 43691, PS_RATIO_MAX = 131072;     // 2/3 .. 2 in Q16
constexpr int PS_STEP_MIN = PS_PERIOD_MIN - PS_PERIOD_MIN / 8; // analysis marks are at least this far apart (P - P/8 grows with P)
constexpr int PS_GRAIN_STEP_MIN = PS_STEP_MIN / 2;             // and grain centres at least this far, at ratio 2

struct PsGeom { int H, pmin, pmax, U, r; };                    // hop, period bounds, unvoiced period, the call's ratio

// nullptr: the options are in range; else the message (in buf), naming the field
inline const char* ps_check_opts(const vx_psola_opts& o, char* buf, size_t nbuf) {
  if (o.hop < PS_HOP_MIN || o.hop > PS_HOP_MAX) snprintf(buf, nbuf, "hop %d outside %d .. %d", o.hop, PS_HOP_MIN, PS_HOP_MAX);
  else if (o.period_min < PS_PERIOD_MIN || o.period_min > PS_PERIOD_MAX)
    snprintf(buf, nbuf, "period_min %d outside %d .. %d", o.period_min, PS_PERIOD_MIN, PS_PERIOD_MAX);
  else if (o.period_max < o.period_min || o.period_max > PS_PERIOD_MAX)
    snprintf(buf, nbuf, "period_max %d outside period_min = %d .. %d", o.period_max, o.period_min, PS_PERIOD_MAX);
  else if (o.unvoiced_period < o.period_min || o.unvoiced_period > o.period_max)
    snprintf(buf, nbuf, "unvoiced_period %d outside period_min = %d .. period_max = %d", o.unvoiced_period, o.period_min, o.period_max);
  else if (o.ratio_q16 < PS_RATIO_MIN || o.ratio_q16 > PS_RATIO_MAX)
    snprintf(buf, nbuf, "ratio_q16 %d outside %d .. %d", o.ratio_q16, PS_RATIO_MIN, PS_RATIO_MAX);
  else return nullptr;
  return buf;
}

inline PsGeom ps_geometry(const vx_psola_opts& o) { return {o.hop, o.period_min, o.period_max, o.unvoiced_period, o.ratio_q16}; }

inline long ps_frames(const PsGeom& g, long L) { return (L + g.H - 1) / g.H; }                   // Mf = ceil(L / Hf)
inline long ps_mark_bound(long L) { return L / PS_STEP_MIN + 2; }                                // marks a_0 .. a_N of a row, at most
inline long ps_grain_bound(long L) { return L / PS_GRAIN_STEP_MIN + 2; }                         // grains of a row, at most
inline int ps_wmax(const PsGeom& g) { return g.pmax + g.pmax / 8; }                              // no grain side is wider

#if defined(__HIPCC__)
#define VX_PS_HD __host__ __device__
#else
#define VX_PS_HD
#endif

// the period at sample a of a row with Mf >= 1 frames: the return value is P, *voiced its voicing
VX_PS_HD inline int ps_period(const PsGeom& g, const int32_t* lag, long Mf, long a, bool* voiced) {
  long k = a / g.H;
  if (k > Mf - 1) k = Mf - 1;
  const int t = lag[k];
  *voiced = t >= g.pmin && t <= g.pmax;
  return *voiced ? t : g.U;
}

// the total order of the search (ws_walk.h): smaller cost, then smaller |d|, then the negative d
VX_PS_HD inline bool ps_better(double Ca, int da, double Cb, int db) { return ws_better(Ca, da, Cb, db); }

struct PsGrain { int32_t s, a, Wl, Wr; };                       // centre, source centre, left and right width

// The synthesis marks and the grain table of one row from its analysis marks a [N + 1]: serial integer arithmetic.
// ratio: the row's per-frame Q16 ratios, or nullptr for g.r.  *voiced_marks: the voiced ones of a_0 .. a_{N-1}.
inline void ps_grains(const PsGeom& g, long L, const int32_t* lag, const int32_t* ratio, const int32_t* a, long N, std::vector<PsGrain>* out,
                      int* voiced_marks) {
  out->clear();
  const long Mf = ps_frames(g, L);
  int nv = 0;
  for (long i = 0; i < N; ++i) {
    bool v;
    ps_period(g, lag, Mf, a[i], &v);
    nv += v ? 1 : 0;
  }
  *voiced_marks = nv;
  if (N < 1) return;
  int64_t S = 0;
  long i = 0;
  for (;;) {
    const long s = (long)((S + 32768) >> 16);
    if (s >= L) break;
    while (i + 1 <= N - 1 && labs((long)a[i + 1] - s) < labs((long)a[i] - s)) ++i;      // nearest mark, ties to the lower index
    const long gap = (long)a[i + 1] - a[i];
    bool v;
    ps_period(g, lag, Mf, a[i], &v);
    long k = a[i] / g.H;
    if (k > Mf - 1) k = Mf - 1;
    const int64_t r = v ? (ratio ? ratio[k] : g.r) : 65536;
    out->push_back({(int32_t)s, a[i], (int32_t)(i ? a[i] - a[i - 1] : a[1] - a[0]), (int32_t)gap});
    S += (int64_t)(((int64_t)gap << 32) / r);
  }
}

// samples of [0, L) no grain covers: every weight is positive, so these are the samples with den == 0
inline int ps_gaps(const std::vector<PsGrain>& gr, long L) {
  std::vector<std::pair<long, long>> iv;
  iv.reserve(gr.size());
  for (const PsGrain& q : gr) {
    const long lo = std::max(0L, (long)q.s - q.Wl), hi = std::min(L, (long)q.s + q.Wr);
    if (hi > lo) iv.push_back({lo, hi});
  }
  std::sort(iv.begin(), iv.end());
  long covered = 0, end = 0;
  for (const auto& p : iv) {
    const long lo = std::max(p.first, end);
    if (p.second > lo) { covered += p.second - lo; end = p.second; }
  }
  return (int)(L - covered);
}

// The planner.  A launch holds at most `win` samples, `mark_cap` marks, `grain_cap` grains (both by their bounds), `lag_cap` lags and
// `max_jobs` rows.  A row is never cut: rows are packed into launches greedily in order.
struct PsJob {
  int launch, row;
  long in_off;           // first sample of the row in the launch's input and output buffers
  long lag_off, m_off, g_off;   // first lag, mark and (bound of the first) grain of the row in the launch's tables
};

// false: a row does not fit an EMPTY launch
inline bool ps_plan(const PsGeom& g, const int* lens, int batch, long win, long mark_cap, long grain_cap, long lag_cap, long max_jobs,
                    std::vector<PsJob>* jobs) {
  jobs->clear();
  if (max_jobs < 1) return false;
  int launch = 0;
  long in_used = 0, m_used = 0, g_used = 0, l_used = 0, njobs = 0;
  for (int i = 0; i < batch;) {
    const long L = lens[i], nm = ps_mark_bound(L), ng = ps_grain_bound(L), nl = ps_frames(g, L);
    if (njobs < max_jobs && in_used + L <= win && m_used + nm <= mark_cap && g_used + ng <= grain_cap && l_used + nl <= lag_cap) {
      jobs->push_back({launch, i, in_used, l_used, m_used, g_used});
      in_used += L; m_used += nm; g_used += ng; l_used += nl;
      ++njobs; ++i;
      continue;
    }
    if (njobs == 0) return false;
    ++launch; in_used = m_used = g_used = l_used = njobs = 0;
  }
  return true;
}

inline bool ps_finite(float x) {
  uint32_t u;
  memcpy(&u, &x, sizeof u);
  return (u & 0x7f800000u) != 0x7f800000u;
}

inline int ps_nonfinite(const float* x, long L) {
  long n = 0;
  for (long i = 0; i < L; ++i) n += ps_finite(x[i]) ? 0 : 1;
  return (int)std::min(n, 0x7fffffffL);
}

#if defined(__clang__)
#define VX_PS_NO_CONTRACT _Pragma("clang fp contract(off)")
#define VX_PS_NO_CONTRACT_FN
#elif defined(__GNUC__)
#define VX_PS_NO_CONTRACT
#define VX_PS_NO_CONTRACT_FN __attribute__((optimize("fp-contract=off")))
#else
#define VX_PS_NO_CONTRACT
#define VX_PS_NO_CONTRACT_FN
#endif

// the weight of a grain with widths Wl, Wr at offset rr in [-Wl, Wr) from its centre.  The kernel runs this function.
VX_PS_NO_CONTRACT_FN VX_PS_HD inline float ps_weight(int rr, int Wl, int Wr) {
  VX_PS_NO_CONTRACT
  const double u = rr < 0 ? ((double)(rr + Wl) + 0.5) / (double)Wl : ((double)(Wr - rr) - 0.5) / (double)Wr;
  return (float)((u * u) * (3.0 - 2.0 * u));
}

// The sequential reference of the whole contract for one row.  marks: a_0 .. a_N; cost: the winning cost of every voiced mark below L,
// 0 for the others; grains; out [L]; info.
VX_PS_NO_CONTRACT_FN inline void psola_reference(const PsGeom& g, const float* x, long L, const int32_t* lag, const int32_t* ratio,
                                                 std::vector<int32_t>* marks, std::vector<double>* cost, std::vector<PsGrain>* grains, float* out,
                                                 vx_psola_info* info) {
  VX_PS_NO_CONTRACT
  const long Mf = ps_frames(g, L);
  auto y = [&](long s) -> double { return s >= 0 && s < L && ps_finite(x[s]) ? (double)x[s] : 0.0; };
  marks->clear();
  cost->clear();
  long a = 0;
  for (;;) {
    marks->push_back((int32_t)a);
    if (a >= L) break;
    bool v;
    const int P = ps_period(g, lag, Mf, a, &v);
    if (!v) { cost->push_back(0.0); a += g.U; continue; }
    const int D = P / 8;
    double bC = 0.0;
    int bd = 0;
    for (int d = -D; d <= D; ++d) {
      double c = 0.0, e = 0.0;
      for (int j = 0; j < P; ++j) {
        const double p = y(a + P + d + j), t = y(a + j);
        c = c + p * t;
        e = e + p * p;
      }
      const double C = e - 2.0 * c;
      if (d == -D || ps_better(C, d, bC, bd)) { bC = C; bd = d; }
    }
    cost->push_back(bC);
    a += P + bd;
  }
  cost->push_back(0.0);                                           // of the closing mark
  const long N = (long)marks->size() - 1;
  int nv;
  ps_grains(g, L, lag, ratio, marks->data(), N, grains, &nv);
  int gaps = 0;
  for (long n = 0; n < L; ++n) {
    double num = 0.0, den = 0.0;
    for (const PsGrain& q : *grains) {
      const long rr = n - q.s;
      if (rr < -(long)q.Wl || rr >= q.Wr) continue;
      const float w = ps_weight((int)rr, q.Wl, q.Wr);
      num = num + y(q.a + rr) * (double)w;
      den = den + (double)w;
    }
    out[n] = den > 0.0 ? (float)(num / den) : 0.f;
    gaps += den > 0.0 ? 0 : 1;
  }
  info->marks = (int32_t)N;
  info->voiced_marks = nv;
  info->grains = (int32_t)grains->size();
  info->gaps = gaps;
  info->nonfinite = ps_nonfinite(x, L);
}

}  // namespace vxe
