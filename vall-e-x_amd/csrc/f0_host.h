// Host side of the pitch tracker (f0.hip, vx_f0): option checking, the frame geometry, the launch planner, the per-row summary and a
// sequential reference of the whole contract.
// Plain C++17 without the GPU runtime, so a stand-alone program (tools/f0_host_check.cpp) runs exactly this code on a CPU -- against
// the numpy restatement of the contract (tests/_f0_refs.py), through the planner's invariants, under a sanitizer.
// Every frame position is 64-bit integer arithmetic and every floating-point operation is a separately rounded double operation, as
// include/vallex_hip.h states them: the arithmetic below is compiled with contraction off.
#pragma once

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/vallex_hip.h"

namespace vxe {

constexpr int F0_RATE_MIN = 8000, F0_RATE_MAX = 192000;
constexpr int F0_HOP_MIN = 16, F0_HOP_MAX = 4096;
constexpr int F0_WIN_MIN = 16, F0_WIN_MAX = 2048;
constexpr int F0_LAG_MIN = 2, F0_LAG_MAX = 1024;

struct F0Geom { int rate, H, W, t0, T; double thr; };      // hop, window, lag_min, lag_max, the threshold widened

// nullptr: the options are in range; else the message (in buf), naming the field
inline const char* f0_check_opts(const vx_f0_opts& o, char* buf, size_t nbuf) {
  if (o.sample_rate < F0_RATE_MIN || o.sample_rate > F0_RATE_MAX)
    snprintf(buf, nbuf, "sample_rate %d outside %d .. %d", o.sample_rate, F0_RATE_MIN, F0_RATE_MAX);
  else if (o.hop < F0_HOP_MIN || o.hop > F0_HOP_MAX) snprintf(buf, nbuf, "hop %d outside %d .. %d", o.hop, F0_HOP_MIN, F0_HOP_MAX);
  else if (o.window < F0_WIN_MIN || o.window > F0_WIN_MAX) snprintf(buf, nbuf, "window %d outside %d .. %d", o.window, F0_WIN_MIN, F0_WIN_MAX);
  else if (o.lag_min < F0_LAG_MIN || o.lag_min >= F0_LAG_MAX)
    snprintf(buf, nbuf, "lag_min %d outside %d .. %d", o.lag_min, F0_LAG_MIN, F0_LAG_MAX - 1);
  else if (o.lag_max <= o.lag_min || o.lag_max > F0_LAG_MAX)
    snprintf(buf, nbuf, "lag_max %d outside lag_min + 1 = %d .. %d", o.lag_max, o.lag_min + 1, F0_LAG_MAX);
  else if (!(o.threshold > 0.f && o.threshold <= 1.f)) snprintf(buf, nbuf, "threshold %g outside (0, 1]", (double)o.threshold);
  else return nullptr;
  return buf;
}

inline F0Geom f0_geometry(const vx_f0_opts& o) { return {o.sample_rate, o.hop, o.window, o.lag_min, o.lag_max, (double)o.threshold}; }

inline long f0_frames(const F0Geom& g, long L) { return (L + g.H - 1) / g.H; }                              // ceil(L / H)
inline long f0_reach(const F0Geom& g) { return (long)g.W + g.T; }                                           // samples a frame reads
inline long f0_first(const F0Geom& g, long k) { return k * g.H + g.H / 2 - (g.W + g.T) / 2; }               // s_k, may be negative

// the row samples the frames [k0, k1) read, cut to [0, L)
inline void f0_span(const F0Geom& g, long L, long k0, long k1, long* lo, long* hi) {
  const long a = std::max(0L, std::min(f0_first(g, k0), L));
  const long b = std::max(a, std::min(f0_first(g, k1 - 1) + f0_reach(g), L));
  *lo = a; *hi = b;
}

// The planner.  A launch holds at most `win` staged samples, `frame_cap` frames and `max_jobs` jobs.  A job is the frames [k0, k1) of
// one row with exactly the span f0_span gives; rows are packed into launches greedily in order, a row that does not fit the rest of a
// launch is cut at a frame boundary and goes on in the next one.  Frames are independent: no job needs another's result.
struct F0Job {
  int launch, row;
  long k0, k1;           // frames [k0, k1) of the row
  long s_lo, s_hi;       // staged samples [s_lo, s_hi) of the row, at in_off of the launch's input buffer
  long in_off;
  long f_off;            // first record of the job in the launch's frame tables
};

// false: one frame does not fit an EMPTY launch (its span above win, or a cap below 1)
inline bool f0_plan(const F0Geom& g, const int* lens, int batch, long win, long frame_cap, long max_jobs, std::vector<F0Job>* jobs) {
  jobs->clear();
  if (max_jobs < 1 || frame_cap < 1) return false;
  int launch = 0;
  long in_used = 0, f_used = 0, njobs = 0;
  for (int i = 0; i < batch; ++i) {
    const long L = lens[i], M = f0_frames(g, L);
    long k0 = 0;
    while (k0 < M) {
      const long in_free = win - in_used, f_free = frame_cap - f_used;
      auto fits = [&](long k1) {                                   // both grow with k1: bisection
        long lo, hi;
        f0_span(g, L, k0, k1, &lo, &hi);
        return hi - lo <= in_free && k1 - k0 <= f_free;
      };
      long k1 = k0;
      if (njobs < max_jobs && fits(k0 + 1)) {
        long a = k0 + 1, b = M;                                    // fits(a) holds
        while (a < b) {
          const long m = a + (b - a + 1) / 2;
          if (fits(m)) a = m; else b = m - 1;
        }
        k1 = a;
      }
      if (k1 == k0) {                                              // nothing more fits this launch
        if (njobs == 0) return false;
        ++launch; in_used = f_used = njobs = 0;
        continue;
      }
      long lo, hi;
      f0_span(g, L, k0, k1, &lo, &hi);
      jobs->push_back({launch, i, k0, k1, lo, hi, in_used, f_used});
      in_used += hi - lo;
      f_used += k1 - k0;
      ++njobs;
      k0 = k1;
    }
  }
  return true;
}

inline bool f0_finite(float x) {
  uint32_t u;
  memcpy(&u, &x, sizeof u);
  return (u & 0x7f800000u) != 0x7f800000u;
}

inline int f0_nonfinite(const float* x, long L) {
  long n = 0;
  for (long i = 0; i < L; ++i) n += f0_finite(x[i]) ? 0 : 1;
  return (int)std::min(n, 0x7fffffffL);
}

// the summary of one row over its voiced frames (lag > 0): the lower median, the smallest and the largest of the fp32 values
inline void f0_summary(const float* f0, const int32_t* lag, long M, int nonfinite, vx_f0_info* info) {
  std::vector<float> v;
  for (long k = 0; k < M; ++k)
    if (lag[k] > 0) v.push_back(f0[k]);
  info->frames = (int32_t)M;
  info->voiced_frames = (int32_t)v.size();
  info->nonfinite = nonfinite;
  info->f0_median = info->f0_min = info->f0_max = 0.f;
  if (v.empty()) return;
  std::sort(v.begin(), v.end());
  info->f0_median = v[(v.size() - 1) / 2];
  info->f0_min = v.front();
  info->f0_max = v.back();
}

#if defined(__clang__)
#define VX_F0_NO_CONTRACT _Pragma("clang fp contract(off)")
#define VX_F0_NO_CONTRACT_FN
#elif defined(__GNUC__)
#define VX_F0_NO_CONTRACT
#define VX_F0_NO_CONTRACT_FN __attribute__((optimize("fp-contract=off")))
#else
#define VX_F0_NO_CONTRACT
#define VX_F0_NO_CONTRACT_FN
#endif

#if defined(__HIPCC__)
#define VX_F0_HD __host__ __device__
#else
#define VX_F0_HD
#endif

// d'(t) from d(t) and the running sum c(t) = d(1) + .. + d(t)
VX_F0_NO_CONTRACT_FN VX_F0_HD inline double f0_norm(double d, int t, double c) {
  VX_F0_NO_CONTRACT
  return c > 0.0 ? (d * (double)t) / c : 1.0;
}

// pick and refinement of one frame from d' [T + 1]: the signed lag is returned.  The kernel's single lane runs this function.
VX_F0_NO_CONTRACT_FN VX_F0_HD inline int f0_choose(const F0Geom& g, const double* dp, float* f0, float* ap) {
  VX_F0_NO_CONTRACT
  int t = 0;
  bool voiced = false;
  for (int u = g.t0; u <= g.T; ++u)
    if (dp[u] < g.thr) { t = u; voiced = true; break; }
  if (voiced) {
    while (t + 1 <= g.T && dp[t + 1] < dp[t]) ++t;
  } else {
    t = g.t0;
    for (int u = g.t0 + 1; u <= g.T; ++u)
      if (dp[u] < dp[t]) t = u;
  }
  double off = 0.0;
  if (t + 1 <= g.T) {
    const double a = dp[t - 1], b = dp[t], cc = dp[t + 1];
    const double den = (a - 2.0 * b) + cc;
    if (b <= a && b <= cc && den > 0.0) off = (0.5 * (a - cc)) / den;
  }
  *f0 = (float)((double)g.rate / ((double)t + off));
  *ap = (float)dp[t];
  return voiced ? t : -t;
}

// normalisation, pick and refinement of one frame from its difference d [T + 1]: dp [T + 1] is written, the signed lag returned
VX_F0_NO_CONTRACT_FN inline int f0_pick(const F0Geom& g, const double* d, double* dp, float* f0, float* ap) {
  VX_F0_NO_CONTRACT
  double c = 0.0;
  dp[0] = 1.0;
  for (int t = 1; t <= g.T; ++t) {
    c = c + d[t];                                                  // the serial prefix, in lag order
    dp[t] = f0_norm(d[t], t, c);
  }
  return f0_choose(g, dp, f0, ap);
}

// The sequential reference of the whole contract for one row: f0, lag, ap [M]; d, dp [M][T + 1] when given.
VX_F0_NO_CONTRACT_FN inline void f0_reference(const F0Geom& g, const float* x, long L, float* f0, int32_t* lag, float* ap, double* dtab,
                                              double* dptab) {
  VX_F0_NO_CONTRACT
  const long M = f0_frames(g, L), R = f0_reach(g);
  std::vector<double> y((size_t)R), d((size_t)g.T + 1), dp((size_t)g.T + 1);
  for (long k = 0; k < M; ++k) {
    const long s = f0_first(g, k);
    for (long i = 0; i < R; ++i) {
      const long p = s + i;
      y[(size_t)i] = p >= 0 && p < L && f0_finite(x[p]) ? (double)x[p] : 0.0;
    }
    for (int t = 0; t <= g.T; ++t) {
      double acc = 0.0;
      for (int j = 0; j < g.W; ++j) {
        const double e = y[(size_t)j] - y[(size_t)(j + t)];
        acc = acc + e * e;
      }
      d[(size_t)t] = acc;
    }
    lag[k] = f0_pick(g, d.data(), dp.data(), &f0[k], &ap[k]);
    if (dtab) memcpy(dtab + k * (g.T + 1), d.data(), sizeof(double) * (size_t)(g.T + 1));
    if (dptab) memcpy(dptab + k * (g.T + 1), dp.data(), sizeof(double) * (size_t)(g.T + 1));
  }
}

}  // namespace vxe
