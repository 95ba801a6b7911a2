// Host side of the equaliser (eq.hip, vx_eq / vx_eq_design / vx_eq_plan): the cookbook designs, the checks of a cascade, the warm-up
// W of a filter, the launch planner and a sequential reference of the whole contract for one row.
// Plain C++17 without the GPU runtime, so a stand-alone program (tools/eq_host_check.cpp) runs exactly this code on a CPU --
// against the numpy restatement of the contract (tests/_eq_refs.py), through the planner's invariants, under a sanitizer.
// Every quantity is computed as include/vallex_hip.h states it: in double, every operation rounded on its own (the recursion below
// is compiled with contraction off, here and in the kernel), with one rounding where a float leaves.
#pragma once

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/vallex_hip.h"
#include "loudness_host.h"

#if defined(__clang__)
#define VX_EQ_NO_CONTRACT _Pragma("clang fp contract(off)")
#define VX_EQ_NO_CONTRACT_FN
#elif defined(__GNUC__)
#define VX_EQ_NO_CONTRACT
#define VX_EQ_NO_CONTRACT_FN __attribute__((optimize("fp-contract=off")))
#else
#define VX_EQ_NO_CONTRACT
#define VX_EQ_NO_CONTRACT_FN
#endif

#if defined(__HIPCC__)
#define VX_EQ_HD __host__ __device__
#else
#define VX_EQ_HD
#endif

namespace vxe {

constexpr int EQ_S = VX_EQ_STEP;                 // samples of a step
constexpr int EQ_MAX = VX_EQ_MAX_SECTIONS;
constexpr int EQ_WARM_MAX = VX_EQ_WARM_MAX;
constexpr int EQ_TILE = 64;                      // steps of a tile (eq.hip: one wavefront); a tile writes one record
static_assert(EQ_S >= 32 && EQ_S % 32 == 0 && EQ_WARM_MAX % 32 == 0, "the kernel walks chunks of 32 samples: W and S are multiples");

inline long eq_nsteps(long n, int S) { return (n + S - 1) / S; }
inline long eq_ntiles(long n, int S) { return (eq_nsteps(n, S) + EQ_TILE - 1) / EQ_TILE; }

// One sample through one section {b0, b1, b2, a1, a2}, transposed direct form II: the recursion of the contract, the one the kernel
// runs.  NS is a compile-time count in the kernel (the states stay in registers) and a runtime one here.
VX_EQ_HD VX_EQ_NO_CONTRACT_FN inline double eq_section(const double* c, double x, double& s1, double& s2) {
  VX_EQ_NO_CONTRACT
  const double u = c[0] * x + s1;
  s1 = (c[1] * x - c[3] * u) + s2;
  s2 = c[2] * x - c[4] * u;
  return u;
}

// nullptr: c[5] holds the section; else the message (in buf), naming the field
inline const char* eq_design(int kind, int rate, double f0, double q, double gain_db, double c[5], char* buf, size_t nbuf) {
  if (ln_check_rate(rate, buf, nbuf)) return buf;
  if (kind < VX_EQ_HIGHPASS || kind > VX_EQ_HIGHSHELF) snprintf(buf, nbuf, "kind %d outside %d .. %d", kind, VX_EQ_HIGHPASS, VX_EQ_HIGHSHELF);
  else if (!(f0 > 0.0 && f0 < 0.5 * (double)rate)) snprintf(buf, nbuf, "f0 %g outside (0, sample_rate / 2 = %g)", f0, 0.5 * (double)rate);
  else if (!(q > 0.0 && q <= DBL_MAX)) snprintf(buf, nbuf, "q %g is not a finite value above 0", q);
  else if (!(fabs(gain_db) <= 24.0)) snprintf(buf, nbuf, "gain_db %g outside -24 .. 24", gain_db);
  else {
    // the cookbook forms; 1 - cos w0 and 1 + cos w0 from the half angle, which loses no digits at a low or a high f0
    const double pi = 3.14159265358979323846, w0 = 2.0 * pi * f0 / (double)rate, cw = cos(w0), sw = sin(w0), sh = sin(0.5 * w0), ch = cos(0.5 * w0);
    const double al = sw / (2.0 * q), omc = 2.0 * sh * sh, opc = 2.0 * ch * ch;
    double b0, b1, b2, a0, a1, a2;
    if (kind == VX_EQ_HIGHPASS || kind == VX_EQ_LOWPASS || kind == VX_EQ_BANDPASS || kind == VX_EQ_NOTCH) {
      a0 = 1.0 + al; a1 = -2.0 * cw; a2 = 1.0 - al;
      if (kind == VX_EQ_HIGHPASS) { b0 = 0.5 * opc; b1 = -opc; b2 = 0.5 * opc; }
      else if (kind == VX_EQ_LOWPASS) { b0 = 0.5 * omc; b1 = omc; b2 = 0.5 * omc; }
      else if (kind == VX_EQ_BANDPASS) { b0 = al; b1 = 0.0; b2 = -al; }
      else { b0 = 1.0; b1 = -2.0 * cw; b2 = 1.0; }
    } else {
      const double A = pow(10.0, gain_db / 40.0);
      if (kind == VX_EQ_PEAK) {
        b0 = 1.0 + al * A; b1 = -2.0 * cw; b2 = 1.0 - al * A;
        a0 = 1.0 + al / A; a1 = -2.0 * cw; a2 = 1.0 - al / A;
      } else {
        const double r = 2.0 * sqrt(A) * al, p = A + 1.0, m = A - 1.0;
        if (kind == VX_EQ_LOWSHELF) {
          b0 = A * ((p - m * cw) + r); b1 = 2.0 * A * (m - p * cw); b2 = A * ((p - m * cw) - r);
          a0 = (p + m * cw) + r; a1 = -2.0 * (m + p * cw); a2 = (p + m * cw) - r;
        } else {
          b0 = A * ((p + m * cw) + r); b1 = -2.0 * A * (m + p * cw); b2 = A * ((p + m * cw) - r);
          a0 = (p - m * cw) + r; a1 = 2.0 * (m - p * cw); a2 = (p - m * cw) - r;
        }
      }
    }
    c[0] = b0 / a0; c[1] = b1 / a0; c[2] = b2 / a0; c[3] = a1 / a0; c[4] = a2 / a0;
    return nullptr;
  }
  return buf;
}

// nullptr: 1 .. 8 sections, every coefficient finite, every section stable; else the message (in buf)
inline const char* eq_check_sections(const double* sec, int n, char* buf, size_t nbuf) {
  if (n < 1 || n > EQ_MAX) { snprintf(buf, nbuf, "nsections %d outside 1 .. %d", n, EQ_MAX); return buf; }
  for (int k = 0; k < n; ++k) {
    const double* c = sec + 5 * k;
    for (int i = 0; i < 5; ++i)
      if (!(fabs(c[i]) <= DBL_MAX)) { snprintf(buf, nbuf, "section %d: coefficient %d (of b0 b1 b2 a1 a2) is not finite", k, i); return buf; }
    if (fabs(c[4]) >= 1.0 || fabs(c[3]) >= 1.0 + c[4]) {
      snprintf(buf, nbuf, "section %d is unstable: a1 %g, a2 %g (needs |a2| < 1 and |a1| < 1 + a2)", k, c[3], c[4]);
      return buf;
    }
  }
  return nullptr;
}

// The warm-up of a cascade: a unit impulse through it for 2 EQ_WARM_MAX samples, T(k) = |h[k]| + T(k + 1) from the far end, W the
// smallest multiple of 32 with T(W) <= 2^-24.  nullptr and *W; else the message (eq_check_sections' included).
VX_EQ_NO_CONTRACT_FN inline const char* eq_warm(const double* sec, int n, int* W, char* buf, size_t nbuf) {
  if (eq_check_sections(sec, n, buf, nbuf)) return buf;
  const int N = 2 * EQ_WARM_MAX;
  std::vector<double> h((size_t)N);
  double s1[EQ_MAX] = {0}, s2[EQ_MAX] = {0};
  for (int i = 0; i < N; ++i) {
    double x = i == 0 ? 1.0 : 0.0;
    for (int k = 0; k < n; ++k) x = eq_section(sec + 5 * k, x, s1[k], s2[k]);
    h[(size_t)i] = x;
  }
  const double bound = 1.0 / 16777216.0;
  double T = 0.0;
  int best = -1;                                                     // the smallest k (a multiple of 32) with T(j) <= bound from k on
  for (int k = N - 1; k >= 0; --k) {
    T = fabs(h[(size_t)k]) + T;
    if (!(T <= bound)) break;                                        // T grows towards 0: nothing in front of k passes (NaN: nothing does)
    if (k % 32 == 0) best = k;
  }
  if (best < 0 || best > EQ_WARM_MAX) {
    snprintf(buf, nbuf, "the filter's memory is too long: its impulse response is not below 2^-24 within VX_EQ_WARM_MAX = %d samples", EQ_WARM_MAX);
    return buf;
  }
  *W = best;
  return nullptr;
}

// The planner.  A job is a run of consecutive steps [j0, j0 + ceil(cnt / S)) of one row together with the `pre` = min(W, j0 S)
// samples in front of its first step (the warm-up: what lies before the row is 0 and is not carried).  A launch holds at most `win`
// staged samples, warm-ups included, `out_cap` outputs and `max_jobs` jobs; rows are packed greedily in order, a row that does not fit
// is cut at a step.  A row of length 0 has no job.
struct EqJob {
  int launch, row;
  long j0;               // first step of the job in its row
  long pre, cnt;         // the job's samples: row samples [j0 S - pre, j0 S + cnt), the last cnt of them written
  long off;              // first sample of the job (its warm-up) in the launch's input buffer
  long out_off;          // first output of the job in the launch's output buffer
  long rec_off;          // first tile record of the job in the launch's record table
};

inline bool eq_plan(const int32_t* lens, int batch, int S, long W, long win, long out_cap, long max_jobs, std::vector<EqJob>* jobs) {
  jobs->clear();
  if (S < 1 || W < 0 || win < W + S || out_cap < S || max_jobs < 1) return false;      // a warm-up and one step fit an empty launch
  int launch = 0;
  long used = 0, oused = 0, rused = 0, njobs = 0;
  for (int i = 0; i < batch; ++i) {
    const long n = lens[i];
    long s = 0;                                                      // a multiple of S
    while (s < n) {
      const long pre = std::min(W, s), room = std::min(win - used - pre, out_cap - oused), rest = n - s;
      const long take = rest <= room ? rest : room > 0 ? room / S * S : 0;
      if (take <= 0 || njobs == max_jobs) {                          // nothing more fits this launch
        ++launch;
        used = oused = rused = njobs = 0;
        continue;
      }
      jobs->push_back({launch, i, s / S, pre, take, used, oused, rused});
      used += pre + take;
      oused += take;
      rused += eq_ntiles(take, S);
      ++njobs;
      s += take;
    }
  }
  return true;
}

// The whole contract for one row, one output after the other in step order: out [L]; nonfinite inputs, nonfinite results, peak
VX_EQ_NO_CONTRACT_FN inline void eq_reference(const float* x, long L, const double* sec, int n, int W, int S, float* out, vx_eq_info* info) {
  info->warm = W; info->nonfinite = 0; info->nonfinite_out = 0; info->peak = 0.f;
  for (long j = 0; j * S < L; ++j) {
    double s1[EQ_MAX] = {0}, s2[EQ_MAX] = {0};
    const long end = std::min<long>((j + 1) * S, L);
    for (long i = j * S - W; i < end; ++i) {
      const float xf = i >= 0 ? x[i] : 0.f;
      const bool fin = xf - xf == 0.f;
      double u = fin ? (double)xf : 0.0;
      for (int k = 0; k < n; ++k) u = eq_section(sec + 5 * k, u, s1[k], s2[k]);
      if (i < j * S) continue;
      float y = (float)u;
      if (!fin) ++info->nonfinite;
      if (!(y - y == 0.f)) { y = 0.f; ++info->nonfinite_out; }
      out[i] = y;
      info->peak = std::max(info->peak, fabsf(y));
    }
  }
}

}  // namespace vxe
