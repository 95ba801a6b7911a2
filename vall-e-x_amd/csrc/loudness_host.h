// Host side of the loudness measurement (loudness.hip, vx_loudness / vx_finish_loud): option checking, the K-weighting coefficients,
// the reduction of a row's step table to blocks, gates, loudness and gain, and the launch planner of the steps pass.
// Plain C++17 without the GPU runtime, so a stand-alone program (tools/loudness_host_check.cpp) runs exactly this code on a CPU --
// against the numpy restatement of the contract (tests/_loudness_refs.py), through the planner's invariants, under a sanitizer.
// Every quantity is computed as include/vallex_hip.h states it: in double, in block order, with one rounding where a float leaves.
#pragma once

#include <float.h>
#include <math.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../include/vallex_hip.h"

namespace vxe {

constexpr int LN_RATE_MIN = 8000, LN_RATE_MAX = 192000;
constexpr int LN_STEP_MIN = LN_RATE_MIN / 10;

inline int ln_step(int rate) { return rate / 10; }                 // S: 100 ms, integer division
inline long ln_nsteps(long n, int S) { return (n + S - 1) / S; }

// nullptr: the rate is in range; else the message (in buf), naming the field
inline const char* ln_check_rate(int rate, char* buf, size_t nbuf) {
  if (rate >= LN_RATE_MIN && rate <= LN_RATE_MAX) return nullptr;
  snprintf(buf, nbuf, "sample_rate %d outside %d .. %d", rate, LN_RATE_MIN, LN_RATE_MAX);
  return buf;
}

inline const char* ln_check_opts(const vx_loudness_opts& o, char* buf, size_t nbuf) {
  auto fin = [](float v) { return v - v == 0.f; };
  if (ln_check_rate(o.sample_rate, buf, nbuf)) return buf;
  if (!fin(o.target_lufs) || o.target_lufs < -70.f || o.target_lufs > 0.f) snprintf(buf, nbuf, "target_lufs %g is not a finite value in -70 .. 0", (double)o.target_lufs);
  else if (!fin(o.ceiling_db) || o.ceiling_db > 0.f) snprintf(buf, nbuf, "ceiling_db %g is not a finite value <= 0", (double)o.ceiling_db);
  else return nullptr;
  return buf;
}

// c = {b0, b1, b2, a1, a2} of the shelf, then of the high-pass (the derivation of include/vallex_hip.h)
inline void ln_coeffs(int rate, double c[10]) {
  const double pi = 3.14159265358979323846, fs = (double)rate;
  {
    const double K = tan(pi * 1681.974450955533 / fs), Vh = pow(10.0, 3.999843853973347 / 20.0), Vb = pow(Vh, 0.4996667741545416);
    const double Q = 0.7071752369554196, KQ = K / Q, KK = K * K, a0 = 1.0 + KQ + KK;
    c[0] = (Vh + Vb * KQ + KK) / a0;
    c[1] = 2.0 * (KK - Vh) / a0;
    c[2] = (Vh - Vb * KQ + KK) / a0;
    c[3] = 2.0 * (KK - 1.0) / a0;
    c[4] = (1.0 - KQ + KK) / a0;
  }
  {
    const double K = tan(pi * 38.13547087602444 / fs), Q = 0.5003270373238773, KQ = K / Q, KK = K * K, a0 = 1.0 + KQ + KK;
    c[5] = 1.0; c[6] = -2.0; c[7] = 1.0;
    c[8] = 2.0 * (KK - 1.0) / a0;
    c[9] = (1.0 - KQ + KK) / a0;
  }
}

inline double ln_abs_gate() { return pow(10.0, (-70.0 + 0.691) / 10.0); }
inline double ln_lufs(double ms) { return ms > 0.0 ? -0.691 + 10.0 * log10(ms) : -HUGE_VAL; }

// the block energies of a span of n samples from its step table z [ceil(n / S)]
inline void ln_blocks(const double* z, long n, int S, std::vector<double>& m) {
  m.clear();
  if (n <= 0) return;
  if (n < 4L * S) {
    double s = 0.0;
    for (long j = 0; j < ln_nsteps(n, S); ++j) s = s + z[j];
    m.push_back(s / (double)n);
    return;
  }
  const long nb = (n - 4L * S) / S + 1;
  const double den = (double)(4L * S);
  for (long k = 0; k < nb; ++k) m.push_back((((z[k] + z[k + 1]) + z[k + 2]) + z[k + 3]) / den);
}

// what the step table of a span says: blocks, both gates, loudness, the loudest block
inline void ln_reduce(const double* z, long n, int S, int nonfinite, vx_loudness_info* w) {
  std::vector<double> m;
  ln_blocks(z, n, S, m);
  const double A = ln_abs_gate();
  double sum = 0.0, top = 0.0;
  long above = 0, gated = 0;
  for (double v : m) {
    top = std::max(top, v);
    if (v > A) { sum = sum + v; ++above; }
  }
  double gsum = 0.0;
  if (above) {
    const double rel = 0.1 * (sum / (double)above);
    for (double v : m)
      if (v > A && v > rel) { gsum = gsum + v; ++gated; }
  }
  w->mean_square = gated ? gsum / (double)gated : 0.0;
  w->loudness = gated ? ln_lufs(w->mean_square) : -HUGE_VAL;
  w->max_momentary = m.empty() ? -HUGE_VAL : ln_lufs(top);
  w->blocks = (int32_t)m.size(); w->above_abs = (int32_t)above; w->gated = (int32_t)gated; w->nonfinite = nonfinite;
}

// the gain that brings `loudness` to the target: double on the host, rounded once; 1 when nothing passed the gates
inline float ln_gain(double loudness, float target_lufs, float ceiling_db, float max_gain_db, float peak) {
  if (!(loudness > -HUGE_VAL)) return 1.f;
  double g = pow(10.0, ((double)target_lufs - loudness) / 20.0);
  g = std::min(g, pow(10.0, (double)max_gain_db / 20.0));
  if (peak > 0.f) g = std::min(g, pow(10.0, (double)ceiling_db / 20.0) / (double)peak);
  return (float)std::min(g, (double)FLT_MAX);
}

// The planner.  A job is a run of consecutive steps [j0, j0 + ceil(cnt / S)) of one row's span together with the `pre` = min(W, j0 S)
// samples in front of its first step (the warm-up: what lies before the span is 0 and is not carried).  A launch holds at most `win`
// samples, warm-ups included, and `max_jobs` jobs; rows are packed greedily in order, a row that does not fit is cut at a step.
struct LnJob {
  int launch, row;
  long j0;               // first step of the job in its row
  long pre, cnt;         // the job's samples: span samples [j0 S - pre, j0 S + cnt)
  long off;              // first sample of the job (its warm-up) in the launch's input buffer
  long z_off;            // first record of the job in the launch's step table
};

inline bool ln_plan(const long* lo, const long* hi, int batch, int S, long win, long max_jobs, std::vector<LnJob>* jobs) {
  jobs->clear();
  const long W = 2L * S;
  if (S < 1 || win < W + S || max_jobs < 1) return false;          // a warm-up and one step fit an empty launch
  int launch = 0;
  long used = 0, zused = 0, njobs = 0;
  for (int i = 0; i < batch; ++i) {
    const long n = hi[i] - lo[i];
    long s = 0;                                                    // a multiple of S
    while (s < n) {
      const long pre = std::min(W, s), room = win - used - pre, rest = n - s;
      const long take = rest <= room ? rest : room > 0 ? room / S * S : 0;
      if (take <= 0 || njobs == max_jobs) {                        // nothing more fits this launch
        ++launch;
        used = zused = njobs = 0;
        continue;
      }
      jobs->push_back({launch, i, s / S, pre, take, used, zused});
      used += pre + take;
      zused += ln_nsteps(take, S);
      ++njobs;
      s += take;
    }
  }
  return true;
}

}  // namespace vxe
