// Host side of the true-peak look-ahead limiter (limit.hip, vx_limit / vx_finish_limited): option checking, the detector's taps, the
// ceiling, the gain of vx_finish_limited, the launch planner and a plain sequential reference of the whole contract for one row.
// Plain C++17 without the GPU runtime, so a stand-alone program (tools/limit_host_check.cpp) runs exactly this code on a CPU --
// against the numpy restatement of the contract (tests/_limit_refs.py), through the planner's invariants, under a sanitizer.
// Every quantity is computed as include/vallex_hip.h states it.
#pragma once

#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../include/vallex_hip.h"
#include "resample_host.h"

namespace vxe {

constexpr int LM_LOOKAHEAD_MAX = 1024;
constexpr int LM_WIDTH = 7, LM_K = 15;                 // rs_geometry(1, n) for n = 2, 4, 8
constexpr int LM_OVERSAMPLE_MAX = 8;
constexpr long LM_ONE = 1L << 24;                      // the demand of "no reduction"

inline bool lm_oversample_ok(int n) { return n == 1 || n == 2 || n == 4 || n == 8; }
inline long lm_halo(int Wn) { return 2L * Wn + LM_WIDTH; }

// nullptr: the options are in range; else the message (in buf), naming the field
inline const char* lm_check_opts(const vx_limit_opts& o, float pre_gain, float ceiling_db, char* buf, size_t nbuf) {
  auto fin = [](float v) { return v - v == 0.f; };
  if (!fin(pre_gain) || !(pre_gain > 0.f)) snprintf(buf, nbuf, "pre_gain %g is not a finite value > 0", (double)pre_gain);
  else if (!fin(ceiling_db) || ceiling_db > 0.f) snprintf(buf, nbuf, "ceiling_db %g is not a finite value <= 0", (double)ceiling_db);
  else if (o.lookahead < 1 || o.lookahead > LM_LOOKAHEAD_MAX) snprintf(buf, nbuf, "lookahead %d outside 1 .. %d", o.lookahead, LM_LOOKAHEAD_MAX);
  else if (!lm_oversample_ok(o.oversample)) snprintf(buf, nbuf, "oversample %d is not one of 1, 2, 4, 8", o.oversample);
  else return nullptr;
  return buf;
}

// the detector's taps [n][15]: the resampler's table of the pair (1, n); none for n = 1.  false: n is no oversampling factor
inline bool lm_taps(int n, std::vector<float>& t) {
  t.clear();
  if (!lm_oversample_ok(n)) return false;
  if (n == 1) return true;
  RsGeom g;
  if (!rs_geometry(1, n, &g) || g.width != LM_WIDTH || g.K != LM_K) return false;
  rs_build_taps(g, t);
  return true;
}

inline float lm_ceiling(float ceiling_db) { return (float)pow(10.0, (double)ceiling_db / 20.0); }

// the gain of vx_finish_limited: vx_finish_loud's without the ceiling term; 1 when nothing passed the gates
inline float lm_gain(double loudness, float target_lufs, float max_gain_db) {
  if (!(loudness > -HUGE_VAL)) return 1.f;
  double g = pow(10.0, ((double)target_lufs - loudness) / 20.0);
  g = std::min(g, pow(10.0, (double)max_gain_db / 20.0));
  return (float)std::min(g, (double)FLT_MAX);
}

inline float lm_sample(float x) { return x - x == 0.f ? x : 0.f; }

// the demand of one detector reading
inline int32_t lm_demand(float P, float gs, float c) {
  const double den = (double)P * (double)gs;
  const double r = den > (double)c ? (double)c / den : 1.0;
  return (int32_t)(int64_t)floor(r * 16777216.0);
}

struct LmInfo { float peak, min_gain; int32_t reduced, nonfinite; };

// The whole contract for one row, sample by sample, with no decomposition: P [L], g [L] and out [L] may each be nullptr.
// taps: lm_taps(n).
inline void lm_row_reference(const float* x, long L, float gs, float c, int Wn, int n, const float* taps, float* out, float* P, float* g,
                             LmInfo* info) {
  const long N = 2L * Wn + 1;
  std::vector<float> y((size_t)L), Pv((size_t)L);
  std::vector<int32_t> q((size_t)L);
  info->peak = 0.f; info->min_gain = 1.f; info->reduced = 0; info->nonfinite = 0;
  for (long i = 0; i < L; ++i) {
    y[(size_t)i] = lm_sample(x[i]);
    if (!(x[i] - x[i] == 0.f)) ++info->nonfinite;
  }
  auto Y = [&](long i) { return i >= 0 && i < L ? y[(size_t)i] : 0.f; };
  for (long i = 0; i < L; ++i) {
    double top = fabs((double)y[(size_t)i]);
    for (int p = 0; p < (n > 1 ? n : 0); ++p) {
      double d = 0.0;
      for (int j = 0; j < LM_K; ++j) d += (double)taps[p * LM_K + j] * (double)Y(i + j - LM_WIDTH);
      top = std::max(top, fabs(d));
    }
    Pv[(size_t)i] = (float)top;
    q[(size_t)i] = lm_demand(Pv[(size_t)i], gs, c);
    info->peak = std::max(info->peak, Pv[(size_t)i]);
    if (P) P[i] = Pv[(size_t)i];
  }
  auto Q = [&](long k) { return k >= 0 && k < L ? (int64_t)q[(size_t)k] : (int64_t)LM_ONE; };
  auto M = [&](long i) {
    int64_t m = LM_ONE;
    for (long k = i - Wn; k <= i + Wn; ++k) m = std::min(m, Q(k));
    return m;
  };
  for (long i = 0; i < L; ++i) {
    int64_t s = 0;
    for (long k = i - Wn; k <= i + Wn; ++k) s += M(k);
    const float gi = (float)((double)s / (double)(N * LM_ONE));
    if (g) g[i] = gi;
    if (out) out[i] = (y[(size_t)i] * gs) * gi;
    info->min_gain = std::min(info->min_gain, gi);
    if (gi < 1.f) ++info->reduced;
  }
}

// The planner.  A part is the outputs [s, s + cnt) of one row together with the hl = min(2 Wn + 7, s) real samples in front of them and
// the hr = min(2 Wn + 7, L - s - cnt) behind them (zeros exist only outside the row).  A launch holds at most `win` samples, halos
// included, and `max_jobs` parts; rows are packed greedily in order, a row that does not fit the rest of a launch is cut anywhere.
// Tile records: ceil(cnt / tile) per part.
struct LmJob {
  int launch, row;
  long s, cnt, hl, hr;   // row samples [s - hl, s + cnt + hr), outputs [s, s + cnt)
  long off;              // first sample of the part (its front halo) in the launch's input buffer
  long out_off;          // first output of the part in the launch's output buffer
  long rec_off;          // first tile record of the part
};

// false: the window cannot hold a part's two halos plus one sample
inline bool lm_plan(const long* len, int batch, int Wn, long win, long max_jobs, int tile, std::vector<LmJob>* jobs) {
  jobs->clear();
  const long H = lm_halo(Wn);
  if (Wn < 1 || tile < 1 || max_jobs < 1 || win < 2 * H + 1) return false;
  int launch = 0;
  long used = 0, oused = 0, rused = 0, njobs = 0;
  for (int i = 0; i < batch; ++i) {
    const long L = len[i];
    long s = 0;
    while (s < L) {
      const long hl = std::min(H, s), room = win - used, rest = L - s;
      long take = rest, hr = 0;
      if (hl + rest > room) {                                      // cut: the part keeps a whole halo behind it (rest - take > H)
        take = room - hl - H;
        hr = H;
      }
      if (take <= 0 || njobs == max_jobs) {                        // nothing more fits this launch
        ++launch;
        used = oused = rused = njobs = 0;
        continue;
      }
      jobs->push_back({launch, i, s, take, hl, hr, used, oused, rused});
      used += hl + take + hr;
      oused += take;
      rused += (take + tile - 1) / tile;
      ++njobs;
      s += take;
    }
  }
  return true;
}

}  // namespace vxe
