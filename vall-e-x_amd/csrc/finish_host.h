// Host side of the output stage (finish.hip, vx_finish): option checking, the silence threshold, the reduction of a row's frame table
// to its span, peak, mean square and gain, the fade tables and the launch planner of both passes.
// Plain C++17 without the GPU runtime, so a stand-alone program (tools/finish_host_check.cpp) runs exactly this code on a CPU --
// against the numpy restatement of the contract (tests/_finish_refs.py), through the planner's invariants, under a sanitizer.
// Every quantity is computed as include/vallex_hip.h states it: in double, in frame order, with one rounding where a float leaves.
#pragma once

#include <float.h>
#include <math.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../include/vallex_hip.h"

namespace vxe {

constexpr int FN_FRAME_MIN = 16, FN_FRAME_MAX = 4096;
constexpr int FN_FADE_MAX = 1 << 20;

struct FnFrame { double e; float p; int z; };       // one frame of the table: sum of squares, max |y|, non-finite samples
static_assert(sizeof(FnFrame) == 16, "the kernel writes 16-byte frame records");

// nullptr: the options are in range; else the message (in buf), naming the field
inline const char* fn_check_opts(const vx_finish_opts& o, char* buf, size_t nbuf) {
  auto fin = [](float v) { return v - v == 0.f; };
  if (o.frame < FN_FRAME_MIN || o.frame > FN_FRAME_MAX) snprintf(buf, nbuf, "frame %d outside %d .. %d", o.frame, FN_FRAME_MIN, FN_FRAME_MAX);
  else if (!fin(o.silence_db) || o.silence_db > 0.f) snprintf(buf, nbuf, "silence_db %g is not a finite value <= 0", (double)o.silence_db);
  else if (o.trim < 0 || o.trim > 3) snprintf(buf, nbuf, "trim %d outside 0 .. 3", o.trim);
  else if (o.keep < 0) snprintf(buf, nbuf, "keep %d below 0", o.keep);
  else if (o.level_mode < VX_LEVEL_NONE || o.level_mode > VX_LEVEL_RMS) snprintf(buf, nbuf, "level_mode %d is no VX_LEVEL_*", o.level_mode);
  else if (!fin(o.level_db) || o.level_db > 0.f) snprintf(buf, nbuf, "level_db %g is not a finite value <= 0", (double)o.level_db);
  else if (!fin(o.max_gain_db) || o.max_gain_db < 0.f) snprintf(buf, nbuf, "max_gain_db %g is not a finite value >= 0", (double)o.max_gain_db);
  else if (o.fade_in < 0 || o.fade_in > FN_FADE_MAX) snprintf(buf, nbuf, "fade_in %d outside 0 .. %d", o.fade_in, FN_FADE_MAX);
  else if (o.fade_out < 0 || o.fade_out > FN_FADE_MAX) snprintf(buf, nbuf, "fade_out %d outside 0 .. %d", o.fade_out, FN_FADE_MAX);
  else if (o.format != VX_PCM_F32 && o.format != VX_PCM_S16) snprintf(buf, nbuf, "format %d is no VX_PCM_*", o.format);
  else return nullptr;
  return buf;
}

inline double fn_thr2(float silence_db) { return pow(10.0, (double)silence_db / 10.0); }
inline long fn_nframes(long L, int F) { return (L + F - 1) / F; }

// what the frame table of a row says: the kept span, the counts, the peak over the frames that intersect the span, the mean square
// over the active frames (frame order, double), the gain (double, rounded once)
inline void fn_reduce(const FnFrame* t, long L, const vx_finish_opts& o, double thr2, vx_wave_info* w) {
  const int F = o.frame;
  const long nf = fn_nframes(L, F);
  long a = -1, z = -1, nact = 0, cnt = 0, nonfinite = 0;
  double esum = 0.0;
  for (long f = 0; f < nf; ++f) {
    const long n_f = std::min<long>(F, L - f * F);
    nonfinite += t[f].z;
    if (t[f].e > thr2 * (double)n_f) {
      if (a < 0) a = f;
      z = f;
      ++nact;
      esum += t[f].e;
      cnt += n_f;
    }
  }
  long begin = 0, end = L;
  if (nact == 0) {
    if (o.trim & 1) end = 0;                 // begin = end = 0 on any trimmed side
    if (o.trim & 2) end = 0;
  } else {
    if (o.trim & 1) begin = std::max<long>(0, a * F - o.keep);
    if (o.trim & 2) end = std::min<long>(L, (z + 1) * F + (long)o.keep);
  }
  float peak = 0.f;
  if (end > begin)
    for (long f = begin / F; f <= (end - 1) / F; ++f) peak = std::max(peak, t[f].p);
  const double ms = nact ? esum / (double)cnt : 0.0;
  double g = 1.0;
  if (nact && o.level_mode != VX_LEVEL_NONE) {
    const double den = o.level_mode == VX_LEVEL_PEAK ? (double)peak : sqrt(ms);
    if (den != 0.0) {
      const double tgt = pow(10.0, (double)o.level_db / 20.0), cap = pow(10.0, (double)o.max_gain_db / 20.0);
      g = std::min(std::min(tgt / den, cap), (double)FLT_MAX);
    }
  }
  w->begin = (int32_t)begin; w->end = (int32_t)end;
  w->active_frames = (int32_t)nact; w->nonfinite = (int32_t)nonfinite; w->clipped = 0;
  w->peak = peak; w->gain = (float)g; w->mean_square = ms;
}

// the smoothstep table of an n-sample fade: w(u) = u u (3 - 2u) at u = (j + 0.5) / n, double with + - * / only, rounded once
inline void fn_fade_table(int n, std::vector<float>& t) {
  t.resize((size_t)std::max(n, 0));
  for (int j = 0; j < n; ++j) {
    const double u = ((double)j + 0.5) / (double)n;
    const double uu = u * u;
    const double r = 3.0 - 2.0 * u;          // 2u is exact: a contraction to an fma changes no bit
    const double w = uu * r;
    t[(size_t)j] = (float)w;
  }
}

// The planner.  A launch holds at most `win` input samples and `max_jobs` jobs; rows are packed into launches greedily in order.
// Measure pass: the samples [0, L) of every row, a row that does not fit the rest of a launch is cut at a multiple of the frame
// (win >= frame).  Apply pass: the kept span [begin, end) of every row, cut anywhere.
struct FnJob {
  int launch, row;
  long s_lo, cnt;        // row samples [s_lo, s_lo + cnt)
  long off;              // first sample of the job in the launch's input buffer (and, apply pass, in its output buffer)
  long f_off;            // measure pass: first record of the job in the launch's frame table
};

inline bool fn_plan(const long* lo, const long* hi, int batch, long win, long max_jobs, int frame /* 0: cut anywhere */,
                    std::vector<FnJob>* jobs) {
  jobs->clear();
  if (win < std::max(1, frame) || max_jobs < 1) return false;
  int launch = 0;
  long used = 0, fused = 0, njobs = 0;
  for (int i = 0; i < batch; ++i) {
    long s = lo[i];
    while (s < hi[i]) {
      const long room = win - used, rest = hi[i] - s;
      long take = rest <= room ? rest : frame ? room / frame * frame : room;
      if (take <= 0 || njobs == max_jobs) {                      // nothing more fits this launch
        ++launch;
        used = fused = njobs = 0;
        continue;
      }
      jobs->push_back({launch, i, s, take, used, fused});
      used += take;
      if (frame) fused += fn_nframes(take, frame);
      ++njobs;
      s += take;
    }
  }
  return true;
}

}  // namespace vxe
