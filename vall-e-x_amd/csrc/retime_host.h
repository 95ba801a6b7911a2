// Host side of the time map (retime.hip, vx_pauses and vx_retime): option checking, the reduction of a row's frame table to its
// pauses, the anchor checks, the frames and nominal positions of a walked segment and the launch planner.
// Plain C++17 without the GPU runtime, so a stand-alone program (tools/retime_host_check.cpp) runs exactly this code on a CPU --
// against the numpy restatement of the contract (tests/_retime_refs.py), through the planner's invariants, under a sanitizer.
// Every length and position is 64-bit integer arithmetic as include/vallex_hip.h states it.
#pragma once

#include "finish_host.h"
#include "stretch_host.h"

namespace vxe {

constexpr long RT_TILE = 16384;                  // samples of a copy job at the most

// ---- vx_pauses -----------------------------------------------------------------------------------------------------------------
// nullptr: the options are in range; else the message (in buf), naming the field
inline const char* rt_check_pause_opts(const vx_pause_opts& o, char* buf, size_t nbuf) {
  if (o.frame < FN_FRAME_MIN || o.frame > FN_FRAME_MAX) snprintf(buf, nbuf, "frame %d outside %d .. %d", o.frame, FN_FRAME_MIN, FN_FRAME_MAX);
  else if (!(o.silence_db - o.silence_db == 0.f) || o.silence_db > 0.f) snprintf(buf, nbuf, "silence_db %g is not a finite value <= 0", (double)o.silence_db);
  else if (o.min_frames < 1) snprintf(buf, nbuf, "min_frames %d below 1", o.min_frames);
  else if (o.keep < 0) snprintf(buf, nbuf, "keep %d below 0", o.keep);
  else return nullptr;
  return buf;
}

// the pauses of a row from its frame table: begin, end of every pause appended to spans.  Quiet is the negation of fn_reduce's
// active test, operand for operand.
inline void rt_pauses(const FnFrame* t, long L, const vx_pause_opts& o, double thr2, std::vector<int>* spans) {
  const int F = o.frame;
  const long nf = fn_nframes(L, F);
  auto quiet = [&](long f) { return !(t[f].e > thr2 * (double)std::min<long>(F, L - f * F)); };
  long first = -1, last = -1;
  for (long f = 0; f < nf; ++f)
    if (!quiet(f)) {
      if (first < 0) first = f;
      last = f;
    }
  if (first < 0) return;                         // an all-quiet row has no pauses
  for (long f = first + 1; f < last;) {
    if (!quiet(f)) { ++f; continue; }
    long g = f;
    while (g < last && quiet(g)) ++g;            // frame `last` is active: the run ends in front of it at the latest
    if (g - f >= o.min_frames) {
      const long b = f * F + o.keep, e = g * F - (long)o.keep;
      if (b < e) { spans->push_back((int)b); spans->push_back((int)e); }
    }
    f = g;
  }
}

// ---- vx_retime -----------------------------------------------------------------------------------------------------------------
inline const char* rt_check_opts(const vx_retime_opts& o, char* buf, size_t nbuf) {
  if (o.hop < ST_HOP_MIN || o.hop > ST_HOP_MAX) snprintf(buf, nbuf, "hop %d outside %d .. %d", o.hop, ST_HOP_MIN, ST_HOP_MAX);
  else if (o.search < 0 || o.search > ST_SEARCH_MAX) snprintf(buf, nbuf, "search %d outside 0 .. %d", o.search, ST_SEARCH_MAX);
  else return nullptr;
  return buf;
}

// a walked segment of la input and lb output samples: its frames, and n_k - a_i for 1 <= k <= M - 1 (M >= 2)
inline long rt_frames(long lb, int H) { return lb / H; }
inline long rt_nominal(long la, long lb, int H, long k) {
  const long M = lb / H;
  return k * (la - lb + (M - 1) * H) / (M - 1);
}

// the anchors of one row of L samples, n of them at an[2 i], an[2 i + 1].  nullptr: they are a time map; *Lout = b_m and *frames =
// the frames of the walked segments.  Else the message (in buf), naming the anchor or the segment.
inline const char* rt_check_anchors(const int* an, long n, long L, int H, long* Lout, long* frames, char* buf, size_t nbuf) {
  *Lout = 0; *frames = 0;
  if (n < 1) { snprintf(buf, nbuf, "n_anchors %ld below 1", n); return buf; }
  if (an[0] != 0 || an[1] != 0) { snprintf(buf, nbuf, "anchors[0] = (%d, %d) is not (0, 0)", an[0], an[1]); return buf; }
  for (long i = 1; i < n; ++i) {
    const long la = (long)an[2 * i] - an[2 * i - 2], lb = (long)an[2 * i + 1] - an[2 * i - 1];
    if (la <= 0 || lb <= 0) {
      snprintf(buf, nbuf, "anchors[%ld] = (%d, %d) does not increase over anchors[%ld] = (%d, %d)", i, an[2 * i], an[2 * i + 1], i - 1,
               an[2 * i - 2], an[2 * i - 1]);
      return buf;
    }
    if (la == lb) continue;
    if (la < 2L * H || lb < 2L * H) {
      snprintf(buf, nbuf, "segment %ld is walked (la %ld, lb %ld) and shorter than 2 hop = %d", i - 1, la, lb, 2 * H);
      return buf;
    }
    if (la > 4 * lb || lb > 4 * la) { snprintf(buf, nbuf, "segment %ld: la / lb = %ld / %ld outside 1/4 .. 4", i - 1, la, lb); return buf; }
    *frames += rt_frames(lb, H);
  }
  if (an[2 * (n - 1)] != L) {
    snprintf(buf, nbuf, "anchors[%ld] = (%d, %d): a_m is not the row's length %ld", n - 1, an[2 * (n - 1)], an[2 * (n - 1) + 1], L);
    return buf;
  }
  *Lout = an[2 * (n - 1) + 1];
  return nullptr;
}

// The planner.  A launch holds at most `win` input samples, `out_cap` output samples, `frame_cap` frames and `max_jobs` jobs.  A
// walked segment is exactly one job with the span [a - D, a1 + D + H) cut to the row: everything its frames can read.  The copy
// segments between two walked ones are one span, cut into jobs of at most `tile` samples and at the end of a launch.  Jobs are packed
// into launches greedily in order; no job needs another's result.
struct RtJob {
  int launch, row, walk;   // walk: 1 a walked segment, 0 a copy tile
  long a, a1;              // input samples [a, a1) of the row
  long b, lb;              // output samples [b, b + lb) of the row
  long s_lo, s_hi;         // staged samples [s_lo, s_hi) of the row, at in_off of the launch's input buffer
  long in_off, out_off;    // first input / output sample of the job in the launch's buffers
  long f_off, f_row;       // walked: first record of the job in the launch's position / cost tables, and in the row's
};

// false: a walked segment does not fit an EMPTY launch (*bad_row, *bad_seg say which), or a cap is below 1
inline bool rt_plan(const int* anchors, long anchor_stride, const int* n_anchors, const int* lens, int batch, int H, int D, long win,
                    long out_cap, long frame_cap, long max_jobs, long tile, std::vector<RtJob>* jobs, int* bad_row, long* bad_seg) {
  jobs->clear();
  *bad_row = -1; *bad_seg = -1;
  if (win < 1 || out_cap < 1 || frame_cap < 1 || max_jobs < 1 || tile < 1) return false;
  int launch = 0;
  long in_used = 0, out_used = 0, f_used = 0, njobs = 0;
  auto next_launch = [&]() { ++launch; in_used = out_used = f_used = njobs = 0; };
  for (int r = 0; r < batch; ++r) {
    const int* an = anchors + (long)r * anchor_stride;
    const long L = lens[r], n = n_anchors[r];
    long f_row = 0, ra = 0, ra1 = 0, rb = 0;                        // the open run of copy segments: input [ra, ra1), output from rb
    auto flush = [&]() {
      for (long s = ra; s < ra1;) {
        const long take = std::min(std::min(ra1 - s, tile), std::min(win - in_used, out_cap - out_used));
        if (take <= 0 || njobs == max_jobs) { next_launch(); continue; }
        jobs->push_back({launch, r, 0, s, s + take, rb + (s - ra), take, s, s + take, in_used, out_used, f_used, f_row});
        in_used += take; out_used += take; ++njobs;
        s += take;
      }
      ra = ra1;
    };
    for (long i = 0; i + 1 < n; ++i) {
      const long a = an[2 * i], b = an[2 * i + 1], a1 = an[2 * i + 2], b1 = an[2 * i + 3];
      const long la = a1 - a, lb = b1 - b;
      if (la == lb) {
        if (ra == ra1) { ra = a; rb = b; }
        ra1 = a1;
        continue;
      }
      flush();
      const long lo = std::max(0L, a - D), hi = std::min(L, a1 + D + H), M = rt_frames(lb, H);
      if (hi - lo > win || lb > out_cap || M > frame_cap) { *bad_row = r; *bad_seg = i; return false; }
      if (hi - lo > win - in_used || lb > out_cap - out_used || M > frame_cap - f_used || njobs == max_jobs) next_launch();
      jobs->push_back({launch, r, 1, a, a1, b, lb, lo, hi, in_used, out_used, f_used, f_row});
      in_used += hi - lo; out_used += lb; f_used += M; f_row += M; ++njobs;
      ra = ra1 = a1;
    }
    flush();
  }
  return true;
}

}  // namespace vxe
