// Host side of the time-stretch (stretch.hip, vx_stretch): option checking, the lengths and nominal positions of the WSOLA frames and
// the launch planner.
// Plain C++17 without the GPU runtime, so a stand-alone program (tools/stretch_host_check.cpp) runs exactly this code on a CPU --
// against the numpy restatement of the contract (tests/_stretch_refs.py), through the planner's invariants, under a sanitizer.
// Every length and position is 64-bit integer arithmetic as include/vallex_hip.h states it.
#pragma once

#include <stdio.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "../../include/vallex_hip.h"

namespace vxe {

constexpr int ST_HOP_MIN = 16, ST_HOP_MAX = 2048;
constexpr int ST_SEARCH_MAX = 1024;
constexpr int ST_SPEED_MAX = 32767;

struct StGeom { long num, den; int H, D; };      // the speed over its gcd, the hop, the search radius

// LDS of a workgroup that walks frames of hop H, search D (ws_walk.h: WsLds): four winners, two regions of 2D + 2H floats, the template
constexpr size_t ws_lds_bytes(int H, int D) { return 48 + (size_t)(2 * (2 * D + 2 * H) + H) * sizeof(float); }
static_assert(ws_lds_bytes(ST_HOP_MAX, ST_SEARCH_MAX) <= 65536, "LDS of the largest options");

// nullptr: the options are in range; else the message (in buf), naming the field
inline const char* st_check_opts(const vx_stretch_opts& o, char* buf, size_t nbuf) {
  if (o.hop < ST_HOP_MIN || o.hop > ST_HOP_MAX) snprintf(buf, nbuf, "hop %d outside %d .. %d", o.hop, ST_HOP_MIN, ST_HOP_MAX);
  else if (o.search < 0 || o.search > ST_SEARCH_MAX) snprintf(buf, nbuf, "search %d outside 0 .. %d", o.search, ST_SEARCH_MAX);
  else if (o.speed_num < 1 || o.speed_num > ST_SPEED_MAX) snprintf(buf, nbuf, "speed_num %d outside 1 .. %d", o.speed_num, ST_SPEED_MAX);
  else if (o.speed_den < 1 || o.speed_den > ST_SPEED_MAX) snprintf(buf, nbuf, "speed_den %d outside 1 .. %d", o.speed_den, ST_SPEED_MAX);
  else if (2 * (long)o.speed_num < (long)o.speed_den || (long)o.speed_num > 2 * (long)o.speed_den)
    snprintf(buf, nbuf, "speed_num / speed_den = %d / %d outside 1/2 .. 2", o.speed_num, o.speed_den);
  else return nullptr;
  return buf;
}

inline void st_reduce_speed(long num, long den, long* rn, long* rd) {
  const long g = std::gcd(num, den);
  *rn = num / g; *rd = den / g;
}

inline StGeom st_geometry(const vx_stretch_opts& o) {
  StGeom g;
  st_reduce_speed(o.speed_num, o.speed_den, &g.num, &g.den);
  g.H = o.hop; g.D = o.search;
  return g;
}

inline long st_out_len(const StGeom& g, long L) { return (L * g.den + g.num - 1) / g.num; }    // ceil(L den / num)
inline long st_frames(const StGeom& g, long L) { return (st_out_len(g, L) + g.H - 1) / g.H; }  // ceil(Lout / H)
inline long st_nominal(const StGeom& g, long k) { return k * g.H * g.num / g.den; }            // floor(k H num / den)

// The row samples the frames [k0, k1) of a row of L samples can read for any admissible p, cut to [0, L):
//   the regions [n_k - D, n_k + D + 2H) of the frames k >= 1 (search, new segment, next template), [0, 2H) of frame 0, and the first
//   template y[p_{k0-1} + H ..), which lies in [n_{k0-1} - D + H, n_{k0-1} + D + 2H).  n_k grows by at most 2H per frame, so the union
//   is one interval.
inline void st_span(const StGeom& g, long L, long k0, long k1, long* lo, long* hi) {
  long a = 0, b = 2L * g.H;
  if (k0 >= 1) a = std::min(st_nominal(g, k0 - 1) - g.D + g.H, st_nominal(g, k0) - g.D);
  if (k1 - 1 >= 1) b = st_nominal(g, k1 - 1) + g.D + 2L * g.H;        // n_k does not fall: this end covers the first template's too
  a =std::max(0L, std::min(a, L));
  b = std::max(a, std::min(b, L));
  *lo = a; *hi = b;
}

// The planner.  A launch holds at most `win` input samples, `out_cap` output samples, `frame_cap` frames and `max_jobs` jobs.  A job
// is the frames [k0, k1) of one row with exactly the span st_span gives; rows are packed into launches greedily in order.  A row that
// does not fit the rest of a launch is cut at a frame boundary and goes on in the NEXT launch: its next job starts from the position
// the previous launch found for frame k0 - 1.
struct StJob {
  int launch, row;
  long k0, k1;           // frames [k0, k1) of the row
  long s_lo, s_hi;       // staged samples [s_lo, s_hi) of the row, at in_off of the launch's input buffer
  long in_off, out_off;  // first input / output sample of the job in the launch's buffers
  long out_cnt;          // outputs of the job: [k0 H, min(k1 H, Lout))
  long f_off;            // first record of the job in the launch's position / cost tables
};

// false: one frame does not fit an EMPTY launch (its span above win, H above out_cap, or a cap below 1)
inline bool st_plan(const StGeom& g, const int* lens, int batch, long win, long out_cap, long frame_cap, long max_jobs,
                    std::vector<StJob>* jobs) {
  jobs->clear();
  if (max_jobs < 1 || frame_cap < 1) return false;
  int launch = 0;
  long in_used = 0, out_used = 0, f_used = 0, njobs = 0;
  auto next_launch = [&]() { ++launch; in_used = out_used = f_used = njobs = 0; };
  for (int i = 0; i < batch; ++i) {
    const long L = lens[i], olen = st_out_len(g, L), M = st_frames(g, L);
    long k0 = 0;
    while (k0 < M) {
      const long in_free = win - in_used, out_free = out_cap - out_used, f_free = frame_cap - f_used;
      // the largest k1 in (k0, M] whose span, outputs and frames fit (all three grow with k1): bisection
      auto fits = [&](long k1) {
        long lo, hi;
        st_span(g, L, k0, k1, &lo, &hi);
        return hi - lo <= in_free && std::min(k1 * g.H, olen) - k0 * g.H <= out_free && k1 - k0 <= f_free;
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
        next_launch();
        continue;
      }
      long lo, hi;
      st_span(g, L, k0, k1, &lo, &hi);
      const long cnt = std::min(k1 * g.H, olen) - k0 * g.H;
      jobs->push_back({launch, i, k0, k1, lo, hi, in_used, out_used, cnt, f_used});
      in_used += hi - lo;
      out_used += cnt;
      f_used += k1 - k0;
      ++njobs;
      k0 = k1;
      if (k0 < M) next_launch();                                   // the rest of the row needs this launch's positions
    }
  }
  return true;
}

}  // namespace vxe
