// Host side of the resampler (resample.hip, vx_resample): the geometry of a rate pair, the tap table and the window planner.
// Plain C++17 without the GPU runtime, so a stand-alone program (tools/resample_host_check.cpp) runs exactly this code on a CPU --
// against the torch taps, through the planner's invariants, under a sanitizer.
#pragma once

#include <math.h>

#include <algorithm>
#include <numeric>
#include <vector>

namespace vxe {

constexpr long RS_MAX_TAPS = 1L << 18;     // n K of a pair vx_resample accepts (1 MiB of fp32)

struct RsGeom { long o, n, width, K; };

// geometry of a rate pair (both rates > 0); false: more than 2^18 taps (K alone, or n K)
inline bool rs_geometry(long orig, long neu, RsGeom* g) {
  const long d = std::gcd(orig, neu);
  g->o = orig / d; g->n = neu / d;
  const double base = (double)std::min(g->o, g->n) * 0.99;
  const double w = ceil((double)(6 * g->o) / base);
  g->width = w < 1e9 ? (long)w : 1000000000L;
  g->K = 2 * g->width + g->o;
  return g->K <= RS_MAX_TAPS && g->n * g->K <= RS_MAX_TAPS;
}

inline long rs_out_len(const RsGeom& g, long L) { return (g.n * L + g.o - 1) / g.o; }      // ceil(n L / o)

// the n phase kernels, [n][K]: resample_sinc_hann's operations in its order.  The phase term is an fp32 quotient widened to double,
// everything else is double, one rounding to fp32 at the end.
inline void rs_build_taps(const RsGeom& g, std::vector<float>& t) {
  const double pi = 3.141592653589793, lpw = 6.0;
  const double base = (double)std::min(g.o, g.n) * 0.99, scale = base / (double)g.o;
  t.resize((size_t)(g.n * g.K));
  for (long p = 0; p < g.n; ++p) {
    const double ph = (double)((float)(-p) / (float)g.n);
    for (long j = 0; j < g.K; ++j) {
      double x = (ph + (double)(j - g.width) / (double)g.o) * base;
      x = x < -lpw ? -lpw : x > lpw ? lpw : x;
      const double c = cos(x * pi / lpw / 2.0), win = c * c;
      x = x * pi;
      const double sinc = x == 0.0 ? 1.0 : sin(x) / x;
      t[(size_t)(p * g.K + j)] = (float)(sinc * win * scale);
    }
  }
}

// The planner.  A launch holds at most `win` input samples, `out_cap` output samples and `max_jobs` jobs.  A row of L samples is a run
// of blocks [0, nblk), nblk = ceil(out_len / n); the blocks [a, b) need the row's samples [a o - width, (b - 1) o - width + K) cut to
// [0, L) -- real samples on both sides of a window, zeros only outside the row -- and give the outputs [a n, min(b n, out_len)).
// Rows are packed into launches greedily in order; a row that does not fit the rest of a launch is cut there.
struct RsJob {
  int launch, row;
  long a, b;             // blocks [a, b) of the row
  long s_lo, s_hi;       // staged samples [s_lo, s_hi) of the row, at in_off of the launch's input buffer
  long in_off, out_off;  // first input / output sample of the job in the launch's buffers
  long out_cnt;          // outputs of the job
};

// false: a block does not fit an EMPTY launch (K > win or n > out_cap: the caller rules both out)
inline bool rs_plan(const RsGeom& g, const int* lens, int batch, long win, long out_cap, long max_jobs, std::vector<RsJob>* jobs) {
  jobs->clear();
  int launch = 0;
  long in_used = 0, out_used = 0, njobs = 0;
  for (int i = 0; i < batch; ++i) {
    const long L = lens[i], olen = rs_out_len(g, L), nblk = (olen + g.n - 1) / g.n;
    long a = 0;
    while (a < nblk) {
      const long in_free = win - in_used, out_free = out_cap - out_used;
      const long s_lo = std::max<long>(0, a * g.o - g.width);
      long b = nblk;                                             // the rest of the row, if it fits
      if (L - s_lo > in_free) {                                  // else up to the last block whose span ends inside the free input
        const long room = in_free + s_lo + g.width - g.K;        // (b - 1) o <= room
        b = room < 0 ? a : std::min(nblk, room / g.o + 1);
      }
      b = std::min(b, a + out_free / g.n);
      if (b <= a || njobs == max_jobs) {                         // nothing more fits this launch
        if (njobs == 0) return false;
        ++launch;
        in_used = out_used = njobs = 0;
        continue;
      }
      const long s_hi = std::max(s_lo, std::min(L, (b - 1) * g.o - g.width + g.K));
      const long cnt = std::min(b * g.n, olen) - a * g.n;
      jobs->push_back({launch, i, a, b, s_lo, s_hi, in_used, out_used, cnt});
      in_used += s_hi - s_lo;
      out_used += cnt;
      ++njobs;
      a = b;
    }
  }
  return true;
}

}  // namespace vxe
