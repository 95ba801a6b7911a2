// Host side of the spectral noise suppression (denoise.hip, vx_denoise): the tables, option checking, the frame counts, the choice of
// the noise frames (which runs between the power and the profile launch), the launch planner and a sequential reference of the whole
// contract.
// Plain C++17 without the GPU runtime, so a stand-alone program (tools/denoise_host_check.cpp) runs exactly this code on a CPU -- against
// the numpy restatement of the contract (tests/_denoise_refs.py), through the planner's invariants, under a sanitizer.
// Every floating-point operation is a separately rounded double operation, as include/vallex_hip.h states them: the arithmetic below is
// compiled with contraction off.
#pragma once

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../include/vallex_hip.h"

namespace vxe {

constexpr int DN_N = 512, DN_H = 128, DN_B = 257;              // frame, hop, bins
constexpr int DN_MAX_JOBS = 256;                               // rows of a launch
static_assert(DN_N == VX_DENOISE_N && DN_H == VX_DENOISE_HOP && DN_B == VX_DENOISE_BINS, "the constants of the header");

#if defined(__clang__)
#define VX_DN_NO_CONTRACT _Pragma("clang fp contract(off)")
#define VX_DN_NO_CONTRACT_FN
#elif defined(__GNUC__)
#define VX_DN_NO_CONTRACT
#define VX_DN_NO_CONTRACT_FN __attribute__((optimize("fp-contract=off")))
#else
#define VX_DN_NO_CONTRACT
#define VX_DN_NO_CONTRACT_FN
#endif

// the tables the library uses, [w 512][c 256][s 256]: vx_denoise_tables reports these words
VX_DN_NO_CONTRACT_FN inline void dn_tables(double* t) {
  VX_DN_NO_CONTRACT
  const double two_pi = 2.0 * 3.14159265358979323846;
  for (int n = 0; n < DN_N; ++n) t[n] = sqrt(0.5 - 0.5 * cos(two_pi * (double)n / (double)DN_N));
  for (int k = 0; k < DN_N / 2; ++k) {
    t[DN_N + k] = cos(two_pi * (double)k / (double)DN_N);
    t[DN_N + DN_N / 2 + k] = -sin(two_pi * (double)k / (double)DN_N);
  }
}

// the twiddles in the order the stages read them: at [h + p], h = 1, 2 .. 256, p in [0, h), the word c[q] / s[q] of q = p (256 / h)
inline void dn_stage_tables(const double* t, double* tc, double* ts) {
  tc[0] = ts[0] = 0.0;
  for (int h = 1; h < DN_N; h <<= 1)
    for (int p = 0; p < h; ++p) {
      tc[h + p] = t[DN_N + p * (DN_N / 2 / h)];
      ts[h + p] = t[DN_N + DN_N / 2 + p * (DN_N / 2 / h)];
    }
}

// nullptr: the options are in range; else the message (in buf), naming the field
inline const char* dn_check_opts(const vx_denoise_opts& o, char* buf, size_t nbuf) {
  if (!(o.alpha >= 0.f) || !(o.alpha <= 3.0e38f)) snprintf(buf, nbuf, "alpha %g not finite or below 0", (double)o.alpha);
  else if (!(o.floor > 0.f) || !(o.floor <= 1.f)) snprintf(buf, nbuf, "floor %g outside (0, 1]", (double)o.floor);
  else if (!(o.frac >= 0.f) || !(o.frac <= 1.f)) snprintf(buf, nbuf, "frac %g outside [0, 1]", (double)o.frac);
  else if (o.kmin < 0) snprintf(buf, nbuf, "kmin %d below 0", o.kmin);
  else return nullptr;
  return buf;
}

inline long dn_frames(long L) { return (L + DN_H - 1) / DN_H + 3; }                               // T
inline long dn_hops(long L) { return (L + DN_H - 1) / DN_H; }                                     // synthesis workgroups of a row
inline long dn_full(long L) { return std::max(0L, L / DN_H - 3); }                                // F: frames 3 .. L / H - 1
inline long dn_frame_cap(long win) { return win / DN_H + 3L * DN_MAX_JOBS; }                      // frames of a launch, at most

VX_DN_NO_CONTRACT_FN inline long dn_k(const vx_denoise_opts& o, long F) {                         // K = min(max(kmin, floor(frac F)), F)
  VX_DN_NO_CONTRACT
  const long k = (long)floor((double)o.frac * (double)F);
  return std::min(std::max((long)o.kmin, k), F);
}

// the K full frames smallest in the total order (E[t], t), in ascending t.  E: the row's T energies.
inline void dn_select(const double* E, long L, long K, std::vector<int32_t>* sel) {
  sel->clear();
  const long F = dn_full(L);
  if (K <= 0 || F <= 0) return;
  std::vector<std::pair<double, int32_t>> v;
  v.reserve((size_t)F);
  for (long t = 3; t < 3 + F; ++t) v.push_back({E[t], (int32_t)t});
  std::sort(v.begin(), v.end());
  for (long i = 0; i < std::min(K, F); ++i) sel->push_back(v[(size_t)i].second);
  std::sort(sel->begin(), sel->end());
}

// The planner.  A launch holds at most `win` samples, `frame_cap` frames and `max_jobs` rows.  A row is never cut: rows are packed
// into launches greedily in order.
struct DnJob {
  int launch, row;
  long in_off;           // first sample of the row in the launch's input and output buffers
  long f_off, h_off;     // first frame (of P and E) and first synthesis workgroup of the row in the launch
};

// false: a row does not fit an EMPTY launch
inline bool dn_plan(const int* lens, int batch, long win, long frame_cap, long max_jobs, std::vector<DnJob>* jobs) {
  jobs->clear();
  if (max_jobs < 1) return false;
  int launch = 0;
  long in_used = 0, f_used = 0, h_used = 0, njobs = 0;
  for (int i = 0; i < batch;) {
    const long L = lens[i], T = dn_frames(L);
    if (njobs < max_jobs && in_used + L <= win && f_used + T <= frame_cap) {
      jobs->push_back({launch, i, in_used, f_used, h_used});
      in_used += L; f_used += T; h_used += dn_hops(L);
      ++njobs; ++i;
      continue;
    }
    if (njobs == 0) return false;
    ++launch; in_used = f_used = h_used = njobs = 0;
  }
  return true;
}

inline bool dn_finite(float x) {
  uint32_t u;
  memcpy(&u, &x, sizeof u);
  return (u & 0x7f800000u) != 0x7f800000u;
}

inline int dn_nonfinite(const float* x, long L) {
  long n = 0;
  for (long i = 0; i < L; ++i) n += dn_finite(x[i]) ? 0 : 1;
  return (int)std::min(n, 0x7fffffffL);
}

// a usable noise profile: 257 finite words, none below 0
inline bool dn_psd_ok(const double* psd) {
  for (int k = 0; k < DN_B; ++k)
    if (!(psd[k] >= 0.0) || !(psd[k] <= 1.7e308)) return false;
  return true;
}

inline int dn_rev9(int i) {
  int r = 0;
  for (int b = 0; b < 9; ++b) r |= ((i >> b) & 1) << (8 - b);
  return r;
}

// the network of the contract on natural-order input: re / im [512] in, [512] out (in place); t the tables
VX_DN_NO_CONTRACT_FN inline void dn_fft_ref(const double* t, double* re, double* im, bool inverse) {
  VX_DN_NO_CONTRACT
  const double *c = t + DN_N, *s = t + DN_N + DN_N / 2;
  double br[DN_N], bi[DN_N];
  for (int i = 0; i < DN_N; ++i) { br[i] = re[dn_rev9(i)]; bi[i] = im[dn_rev9(i)]; }
  for (int m = 2; m <= DN_N; m <<= 1) {
    const int h = m / 2;
    for (int j = 0; j < DN_N / 2; ++j) {
      const int g = j / h, p = j % h, i0 = g * m + p, i1 = i0 + h, q = p * (DN_N / m);
      const double cq = c[q], sq = inverse ? -s[q] : s[q];
      const double tr = cq * br[i1] - sq * bi[i1], ti = cq * bi[i1] + sq * br[i1];
      const double ar = br[i0], ai = bi[i0];
      br[i0] = ar + tr; bi[i0] = ai + ti;
      br[i1] = ar - tr; bi[i1] = ai - ti;
    }
  }
  memcpy(re, br, sizeof br);
  memcpy(im, bi, sizeof bi);
}

struct DnRef {
  std::vector<double> P, E, Nz, gain;      // [T][257], [T], [257], [T][257]
  std::vector<int32_t> sel;
  vx_denoise_info info;
};

// The sequential reference of the whole contract for one row.  psd: the caller's profile or nullptr.
VX_DN_NO_CONTRACT_FN inline void denoise_reference(const vx_denoise_opts& o, const float* x, long L, const double* psd, float* out, DnRef* r) {
  VX_DN_NO_CONTRACT
  std::vector<double> t(2 * DN_N);
  dn_tables(t.data());
  const double* w = t.data();
  const long T = dn_frames(L), F = dn_full(L);
  auto y = [&](long s) -> double { return s >= 0 && s < L && dn_finite(x[s]) ? (double)x[s] : 0.0; };
  std::vector<double> re((size_t)T * DN_N), im((size_t)T * DN_N, 0.0);
  r->P.assign((size_t)T * DN_B, 0.0);
  r->E.assign((size_t)T, 0.0);
  for (long f = 0; f < T; ++f) {
    double* fr = re.data() + f * DN_N;
    double* fi = im.data() + f * DN_N;
    for (int n = 0; n < DN_N; ++n) fr[n] = y((f - 3) * DN_H + n) * w[n];
    dn_fft_ref(t.data(), fr, fi, false);
    double e = 0.0;
    for (int k = 0; k < DN_B; ++k) {
      const double p = fr[k] * fr[k] + fi[k] * fi[k];
      r->P[(size_t)f * DN_B + k] = p;
      e = e + p;
    }
    r->E[(size_t)f] = e;
  }
  r->Nz.assign(DN_B, 0.0);
  long K = 0;
  r->sel.clear();
  if (psd) {
    for (int k = 0; k < DN_B; ++k) r->Nz[(size_t)k] = psd[k];
  } else {
    K = dn_k(o, F);
    dn_select(r->E.data(), L, K, &r->sel);
    if (K > 0)
      for (int k = 0; k < DN_B; ++k) {
        double a = 0.0;
        for (int32_t f : r->sel) a = a + r->P[(size_t)f * DN_B + k];
        r->Nz[(size_t)k] = a / (double)K;
      }
  }
  const double alpha = (double)o.alpha, fl = (double)o.floor;
  r->gain.assign((size_t)T * DN_B, 0.0);
  std::vector<double> acc((size_t)(dn_hops(L) * DN_H), 0.0);
  for (long f = 0; f < T; ++f) {
    auto cl = [&](long q) { return (size_t)std::min(std::max(q, 0L), T - 1) * DN_B; };
    double* fr = re.data() + f * DN_N;
    double* fi = im.data() + f * DN_N;
    for (int k = 0; k < DN_B; ++k) {
      const double S = ((((r->P[cl(f - 2) + k] + r->P[cl(f - 1) + k]) + r->P[cl(f) + k]) + r->P[cl(f + 1) + k]) + r->P[cl(f + 2) + k]) / 5.0;
      double g = S > 0.0 ? 1.0 - (alpha * r->Nz[(size_t)k]) / S : fl;
      g = g > fl ? g : fl;
      r->gain[(size_t)f * DN_B + k] = g;
    }
    for (int i = 0; i < DN_N; ++i) {
      const double g = r->gain[(size_t)f * DN_B + (i <= DN_N / 2 ? i : DN_N - i)];
      fr[i] = fr[i] * g;
      fi[i] = fi[i] * g;
    }
    dn_fft_ref(t.data(), fr, fi, true);
    for (int n = 0; n < DN_N; ++n) {                                 // ascending f: the order of the contract's accumulation
      const long i = (f - 3) * DN_H + n;
      if (i >= 0 && i < L) acc[(size_t)i] = acc[(size_t)i] + (fr[n] * (1.0 / DN_N)) * w[n];
    }
  }
  for (long i = 0; i < L; ++i) out[i] = (float)(0.5 * acc[(size_t)i]);
  r->info.frames = (int32_t)T;
  r->info.full_frames = (int32_t)F;
  r->info.k = (int32_t)K;
  r->info.nonfinite = dn_nonfinite(x, L);
}

}  // namespace vxe
