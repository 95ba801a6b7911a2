// The fundamental frequency (vx_f0, include/vallex_hip.h): F0 per frame of mono fp32 rows by YIN.
//
// Frame k of a row reads y[s_k, s_k + W + lag_max), s_k = k H + H/2 - (W + lag_max)/2: the difference d(t) = sum_j (y[j] - y[j + t])^2
// for every lag t in [0, lag_max], its cumulative-mean normalisation d'(t) = d(t) t / (d(1) + .. + d(t)), the first dip of d' under the
// threshold (else its minimum), and a parabola through the three values around it.  The contract -- sums, prefix, tie rules, every
// rounding -- is in the header; f0_host.h has the integers, the pick (f0_choose, which the kernel runs as it stands) and a sequential
// reference.
//
// Arithmetic (the contract the tests rest on): lag t is summed by ONE lane in double in sample order from 0.0, with the subtraction,
// the product and the addition rounded separately (contraction is off: e * e is not exact in double, so an fma would change bits); the
// prefix c(t) is one lane's serial walk in lag order; d'(t) is one product and one division.  The bits therefore depend neither on the
// lane, the group, the job, the window nor the launch a frame lands in.  No atomics, no inline assembly.
//
// Work decomposition: frames are independent.  A launch covers a ragged list of JOBS (the frames [k0, k1) of one row: a whole row, or
// one part of a long one); a 256-thread workgroup takes G consecutive frames of one job, P lanes each (P = 64, 128 or 256: the smallest
// that gives every lag up to lag_max a lane, or 256; G = 256 / P, cut down until the frames fit 60 KiB of LDS).  A frame's samples
// are widened once to double in LDS (with zeros outside the row and in place of non-finite samples: the padding never exists in HBM);
// lane t of the frame reads y[j] as a broadcast and y[j + t] at stride 1 across the lanes (8-byte reads: no bank conflict).  d and d'
// stay in LDS: lane 0 of the frame walks the prefix, all lanes divide, lane 0 picks.
// LDS per frame: (W + lag_max + 2 (lag_max + 1)) doubles -- 40 976 bytes at the largest options, 11.2 KiB at W 600, lag_max 400.
#include "wave_stage.h"
#include "f0_host.h"

#include "../../include/vallex_hip_dev.h"

namespace vxe {

constexpr int F0_TAB = RS_TAB;                               // ints of a job record
constexpr int F0_MAX_JOBS = RS_MAX_JOBS;                     // the records of a launch fill rs_meta
constexpr long F0_FRAME_CAP = 1L << 20;                      // frames of a launch: f0, lag and ap take the first 3 F0_FRAME_CAP words of rs_out
constexpr long F0_TABLE_AT = 4 * F0_FRAME_CAP;               // first float of the d table in rs_out (vx_dev_f0_table); d' half-way behind it
constexpr long F0_TABLE_CAP = (RS_OUT_CAP - F0_TABLE_AT) / 4;   // doubles of each table
constexpr size_t F0_LDS_MAX = 60 * 1024;
static_assert(VX_F0_WINDOW == RS_IN_CAP, "vx_f0 runs in the resampler's launch buffers");
static_assert(VX_DEV_F0_WINDOW_MIN >= F0_WIN_MAX + F0_LAG_MAX && VX_DEV_F0_WINDOW_MIN <= VX_F0_WINDOW, "window bounds of the dev header");
static_assert((F0_WIN_MAX + F0_LAG_MAX + 2 * (F0_LAG_MAX + 1)) * sizeof(double) <= F0_LDS_MAX, "LDS of the largest options");
static_assert(F0_TABLE_CAP >= F0_LAG_MAX + 1 && F0_TABLE_AT % 2 == 0, "the dev tables hold a frame and are 8-byte aligned");

// tab [njobs][F0_TAB]:
//   0 in_off   first float of the job's staged samples in `in`
//   1 s_lo     row sample index of that float;  2 in_cnt  staged samples: the job's span cut to [0, L)
//   3 k0, 4 k1 frames of the job;  5 f_off  first record of the job in f0 / lag / ap (and the tables)
//   6 b_off    first workgroup of the job: workgroup b_off + i takes the frames k0 + i G .. of it
// lp: log2 of the lanes per frame
__global__ __launch_bounds__(256) void f0_frames_kernel(const float* __restrict__ in, const int* __restrict__ tab, int njobs,
                                                        float* __restrict__ f0, int* __restrict__ lag, float* __restrict__ ap,
                                                        double* __restrict__ dtab, double* __restrict__ dptab, F0Geom g, int lp, int G) {
  extern __shared__ double f0_lds[];
  const int tid = threadIdx.x, P = 1 << lp, grp = tid >> lp, ln = tid & (P - 1);
  int jl = 0, jh = njobs - 1;                                    // the job of this workgroup: the last one with b_off <= blockIdx.x
  while (jl < jh) {
    const int m = (jl + jh + 1) >> 1;
    if (tab[m * F0_TAB + 6] <= (int)blockIdx.x) jl = m; else jh = m - 1;
  }
  const int* tb = tab + jl * F0_TAB;
  const long in_off = tb[0], s_lo = tb[1], in_cnt = tb[2], f_off = tb[5];
  const long k = (long)tb[3] + (long)((int)blockIdx.x - tb[6]) * G + grp;
  const bool live = grp < G && k < tb[4];
  const int R = g.W + g.T, T1 = g.T + 1;
  double* y = f0_lds + (live ? (size_t)grp * (size_t)(R + 2 * T1) : 0);      // [R] the frame's samples
  double* d = y + R;                                                          // [T1]
  double* dp = d + T1;                                                        // [T1] c(t), then d'(t)
  if (live) {
    // sample s of the row: 0 outside the row and where it is not finite; the job holds every sample of the row its frames read
    // (f0_host.h: f0_span) -- the range test keeps a wrong table inside the buffer
    const long s = k * g.H + g.H / 2 - R / 2;
    for (int i = ln; i < R; i += P) {
      const long r = s + i - s_lo;
      float x = 0.f;
      if (r >= 0 && r < in_cnt) x = in[in_off + r];
      y[i] = (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u ? (double)x : 0.0;
    }
  }
  __syncthreads();
  if (live) {
    for (int t = ln; t < T1; t += P) {
      const double* yt = y + t;
      double acc = 0.0;
      {
#pragma clang fp contract(off)
#pragma unroll 8
        for (int j = 0; j < g.W; ++j) {
          const double e = y[j] - yt[j];
          acc = acc + e * e;
        }
      }
      d[t] = acc;
    }
  }
  __syncthreads();
  if (live && ln == 0) {                                         // the serial prefix, in lag order
    double c = 0.0;
    for (int t = 1; t < T1; ++t) {
      c = c + d[t];
      dp[t] = c;
    }
  }
  __syncthreads();
  if (live)
    for (int t = ln; t < T1; t += P) dp[t] = t ? f0_norm(d[t], t, dp[t]) : 1.0;
  __syncthreads();
  if (!live) return;
  const long rec = f_off + (k - tb[3]);
  if (ln == 0) {
    float f, a;
    lag[rec] = f0_choose(g, dp, &f, &a);
    f0[rec] = f;
    ap[rec] = a;
  }
  if (dtab)
    for (int t = ln; t < T1; t += P) {
      dtab[rec * T1 + t] = d[t];
      dptab[rec * T1 + t] = dp[t];
    }
}

// every check of vx_f0 behind the pointers: options, lengths, the frame stride
static int f0_check(vx_ctx* c, const char* who, const int32_t* lens, int batch, const vx_f0_opts* o, int64_t frame_stride, F0Geom* g) {
  CHECK_STRUCT(*o, vx_f0_opts);
  char why[160];
  if (f0_check_opts(*o, why, sizeof why)) FAIL(VX_EINVAL, "%s: %s", who, why);
  *g = f0_geometry(*o);
  for (int i = 0; i < batch; ++i) {
    const long L = lens[i];
    if (f0_frames(*g, L) > frame_stride)
      FAIL(VX_EINVAL, "%s: frame_stride %ld below the %ld frames of row %d", who, (long)frame_stride, f0_frames(*g, L), i);
  }
  return VX_OK;
}

// plan, then one launch per group of jobs, everything of a launch behind one stream sync.  dtab / dptab: one row only.
static int f0_run(vx_ctx* c, const char* who, const float* wav, int64_t wav_stride, const int32_t* lens, int batch, const F0Geom& g, float* f0,
                  int32_t* lag, float* ap, int64_t frame_stride, double* dtab, double* dptab) {
  const long win = wave_window(c->f0_window, VX_F0_WINDOW);
  const int R = g.W + g.T, T1 = g.T + 1;
  const long fcap = dtab ? std::min(F0_FRAME_CAP, F0_TABLE_CAP / T1) : F0_FRAME_CAP;
  std::vector<F0Job> jobs;
  if (!f0_plan(g, lens, batch, win, fcap, F0_MAX_JOBS, &jobs))
    FAIL(VX_EINVAL, "%s: the window of %ld samples (vx_dev_f0_window) is below one frame's reach at window %d, lag_max %d", who, win, g.W, g.T);
  if (jobs.empty()) return VX_OK;
  HIPCHK(hipSetDevice(c->dev));
  if (int e = rs_buffers(c)) return e;
  int lp = 6;
  while ((1 << lp) < T1 && lp < 8) ++lp;
  const size_t per = (size_t)(R + 2 * T1) * sizeof(double);
  const int G = (int)std::max<size_t>(1, std::min<size_t>(256 >> lp, F0_LDS_MAX / per));
  float* of0 = c->rs_out;
  int* olag = reinterpret_cast<int*>(c->rs_out + F0_FRAME_CAP);
  float* oap = c->rs_out + 2 * F0_FRAME_CAP;
  double* od = reinterpret_cast<double*>(c->rs_out + F0_TABLE_AT);
  double* odp = od + F0_TABLE_CAP;
  std::vector<int> tab;
  return wave_launches(c, jobs, [&](size_t j0, size_t j1) -> int {
    tab.clear();
    long blocks = 0;
    for (size_t k = j0; k < j1; ++k) {
      const F0Job& j = jobs[k];
      for (long v : {j.in_off, j.s_lo, j.s_hi - j.s_lo, j.k0, j.k1, j.f_off, blocks, 0L}) tab.push_back((int)v);
      blocks += (j.k1 - j.k0 + G - 1) / G;
      if (j.s_hi > j.s_lo)
        H2D(c->rs_in + j.in_off, wav + (long)j.row * wav_stride + j.s_lo, (size_t)(j.s_hi - j.s_lo) * sizeof(float));
    }
    H2D(c->rs_meta, tab.data(), tab.size() * sizeof(int));
    hipLaunchKernelGGL(f0_frames_kernel, dim3((unsigned)blocks), dim3(256), (size_t)G * per, c->stream, c->rs_in, c->rs_meta, (int)(j1 - j0), of0,
                       olag, oap, dtab ? od : nullptr, dtab ? odp : nullptr, g, lp, G);
    for (size_t k = j0; k < j1; ++k) {
      const F0Job& j = jobs[k];
      const size_t nf = (size_t)(j.k1 - j.k0);
      const long at = (long)j.row * frame_stride + j.k0;
      D2H(f0 + at, of0 + j.f_off, nf * sizeof(float));
      D2H(lag + at, olag + j.f_off, nf * sizeof(int));
      if (ap) D2H(ap + at, oap + j.f_off, nf * sizeof(float));
      if (dtab) {
        D2H(dtab + j.k0 * T1, od + j.f_off * T1, nf * T1 * sizeof(double));
        D2H(dptab + j.k0 * T1, odp + j.f_off * T1, nf * T1 * sizeof(double));
      }
    }
    return VX_OK;
  });
}

}  // namespace vxe

extern "C" {

int vx_f0(vx_ctx* c, const float* wav, int64_t wav_stride, const int32_t* lens, int32_t batch, const vx_f0_opts* o, float* f0, int32_t* lag,
          float* ap, int64_t frame_stride, vx_f0_info* info) {
  using namespace vxe;
  if (!c) return VX_EINVAL;
  if (int e = wave_check_rows(c, "vx_f0", wav, wav_stride, lens, batch)) return e;
  if (!o) FAIL(VX_EINVAL, "vx_f0: o is NULL");
  if (!f0) FAIL(VX_EINVAL, "vx_f0: f0 is NULL");
  if (!lag) FAIL(VX_EINVAL, "vx_f0: lag is NULL");
  if (!info) FAIL(VX_EINVAL, "vx_f0: info is NULL");
  F0Geom g;
  if (int e = f0_check(c, "vx_f0", lens, batch, o, frame_stride, &g)) return e;
  if (int e = f0_run(c, "vx_f0", wav, wav_stride, lens, batch, g, f0, lag, ap, frame_stride, nullptr, nullptr)) return e;
  for (int i = 0; i < batch; ++i) {
    const float* x = wav + (long)i * wav_stride;
    f0_summary(f0 + (long)i * frame_stride, lag + (long)i * frame_stride, f0_frames(g, lens[i]), f0_nonfinite(x, lens[i]), &info[i]);
  }
  return VX_OK;
}

int vx_dev_f0_table(vx_ctx* c, const float* wav, int32_t len, const vx_f0_opts* o, double* d, double* dp) {
  using namespace vxe;
  if (!c) return VX_EINVAL;
  if (!wav) FAIL(VX_EINVAL, "vx_dev_f0_table: wav is NULL");
  if (!o) FAIL(VX_EINVAL, "vx_dev_f0_table: o is NULL");
  if (!d || !dp) FAIL(VX_EINVAL, "vx_dev_f0_table: d or dp is NULL");
  if (len < 0) FAIL(VX_EINVAL, "vx_dev_f0_table: len %d below 0", len);
  F0Geom g;
  const int64_t big = 0x7fffffffL;
  if (int e = f0_check(c, "vx_dev_f0_table", &len, 1, o, big, &g)) return e;
  const size_t M = (size_t)f0_frames(g, len);
  std::vector<float> f(M + 1), a(M + 1);
  std::vector<int32_t> l(M + 1);
  return f0_run(c, "vx_dev_f0_table", wav, len, &len, 1, g, f.data(), l.data(), a.data(), big, d, dp);
}

int vx_dev_f0_window(vx_ctx* c, int32_t samples) {
  return vxe::wave_set_window(c, &vx_ctx::f0_window, "vx_dev_f0_window", "samples", samples, VX_DEV_F0_WINDOW_MIN, VX_F0_WINDOW);
}

}  // extern "C"
