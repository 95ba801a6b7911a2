// Programme loudness after ITU-R BS.1770 (vx_loudness, vx_finish_loud, include/vallex_hip.h): the K-weighted energy of every 100 ms
// step of mono fp32 rows on the device; blocks, gates, loudness and gain on the host (loudness_host.h: ln_reduce).
//
//   steps    loudness_steps_kernel: step j of a span = samples [j S, min((j + 1) S, n)).  ONE lane starts the two biquads (shelf, then
//            high-pass, transposed direct form II, double, every operation separately rounded: contraction is off) from rest at sample
//            j S - W, W = 2 S, runs them to the end of the step and sums z = z + v v over the step's own samples in sample order.
//            Samples before the span are 0, a non-finite sample is 0.  The lane writes z_j and the non-finite samples of its step.
//
// Arithmetic (the contract the tests rest on): a step is a function of the W + S samples it reads and of the ten coefficients.  Its
// bits therefore do not depend on the row, the batch, the job, the tile, the window or the launch it lands in.  No atomics, no inline
// assembly.
//
// Work decomposition: a launch covers a ragged list of JOBS (a run of consecutive steps of one row with the warm-up in front of the
// first one), grid (tile, job), a tile = LN_LANES consecutive steps, one per lane of one wavefront.  The lanes read streams S samples
// apart, so the tile walks them in chunks of LN_C samples: chunk q of all lanes is loaded with coalesced row loads (the 32 lanes of
// half a wavefront read 32 consecutive samples of one stream), staged in LDS at a lane stride of LN_C + 1 floats -- odd, so the lanes,
// which read the same offset of consecutive streams, fall on different banks -- and then each lane runs its recursion over its row of
// the tile.  LDS use does not depend on S.  The loads of chunk q + 1 are in flight while the recursion runs over chunk q (two tiles).
// The recursion is a dependent chain of fp64 operations: the kernel is latency-bound by construction.
#include "wave_stage.h"
#include "loudness_host.h"

#include "../../include/vallex_hip_dev.h"

namespace vxe {

constexpr int LN_LANES = 64;               // steps of a tile: one wavefront
constexpr int LN_C = 32;                   // samples of a chunk
constexpr int LN_STRIDE = LN_C + 1;        // floats between the lanes of a staged chunk
constexpr long LN_Z_CAP = RS_IN_CAP / LN_STEP_MIN + RS_MAX_JOBS;      // step records of a launch: one per S samples plus a cut one per job
static_assert(VX_LOUDNESS_WINDOW == RS_IN_CAP, "vx_loudness runs in the resampler's launch buffers");
static_assert(VX_DEV_LOUDNESS_WINDOW_MIN >= 3 * LN_STEP_MIN && VX_DEV_LOUDNESS_WINDOW_MIN <= VX_LOUDNESS_WINDOW, "window bounds of the dev header");
static_assert(LN_LANES * LN_C % 64 == 0 && LN_STRIDE % 2 == 1, "tile shape");

struct LnCoef { double c[10]; };

// tab [njobs][RS_TAB]: {in_off, pre, cnt, z_off}: the job's steps cover in[in_off + pre .. in_off + pre + cnt), the `pre` samples in
// front are its warm-up (what a lane would read in front of in_off lies before the span: 0).  Step t of the job -> z[z_off + t],
// nonf[z_off + t].  Every read is inside in[in_off .. in_off + pre + cnt).
__global__ __launch_bounds__(LN_LANES) void loudness_steps_kernel(const float* __restrict__ in, const int* __restrict__ tab,
                                                                  double* __restrict__ z, int* __restrict__ nonf, LnCoef k, int S) {
  __shared__ float xs[2][LN_LANES * LN_STRIDE];
  const int* tb = tab + blockIdx.y * RS_TAB;
  const long in_off = tb[0], z_off = tb[3];
  const int pre = tb[1], cnt = tb[2], nst = (cnt + S - 1) / S, t0 = blockIdx.x * LN_LANES;
  if (t0 >= nst) return;                                           // block-uniform
  const int W = 2 * S, have = pre + cnt, tid = threadIdx.x;
  const int own_first = cnt - t0 * S < S ? cnt - t0 * S : S;        // own samples of the tile's first step: the longest stream
  const int qmax = W + own_first, nchunk = (qmax + LN_C - 1) / LN_C;
  const int my = t0 + tid;                                         // this lane's step
  const int own = my < nst ? (cnt - my * S < S ? cnt - my * S : S) : 0;
  // loader: thread tid fills column (tid & 31) of the lanes 2 i + (tid >> 5); stream position q of lane r is job sample
  // pre + (t0 + r) S - W + q
  const int lcol = tid & (LN_C - 1), lrow = tid >> 5;
  const long lbase = (long)pre + (long)(t0 + lrow) * S - W + lcol;
  float reg[LN_LANES / 2];
  auto fetch = [&](int q0) {
#pragma unroll
    for (int i = 0; i < LN_LANES / 2; ++i) {
      const long p = lbase + (long)(2 * i) * S + q0;
      reg[i] = p >= 0 && p < have ? in[in_off + p] : 0.f;
    }
  };
  auto stage = [&](int b) {
#pragma unroll
    for (int i = 0; i < LN_LANES / 2; ++i) xs[b][(2 * i + lrow) * LN_STRIDE + lcol] = reg[i];
  };
  fetch(0);
  stage(0);
  __syncthreads();
  double s1 = 0.0, s2 = 0.0, t1 = 0.0, t2 = 0.0, acc = 0.0;
  int bad = 0;
  for (int ch = 0; ch < nchunk; ++ch) {
    const int q0 = ch * LN_C;
    if (ch + 1 < nchunk) fetch(q0 + LN_C);                         // in flight behind the recursion
    const float* xp = xs[ch & 1] + tid * LN_STRIDE;
    {
#pragma clang fp contract(off)
#pragma unroll 4
      for (int j = 0; j < LN_C; ++j) {
        const float xf = xp[j];
        const bool fin = (__float_as_uint(xf) & 0x7f800000u) != 0x7f800000u;
        const double x = fin ? (double)xf : 0.0;
        const double u = k.c[0] * x + s1;
        s1 = (k.c[1] * x - k.c[3] * u) + s2;
        s2 = k.c[2] * x - k.c[4] * u;
        const double v = k.c[5] * u + t1;
        t1 = (k.c[6] * u - k.c[8] * v) + t2;
        t2 = k.c[7] * u - k.c[9] * v;
        const int q = q0 + j;
        if (q >= W && q < W + own) {
          acc = acc + v * v;
          bad += fin ? 0 : 1;
        }
      }
    }
    if (ch + 1 < nchunk) stage((ch + 1) & 1);
    __syncthreads();
  }
  if (my < nst) {
    z[z_off + my] = acc;
    nonf[z_off + my] = bad;
  }
}

// (ln_buffers and ln_steps: wave_stage.h)
int ln_buffers(vx_ctx* c) {
  if (int e = rs_buffers(c)) return e;
  if (!c->ln_z) {
    if (int e = dev_alloc(c, &c->ln_z, (size_t)LN_Z_CAP, false)) return e;
    if (int e = dev_alloc(c, &c->ln_nonf, (size_t)LN_Z_CAP, false)) return e;
  }
  return VX_OK;
}

// the steps pass over the spans [lo[i], hi[i]) of the rows: the step table of row i at z[z0[i] ..), its non-finite samples in nonf[i].
// resident: the rows already lie in rs_in, row i's sample 0 at rs_in + base[i]; nothing is uploaded and one launch takes all of them.
int ln_steps(vx_ctx* c, const char* who, const float* wav, int64_t wav_stride, const long* lo, const long* hi, int batch, int rate,
             bool resident, const std::vector<long>& base, std::vector<double>& z, std::vector<long>& z0, std::vector<int>& nonf) {
  const int S = ln_step(rate);
  LnCoef k;
  ln_coeffs(rate, k.c);
  z0.assign(batch + 1, 0);
  for (int i = 0; i < batch; ++i) z0[i + 1] = z0[i] + ln_nsteps(hi[i] - lo[i], S);
  z.assign((size_t)z0[batch], 0.0);
  nonf.assign(batch, 0);
  std::vector<LnJob> jobs;
  // resident rows are not moved: a window that holds every span whole, so that a job is a row (batch <= RS_MAX_JOBS then: the frames
  // pass had a job per row)
  const long win = resident ? std::max<long>(RS_IN_CAP, 3L * S) : wave_window(c->ln_window, VX_LOUDNESS_WINDOW);
  if (!ln_plan(lo, hi, batch, S, win, RS_MAX_JOBS, &jobs))
    FAIL(VX_EINVAL, "%s: the launch window of %ld samples (vx_dev_loudness_window) is below 3 S = %d at sample_rate %d", who, win, 3 * S, rate);
  std::vector<int> tab, cnts;
  return wave_launches(c, jobs, [&](size_t j0, size_t j1) -> int {
    tab.clear();
    long max_st = 0, nz = 0;
    for (size_t q = j0; q < j1; ++q) {
      const LnJob& j = jobs[q];
      const long first = lo[j.row] + j.j0 * S - j.pre;              // row sample the job's buffer starts with
      const long in_off = resident ? base[j.row] + first : j.off;
      for (long v : {in_off, j.pre, j.cnt, j.z_off, 0L, 0L, 0L, 0L}) tab.push_back((int)v);
      max_st = std::max(max_st, ln_nsteps(j.cnt, S));
      nz = j.z_off + ln_nsteps(j.cnt, S);
      if (!resident) H2D(c->rs_in + j.off, wav + (long)j.row * wav_stride + first, (size_t)(j.pre + j.cnt) * sizeof(float));
    }
    if (nz > LN_Z_CAP) FAIL(VX_EINVAL, "%s: %ld steps in one launch exceed the step table of %ld", who, nz, LN_Z_CAP);      // the window rules it out
    H2D(c->rs_meta, tab.data(), tab.size() * sizeof(int));
    const dim3 grid((unsigned)((max_st + LN_LANES - 1) / LN_LANES), (unsigned)(j1 - j0));
    hipLaunchKernelGGL(loudness_steps_kernel, grid, dim3(LN_LANES), 0, c->stream, c->rs_in, c->rs_meta, c->ln_z, c->ln_nonf, k, S);
    cnts.resize((size_t)nz);
    for (size_t q = j0; q < j1; ++q) {
      const LnJob& j = jobs[q];
      D2H(z.data() + z0[j.row] + j.j0, c->ln_z + j.z_off, (size_t)ln_nsteps(j.cnt, S) * sizeof(double));
    }
    D2H(cnts.data(), c->ln_nonf, (size_t)nz * sizeof(int));
    return VX_OK;
  }, [&](size_t j0, size_t j1) -> int {
    for (size_t q = j0; q < j1; ++q) {
      const LnJob& j = jobs[q];
      for (long t = 0; t < ln_nsteps(j.cnt, S); ++t) nonf[j.row] += cnts[(size_t)(j.z_off + t)];
    }
    return VX_OK;
  });
}

}  // namespace vxe

extern "C" {

int vx_loudness_coeffs(int32_t sample_rate, double c[10]) {
  using namespace vxe;
  if (!c || sample_rate < LN_RATE_MIN || sample_rate > LN_RATE_MAX) return VX_EINVAL;
  ln_coeffs(sample_rate, c);
  return VX_OK;
}

int vx_loudness(vx_ctx* c, const float* wav, int64_t wav_stride, const int32_t* lens, int32_t batch, int32_t sample_rate,
                vx_loudness_info* info) {
  using namespace vxe;
  if (!c) return VX_EINVAL;
  if (int e = wave_check_rows(c, "vx_loudness", wav, wav_stride, lens, batch)) return e;
  if (!info) FAIL(VX_EINVAL, "vx_loudness: info is NULL");
  char why[160];
  if (ln_check_rate(sample_rate, why, sizeof why)) FAIL(VX_EINVAL, "vx_loudness: %s", why);
  HIPCHK(hipSetDevice(c->dev));
  if (int e = ln_buffers(c)) return e;
  std::vector<long> lo((size_t)batch, 0), hi((size_t)batch), z0, base;
  for (int i = 0; i < batch; ++i) hi[(size_t)i] = lens[i];
  std::vector<double> z;
  std::vector<int> nonf;
  if (int e = ln_steps(c, "vx_loudness", wav, wav_stride, lo.data(), hi.data(), batch, sample_rate, false, base, z, z0, nonf)) return e;
  for (int i = 0; i < batch; ++i) ln_reduce(z.data() + z0[(size_t)i], lens[i], ln_step(sample_rate), nonf[(size_t)i], &info[i]);
  return VX_OK;
}

int vx_finish_loud(vx_ctx* c, const float* wav, int64_t wav_stride, const int32_t* lens, int32_t batch, const vx_finish_opts* o,
                   const vx_loudness_opts* lo_, void* out, int64_t out_stride, int32_t* out_lens, vx_wave_info* info, vx_loudness_info* linfo) {
  using namespace vxe;
  if (!c) return VX_EINVAL;
  if (int e = wave_check_rows(c, "vx_finish_loud", wav, wav_stride, lens, batch)) return e;
  if (!o) FAIL(VX_EINVAL, "vx_finish_loud: o is NULL");
  if (!lo_) FAIL(VX_EINVAL, "vx_finish_loud: lo is NULL");
  if (!info) FAIL(VX_EINVAL, "vx_finish_loud: info is NULL");
  if (!linfo) FAIL(VX_EINVAL, "vx_finish_loud: linfo is NULL");
  if (out && !out_lens) FAIL(VX_EINVAL, "vx_finish_loud: out is given without out_lens");
  return fn_pipeline(c, "vx_finish_loud", wav, wav_stride, lens, batch, *o, lo_, nullptr, out, out_stride, out_lens, info, linfo, nullptr);
}

int vx_dev_loudness_steps(vx_ctx* c, const float* wav, int32_t n, int32_t sample_rate, double* z) {
  using namespace vxe;
  if (!c) return VX_EINVAL;
  if (!wav) FAIL(VX_EINVAL, "vx_dev_loudness_steps: wav is NULL");
  if (!z) FAIL(VX_EINVAL, "vx_dev_loudness_steps: z is NULL");
  if (n < 0) FAIL(VX_EINVAL, "vx_dev_loudness_steps: n %d below 0", n);
  char why[160];
  if (ln_check_rate(sample_rate, why, sizeof why)) FAIL(VX_EINVAL, "vx_dev_loudness_steps: %s", why);
  HIPCHK(hipSetDevice(c->dev));
  if (int e = ln_buffers(c)) return e;
  const long lo = 0, hi = n;
  std::vector<long> z0, base;
  std::vector<double> tz;
  std::vector<int> nonf;
  if (int e = ln_steps(c, "vx_dev_loudness_steps", wav, n, &lo, &hi, 1, sample_rate, false, base, tz, z0, nonf)) return e;
  for (size_t j = 0; j < tz.size(); ++j) z[j] = tz[j];
  return VX_OK;
}

int vx_dev_loudness_window(vx_ctx* c, int32_t samples) {
  return vxe::wave_set_window(c, &vx_ctx::ln_window, "vx_dev_loudness_window", "samples", samples, VX_DEV_LOUDNESS_WINDOW_MIN, VX_LOUDNESS_WINDOW);
}

}  // extern "C"
