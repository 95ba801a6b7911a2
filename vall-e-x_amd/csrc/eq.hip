// The equaliser (vx_eq, vx_eq_design, vx_eq_plan, include/vallex_hip.h): a cascade of up to eight biquads over mono fp32 rows on the
// device; designs, the warm-up W of a filter, the planner and the sequential reference on the host (eq_host.h).
//
//   rows     eq_rows_kernel: step j of a job = samples [j S, min((j + 1) S, n)).  ONE lane starts the cascade (transposed direct form
//            II, double, every operation separately rounded: contraction is off; eq_host.h: eq_section) from rest at sample j S - W,
//            runs it to the end of the step and keeps the outputs of the step's own samples, each rounded once to fp32.  Samples
//            before the row are 0, a non-finite sample is 0, a result that is not finite in fp32 is written as 0.
//
// Arithmetic (the contract the tests rest on): an output is a function of the at most W + S samples its lane reads and of the
// coefficients.  Its bits therefore do not depend on the row, the batch, the job, the tile, the window or the launch it lands in.  No
// atomics, no inline assembly.
//
// Work decomposition: the one of loudness_steps_kernel.  A launch covers a ragged list of JOBS (a run of consecutive steps of one row
// with the warm-up in front of the first one), grid (tile, job), a tile = EQ_LANES consecutive steps, one per lane of one wavefront.
// The lanes' streams lie S samples apart, so the tile walks them in chunks of EQ_C samples: chunk q of all lanes is loaded with
// coalesced row loads (the 32 lanes of half a wavefront read 32 consecutive samples of one stream), staged in LDS at a lane stride of
// EQ_C + 1 floats -- odd, so the lanes, which read the same offset of consecutive streams, fall on different banks -- and then each lane
// runs its recursion over its row of the tile.  The loads of chunk q + 1 are in flight while the recursion runs over chunk q.  W is a
// multiple of EQ_C, so a chunk is either all warm-up or all output: the outputs of an output chunk leave the same way in reverse, each
// lane into its row of a third LDS tile, then out as coalesced runs of 32 samples.  LDS use does not depend on S or W.
// The section count is a template argument (1 .. 8, no padding section: the bits cannot depend on how a count is rounded up), so the
// 2 x sections state doubles are registers; the coefficients are kernel arguments, wave-uniform.  The recursion is a dependent chain
// of fp64 operations, four deep per section: the kernel is latency-bound by construction.  What runs side by side within a lane is
// section k of sample n + 1 with section k + 1 of sample n.
// Per-row reductions (non-finite inputs, non-finite results, the largest |out|): per lane over its own samples, then over the
// wavefront by shuffles, one record per tile that the host folds.  Sums of counts and a maximum are order-free.
#include "wave_stage.h"
#include "eq_host.h"

#include "../../include/vallex_hip_dev.h"

#include <string>

namespace {
// the message of a refused vx_eq_design / vx_eq_plan (no context to hang it on): per thread
thread_local std::string g_eq_err;
// the cascade of this thread's last vx_eq and its warm-up W: the impulse response is not walked again for the same filter.  Not in the
// context: vx_ctx grows by the window field alone
thread_local struct { double sec[5 * VX_EQ_MAX_SECTIONS]; int n = 0, warm = 0; } g_eq_last;
}  // namespace

namespace vxe {

constexpr int EQ_LANES = EQ_TILE;          // steps of a tile: one wavefront
constexpr int EQ_C = 32;                   // samples of a chunk
constexpr int EQ_STRIDE = EQ_C + 1;        // floats between the lanes of a staged chunk
constexpr int EQ_REC = 4;                  // ints of a tile record: {non-finite inputs, non-finite results, bits of the peak, 0}
// the records of a launch lie in the upper half of rs_out, which the outputs of this stage (at most RS_IN_CAP) never reach
constexpr long EQ_REC_CAP = RS_IN_CAP / EQ_S / EQ_TILE + RS_MAX_JOBS;      // a record per full tile plus a cut one per job
static_assert(VX_EQ_WINDOW == RS_IN_CAP, "vx_eq runs in the resampler's launch buffers");
static_assert(EQ_REC_CAP * EQ_REC <= RS_OUT_CAP - RS_IN_CAP, "the record table fits behind the outputs");
static_assert(VX_DEV_EQ_WINDOW_MIN >= 2 * EQ_S && VX_DEV_EQ_WINDOW_MIN <= VX_EQ_WINDOW, "window bounds of the dev header");
static_assert(EQ_LANES == 64 && EQ_LANES * EQ_C % 64 == 0 && EQ_STRIDE % 2 == 1 && EQ_S % EQ_C == 0, "tile shape");

struct EqCoef { double c[5 * EQ_MAX]; };

// tab [njobs][RS_TAB]: {in_off, pre, cnt, out_off, rec_off}: the job's steps cover in[in_off + pre .. in_off + pre + cnt), the `pre`
// samples in front are its warm-up (what a lane would read in front of in_off lies before the row: 0).  Sample r of the job's steps
// -> out[out_off + r]; tile t -> rec[(rec_off + t) EQ_REC ..].  Every read is inside in[in_off .. in_off + pre + cnt), every write
// inside out[out_off .. out_off + cnt).
template <int NS>
__global__ __launch_bounds__(EQ_LANES) void eq_rows_kernel(const float* __restrict__ in, const int* __restrict__ tab, float* __restrict__ out,
                                                           int* __restrict__ rec, EqCoef k, int S, int W) {
  __shared__ float xs[2][EQ_LANES * EQ_STRIDE];
  __shared__ float ys[EQ_LANES * EQ_STRIDE];
  const int* tb = tab + blockIdx.y * RS_TAB;
  const long in_off = tb[0], out_off = tb[3];
  const int pre = tb[1], cnt = tb[2], nst = (cnt + S - 1) / S, t0 = blockIdx.x * EQ_LANES;
  if (t0 >= nst) return;                                           // block-uniform
  const int have = pre + cnt, tid = threadIdx.x;
  const int own_first = cnt - t0 * S < S ? cnt - t0 * S : S;        // own samples of the tile's first step: the longest stream
  const int qmax = W + own_first, nchunk = (qmax + EQ_C - 1) / EQ_C;
  const int my = t0 + tid;                                         // this lane's step
  const int own = my < nst ? (cnt - my * S < S ? cnt - my * S : S) : 0;
  // loader: thread tid fills column (tid & 31) of the lanes 2 i + (tid >> 5); stream position q of lane r is job sample
  // pre + (t0 + r) S - W + q
  const int lcol = tid & (EQ_C - 1), lrow = tid >> 5;
  const long lbase = (long)pre + (long)(t0 + lrow) * S - W + lcol;
  float reg[EQ_LANES / 2];
  auto fetch = [&](int q0) {
#pragma unroll
    for (int i = 0; i < EQ_LANES / 2; ++i) {
      const long p = lbase + (long)(2 * i) * S + q0;
      reg[i] = p >= 0 && p < have ? in[in_off + p] : 0.f;
    }
  };
  auto stage = [&](int b) {
#pragma unroll
    for (int i = 0; i < EQ_LANES / 2; ++i) xs[b][(2 * i + lrow) * EQ_STRIDE + lcol] = reg[i];
  };
  fetch(0);
  stage(0);
  __syncthreads();
  double s1[NS], s2[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) s1[s] = s2[s] = 0.0;
  int bad_in = 0, bad_out = 0;
  float peak = 0.f;
  for (int ch = 0; ch < nchunk; ++ch) {
    const int q0 = ch * EQ_C;
    const bool writes = q0 >= W;                                   // chunk-uniform: W is a multiple of EQ_C
    if (ch + 1 < nchunk) fetch(q0 + EQ_C);                         // in flight behind the recursion
    const float* xp = xs[ch & 1] + tid * EQ_STRIDE;
    float* yp = ys + tid * EQ_STRIDE;
#pragma unroll 4
    for (int j = 0; j < EQ_C; ++j) {
      const float xf = xp[j];
      const bool fin = (__float_as_uint(xf) & 0x7f800000u) != 0x7f800000u;
      double u = fin ? (double)xf : 0.0;
#pragma unroll
      for (int s = 0; s < NS; ++s) u = eq_section(k.c + 5 * s, u, s1[s], s2[s]);
      if (writes) {
        float y = (float)u;
        const bool ok = (__float_as_uint(y) & 0x7f800000u) != 0x7f800000u;
        y = ok ? y : 0.f;
        if (q0 + j - W < own) {
          bad_in += fin ? 0 : 1;
          bad_out += ok ? 0 : 1;
          peak = fmaxf(peak, fabsf(y));
        }
        yp[j] = y;
      }
    }
    if (ch + 1 < nchunk) stage((ch + 1) & 1);
    __syncthreads();
    if (writes) {                                                  // thread tid stores column lcol of the lanes 2 i + lrow
      const int r = q0 - W + lcol;                                 // sample of the step
#pragma unroll
      for (int i = 0; i < EQ_LANES / 2; ++i) {
        const long o = (long)(t0 + 2 * i + lrow) * S + r;          // sample of the job's steps
        if (o < cnt) out[out_off + o] = ys[(2 * i + lrow) * EQ_STRIDE + lcol];
      }
      __syncthreads();                                             // ys is written again by the next chunk
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    bad_in += __shfl_xor(bad_in, m);
    bad_out += __shfl_xor(bad_out, m);
    peak = fmaxf(peak, __shfl_xor(peak, m));
  }
  if (tid == 0) {
    int* r = rec + ((long)tb[4] + blockIdx.x) * EQ_REC;
    r[0] = bad_in; r[1] = bad_out; r[2] = (int)__float_as_uint(peak); r[3] = 0;
  }
}

using EqKernel = void (*)(const float*, const int*, float*, int*, EqCoef, int, int);
static const EqKernel eq_kernels[EQ_MAX] = {eq_rows_kernel<1>, eq_rows_kernel<2>, eq_rows_kernel<3>, eq_rows_kernel<4>,
                                            eq_rows_kernel<5>, eq_rows_kernel<6>, eq_rows_kernel<7>, eq_rows_kernel<8>};

}  // namespace vxe

extern "C" {

const char* vx_eq_last_error(void) { return g_eq_err.c_str(); }

int vx_eq_design(int32_t kind, int32_t sample_rate, double f0, double q, double gain_db, double c[5]) {
  char why[240];
  if (!c) { g_eq_err = "vx_eq_design: c is NULL"; return VX_EINVAL; }
  if (vxe::eq_design(kind, sample_rate, f0, q, gain_db, c, why, sizeof why)) { g_eq_err = std::string("vx_eq_design: ") + why; return VX_EINVAL; }
  return VX_OK;
}

int vx_eq_plan(const double* sections, int32_t nsections, int32_t* warm, int32_t* step) {
  char why[240];
  if (!sections || !warm || !step) { g_eq_err = "vx_eq_plan: sections, warm or step is NULL"; return VX_EINVAL; }
  int W = 0;
  if (vxe::eq_warm(sections, nsections, &W, why, sizeof why)) { g_eq_err = std::string("vx_eq_plan: ") + why; return VX_EINVAL; }
  *warm = W;
  *step = vxe::EQ_S;
  return VX_OK;
}

int vx_eq(vx_ctx* c, const float* wav, int64_t wav_stride, const int32_t* lens, int32_t batch, const double* sections, int32_t nsections,
          float* out, int64_t out_stride, vx_eq_info* info) {
  using namespace vxe;
  if (!c) return VX_EINVAL;
  if (int e = wave_check_rows(c, "vx_eq", wav, wav_stride, lens, batch)) return e;
  if (!sections) FAIL(VX_EINVAL, "vx_eq: sections is NULL");
  if (!out) FAIL(VX_EINVAL, "vx_eq: out is NULL");
  if (!info) FAIL(VX_EINVAL, "vx_eq: info is NULL");
  if (int e = wave_check_out_stride(c, "vx_eq", lens, batch, out_stride, "")) return e;
  char why[240];
  if (eq_check_sections(sections, nsections, why, sizeof why)) FAIL(VX_EINVAL, "vx_eq: %s", why);
  if (g_eq_last.n != nsections || memcmp(g_eq_last.sec, sections, (size_t)nsections * 5 * sizeof(double))) {
    int W = 0;
    if (eq_warm(sections, nsections, &W, why, sizeof why)) FAIL(VX_EINVAL, "vx_eq: %s", why);
    memcpy(g_eq_last.sec, sections, (size_t)nsections * 5 * sizeof(double));
    g_eq_last.n = nsections;
    g_eq_last.warm = W;
  }
  const int W = g_eq_last.warm, S = EQ_S;
  const long win = wave_window(c->eq_window, VX_EQ_WINDOW);
  std::vector<EqJob> jobs;
  if (!eq_plan(lens, batch, S, W, win, RS_IN_CAP, RS_MAX_JOBS, &jobs))
    FAIL(VX_EINVAL, "vx_eq: the launch window of %ld samples (vx_dev_eq_window) is below W + S = %d + %d of this filter", win, W, S);
  HIPCHK(hipSetDevice(c->dev));
  if (int e = rs_buffers(c)) return e;
  for (int i = 0; i < batch; ++i) info[i] = {W, 0, 0, 0.f};
  EqCoef k;
  memset(&k, 0, sizeof k);
  memcpy(k.c, sections, (size_t)nsections * 5 * sizeof(double));
  int* rec = reinterpret_cast<int*>(c->rs_out + RS_IN_CAP);
  std::vector<int> tab, recs;
  return wave_launches(c, jobs, [&](size_t j0, size_t j1) -> int {
    tab.clear();
    long max_st = 0, nrec = 0;
    for (size_t q = j0; q < j1; ++q) {
      const EqJob& j = jobs[q];
      for (long v : {j.off, j.pre, j.cnt, j.out_off, j.rec_off, 0L, 0L, 0L}) tab.push_back((int)v);
      max_st = std::max(max_st, eq_nsteps(j.cnt, S));
      nrec = j.rec_off + eq_ntiles(j.cnt, S);
      H2D(c->rs_in + j.off, wav + (long)j.row * wav_stride + j.j0 * S - j.pre, (size_t)(j.pre + j.cnt) * sizeof(float));
    }
    if (nrec > EQ_REC_CAP) FAIL(VX_EINVAL, "vx_eq: %ld tiles in one launch exceed the record table of %ld", nrec, EQ_REC_CAP);      // the window rules it out
    H2D(c->rs_meta, tab.data(), tab.size() * sizeof(int));
    const dim3 grid((unsigned)((max_st + EQ_LANES - 1) / EQ_LANES), (unsigned)(j1 - j0));
    hipLaunchKernelGGL(eq_kernels[nsections - 1], grid, dim3(EQ_LANES), 0, c->stream, c->rs_in, c->rs_meta, c->rs_out, rec, k, S, W);
    for (size_t q = j0; q < j1; ++q) {
      const EqJob& j = jobs[q];
      D2H(out + (long)j.row * out_stride + j.j0 * S, c->rs_out + j.out_off, (size_t)j.cnt * sizeof(float));
    }
    recs.resize((size_t)nrec * EQ_REC);
    D2H(recs.data(), rec, recs.size() * sizeof(int));
    return VX_OK;
  }, [&](size_t j0, size_t j1) -> int {
    for (size_t q = j0; q < j1; ++q) {
      const EqJob& j = jobs[q];
      vx_eq_info& w = info[j.row];
      for (long t = 0; t < eq_ntiles(j.cnt, S); ++t) {
        const int* r = recs.data() + (size_t)(j.rec_off + t) * EQ_REC;
        float p;
        memcpy(&p, r + 2, sizeof p);
        w.nonfinite += r[0];
        w.nonfinite_out += r[1];
        w.peak = std::max(w.peak, p);
      }
    }
    return VX_OK;
  });
}

int vx_dev_eq_window(vx_ctx* c, int32_t samples) {
  return vxe::wave_set_window(c, &vx_ctx::eq_window, "vx_dev_eq_window", "samples", samples, VX_DEV_EQ_WINDOW_MIN, VX_EQ_WINDOW);
}

}  // extern "C"
