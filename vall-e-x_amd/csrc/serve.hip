// Serving session (vx_serve_*, schedule.hip serve_admit): the per-admission kernel of a beam-group admission.  Everything else an admission runs
// is existing code: the prefill of the admitted requests (engine.hip prefill_layers, K / V into the arena slot of every request's
// first beam row), the K / V copy to the other beams' slots (beams.hip, pairs only), the decode state of every beam row
// (admit.hip admit_rows_kernel, one entry per beam row, all pointing at the request's prefill row), the final norm + predict layer
// into scratch buffers and the masked first sample (admit.hip admit_mask_kernel).
//
// serve_uniforms_kernel generalises admit_uniforms_kernel: there one seed serves the whole call and the draws are keyed on the caller
// row; here every admitted beam row has its own request seed and is keyed on its beam index j, so beam j of a request with seed s
// draws exactly what decode row j of a batch-1 vx_infer call with seed s draws (dec_sample_kernel's counter formula).  It also
// zeroes sum_logp of the admitted rows (the rows still decoding keep theirs) and writes their sampling record row_smp[4 d ..] =
// {top_k, temperature bits, force_eos_at, 0} and their filter record row_flt[4 d ..] = {top_p bits, repetition penalty bits,
// repetition window, min_frames}, which the session's sampler (serve_sample.hip) reads per decode row.
//
// serve_cancel_kernel stops the beam rows of cancelled requests between two vx_serve_run calls: their active flags and slot records
// go to 0 and n_active is recounted from the flags, as admit_mask_kernel's phase 1 recounts it.  A later admission into those rows
// rewrites everything a row carries (admit_rows_kernel, serve_uniforms_kernel, the prefill's K / V scatter).
#include "engine_ctx.h"

namespace vxe {
namespace {

__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {      // splitmix64, as dec_sample_kernel's
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// grid (ceil(max steps / 256), n), 256 threads.  tab[13 i .. 13 i + 12] = {decode row d, beam j, offset of the staged draws in
// `staged` (-1: counter-based), draws to write, seed low word, seed high word, top_k, temperature bits, force_eos_at, top_p bits,
// repetition penalty bits, repetition window, min_frames}.  Column d of u gets steps 0 .. draws-1.
__global__ __launch_bounds__(256) void serve_uniforms_kernel(const int* __restrict__ tab, const float* __restrict__ staged,
                                                             float* __restrict__ u, int ncols, float* __restrict__ sum_logp,
                                                             int* __restrict__ row_smp, int* __restrict__ row_flt) {
  const int* e = tab + SERVE_UTAB * blockIdx.y;
  const int d = e[0], j = e[1], off = e[2], steps = e[3];
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    sum_logp[d] = 0.f;
    *reinterpret_cast<int4*>(row_smp + 4 * d) = make_int4(e[6], e[7], e[8], 0);
    *reinterpret_cast<int4*>(row_flt + 4 * d) = make_int4(e[9], e[10], e[11], e[12]);
  }
  if (t >= steps) return;
  float x;
  if (off >= 0) x = staged[(long)off + t];
  else {
    const unsigned long long seed = (unsigned long long)(unsigned)e[4] | ((unsigned long long)(unsigned)e[5] << 32);
    x = (float)(mix64(mix64(mix64(seed) + (unsigned long long)j) + (unsigned long long)t) >> 40) * (1.0f / 16777216.0f);
  }
  u[(long)t * ncols + d] = x;
}

// one wave: lane d < nrows handles decode row d
__global__ __launch_bounds__(64) void serve_cancel_kernel(unsigned rows, int nrows, int* active, int* slot_meta,
                                                          const int* __restrict__ slot_of, int* n_active) {
  const int d = threadIdx.x;
  int v = 0;
  if (d < nrows) {
    v = ((rows >> d) & 1u) ? 0 : (active[d] != 0);
    active[d] = v;
    slot_meta[4 * slot_of[d] + 2] = v;
  }
  const int n = __popcll(__ballot(v));
  if (d == 0) *n_active = n;
}

}  // namespace

void launch_serve_uniforms(const int* tab, int n, int max_steps, const float* staged, float* u, int ncols, float* sum_logp,
                           int* row_smp, int* row_flt, hipStream_t s) {
  if (n <= 0) return;
  const int gx = std::max(1, (max_steps + 255) / 256);
  hipLaunchKernelGGL(serve_uniforms_kernel, dim3(gx, n), dim3(256), 0, s, tab, staged, u, ncols, sum_logp, row_smp, row_flt);
}

void launch_serve_cancel(unsigned rows, int nrows, int* active, int* slot_meta, const int* slot_of, int* n_active, hipStream_t s) {
  hipLaunchKernelGGL(serve_cancel_kernel, dim3(1), dim3(64), 0, s, rows, nrows, active, slot_meta, slot_of, n_active);
}

}  // namespace vxe
