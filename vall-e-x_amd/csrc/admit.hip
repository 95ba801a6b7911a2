// Continuous schedule (vx_infer_continuous, schedule.hip admit_common / admit_rows): the kernels that admit waiting caller rows into the decode rows that
// finished rows left free, between two decode steps of a running batch.  Everything else an admission runs is the existing code:
// the full-sequence prefill (engine.hip prefill_layers, K / V into the free rows' arena slots), the final norm + predict layer
// (dec_reduce_ln_pack + skinny GEMM, here into scratch buffers the step does not carry: dh2 / xp_att) and the unchanged sampler,
// whose fused start of the next step is the only writer of a row's next-step input (dh, xp).
//
// State a decode row carries between steps (engine_ctx.h): cur_tok, cur_pos, ctx_len, n_gen, active, text_len, its gen row, its
// slot record slot_meta[4 slot_of[d] ..] = (row, context, active), n_active, its KV slot, its d_uniforms column and dh[d] / xp row d.
// The rows still decoding must not see any of theirs change: every kernel here touches the admitted rows only, except the mask
// kernel, which saves and restores the active flags around the first sample of the admitted rows.
#include "engine_ctx.h"

namespace vxe {
namespace {

__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {      // splitmix64, as dec_sample_kernel's
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// one workgroup per admitted row: thread 0 writes the row's decode state, all 256 threads move its residual row (1024 floats)
__global__ __launch_bounds__(256) void admit_rows_kernel(const int* __restrict__ tab, const float* __restrict__ hsrc,
                                                         float* __restrict__ hres, int* cur_tok, int* cur_pos, int* ctx_len,
                                                         int* n_gen, int* text_len, int* slot_meta, const int* __restrict__ slot_of) {
  const int* t = tab + 5 * blockIdx.x;
  const int d = t[0], tid = threadIdx.x;
  const f32x4 v = reinterpret_cast<const f32x4*>(hsrc + (long)t[4] * D_MODEL)[tid];
  reinterpret_cast<f32x4*>(hres + (long)d * D_MODEL)[tid] = v;
  if (tid == 0) {
    cur_pos[d] = t[1];
    ctx_len[d] = t[2];
    n_gen[d] = 0;
    cur_tok[d] = 0;
    text_len[d] = t[3];
    slot_meta[4 * slot_of[d] + 1] = t[2];
  }
}

__global__ __launch_bounds__(64) void admit_mask_kernel(int phase, const int* __restrict__ admitted, int* saved, int nrows,
                                                        int* active, int* slot_meta, const int* __restrict__ slot_of, int* n_active) {
  const int d = threadIdx.x;
  int v = 0;
  if (d < nrows) {
    if (phase == 0) {
      const int a = admitted[d];
      saved[d] = a ? 0 : active[d];      // an admitted row was free: nothing of its predecessor survives (also on a re-run)
      active[d] = a;
    } else {
      v = (active[d] | saved[d]) != 0;
      active[d] = v;
      slot_meta[4 * slot_of[d] + 2] = v;
    }
  }
  if (phase == 1) {
    const int n = __popcll(__ballot(v));
    if (d == 0) *n_active = n;
  }
}

// grid (ceil(steps / 256), n): column pairs[2i] of u gets the draws of caller row pairs[2i + 1]
__global__ __launch_bounds__(256) void admit_uniforms_kernel(const int* __restrict__ pairs, const float* __restrict__ staged, int steps,
                                                             unsigned long long seed, float* __restrict__ u, int ncols) {
  const int i = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
  if (t >= steps) return;
  const int d = pairs[2 * i], r = pairs[2 * i + 1];
  float x;
  if (staged) x = staged[(long)i * steps + t];
  else x = (float)(mix64(mix64(mix64(seed) + (unsigned long long)r) + (unsigned long long)t) >> 40) * (1.0f / 16777216.0f);
  u[(long)t * ncols + d] = x;
}

}  // namespace

void launch_admit_rows(const int* tab, int n, const float* hsrc, float* hres, int* cur_tok, int* cur_pos, int* ctx_len, int* n_gen,
                       int* text_len, int* slot_meta, const int* slot_of, hipStream_t s) {
  static_assert(D_MODEL == 256 * 4, "admit_rows_kernel moves one residual row as 256 x 16 bytes");
  if (n <= 0) return;
  hipLaunchKernelGGL(admit_rows_kernel, dim3(n), dim3(256), 0, s, tab, hsrc, hres, cur_tok, cur_pos, ctx_len, n_gen, text_len,
                     slot_meta, slot_of);
}

void launch_admit_mask(int phase, const int* admitted, int* saved, int nrows, int* active, int* slot_meta, const int* slot_of,
                       int* n_active, hipStream_t s) {
  hipLaunchKernelGGL(admit_mask_kernel, dim3(1), dim3(64), 0, s, phase, admitted, saved, nrows, active, slot_meta, slot_of, n_active);
}

void launch_admit_uniforms(const int* pairs, int n, const float* staged, int steps, unsigned long long seed, float* u, int ncols,
                           hipStream_t s) {
  if (n <= 0 || steps <= 0) return;
  hipLaunchKernelGGL(admit_uniforms_kernel, dim3((steps + 255) / 256, n), dim3(256), 0, s, pairs, staged, steps, seed, u, ncols);
}

}  // namespace vxe
