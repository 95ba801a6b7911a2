// best_of fan-out (vx_infer with best_of = N > 1, schedule.hip; the beam groups of a serving session): every caller row of a micro-batch is prefilled ONCE and decoded as N beams
// (the reference repeats the prompt N times and prefills N times, models/vallex.py:525-527).  One launch per prefill copies
//   - the prefilled K / V of row i (its seq_len[i] cached rows of every layer and head) from the arena slot of decode row i*N to the
//     arena slots of decode rows i*N + 1 .. i*N + N-1 (the KV arena is indexed by launch slot, engine.hip ar_prefill), and
//   - the decode residual row of EVERY decode row d = i*N + j (j = 0 included) straight from the prefill's last-row buffer: reading
//     from there, not from dh itself, is what keeps row i from being overwritten by the beams of a row i' < i.
// The final norm and the predict layer then run on all R*N decode rows: no logits are copied.
#include "engine_ctx.h"

namespace vxe {

// grid: npairs x 2 x layers x N_HEAD copy workgroups (pair, layer, K | V, head; head fastest), then nrows residual-row workgroups.
// pairs[3p .. 3p+2] = {source slot, destination slot, cached rows}; hsrc_row[d] = row of hsrc that decode row d starts from.
__global__ __launch_bounds__(256) void beam_fanout_kernel(float* __restrict__ kc, float* __restrict__ vc, long cache_layer, int Tmax,
                                                          int layers, const int* __restrict__ pairs, int ncopy,
                                                          const float* __restrict__ hsrc, const int* __restrict__ hsrc_row,
                                                          float* __restrict__ dh) {
  const int blk = blockIdx.x, tid = threadIdx.x;
  if (blk >= ncopy) {                                   // the residual row of one decode row: 1024 floats = 256 x 16 bytes
    const int d = blk - ncopy;
    const f32x4 v = reinterpret_cast<const f32x4*>(hsrc + (long)hsrc_row[d] * D_MODEL)[tid];
    reinterpret_cast<f32x4*>(dh + (long)d * D_MODEL)[tid] = v;
    return;
  }
  const int per_pair = 2 * layers * N_HEAD;
  const int p = blk / per_pair, rem = blk - p * per_pair, lkv = rem / N_HEAD, h = rem - lkv * N_HEAD;
  const int src_slot = pairs[3 * p], dst_slot = pairs[3 * p + 1], len = pairs[3 * p + 2];
  float* base = ((lkv & 1) ? vc : kc) + (long)(lkv >> 1) * cache_layer;
  const f32x4* src = reinterpret_cast<const f32x4*>(base + ((long)src_slot * N_HEAD + h) * Tmax * D_HEAD);
  f32x4* dst = reinterpret_cast<f32x4*>(base + ((long)dst_slot * N_HEAD + h) * Tmax * D_HEAD);
  const int n4 = len * (D_HEAD / 4);                    // a head's cached rows are one contiguous stream of len x 64 floats
  int i = tid;
  // four 16-byte loads in flight per thread before the stores (source and destination come from the same arena pointer: the
  // compiler may not reorder a load past a store on its own)
  for (; i + 3 * 256 < n4; i += 4 * 256) {
    const f32x4 a0 = src[i], a1 = src[i + 256], a2 = src[i + 512], a3 = src[i + 768];
    dst[i] = a0; dst[i + 256] = a1; dst[i + 512] = a2; dst[i + 768] = a3;
  }
  for (; i < n4; i += 256) dst[i] = src[i];
}

void launch_beam_fanout(float* kc, float* vc, long cache_layer, int layers, int Tmax, const int* pairs, int npairs,
                        const float* hsrc, const int* hsrc_row, float* dh, int nrows, hipStream_t s) {
  const int ncopy = npairs * 2 * layers * N_HEAD;
  if (ncopy + nrows <= 0) return;
  hipLaunchKernelGGL(beam_fanout_kernel, dim3(ncopy + nrows), dim3(256), 0, s, kc, vc, cache_layer, Tmax, layers, pairs, ncopy, hsrc,
                     hsrc_row, dh);
}

}  // namespace vxe
