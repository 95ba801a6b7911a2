// Sample-rate conversion of mono fp32 rows (vx_resample, include/vallex_hip.h): the Hann-windowed sinc resampler of
// utils/prompt_making.resample_sinc_hann (torchaudio's published default; unpinned: the package is not installed) on the device.
//
// With o, n = the two rates over their gcd, lpw = 6, rolloff = 0.99: base = min(o, n) * rolloff, width = ceil(lpw * o / base),
// K = 2 * width + o.  There are n phase kernels of K taps, built on the host in double and rounded once to fp32 (rs_build_taps of resample_host.h, the
// order of operations of resample_sinc_hann), cached in the context per (o, n) and kept in global memory TRANSPOSED, [K][n]: the
// lanes of a wavefront take consecutive output samples, i.e. consecutive phases, so tap j of 64 phases is one coalesced load.  The
// n * K <= 2^18 cap of the entry keeps a table at 1 MiB, far inside L2.
//
//   out[i * n + p] = sum_j k_p[j] * x[i * o + j - width],    x = 0 outside [0, L),    i * n + p < ceil(n * L / o)
//
// Arithmetic (the contract the tests rest on): every output element is computed by ONE lane, from a zero accumulator, by K fmaf in
// tap order j = 0 .. K-1.  Its bits therefore do not depend on the tile, the window, the row or the launch it lands in.
//
// Work decomposition: a launch covers a ragged list of JOBS (one job = a run of input blocks i of one row: a whole row, or one window
// of a long row), grid (tile, job).  A 256-thread workgroup takes B consecutive blocks = B * n outputs and stages its input span,
// (B - 1) * o + K floats, into LDS once, writing 0 for samples outside the row -- the padding never exists in HBM.  B is chosen per
// (o, n) on the host: about 2048 outputs per workgroup, the span within RS_LDS floats (32 KiB: two workgroups per CU leave LDS to
// spare).  Lane e of a tile reads xs[(e / n) * o + j]: the same word for the lanes of one block (a broadcast) and an odd or small
// stride across blocks.  A pair whose K alone exceeds RS_LDS (a rate ratio in the hundreds) runs the same loop on global memory
// instead (STAGED = false): same taps, same order, same bits.
// No atomics, no inline assembly.
#include <utility>

#include "wave_stage.h"
#include "resample_host.h"

#include "../../include/vallex_hip_dev.h"

namespace vxe {

// job record (RS_TAB ints, wave_stage.h): {in_off, s_lo, in_cnt, L, blk0, nblk, out_off, out_cnt}
constexpr int RS_LDS = 8192;               // floats of input span a workgroup stages
constexpr int RS_TILE_OUT = 2048;          // outputs a workgroup aims at
static_assert(VX_DEV_RESAMPLE_WINDOW_MIN >= 256 && VX_DEV_RESAMPLE_WINDOW_MIN <= RS_IN_CAP, "window bounds of the dev header");

// tab [njobs][8]:
//   in_off   first float of the job's staged samples in `in`
//   s_lo     row sample index of that float;  in_cnt  staged samples: the job's span cut to [0, L)
//   L        length of the row
//   blk0     first input block i of the job (row-global);  nblk  its blocks
//   out_off  first float of the job's outputs in `out`;  out_cnt  outputs of the job (the last block of a row may be cut)
template <bool STAGED>
__global__ __launch_bounds__(256) void resample_rows_kernel(const float* __restrict__ in, const int* __restrict__ tab,
                                                            const float* __restrict__ taps, float* __restrict__ out, int o, int n,
                                                            int width, int K, int B) {
  __shared__ float xs[STAGED ? RS_LDS : 1];
  const int* tb = tab + blockIdx.y * RS_TAB;
  const int nblk = tb[5], b0 = blockIdx.x * B;
  if (b0 >= nblk) return;                                        // block-uniform
  const int Bc = nblk - b0 < B ? nblk - b0 : B;
  const long in_off = tb[0], s_lo = tb[1], in_cnt = tb[2], L = tb[3], out_off = tb[6], out_cnt = tb[7];
  const long s0 = ((long)tb[4] + b0) * o - width;                // row sample under tap 0 of the tile's first block
  const int tid = threadIdx.x;
  // sample s of the row: 0 outside the row; the job holds every sample of the row its span touches (the second test never cuts a
  // sample the planner promised -- it keeps a wrong table inside the buffer)
  auto x_at = [&](long s) -> float {
    const long r = s - s_lo;
    return (s >= 0 && s < L && r >= 0 && r < in_cnt) ? in[in_off + r] : 0.f;
  };
  if (STAGED) {
    const int span = (Bc - 1) * o + K;                           // <= RS_LDS by the host's choice of B
    for (int t = tid; t < span; t += 256) xs[t] = x_at(s0 + t);
    __syncthreads();
  }
  const long e0 = (long)b0 * n;                                  // job-local index of the tile's first output
  const int nout = Bc * n;
  for (int e = tid; e < nout; e += 256) {
    if (e0 + e >= out_cnt) break;
    const int il = e / n, p = e - il * n;
    const float* kp = taps + p;
    float acc = 0.f;
    if (STAGED) {
      const float* xp = xs + il * o;
#pragma unroll 4
      for (int j = 0; j < K; ++j) acc = fmaf(kp[(long)j * n], xp[j], acc);
    } else {
      const long sb = s0 + (long)il * o;
      for (int j = 0; j < K; ++j) acc = fmaf(kp[(long)j * n], x_at(sb + j), acc);
    }
    out[out_off + e0 + e] = acc;
  }
}

// the cached device table of a pair ([K][n]), built and uploaded at its first use
static int rs_table(vx_ctx* c, const RsGeom& g, const float** dev) {
  const auto key = std::make_pair((int)g.o, (int)g.n);
  auto it = c->rs_taps.find(key);
  if (it == c->rs_taps.end()) {
    std::vector<float> t, tt;
    rs_build_taps(g, t);
    tt.resize(t.size());
    for (long p = 0; p < g.n; ++p)
      for (long j = 0; j < g.K; ++j) tt[(size_t)(j * g.n + p)] = t[(size_t)(p * g.K + j)];
    float* d = nullptr;
    if (int e = dev_alloc(c, &d, tt.size(), false)) return e;
    H2D(d, tt.data(), tt.size() * sizeof(float));
    it = c->rs_taps.emplace(key, d).first;
  }
  *dev = it->second;
  return VX_OK;
}

int rs_buffers(vx_ctx* c) {
  if (c->rs_in) return VX_OK;
  if (int e = dev_alloc(c, &c->rs_meta, (size_t)RS_MAX_JOBS * RS_TAB, false)) return e;
  if (int e = dev_alloc(c, &c->rs_out, (size_t)RS_OUT_CAP, false)) return e;
  return dev_alloc(c, &c->rs_in, (size_t)RS_IN_CAP, false);
}

int wave_check_rows(vx_ctx* c, const char* who, const float* wav, int64_t wav_stride, const int32_t* lens, int batch) {
  if (!wav) FAIL(VX_EINVAL, "%s: wav is NULL", who);
  if (!lens) FAIL(VX_EINVAL, "%s: lens is NULL", who);
  if (batch <= 0) FAIL(VX_EINVAL, "%s: batch %d below 1", who, batch);
  for (int i = 0; i < batch; ++i)
    if (lens[i] < 0 || lens[i] > wav_stride) FAIL(VX_EINVAL, "%s: lens[%d] = %ld outside 0 .. wav_stride %ld", who, i, (long)lens[i], (long)wav_stride);
  return VX_OK;
}

int wave_check_out_stride(vx_ctx* c, const char* who, const int32_t* lens, int batch, int64_t out_stride, const char* note) {
  for (int i = 0; i < batch; ++i)
    if (lens[i] > out_stride) FAIL(VX_EINVAL, "%s: out_stride %ld below the %ld samples of row %d%s", who, (long)out_stride, (long)lens[i], i, note);
  return VX_OK;
}

int wave_set_window(vx_ctx* c, long vx_ctx::*field, const char* who, const char* arg, int32_t samples, long lo, long hi) {
  if (!c) return VX_EINVAL;
  if (samples != 0 && (samples < lo || samples > hi)) FAIL(VX_EINVAL, "%s: %s %d outside %ld .. %ld (0 restores the default)", who, arg, samples, lo, hi);
  c->*field = samples;
  return VX_OK;
}

static int rs_blocks_per_tile(const RsGeom& g) {
  const long b_out = (RS_TILE_OUT + g.n - 1) / g.n;
  const long b_lds = g.K <= RS_LDS ? (RS_LDS - g.K) / g.o + 1 : 1;
  return (int)std::max<long>(1, std::min(b_out, b_lds));
}

}  // namespace vxe

extern "C" {

int vx_resample(vx_ctx* c, const float* wav, int64_t wav_stride, const int32_t* lens, int32_t batch, int32_t orig_rate,
                int32_t new_rate, float* out, int64_t out_stride, int32_t* out_lens) {
  using namespace vxe;
  if (!c) return VX_EINVAL;
  if (int e = wave_check_rows(c, "vx_resample", wav, wav_stride, lens, batch)) return e;
  if (!out) FAIL(VX_EINVAL, "vx_resample: out is NULL");
  if (!out_lens) FAIL(VX_EINVAL, "vx_resample: out_lens is NULL");
  if (orig_rate <= 0) FAIL(VX_EINVAL, "vx_resample: orig_rate %d below 1", orig_rate);
  if (new_rate <= 0) FAIL(VX_EINVAL, "vx_resample: new_rate %d below 1", new_rate);
  RsGeom g;
  const bool fits = rs_geometry(orig_rate, new_rate, &g);
  const bool same = g.o == g.n;
  if (!same && !fits)
    FAIL(VX_EINVAL, "vx_resample: orig_rate %d -> new_rate %d needs more than %ld filter taps (n K with o = %ld, n = %ld)", orig_rate,
         new_rate, RS_MAX_TAPS, g.o, g.n);
  std::vector<long> olen(batch);
  for (int i = 0; i < batch; ++i) {
    const long L = lens[i];
    olen[i] = same ? L : rs_out_len(g, L);
    if (olen[i] > 0x7fffffffL) FAIL(VX_EINVAL, "vx_resample: lens[%d] = %ld gives %ld output samples, more than out_lens holds", i, L, olen[i]);
    if (olen[i] > out_stride) FAIL(VX_EINVAL, "vx_resample: out_stride %ld below the %ld output samples of row %d", (long)out_stride, olen[i], i);
  }
  if (same) {                                                    // nothing to filter: the input bits
    for (int i = 0; i < batch; ++i) {
      if (olen[i]) memmove(out + (long)i * out_stride, wav + (long)i * wav_stride, (size_t)olen[i] * sizeof(float));
      out_lens[i] = (int32_t)olen[i];
    }
    return VX_OK;
  }
  const long win = wave_window(c->rs_window, RS_IN_CAP);
  if (g.K > win) FAIL(VX_EINVAL, "vx_resample: the window of %ld input samples (vx_dev_resample_window) is below the %ld taps of %d -> %d", win, g.K, orig_rate, new_rate);
  HIPCHK(hipSetDevice(c->dev));
  if (int e = rs_buffers(c)) return e;
  const float* taps = nullptr;
  if (int e = rs_table(c, g, &taps)) return e;
  const int B = rs_blocks_per_tile(g);
  const bool staged = g.K <= RS_LDS;

  // one launch per group of jobs (resample_host.h: rs_plan), everything of a launch behind one stream sync
  std::vector<RsJob> jobs;
  if (!rs_plan(g, lens, batch, win, RS_OUT_CAP, RS_MAX_JOBS, &jobs)) FAIL(VX_EINVAL, "vx_resample: no block fits an empty launch (window %ld)", win);   // K <= win rules it out
  std::vector<int> tab;
  const int err = wave_launches(c, jobs, [&](size_t j0, size_t j1) -> int {
    tab.clear();
    long max_blk = 0;
    for (size_t k = j0; k < j1; ++k) {
      const RsJob& j = jobs[k];
      for (long v : {j.in_off, j.s_lo, j.s_hi - j.s_lo, (long)lens[j.row], j.a, j.b - j.a, j.out_off, j.out_cnt}) tab.push_back((int)v);
      max_blk = std::max(max_blk, j.b - j.a);
      if (j.s_hi > j.s_lo)
        H2D(c->rs_in + j.in_off, wav + (long)j.row * wav_stride + j.s_lo, (size_t)(j.s_hi - j.s_lo) * sizeof(float));
    }
    H2D(c->rs_meta, tab.data(), tab.size() * sizeof(int));
    const dim3 grid((unsigned)((max_blk + B - 1) / B), (unsigned)(j1 - j0));
    if (staged)
      hipLaunchKernelGGL(resample_rows_kernel<true>, grid, dim3(256), 0, c->stream, c->rs_in, c->rs_meta, taps, c->rs_out, (int)g.o,
                         (int)g.n, (int)g.width, (int)g.K, B);
    else
      hipLaunchKernelGGL(resample_rows_kernel<false>, grid, dim3(256), 0, c->stream, c->rs_in, c->rs_meta, taps, c->rs_out, (int)g.o,
                         (int)g.n, (int)g.width, (int)g.K, B);
    for (size_t k = j0; k < j1; ++k) {
      const RsJob& j = jobs[k];
      D2H(out + (long)j.row * out_stride + j.a * g.n, c->rs_out + j.out_off, (size_t)j.out_cnt * sizeof(float));
    }
    return VX_OK;
  });
  if (err) return err;
  for (int i = 0; i < batch; ++i) out_lens[i] = (int32_t)olen[i];
  return VX_OK;
}

int vx_dev_resample_taps(vx_ctx* c, int32_t orig_rate, int32_t new_rate, float* taps, int32_t* geom) {
  using namespace vxe;
  if (!c) return VX_EINVAL;
  if (!geom) FAIL(VX_EINVAL, "vx_dev_resample_taps: geom is NULL");
  if (orig_rate <= 0 || new_rate <= 0) FAIL(VX_EINVAL, "vx_dev_resample_taps: orig_rate %d or new_rate %d below 1", orig_rate, new_rate);
  RsGeom g;
  if (!rs_geometry(orig_rate, new_rate, &g)) FAIL(VX_EINVAL, "vx_dev_resample_taps: orig_rate %d -> new_rate %d needs more than %ld filter taps", orig_rate, new_rate, RS_MAX_TAPS);
  geom[0] = (int32_t)g.o; geom[1] = (int32_t)g.n; geom[2] = (int32_t)g.width; geom[3] = (int32_t)g.K;
  if (!taps) return VX_OK;
  HIPCHK(hipSetDevice(c->dev));
  const float* dev = nullptr;
  if (int e = rs_table(c, g, &dev)) return e;
  std::vector<float> tt((size_t)(g.n * g.K));
  D2H(tt.data(), dev, tt.size() * sizeof(float));
  SYNC();
  for (long p = 0; p < g.n; ++p)
    for (long j = 0; j < g.K; ++j) taps[p * g.K + j] = tt[(size_t)(j * g.n + p)];
  return VX_OK;
}

int vx_dev_resample_window(vx_ctx* c, int32_t input_samples) {
  return vxe::wave_set_window(c, &vx_ctx::rs_window, "vx_dev_resample_window", "input_samples", input_samples, VX_DEV_RESAMPLE_WINDOW_MIN,
                              vxe::RS_IN_CAP);
}

}  // extern "C"
