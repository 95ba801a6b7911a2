// Text attention of the AR decoder's audio rows (vx_align, include/vallex_hip.h): which text position a frame came from.
// The AR stack runs ONE sequence text ++ BOS ++ prompt ++ frames under the prefix-LM mask (models/vallex.py:535-549): every audio row
// sees all text and the audio up to itself.  The streaming-softmax kernels (attn_full*.hip, dec_attn) never hold a probability; this
// kernel computes, from the packed fp32 q / k rows of one layer's in_proj, for every reported audio row r and text column s < S
//
//   out[out_off + t][s] += sum_h w[h] * softmax_j(0.125 * q_r,h . k_j,h)[s],      j = 0 .. r   (n = r + 1 keys),  r = q_first + t
//
// in exact fp32 on the f32 MFMA (v_mfma_f32_32x32x2_f32, the operand maps of attn_full.hip): q scaled by 0.125 before the product,
// fp32 products and accumulation, libm expf, the denominator over all n keys.
//
// Work decomposition: one 256-thread workgroup = ALIGN_R = 32 audio rows of one sequence, all 16 heads.
//   phase 1  wave w takes heads 4w .. 4w+3: streams the key tiles (ALIGN_KT = 32 keys, K fragments straight from global memory into
//            registers, the next tile's loads in flight under the current tile's MFMAs -- no LDS staging: the four waves read
//            DIFFERENT heads, there is nothing to share) keeping the running maximum m and sum l of every row; (m, l) go to LDS.
//   phase 2  wave w takes the text tiles w, w + 4, ...: per tile, the heads IN INDEX ORDER recompute the 32 x 32 scores of the text
//            columns only (S is a small part of n) and add w[h] * expf(s - m) / l to the accumulator of the element, which one lane
//            owns for all heads; after the last head ONE `+=` per element into `out`.
// The S^T = K . Q^T product leaves one query per lane (column lane & 31) and 16 keys per lane: the row maximum / sum are in-register
// plus one exchange with lane ^ 32.
// The accumulator over the heads is a double: the 16 fp32 terms are added without a rounding of their own, so an element is
// within one rounding of the sum of its fp32 terms whatever the weights are (a float accumulator adds up to 15 more).
// Determinism: no atomics; an element is owned by one lane of one workgroup; heads in index order; layers in stream order by
// successive launches; a sequence's result does not depend on what else is in the launch.
#include <cmath>

#include "engine_ctx.h"

#include "../../include/vallex_hip_dev.h"

namespace vxe {

constexpr int ALIGN_R = 32, ALIGN_KT = 32, ALIGN_TAB = 6;
static_assert(ALIGN_R == VX_DEV_ALIGN_ROW_TILE && ALIGN_KT == VX_DEV_ALIGN_KEY_TILE, "the dev header states the kernel's tiles");
constexpr float ALIGN_MASKED = -1e30f;      // finite stand-in for -inf: expf(ALIGN_MASKED - m) is exactly 0

// tab [nseq][6] = {seq_off, seq_len, S, q_first, n_rows, out_off}; grid (row tiles, nseq)
__global__ __launch_bounds__(256) void align_rows_kernel(const float* __restrict__ qkv, const int* __restrict__ tab,
                                                         const float* __restrict__ w, float* __restrict__ out, int ld_out) {
  __shared__ float ml[N_HEAD][ALIGN_R][2];
  const int* tb = tab + blockIdx.y * ALIGN_TAB;
  const int T = tb[4], t0 = blockIdx.x * ALIGN_R;
  if (t0 >= T) return;                                           // block-uniform
  const long row0 = tb[0];
  const int S = tb[2], qf = tb[3], out_off = tb[5];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, hi = lane >> 5, l31 = lane & 31;
  const int t = t0 + l31;                                        // this lane's reported row
  const bool live = t < T;
  const int qi = qf + (live ? t : T - 1);                        // its query (sequence-local); a dead lane repeats the last one
  const int q_last = qf + (t0 + ALIGN_R - 1 < T ? t0 + ALIGN_R - 1 : T - 1);
  const int kv_end = q_last + 1;                                 // keys the tile's last row sees; <= seq_len
  const int ntiles = (kv_end + ALIGN_KT - 1) / ALIGN_KT;
  const float* qrow = qkv + (row0 + qi) * (long)(3 * D_MODEL) + hi * 4;
  const float* kbase = qkv + row0 * (long)(3 * D_MODEL) + D_MODEL + hi * 4;

  // Q fragment of head h: Q[q][8c + 4hi + j] * 1/sqrt(64)
  auto load_q = [&](int h, float* qreg) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(qrow + h * D_HEAD + c * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j) qreg[c * 4 + j] = v[j] * 0.125f;
    }
  };
  // K fragment of the tile at k0: key k0 + l31 (clamped into the visible range: a clamped key is masked below), columns 8c + 4hi + j
  auto load_k = [&](int h, int k0, f32x4* kf) {
    int kk = k0 + l31;
    kk = kk < kv_end ? kk : kv_end - 1;
    const float* kp = kbase + kk * (long)(3 * D_MODEL) + h * D_HEAD;
#pragma unroll
    for (int c = 0; c < 8; ++c) kf[c] = *reinterpret_cast<const f32x4*>(kp + c * 8);
  };
  // S^T tile = K_tile . Q^T: s[r] = score(query qi, key k0 + (r & 3) + 8 (r >> 2) + 4 hi)
  auto qk = [&](const f32x4* kf, const float* qreg) {
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c)
#pragma unroll
      for (int j = 0; j < 4; ++j) s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[c][j], qreg[c * 4 + j], s, 0, 0, 0);
    return s;
  };

  // ---- phase 1: (m, l) of every row, heads 4 wid .. 4 wid + 3
  for (int h = wid * 4; h < wid * 4 + 4; ++h) {
    if (w[h] == 0.f) continue;                                   // wave-uniform: a skipped head is never read
    float qreg[32];
    load_q(h, qreg);
    float m_run = ALIGN_MASKED, l_run = 0.f;
    f32x4 kf[8], kn[8];
    load_k(h, 0, kf);
    for (int kt = 0; kt < ntiles; ++kt) {
      const int k0 = kt * ALIGN_KT;
      if (kt + 1 < ntiles) load_k(h, k0 + ALIGN_KT, kn);
      f32x16 s = qk(kf, qreg);
      float m_tile = ALIGN_MASKED;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kj = k0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        s[r] = kj <= qi ? s[r] : ALIGN_MASKED;                    // all text (qi >= S) and the audio up to the row itself
        m_tile = fmaxf(m_tile, s[r]);
      }
      m_tile = fmaxf(m_tile, __shfl_xor(m_tile, 32, 64));        // the tile's other 16 keys live in lane ^ 32
      const float m_new = fmaxf(m_run, m_tile);                  // finite from the first tile on: key 0 is visible to every row
      float psum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) psum += expf(s[r] - m_new);
      l_run = l_run * expf(m_run - m_new) + psum;
      m_run = m_new;
      if (kt + 1 < ntiles)
#pragma unroll
        for (int c = 0; c < 8; ++c) kf[c] = kn[c];
    }
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    if (hi == 0) { ml[h][l31][0] = m_run; ml[h][l31][1] = l_tot; }
  }
  __syncthreads();

  // ---- phase 2: the text columns, tiles wid, wid + 4, ...
  for (int k0 = wid * ALIGN_KT; k0 < S; k0 += 4 * ALIGN_KT) {
    double acc[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0;
    for (int h = 0; h < N_HEAD; ++h) {
      const float wh = w[h];
      if (wh == 0.f) continue;
      float qreg[32];
      f32x4 kf[8];
      load_q(h, qreg);
      load_k(h, k0, kf);
      const f32x16 s = qk(kf, qreg);
      const float m = ml[h][l31][0], l = ml[h][l31][1];
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] += (double)((wh * expf(s[r] - m)) / l);
    }
    if (live) {
      float* op = out + (long)(out_off + t) * ld_out;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kj = k0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        if (kj < S) op[kj] += (float)acc[r];
      }
    }
  }
}

void launch_align_rows(const float* qkv, const int* tab, int nseq, int max_rows, const float* w, float* out, int ld_out, hipStream_t s) {
  if (nseq <= 0 || max_rows <= 0) return;
  hipLaunchKernelGGL(align_rows_kernel, dim3((max_rows + ALIGN_R - 1) / ALIGN_R, nseq), dim3(256), 0, s, qkv, tab, w, out, ld_out);
}

}  // namespace vxe

extern "C" {

// vx_dev_align_rows: ONE launch of align_rows_kernel on caller rows (private scratch; `out` goes in and comes back).
int vx_dev_align_rows(vx_ctx* c, int32_t M, int32_t nseq, const int32_t* tab, const float* qkv, const float* w, float* out,
                      int32_t rows_out, int32_t ld_out) {
  using namespace vxe;
  if (!c) return VX_EINVAL;
  if (c->serve) FAIL(VX_ESTATE, "vx_dev_align_rows: a serving session is open on this context (vx_serve_close it first)");
  if (!tab || !qkv || !w || !out) FAIL(VX_EINVAL, "vx_dev_align_rows: null tab, qkv, w or out");
  if (M < 1 || M > 8192) FAIL(VX_EINVAL, "vx_dev_align_rows: M outside 1 .. 8192");
  if (nseq < 1 || nseq > 32) FAIL(VX_EINVAL, "vx_dev_align_rows: nseq outside 1 .. 32");
  if (rows_out < 1 || rows_out > 16384) FAIL(VX_EINVAL, "vx_dev_align_rows: rows_out outside 1 .. 16384");
  if (ld_out < 1 || ld_out > 8192) FAIL(VX_EINVAL, "vx_dev_align_rows: ld_out outside 1 .. 8192");
  int max_rows = 0;
  for (int i = 0; i < nseq; ++i) {
    const int32_t* t = tab + i * ALIGN_TAB;
    const long off = t[0], len = t[1], S = t[2], qf = t[3], T = t[4], oo = t[5];
    if (off < 0 || len < 1 || off + len > M) FAIL(VX_EINVAL, "vx_dev_align_rows: sequence %d: seq_off %ld, seq_len %ld leave [0, M)", i, off, len);
    if (S < 1) FAIL(VX_EINVAL, "vx_dev_align_rows: sequence %d: S %ld below 1", i, S);
    if (qf < S) FAIL(VX_EINVAL, "vx_dev_align_rows: sequence %d: q_first %ld below S %ld", i, qf, S);
    if (T < 0 || qf + T > len) FAIL(VX_EINVAL, "vx_dev_align_rows: sequence %d: q_first %ld + n_rows %ld outside seq_len %ld", i, qf, T, len);
    if (ld_out < S) FAIL(VX_EINVAL, "vx_dev_align_rows: sequence %d: ld_out %d below S %ld", i, ld_out, S);
    if (oo < 0 || oo + T > rows_out) FAIL(VX_EINVAL, "vx_dev_align_rows: sequence %d: out_off %ld + n_rows %ld outside rows_out %d", i, oo, T, rows_out);
    for (int j = 0; j < i; ++j) {                              // an output row belongs to one sequence
      const long oj = tab[j * ALIGN_TAB + 5], Tj = tab[j * ALIGN_TAB + 4];
      if (T > 0 && Tj > 0 && oo < oj + Tj && oj < oo + T) FAIL(VX_EINVAL, "vx_dev_align_rows: out_off of sequences %d and %d overlap", j, i);
    }
    max_rows = std::max(max_rows, (int)T);
  }
  for (int h = 0; h < N_HEAD; ++h)
    if (!std::isfinite(w[h]) || w[h] < 0.f) FAIL(VX_EINVAL, "vx_dev_align_rows: w[%d] is negative or not finite", h);
  HIPCHK(hipSetDevice(c->dev));
  float *dq = nullptr, *dw = nullptr, *dout = nullptr;
  int* dtab = nullptr;
  auto cleanup = [&]() { for (void* p : {(void*)dq, (void*)dw, (void*)dout, (void*)dtab}) if (p) (void)hipFree(p); };
  hipError_t he;
  // an error return drains the ring first: a queued xfer_d2h must not be delivered into host buffers that are gone by then
#define TRY(x) if ((he = (x)) != hipSuccess) { (void)xfer_sync(c); cleanup(); c->err = std::string(#x) + ": " + hipGetErrorString(he); return VX_EHIP; }
#define TRYX(x) do { if (int _e = (x)) { const std::string _m = c->err; (void)xfer_sync(c); c->err = _m; cleanup(); return _e; } } while (0)
  const size_t out_bytes = (size_t)rows_out * ld_out * 4;
  TRY(hipMalloc((void**)&dq, (size_t)M * 3 * D_MODEL * 4));
  TRYX(xfer_h2d(c, dq, qkv, (size_t)M * 3 * D_MODEL * 4));
  TRY(hipMalloc((void**)&dtab, (size_t)nseq * ALIGN_TAB * 4));
  TRYX(xfer_h2d(c, dtab, tab, (size_t)nseq * ALIGN_TAB * 4));
  TRY(hipMalloc((void**)&dw, N_HEAD * 4));
  TRYX(xfer_h2d(c, dw, w, N_HEAD * 4));
  TRY(hipMalloc((void**)&dout, out_bytes));
  TRYX(xfer_h2d(c, dout, out, out_bytes));
  launch_align_rows(dq, dtab, nseq, max_rows, dw, dout, ld_out, c->stream);
  TRYX(xfer_d2h(c, out, dout, out_bytes));
  TRYX(xfer_sync(c));
  TRY(hipGetLastError());
#undef TRY
#undef TRYX
  cleanup();
  return VX_OK;
}

}  // extern "C"
