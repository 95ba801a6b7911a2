// The WSOLA walk that vx_stretch (stretch.hip) and the walked segments of vx_retime (retime.hip) share, and the search order and
// winner reduction that the mark walk of vx_psola (psola.hip) shares with both.  Not part of the public C ABI.
//
// A frame writes one output hop: a crossfade between the continuation of the previous input segment (the template
// t[j] = y[p_{k-1} + H + j]) and a new segment y[p_k + j], where p_k = n_k + d* is searched around the nominal position n_k for the
// smallest D_d = e_d - 2 c_d (the squared distance to the template minus the template's energy).  Where the n_k come from, which
// offsets d a frame may take and where its outputs go is the caller's; the frame itself is ws_frame.
//
// Arithmetic (the contract the tests rest on): candidate d is summed by ONE lane in double in sample order from 0.0, every product
// of two fp32 values is exact in double, the winner is a total order on (D, |d|, d), an output is two exact products, one double
// addition and one rounding.  The bits therefore depend neither on the lane, the wave, the job, the window nor the launch a frame
// lands in.  No atomics, no inline assembly.
//
// Work decomposition: frame k needs p_{k-1}, so a job is a serial walk by one 256-thread workgroup.  Everything frame k reads -- the
// search region, the new segment and the NEXT frame's template -- lies in y[n_k - D, n_k + D + 2H), which is staged into LDS as fp32
// with zeros outside the row (the padding never exists in HBM).  That span depends on n_k alone, not on p_{k-1}: the region of frame
// k + 1 is loaded into registers before frame k is searched and stored into the other LDS buffer behind the search.  The lanes of a
// wavefront take consecutive candidates: they read reg[c + j] at stride 1 (conflict-free) and t[j] as a broadcast.  Each lane keeps its
// best (D, d); six shuffle steps reduce a wavefront, one LDS step the four of them.
// LDS (stretch_host.h: ws_lds_bytes): 2 (2D + 2H) + H floats and 48 bytes -- 57 392 bytes at the largest options (two workgroups of a
// CU's 160 KiB), 6.7 KiB at hop 240, search 150, where the eight-wave limit of 256-thread workgroups per SIMD binds first.
//
// The head of this file is plain C++ (psola_host.h's sequential reference runs the same order); the rest is device code.  What
// psola.hip takes from it -- the order, the clean test, the reduction -- holds no floating-point arithmetic, so that file's
// `fp contract(off)` and the contraction the two walks are compiled with give this header the same bits.
#pragma once

#if defined(__HIPCC__)
#define VX_WS_HD __host__ __device__
#else
#define VX_WS_HD
#endif

namespace vxe {

constexpr int WS_NONE = 0x3fffffff;                          // the offset of a lane that saw no candidate: loses every tie

// the total order of the search: smaller cost, then smaller |d|, then the negative d
VX_WS_HD inline bool ws_better(double Ca, int da, double Cb, int db) {
  if (Ca != Cb) return Ca < Cb;
  const int aa = da < 0 ? -da : da, ab = db < 0 ? -db : db;
  return aa != ab ? aa < ab : da < db;
}

}  // namespace vxe

#if defined(__HIPCC__)
#include "stretch_host.h"

namespace vxe {

static_assert((2 * ST_SEARCH_MAX + 2 * ST_HOP_MAX + 255) / 256 <= 24, "the prefetch registers hold the largest region");

// kernel<NPRE>, NPRE the registers of a lane's prefetch: 256 NPRE >= S = 2D + 2H
#define WS_LAUNCH(kernel, S, ...)                                    \
  do {                                                               \
    if ((S) <= 8 * 256) hipLaunchKernelGGL(kernel<8>, __VA_ARGS__);  \
    else hipLaunchKernelGGL(kernel<24>, __VA_ARGS__);                \
  } while (0)

// a sample where it is finite, else 0
__device__ __forceinline__ float ws_clean(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u ? x : 0.f; }

// sample s of a job's row: 0 outside the row and where it is not finite.  The job stages every sample of the row its frames can read
// (st_span, rt_plan) -- the range test keeps a wrong table inside the buffer
struct WsRow {
  const float* in;                                               // the job's staged samples
  long s_lo, cnt;                                                // row sample index of in[0]; staged samples
  __device__ __forceinline__ float operator()(long s) const {
    const long r = s - s_lo;
    return r < 0 || r >= cnt ? 0.f : ws_clean(in[r]);
  }
};

// the LDS of a walk, behind `extern __shared__ double`
struct WsLds {
  double* redD;                                                  // [4] the wavefronts' winners
  int* redd;                                                     // [4]
  float* reg;                                                    // [2][S] the regions of this frame and the next
  float* t;                                                      // [H] the template
  int S;
  __device__ __forceinline__ WsLds(double* base, int H, int D)
      : redD(base), redd(reinterpret_cast<int*>(base + 4)), reg(reinterpret_cast<float*>(base + 6)), t(reg + 2 * (2 * D + 2 * H)), S(2 * D + 2 * H) {}
  __device__ __forceinline__ float* buf(int par) const { return reg + par * S; }
};

struct WsWin { double D; int d; };                               // the winning cost and offset of a frame

// The winner of the workgroup from every lane's best (C, d), in every lane.  behind_slots() runs between the write of the four slots
// and the barrier.  The caller keeps a barrier between this call and the next one's slot writes.
template <typename F>
__device__ __forceinline__ WsWin ws_reduce(double bC, int bd, double* redC, int* redd, F behind_slots) {
  const int tid = threadIdx.x;
  for (int off = 32; off; off >>= 1) {
    const double oC = __shfl_xor(bC, off, 64);
    const int od = __shfl_xor(bd, off, 64);
    if (ws_better(oC, od, bC, bd)) { bC = oC; bd = od; }
  }
  if ((tid & 63) == 0) { redC[tid >> 6] = bC; redd[tid >> 6] = bd; }
  behind_slots();
  __syncthreads();
  bC = redC[0]; bd = redd[0];
#pragma unroll
  for (int v = 1; v < 4; ++v)
    if (ws_better(redC[v], redd[v], bC, bd)) { bC = redC[v]; bd = redd[v]; }
  return {bC, bd};
}

// One frame.  l.buf(par) holds y[n_k - D, n_k - D + S) and l.t the template (both written, no barrier behind them yet).  more: a
// next frame exists and its region starts at row sample nbase.  [clo, chi]: the frame's candidates cd = d + D, never without D (d = 0).
// o: where output 0 of the frame goes; the first nout of its H outputs are stored.  Behind the call l.t holds the next frame's
// template, l.buf(par ^ 1) its region, and l.buf(par) stays as it is until the next call's barrier.
template <int NPRE>
__device__ __forceinline__ WsWin ws_frame(const WsLds& l, int par, const WsRow& y, bool more, long nbase, int clo, int chi, int H, int D,
                                          const float* __restrict__ w, float* __restrict__ o, int nout) {
  const int tid = threadIdx.x, S = l.S;
  const float* cur = l.buf(par);
  float* oth = l.buf(par ^ 1);
  float* t = l.t;
  __syncthreads();                                               // cur and t are written; nobody reads oth or red* any more
  float pre[NPRE];
  if (more) {
#pragma unroll
    for (int i = 0; i < NPRE; ++i) pre[i] = tid + 256 * i < S ? y(nbase + tid + 256 * i) : 0.f;
  }
  double bD = __builtin_inf();
  int bd = WS_NONE;
  for (int cd = clo + tid; cd <= chi; cd += 256) {
    const float* rp = cur + cd;
    double cs = 0.0, es = 0.0;
#pragma unroll 16
    for (int j = 0; j < H; ++j) {
      const double a = (double)rp[j], b = (double)t[j];
      cs += a * b;                                               // both products are exact in double: an fma gives the same bits
      es += a * a;
    }
    const double Dd = es - 2.0 * cs;                             // 2 c is exact
    if (ws_better(Dd, cd - D, bD, bd)) { bD = Dd; bd = cd - D; }
  }
  WsWin win = ws_reduce(bD, bd, l.redD, l.redd, [&] {
    if (more) {
#pragma unroll
      for (int i = 0; i < NPRE; ++i)
        if (tid + 256 * i < S) oth[tid + 256 * i] = pre[i];
    }
  });
  if (win.d < -D || win.d > D) win.d = 0;                        // d = 0 always qualifies: only a wrong table comes here
  const int r0 = win.d + D;                                      // p_k - (n_k - D), 0 .. 2D
  for (int j = tid; j < H; j += 256) {
    const float a = cur[r0 + j], tt = t[j];
    const float v = (float)((double)a * (double)w[j] + (double)tt * (double)w[H - 1 - j]);
    if (j < nout) o[j] = v;
    t[j] = cur[r0 + H + j];                                      // the next frame's template; lane j alone touches t[j] here
  }
  return win;
}

}  // namespace vxe
#endif
