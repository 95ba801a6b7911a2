// The time map (vx_pauses and vx_retime, include/vallex_hip.h): where the pauses of a row are, and a piecewise map from input to
// output time applied segment by segment -- copies where a segment keeps its length, WSOLA with both ends pinned where it does not.
//
// vx_pauses runs the frames pass of the output stage (fn_measure, wave_frames_kernel) and reduces every row's frame table on the host
// (retime_host.h: rt_pauses); it has no kernel of its own.
//
// vx_retime: a walked segment is the walk of stretch.hip under the same arithmetic contract -- candidate d summed by ONE lane in
// double in sample order from 0.0, exact products, the total order on (D, |d|, d), an output of two exact products, one double
// addition and one rounding -- with three differences: frame 0 starts at the segment's anchor, the nominal positions follow the line
// to the end pin and come from the job record, and the search is clipped to the segment (the last frame to the one offset of the
// pin).  The bits therefore depend neither on the lane, the wave, the job, the window nor the launch a segment lands in.  No atomics,
// no inline assembly.
//
// Work decomposition: inside a walked segment frame k needs p_{k-1}, but a segment starts at a_i and ends at a_{i+1} whatever its
// neighbours find, so the segments of a row -- and of all rows -- are independent JOBS: grid (job), one 256-thread workgroup per job.
// A job is one walked segment, or a tile of a run of copy segments (the bits of the input, as 32-bit words).  As in stretch.hip the
// region y[n_k - D, n_k + D + 2H) of a frame and the template are in LDS, the region of frame k + 1 (it depends on n_{k+1} alone) is
// loaded into registers before frame k is searched and stored into the other LDS buffer behind the search; a wavefront reads
// reg[c + j] at stride 1 (conflict-free) and t[j] as a broadcast; six shuffle steps reduce a wavefront, one LDS step the four.
// LDS: 2 (2D + 2H) + H floats and 48 bytes, as stretch.hip: 57 392 bytes at the largest options (two workgroups of a CU's 160 KiB),
// 6.7 KiB at hop 240, search 150, where the eight-wave limit of 256-thread workgroups per SIMD binds first.
#include "wave_stage.h"
#include "retime_host.h"

#include "../../include/vallex_hip_dev.h"

namespace vxe {

constexpr int RT_TAB = 16;                                   // ints of a job record
constexpr int RT_MAX_JOBS = RS_MAX_JOBS * RS_TAB / RT_TAB;   // the records of a launch fill rs_meta
constexpr long RT_FRAME_CAP = 1L << 18;                      // frames of a launch: the position / cost tables
constexpr int RT_NONE = 0x3fffffff;                          // the offset of a lane that saw no candidate: loses every tie
static_assert(VX_RETIME_WINDOW == RS_IN_CAP, "vx_retime runs in the resampler's launch buffers");
static_assert(VX_DEV_RETIME_WINDOW_MIN >= 1 && VX_DEV_RETIME_WINDOW_MIN <= VX_RETIME_WINDOW, "window bounds of the dev header");
static_assert((2 * ST_SEARCH_MAX + 2 * ST_HOP_MAX + 255) / 256 <= 24, "the prefetch registers hold the largest region");
static_assert(48 + (2 * (2 * ST_SEARCH_MAX + 2 * ST_HOP_MAX) + ST_HOP_MAX) * sizeof(float) <= 65536, "LDS of the largest options");

// the total order of the search: smaller D, then smaller |d|, then the negative d
__device__ __forceinline__ bool rt_better(double Da, int da, double Db, int db) {
  if (Da != Db) return Da < Db;
  const int aa = da < 0 ? -da : da, ab = db < 0 ? -db : db;
  return aa != ab ? aa < ab : da < db;
}

// tab [njobs][RT_TAB]:
//   0 walk     1: a walked segment, 0: a copy tile
//   1 in_off   first float of the job's staged samples in `in`
//   2 s_lo     row sample index of that float;  3 in_cnt  staged samples (a copy tile: the samples to copy)
//   4 a, 5 a1  the segment's input samples [a, a1) of the row
//   6 out_off  first float of the job's outputs in `out`;  7 lb  output samples of the job
//   8 f_off    first record of the job in `pos` / `cost`
// NPRE: registers of the prefetch, 256 NPRE >= 2D + 2H
template <int NPRE>
__global__ __launch_bounds__(256) void retime_rows_kernel(const float* __restrict__ in, const int* __restrict__ tab,
                                                          const float* __restrict__ w, float* __restrict__ out, int* __restrict__ pos,
                                                          double* __restrict__ cost, int H, int D) {
  extern __shared__ double rt_lds[];
  double* redD = rt_lds;                                         // [4] the wavefronts' winners
  int* redd = reinterpret_cast<int*>(rt_lds + 4);                // [4]
  float* reg = reinterpret_cast<float*>(rt_lds + 6);             // [2][S] the regions of this frame and the next
  const int S = 2 * D + 2 * H;
  float* t = reg + 2 * S;                                        // [H] the template
  const int* tb = tab + blockIdx.x * RT_TAB;
  const long in_off = tb[1], s_lo = tb[2], in_cnt = tb[3], a = tb[4], a1 = tb[5], out_off = tb[6], lb = tb[7], f_off = tb[8];
  const int tid = threadIdx.x;
  if (!tb[0]) {                                                  // a copy tile: the words of the input (block-uniform)
    const unsigned* src = reinterpret_cast<const unsigned*>(in + in_off);
    unsigned* dst = reinterpret_cast<unsigned*>(out + out_off);
    for (long i = tid; i < in_cnt && i < lb; i += 256) dst[i] = src[i];
    return;
  }
  // sample s of the row: 0 outside the row and where it is not finite; the job holds every sample of the row its frames can read
  // (retime_host.h: rt_plan) -- the range test keeps a wrong table inside the buffer
  auto y_at = [&](long s) -> float {
    const long r = s - s_lo;
    if (r < 0 || r >= in_cnt) return 0.f;
    const float x = in[in_off + r];
    return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u ? x : 0.f;
  };
  const int M = (int)(lb / H), rem = (int)(lb - (long)M * H);
  if (M < 2) return;                                             // the checks rule it out; a wrong table divides by nothing
  const long slope = (a1 - a) - lb + (long)(M - 1) * H;          // n_k = a + floor(k slope / (M - 1))
  for (int j = tid; j < H; j += 256) out[out_off + j] = y_at(a + j);   // frame 0: p_0 = a, the input itself
  if (tid == 0) { pos[f_off] = (int)a; cost[f_off] = 0.0; }
  for (int j = tid; j < H; j += 256) t[j] = y_at(a + H + j);
  {
    const long base = a + slope / (M - 1) - D;
    for (int i = tid; i < S; i += 256) reg[i] = y_at(base + i);
  }
  for (int k = 1; k < M; ++k) {
    float* cur = reg + ((k - 1) & 1) * S;
    float* oth = reg + (((k - 1) & 1) ^ 1) * S;
    const long nk = a + (long)k * slope / (M - 1);               // cur holds y[n_k - D, n_k - D + S)
    __syncthreads();                                             // cur and t are written; nobody reads oth or red* any more
    const bool more = k + 1 < M;
    float pre[NPRE];
    if (more) {
      const long nbase = a + (long)(k + 1) * slope / (M - 1) - D;
#pragma unroll
      for (int i = 0; i < NPRE; ++i) pre[i] = tid + 256 * i < S ? y_at(nbase + tid + 256 * i) : 0.f;
    }
    // the candidates cd = d + D of this frame: the search clipped to the segment; the pinned last frame has d = 0 alone
    int clo = D, chi = D;
    if (more) {
      const long dlo = a - nk > -(long)D ? a - nk : -(long)D, dhi = a1 - H - nk < (long)D ? a1 - H - nk : (long)D;
      clo = (int)dlo + D; chi = (int)dhi + D;
    }
    double bD = __builtin_inf();
    int bd = RT_NONE;
    for (int cd = clo + tid; cd <= chi; cd += 256) {
      const float* rp = cur + cd;
      double cs = 0.0, es = 0.0;
#pragma unroll 16
      for (int j = 0; j < H; ++j) {
        const double x = (double)rp[j], b = (double)t[j];
        cs += x * b;                                             // both products are exact in double: an fma gives the same bits
        es += x * x;
      }
      const double Dd = es - 2.0 * cs;                           // 2 c is exact
      if (rt_better(Dd, cd - D, bD, bd)) { bD = Dd; bd = cd - D; }
    }
    for (int off = 32; off; off >>= 1) {
      const double oD = __shfl_xor(bD, off, 64);
      const int od = __shfl_xor(bd, off, 64);
      if (rt_better(oD, od, bD, bd)) { bD = oD; bd = od; }
    }
    if ((tid & 63) == 0) { redD[tid >> 6] = bD; redd[tid >> 6] = bd; }
    if (more) {
#pragma unroll
      for (int i = 0; i < NPRE; ++i)
        if (tid + 256 * i < S) oth[tid + 256 * i] = pre[i];
    }
    __syncthreads();
    bD = redD[0]; bd = redd[0];
#pragma unroll
    for (int v = 1; v < 4; ++v)
      if (rt_better(redD[v], redd[v], bD, bd)) { bD = redD[v]; bd = redd[v]; }
    if (bd < -D || bd > D) bd = 0;                               // d = 0 always qualifies: only a wrong table comes here
    const int r0 = bd + D;                                       // p_k - (n_k - D), 0 .. 2D
    const long o0 = out_off + (long)k * H;
    if (!more)                                                   // the pinned frame goes on plainly to the anchor
      for (int j = tid; j < rem; j += 256) out[o0 + H + j] = cur[r0 + H + j];
    for (int j = tid; j < H; j += 256) {
      const float x = cur[r0 + j], tt = t[j];
      out[o0 + j] = (float)((double)x * (double)w[j] + (double)tt * (double)w[H - 1 - j]);
      t[j] = cur[r0 + H + j];                                    // the next frame's template; lane j alone touches t[j] here
    }
    if (tid == 0) { pos[f_off + k] = (int)(nk + bd); cost[f_off + k] = bD; }
  }
}

// the crossfade table, rebuilt when the hop changes, and the position / cost tables of a launch
static int rt_tables(vx_ctx* c, int H) {
  if (!c->rt_fade) {
    if (int e = dev_alloc(c, &c->rt_fade, (size_t)ST_HOP_MAX, false)) return e;
    if (int e = dev_alloc(c, &c->rt_pos, (size_t)RT_FRAME_CAP, false)) return e;
    if (int e = dev_alloc(c, &c->rt_cost, (size_t)RT_FRAME_CAP, false)) return e;
  }
  if (c->rt_fade_n != H) {
    std::vector<float> t;
    fn_fade_table(H, t);
    H2D(c->rt_fade, t.data(), t.size() * sizeof(float));
    c->rt_fade_n = H;
  }
  return VX_OK;
}

}  // namespace vxe

extern "C" {

int vx_pauses(vx_ctx* c, const float* wav, int64_t wav_stride, const int32_t* lens, int32_t batch, const vx_pause_opts* o, int32_t* spans,
              int64_t span_stride, int32_t* counts) {
  using namespace vxe;
  if (!c) return VX_EINVAL;
  if (int e = wave_check_rows(c, "vx_pauses", wav, wav_stride, lens, batch)) return e;
  if (!o) FAIL(VX_EINVAL, "vx_pauses: o is NULL");
  if (!spans) FAIL(VX_EINVAL, "vx_pauses: spans is NULL");
  if (!counts) FAIL(VX_EINVAL, "vx_pauses: counts is NULL");
  CHECK_STRUCT_OF("vx_pauses", *o, vx_pause_opts);
  char why[200];
  if (rt_check_pause_opts(*o, why, sizeof why)) FAIL(VX_EINVAL, "vx_pauses: %s", why);
  HIPCHK(hipSetDevice(c->dev));
  if (int e = rs_buffers(c)) return e;
  std::vector<FnFrame> table;
  std::vector<long> f0, base;
  bool resident = false;
  if (int e = fn_measure(c, wav, wav_stride, lens, batch, o->frame, table, f0, &resident, base)) return e;
  const double thr2 = fn_thr2(o->silence_db);
  std::vector<std::vector<int>> found((size_t)batch);
  for (int i = 0; i < batch; ++i) {
    rt_pauses(table.data() + f0[(size_t)i], lens[i], *o, thr2, &found[(size_t)i]);
    if ((int64_t)found[(size_t)i].size() > span_stride)
      FAIL(VX_EINVAL, "vx_pauses: span_stride %ld below the %zu ints of the %zu pauses of row %d", (long)span_stride, found[(size_t)i].size(),
           found[(size_t)i].size() / 2, i);
  }
  for (int i = 0; i < batch; ++i) {
    const std::vector<int>& f = found[(size_t)i];
    if (!f.empty()) memcpy(spans + (long)i * span_stride, f.data(), f.size() * sizeof(int));
    counts[i] = (int32_t)(f.size() / 2);
  }
  return VX_OK;
}

int vx_retime(vx_ctx* c, const float* wav, int64_t wav_stride, const int32_t* lens, int32_t batch, const int32_t* anchors,
              int64_t anchor_stride, const int32_t* n_anchors, const vx_retime_opts* o, float* out, int64_t out_stride, int32_t* out_lens,
              int32_t* pos, double* cost, int64_t pos_stride) {
  using namespace vxe;
  if (!c) return VX_EINVAL;
  const char* who = "vx_retime";
  if (int e = wave_check_rows(c, who, wav, wav_stride, lens, batch)) return e;
  if (!anchors) FAIL(VX_EINVAL, "%s: anchors is NULL", who);
  if (!n_anchors) FAIL(VX_EINVAL, "%s: n_anchors is NULL", who);
  if (!o) FAIL(VX_EINVAL, "%s: o is NULL", who);
  if (!out) FAIL(VX_EINVAL, "%s: out is NULL", who);
  if (!out_lens) FAIL(VX_EINVAL, "%s: out_lens is NULL", who);
  CHECK_STRUCT_OF(who, *o, vx_retime_opts);
  char why[240];
  if (rt_check_opts(*o, why, sizeof why)) FAIL(VX_EINVAL, "%s: %s", who, why);
  const int H = o->hop, D = o->search;
  std::vector<int32_t> olen((size_t)batch);
  for (int i = 0; i < batch; ++i) {
    if (n_anchors[i] >= 1 && 2 * (int64_t)n_anchors[i] > anchor_stride)
      FAIL(VX_EINVAL, "%s: anchor_stride %ld below the %ld ints of n_anchors[%d] = %d", who, (long)anchor_stride, 2L * n_anchors[i], i, n_anchors[i]);
    long Lout, frames;
    if (rt_check_anchors(anchors + (long)i * anchor_stride, n_anchors[i], lens[i], H, &Lout, &frames, why, sizeof why))
      FAIL(VX_EINVAL, "%s: row %d: %s", who, i, why);
    olen[(size_t)i] = (int32_t)Lout;
    if ((pos || cost) && frames > pos_stride) FAIL(VX_EINVAL, "%s: pos_stride %ld below the %ld frames of row %d", who, (long)pos_stride, frames, i);
  }
  if (int e = wave_check_out_stride(c, who, olen.data(), batch, out_stride, "")) return e;
  const long win = wave_window(c->rt_window, VX_RETIME_WINDOW);
  std::vector<RtJob> jobs;
  int bad_row;
  long bad_seg;
  if (!rt_plan(anchors, anchor_stride, n_anchors, lens, batch, H, D, win, RS_OUT_CAP, RT_FRAME_CAP, RT_MAX_JOBS, RT_TILE, &jobs, &bad_row, &bad_seg))
    FAIL(VX_EINVAL, "%s: row %d: segment %ld is walked and longer than a launch window of %ld input samples (vx_dev_retime_window), %ld output samples "
                    "or %ld frames", who, bad_row, bad_seg, win, RS_OUT_CAP, RT_FRAME_CAP);
  if (!jobs.empty()) {
    HIPCHK(hipSetDevice(c->dev));
    if (int e = rs_buffers(c)) return e;
    if (int e = rt_tables(c, H)) return e;
    const int S = 2 * D + 2 * H;
    const size_t lds = 48 + (size_t)(2 * S + H) * sizeof(float);
    std::vector<int> tab;
    const int e = wave_launches(c, jobs, [&](size_t j0, size_t j1) -> int {
      tab.clear();
      for (size_t k = j0; k < j1; ++k) {
        const RtJob& j = jobs[k];
        for (long v : {(long)j.walk, j.in_off, j.s_lo, j.s_hi - j.s_lo, j.a, j.a1, j.out_off, j.lb, j.f_off, 0L, 0L, 0L, 0L, 0L, 0L, 0L})
          tab.push_back((int)v);
        if (j.s_hi > j.s_lo)
          H2D(c->rs_in + j.in_off, wav + (long)j.row * wav_stride + j.s_lo, (size_t)(j.s_hi - j.s_lo) * sizeof(float));
      }
      H2D(c->rs_meta, tab.data(), tab.size() * sizeof(int));
      const dim3 grid((unsigned)(j1 - j0));
      if (S <= 8 * 256)
        hipLaunchKernelGGL(retime_rows_kernel<8>, grid, dim3(256), lds, c->stream, c->rs_in, c->rs_meta, c->rt_fade, c->rs_out, c->rt_pos,
                           c->rt_cost, H, D);
      else
        hipLaunchKernelGGL(retime_rows_kernel<24>, grid, dim3(256), lds, c->stream, c->rs_in, c->rs_meta, c->rt_fade, c->rs_out, c->rt_pos,
                           c->rt_cost, H, D);
      for (size_t k = j0; k < j1; ++k) {
        const RtJob& j = jobs[k];
        D2H(out + (long)j.row * out_stride + j.b, c->rs_out + j.out_off, (size_t)j.lb * sizeof(float));
        if (!j.walk) continue;
        const long nf = rt_frames(j.lb, H);
        if (pos) D2H(pos + (long)j.row * pos_stride + j.f_row, c->rt_pos + j.f_off, (size_t)nf * sizeof(int));
        if (cost) D2H(cost + (long)j.row * pos_stride + j.f_row, c->rt_cost + j.f_off, (size_t)nf * sizeof(double));
      }
      return VX_OK;
    });
    if (e) return e;
  }
  for (int i = 0; i < batch; ++i) out_lens[i] = olen[(size_t)i];
  return VX_OK;
}

int vx_dev_retime_window(vx_ctx* c, int32_t input_samples) {
  return vxe::wave_set_window(c, &vx_ctx::rt_window, "vx_dev_retime_window", "input_samples", input_samples, VX_DEV_RETIME_WINDOW_MIN,
                              VX_RETIME_WINDOW);
}

}  // extern "C"
