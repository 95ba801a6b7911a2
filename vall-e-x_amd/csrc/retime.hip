// The time map (vx_pauses and vx_retime, include/vallex_hip.h): where the pauses of a row are, and a piecewise map from input to
// output time applied segment by segment -- copies where a segment keeps its length, WSOLA with both ends pinned where it does not.
//
// vx_pauses runs the frames pass of the output stage (fn_measure, wave_frames_kernel) and reduces every row's frame table on the host
// (retime_host.h: rt_pauses); it has no kernel of its own.
//
// vx_retime: a walked segment is the walk of ws_walk.h -- the frame, its arithmetic contract and its LDS are that header's -- with what
// the time map sets: frame 0 starts at the segment's anchor, the nominal positions follow the line to the end pin and come from the
// job record, and the search is clipped to the segment (the last frame to the one offset of the pin, behind which the segment goes on
// plainly to the anchor).
//
// Work decomposition: inside a walked segment frame k needs p_{k-1}, but a segment starts at a_i and ends at a_{i+1} whatever its
// neighbours find, so the segments of a row -- and of all rows -- are independent JOBS: grid (job), one 256-thread workgroup per job.
// A job is one walked segment, or a tile of a run of copy segments (the bits of the input, as 32-bit words).
#include "wave_stage.h"
#include "retime_host.h"
#include "ws_walk.h"

#include "../../include/vallex_hip_dev.h"

namespace vxe {

constexpr int RT_TAB = 16;                                   // ints of a job record
constexpr int RT_MAX_JOBS = RS_MAX_JOBS * RS_TAB / RT_TAB;   // the records of a launch fill rs_meta
static_assert(VX_RETIME_WINDOW == RS_IN_CAP, "vx_retime runs in the resampler's launch buffers");
static_assert(VX_DEV_RETIME_WINDOW_MIN >= 1 && VX_DEV_RETIME_WINDOW_MIN <= VX_RETIME_WINDOW, "window bounds of the dev header");

// tab [njobs][RT_TAB]:
//   0 walk     1: a walked segment, 0: a copy tile
//   1 in_off   first float of the job's staged samples in `in`
//   2 s_lo     row sample index of that float;  3 in_cnt  staged samples (a copy tile: the samples to copy)
//   4 a, 5 a1  the segment's input samples [a, a1) of the row
//   6 out_off  first float of the job's outputs in `out`;  7 lb  output samples of the job
//   8 f_off    first record of the job in `pos` / `cost`
template <int NPRE>
__global__ __launch_bounds__(256) void retime_rows_kernel(const float* __restrict__ in, const int* __restrict__ tab,
                                                          const float* __restrict__ w, float* __restrict__ out, int* __restrict__ pos,
                                                          double* __restrict__ cost, int H, int D) {
  extern __shared__ double rt_lds[];
  const WsLds l(rt_lds, H, D);
  const int* tb = tab + blockIdx.x * RT_TAB;
  const long in_off = tb[1], in_cnt = tb[3], a = tb[4], a1 = tb[5], out_off = tb[6], lb = tb[7], f_off = tb[8];
  const int tid = threadIdx.x;
  if (!tb[0]) {                                                  // a copy tile: the words of the input (block-uniform)
    const unsigned* src = reinterpret_cast<const unsigned*>(in + in_off);
    unsigned* dst = reinterpret_cast<unsigned*>(out + out_off);
    for (long i = tid; i < in_cnt && i < lb; i += 256) dst[i] = src[i];
    return;
  }
  const WsRow y_at{in + in_off, tb[2], in_cnt};
  const int M = (int)(lb / H), rem = (int)(lb - (long)M * H);
  if (M < 2) return;                                             // the checks rule it out; a wrong table divides by nothing
  const long slope = (a1 - a) - lb + (long)(M - 1) * H;          // n_k = a + floor(k slope / (M - 1))
  for (int j = tid; j < H; j += 256) out[out_off + j] = y_at(a + j);   // frame 0: p_0 = a, the input itself
  if (tid == 0) { pos[f_off] = (int)a; cost[f_off] = 0.0; }
  for (int j = tid; j < H; j += 256) l.t[j] = y_at(a + H + j);
  {
    const long base = a + slope / (M - 1) - D;
    for (int i = tid; i < l.S; i += 256) l.reg[i] = y_at(base + i);
  }
  for (int k = 1; k < M; ++k) {
    const long nk = a + (long)k * slope / (M - 1);
    const bool more = k + 1 < M;
    // the candidates cd = d + D of this frame: the search clipped to the segment; the pinned last frame has d = 0 alone
    int clo = D, chi = D;
    if (more) {
      const long dlo = a - nk > -(long)D ? a - nk : -(long)D, dhi = a1 - H - nk < (long)D ? a1 - H - nk : (long)D;
      clo = (int)dlo + D; chi = (int)dhi + D;
    }
    float* o = out + out_off + (long)k * H;
    const WsWin b = ws_frame<NPRE>(l, (k - 1) & 1, y_at, more, a + (long)(k + 1) * slope / (M - 1) - D, clo, chi, H, D, w, o, H);
    if (!more) {                                                 // the pinned frame goes on plainly to the anchor
      const float* cur = l.buf((k - 1) & 1) + b.d + D + H;       // untouched until the next barrier
      for (int j = tid; j < rem; j += 256) o[H + j] = cur[j];
    }
    if (tid == 0) { pos[f_off + k] = (int)(nk + b.d); cost[f_off + k] = b.D; }
  }
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
  if (!rt_plan(anchors, anchor_stride, n_anchors, lens, batch, H, D, win, RS_OUT_CAP, ST_FRAME_CAP, RT_MAX_JOBS, RT_TILE, &jobs, &bad_row, &bad_seg))
    FAIL(VX_EINVAL, "%s: row %d: segment %ld is walked and longer than a launch window of %ld input samples (vx_dev_retime_window), %ld output samples "
                    "or %ld frames", who, bad_row, bad_seg, win, RS_OUT_CAP, ST_FRAME_CAP);
  if (!jobs.empty()) {
    HIPCHK(hipSetDevice(c->dev));
    if (int e = rs_buffers(c)) return e;
    if (int e = ws_tables(c, H)) return e;
    const int S = 2 * D + 2 * H;
    const size_t lds = ws_lds_bytes(H, D);
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
      WS_LAUNCH(retime_rows_kernel, S, grid, dim3(256), lds, c->stream, c->rs_in, c->rs_meta, c->st_fade, c->rs_out, c->st_pos, c->st_cost, H, D);
      for (size_t k = j0; k < j1; ++k) {
        const RtJob& j = jobs[k];
        D2H(out + (long)j.row * out_stride + j.b, c->rs_out + j.out_off, (size_t)j.lb * sizeof(float));
        if (!j.walk) continue;
        const long nf = rt_frames(j.lb, H);
        if (pos) D2H(pos + (long)j.row * pos_stride + j.f_row, c->st_pos + j.f_off, (size_t)nf * sizeof(int));
        if (cost) D2H(cost + (long)j.row * pos_stride + j.f_row, c->st_cost + j.f_off, (size_t)nf * sizeof(double));
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
