// The speaking rate (vx_stretch, include/vallex_hip.h): a pitch-preserving time-stretch of mono fp32 rows by WSOLA.
//
// Frame k of a row writes the output hop [k H, (k + 1) H) from a segment at p_k = n_k + d*, searched over all of [n_k - D, n_k + D]
// around the nominal position n_k = floor(k H num / den); frame 0 is the input itself.  The frame, its arithmetic contract and its
// LDS are ws_walk.h's; the header states every rounding; stretch_host.h has the integers.
//
// Work decomposition: a launch covers a ragged list of JOBS (the frames [k0, k1) of one row: a whole row, or one window of a long
// one, which starts from the position the previous launch found for frame k0 - 1), grid (job): one 256-thread workgroup walks its
// job's frames in order, the rows of a batch run side by side on different CUs.
#include "wave_stage.h"
#include "stretch_host.h"
#include "ws_walk.h"

#include "../../include/vallex_hip_dev.h"

namespace vxe {

constexpr int ST_TAB = 16;                                   // ints of a job record
constexpr int ST_MAX_JOBS = RS_MAX_JOBS * RS_TAB / ST_TAB;   // the records of a launch fill rs_meta
static_assert(VX_STRETCH_WINDOW == RS_IN_CAP, "vx_stretch runs in the resampler's launch buffers");
static_assert(VX_DEV_STRETCH_WINDOW_MIN >= 2 * 300 + 3 * 441 && VX_DEV_STRETCH_WINDOW_MIN <= VX_STRETCH_WINDOW, "window bounds of the dev header");
static_assert(2 * ST_SEARCH_MAX + 3 * ST_HOP_MAX <= VX_STRETCH_WINDOW, "one frame fits the default window");

// tab [njobs][ST_TAB]:
//   0 in_off   first float of the job's staged samples in `in`
//   1 s_lo     row sample index of that float;  2 in_cnt  staged samples: the job's span cut to [0, L)
//   3 k0, 4 k1 frames of the job;  5 p_prev  p_{k0-1} (k0 >= 1)
//   6 out_off  first float of the job's outputs in `out` (output sample k0 H of the row);  7 Lout  output samples of the ROW
//   8 f_off    first record of the job in `pos` / `cost`
template <int NPRE>
__global__ __launch_bounds__(256) void stretch_rows_kernel(const float* __restrict__ in, const int* __restrict__ tab,
                                                           const float* __restrict__ w, float* __restrict__ out, int* __restrict__ pos,
                                                           double* __restrict__ cost, int H, int D, int num, int den) {
  extern __shared__ double st_lds[];
  const WsLds l(st_lds, H, D);
  const int* tb = tab + blockIdx.x * ST_TAB;
  const long out_off = tb[6], Lout = tb[7], f_off = tb[8];
  const int k0 = tb[3], k1 = tb[4], tid = threadIdx.x;
  const WsRow y_at{in + tb[0], tb[1], tb[2]};
  long p_prev = tb[5];
  int ks = k0;
  if (k0 == 0) {                                                 // frame 0: p_0 = 0, the input itself
    for (int j = tid; j < H && j < Lout; j += 256) out[out_off + j] = y_at(j);
    if (tid == 0) { pos[f_off] = 0; cost[f_off] = 0.0; }
    p_prev = 0;
    ks = 1;
  }
  if (ks >= k1) return;                                          // block-uniform
  for (int j = tid; j < H; j += 256) l.t[j] = y_at(p_prev + H + j);
  {
    const long base = (long)ks * H * num / den - D;
    for (int i = tid; i < l.S; i += 256) l.reg[i] = y_at(base + i);
  }
  for (int k = ks; k < k1; ++k) {
    const long nk = (long)k * H * num / den, o0 = (long)k * H;
    const long left = Lout - o0;                                 // the last frame of a row may end in front of its hop
    const WsWin b = ws_frame<NPRE>(l, (k - ks) & 1, y_at, k + 1 < k1, (long)(k + 1) * H * num / den - D, 0, 2 * D, H, D, w,
                                   out + out_off + (o0 - (long)k0 * H), left < H ? (int)left : H);
    if (tid == 0) { pos[f_off + (k - k0)] = (int)(nk + b.d); cost[f_off + (k - k0)] = b.D; }
  }
}

// the crossfade table, rebuilt when the hop changes, and the position / cost tables of a launch (wave_stage.h)
int ws_tables(vx_ctx* c, int H) {
  if (!c->st_fade) {
    if (int e = dev_alloc(c, &c->st_fade, (size_t)ST_HOP_MAX, false)) return e;
    if (int e = dev_alloc(c, &c->st_pos, (size_t)ST_FRAME_CAP, false)) return e;
    if (int e = dev_alloc(c, &c->st_cost, (size_t)ST_FRAME_CAP, false)) return e;
  }
  if (c->st_fade_n != H) {
    std::vector<float> t;
    fn_fade_table(H, t);
    H2D(c->st_fade, t.data(), t.size() * sizeof(float));
    c->st_fade_n = H;
  }
  return VX_OK;
}

// every check of vx_stretch behind the pointers: options, lengths, strides.  olen [batch] = Lout of every row.
static int st_check(vx_ctx* c, const char* who, const int32_t* lens, int batch, const vx_stretch_opts* o,
                    int64_t out_stride, bool has_pos, int64_t pos_stride, StGeom* g, std::vector<long>* olen) {
  CHECK_STRUCT(*o, vx_stretch_opts);
  char why[160];
  if (st_check_opts(*o, why, sizeof why)) FAIL(VX_EINVAL, "%s: %s", who, why);
  *g = st_geometry(*o);
  olen->resize((size_t)batch);
  for (int i = 0; i < batch; ++i) {
    const long L = lens[i];
    const long n = st_out_len(*g, L), M = st_frames(*g, L);
    if (n > 0x7fffffffL || (M > 0 && st_nominal(*g, M - 1) + g->D > 0x7fffffffL))
      FAIL(VX_EINVAL, "%s: lens[%d] = %ld gives %ld output samples or a position above what out_lens / pos hold", who, i, L, n);
    if (n > out_stride) FAIL(VX_EINVAL, "%s: out_stride %ld below the %ld output samples of row %d", who, (long)out_stride, n, i);
    if (has_pos && M > pos_stride) FAIL(VX_EINVAL, "%s: pos_stride %ld below the %ld frames of row %d", who, (long)pos_stride, M, i);
    (*olen)[(size_t)i] = n;
  }
  return VX_OK;
}

// the general path: plan, then one launch per group of jobs, everything of a launch behind one stream sync.  cost: one row only.
static int st_run(vx_ctx* c, const char* who, const float* wav, int64_t wav_stride, const int32_t* lens, int batch, const StGeom& g,
                  float* out, int64_t out_stride, int32_t* pos, int64_t pos_stride, double* cost) {
  const long win = wave_window(c->st_window, VX_STRETCH_WINDOW);
  std::vector<StJob> jobs;
  if (!st_plan(g, lens, batch, win, RS_OUT_CAP, ST_FRAME_CAP, ST_MAX_JOBS, &jobs))
    FAIL(VX_EINVAL, "%s: the window of %ld input samples (vx_dev_stretch_window) is below one frame's span at hop %d, search %d", who, win, g.H, g.D);
  if (jobs.empty()) return VX_OK;
  HIPCHK(hipSetDevice(c->dev));
  if (int e = rs_buffers(c)) return e;
  if (int e = ws_tables(c, g.H)) return e;
  const int S = 2 * g.D + 2 * g.H;
  const size_t lds = ws_lds_bytes(g.H, g.D);
  std::vector<long> p_last((size_t)batch, 0);                    // p of the last frame a launch has walked, per row
  std::vector<int> tab, last;
  return wave_launches(c, jobs, [&](size_t j0, size_t j1) -> int {
    tab.clear();
    last.assign(j1 - j0, 0);
    for (size_t k = j0; k < j1; ++k) {
      const StJob& j = jobs[k];
      for (long v : {j.in_off, j.s_lo, j.s_hi - j.s_lo, j.k0, j.k1, p_last[(size_t)j.row], j.out_off, st_out_len(g, lens[j.row]), j.f_off,
                     0L, 0L, 0L, 0L, 0L, 0L, 0L})
        tab.push_back((int)v);
      if (j.s_hi > j.s_lo)
        H2D(c->rs_in + j.in_off, wav + (long)j.row * wav_stride + j.s_lo, (size_t)(j.s_hi - j.s_lo) * sizeof(float));
    }
    H2D(c->rs_meta, tab.data(), tab.size() * sizeof(int));
    const dim3 grid((unsigned)(j1 - j0));
    WS_LAUNCH(stretch_rows_kernel, S, grid, dim3(256), lds, c->stream, c->rs_in, c->rs_meta, c->st_fade, c->rs_out, c->st_pos, c->st_cost,
              g.H, g.D, (int)g.num, (int)g.den);
    for (size_t k = j0; k < j1; ++k) {
      const StJob& j = jobs[k];
      const long nf = j.k1 - j.k0;
      if (j.out_cnt > 0) D2H(out + (long)j.row * out_stride + j.k0 * g.H, c->rs_out + j.out_off, (size_t)j.out_cnt * sizeof(float));
      if (pos) D2H(pos + (long)j.row * pos_stride + j.k0, c->st_pos + j.f_off, (size_t)nf * sizeof(int));
      if (cost) D2H(cost + j.k0, c->st_cost + j.f_off, (size_t)nf * sizeof(double));
      D2H(&last[k - j0], c->st_pos + j.f_off + nf - 1, sizeof(int));
    }
    return VX_OK;
  }, [&](size_t j0, size_t j1) -> int {
    for (size_t k = j0; k < j1; ++k) p_last[(size_t)jobs[k].row] = last[k - j0];
    return VX_OK;
  });
}

}  // namespace vxe

extern "C" {

int vx_stretch(vx_ctx* c, const float* wav, int64_t wav_stride, const int32_t* lens, int32_t batch, const vx_stretch_opts* o, float* out,
               int64_t out_stride, int32_t* out_lens, int32_t* pos, int64_t pos_stride) {
  using namespace vxe;
  if (!c) return VX_EINVAL;
  if (int e = wave_check_rows(c, "vx_stretch", wav, wav_stride, lens, batch)) return e;
  if (!o) FAIL(VX_EINVAL, "vx_stretch: o is NULL");
  if (!out) FAIL(VX_EINVAL, "vx_stretch: out is NULL");
  if (!out_lens) FAIL(VX_EINVAL, "vx_stretch: out_lens is NULL");
  StGeom g;
  std::vector<long> olen;
  if (int e = st_check(c, "vx_stretch", lens, batch, o, out_stride, pos != nullptr, pos_stride, &g, &olen)) return e;
  if (g.num == g.den) {                                          // nothing to stretch: the input bits
    for (int i = 0; i < batch; ++i) {
      if (olen[(size_t)i]) memmove(out + (long)i * out_stride, wav + (long)i * wav_stride, (size_t)olen[(size_t)i] * sizeof(float));
      if (pos)
        for (long k = 0, M = st_frames(g, lens[i]); k < M; ++k) pos[(long)i * pos_stride + k] = (int32_t)(k * g.H);
      out_lens[i] = (int32_t)olen[(size_t)i];
    }
    return VX_OK;
  }
  if (int e = st_run(c, "vx_stretch", wav, wav_stride, lens, batch, g, out, out_stride, pos, pos_stride, nullptr)) return e;
  for (int i = 0; i < batch; ++i) out_lens[i] = (int32_t)olen[(size_t)i];
  return VX_OK;
}

int vx_dev_stretch_costs(vx_ctx* c, const float* wav, int32_t len, const vx_stretch_opts* o, float* out, int32_t* pos, double* cost) {
  using namespace vxe;
  if (!c) return VX_EINVAL;
  if (!wav) FAIL(VX_EINVAL, "vx_dev_stretch_costs: wav is NULL");
  if (!o) FAIL(VX_EINVAL, "vx_dev_stretch_costs: o is NULL");
  if (!out || !pos || !cost) FAIL(VX_EINVAL, "vx_dev_stretch_costs: out, pos or cost is NULL");
  if (len < 0) FAIL(VX_EINVAL, "vx_dev_stretch_costs: len %d below 0", len);
  StGeom g;
  std::vector<long> olen;
  const int64_t big = 0x7fffffffL;
  if (int e = st_check(c, "vx_dev_stretch_costs", &len, 1, o, big, true, big, &g, &olen)) return e;
  return st_run(c, "vx_dev_stretch_costs", wav, len, &len, 1, g, out, big, pos, big, cost);
}

int vx_dev_stretch_window(vx_ctx* c, int32_t input_samples) {
  return vxe::wave_set_window(c, &vx_ctx::st_window, "vx_dev_stretch_window", "input_samples", input_samples, VX_DEV_STRETCH_WINDOW_MIN,
                              VX_STRETCH_WINDOW);
}

}  // extern "C"
