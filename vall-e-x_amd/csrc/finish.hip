// The output stage of the waveform end (vx_finish, include/vallex_hip.h): trim, level, fade and 16-bit PCM of mono fp32 rows.
//
// Two passes over a ragged batch, both on the launch buffers the resampler allocates (rs_buffers: a context is single-threaded):
//
//   measure  wave_frames_kernel: frame f of a row = samples [f F, min((f + 1) F, L)) -> one record {double e, float p, int z}:
//            e = ONE lane's sum of (double)y * (double)y in sample order from 0.0 (y = the sample, 0 if it is not finite), p = max |y|,
//            z = the frame's non-finite samples.  The host reduces the table of a row (finish_host.h: fn_reduce) to its span, peak,
//            mean square and gain -- in double, in frame order.
//   apply    wave_apply_kernel<S16>: v = y * gain, v *= tab_in[i], v *= tab_out[n - 1 - i] (three separately rounded fp32 multiplies,
//            the two fade tables built on the host), stored as fp32 or as rintf(v * 32768) clamped to int16.
//
// Arithmetic (the contract the tests rest on): a frame is summed by one lane in sample order, an output element is a function of its
// own sample, the row's gain and its index in the row's output.  The bits therefore do not depend on the tile, the window, the row
// or the launch an element lands in.  The only atomics are integer adds of the clip counts.  No inline assembly.
//
// Work decomposition: a launch covers a ragged list of JOBS (a run of samples of one row: a whole row, or one window of a long one),
// grid (tile, job).  A measure tile stages `fpt` whole frames into LDS with coalesced loads at a frame stride of F | 1 floats -- odd,
// so the lanes of a 32-lane LDS group, which read consecutive FRAMES at the same offset, fall on 32 different banks -- and lane t then
// walks frame t.  An apply tile is FN_TILE consecutive elements, lane-contiguous loads and stores.
//
// The three entries of the output stage -- vx_finish here, vx_finish_loud (loudness.hip), vx_finish_limited (limit.hip) -- check their
// pointers and run ONE pipeline, fn_pipeline below: frames -> spans -> [steps -> gain] -> [limiter] -> apply -> infos.
#include "wave_stage.h"
#include "loudness_host.h"
#include "limit_host.h"

#include "../../include/vallex_hip_dev.h"

namespace vxe {

constexpr int FN_LDS = 8192;               // floats of staged frames per workgroup (32 KiB)
constexpr int FN_TILE = 2048;              // elements of an apply tile
constexpr int FN_FADE_CAP = FN_FADE_MAX;   // floats of one device fade table
static_assert(VX_FINISH_WINDOW == RS_IN_CAP, "vx_finish runs in the resampler's launch buffers");
static_assert((FN_FRAME_MAX | 1) <= FN_LDS, "one frame fits the staged span");
static_assert(VX_DEV_FINISH_WINDOW_MIN >= FN_FRAME_MIN && VX_DEV_FINISH_WINDOW_MIN <= VX_FINISH_WINDOW, "window bounds of the dev header");
// the frame table of a launch (at most one record per FN_FRAME_MIN samples plus a cut one per job) and its outputs both fit rs_out
static_assert((RS_IN_CAP / FN_FRAME_MIN + RS_MAX_JOBS) * sizeof(FnFrame) <= RS_OUT_CAP * sizeof(float), "frame table inside rs_out");

// tab [njobs][RS_TAB], measure pass: {in_off, cnt, f_off}: the job's samples in[in_off .. in_off + cnt) are the frames
// ft[f_off .. f_off + ceil(cnt / F)) (the job starts at a frame boundary of its row).  fpt * stride <= FN_LDS.
__global__ __launch_bounds__(256) void wave_frames_kernel(const float* __restrict__ in, const int* __restrict__ tab,
                                                          FnFrame* __restrict__ ft, int F, int stride, int fpt) {
  __shared__ float xs[FN_LDS];
  const int* tb = tab + blockIdx.y * RS_TAB;
  const long in_off = tb[0], f_off = tb[2];
  const int cnt = tb[1], nf = (cnt + F - 1) / F, f0 = blockIdx.x * fpt;
  if (f0 >= nf) return;                                          // block-uniform
  const int fc = nf - f0 < fpt ? nf - f0 : fpt;                  // frames of this tile
  const int s0 = f0 * F, ns = cnt - s0 < fc * F ? cnt - s0 : fc * F;
  const int tid = threadIdx.x;
  for (int t = tid; t < ns; t += 256) {
    const int f = t / F;
    xs[f * stride + (t - f * F)] = in[in_off + s0 + t];
  }
  __syncthreads();
  if (tid >= fc) return;
  const int n = ns - tid * F < F ? ns - tid * F : F;
  const float* xp = xs + tid * stride;
  double e = 0.0;
  float p = 0.f;
  int z = 0;
#pragma unroll 4
  for (int j = 0; j < n; ++j) {
    const float x = xp[j];
    const bool fin = (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u;
    const float y = fin ? x : 0.f;
    z += fin ? 0 : 1;
    e += (double)y * (double)y;                                  // the product is exact in double: an fma gives the same bits
    p = fmaxf(p, fabsf(y));
  }
  FnFrame r;
  r.e = e; r.p = p; r.z = z;
  ft[f_off + f0 + tid] = r;
}

// tab [njobs][RS_TAB], apply pass: {in_off, out_off, count, i0, n, gain bits, clipped}: element e of the job is output sample i0 + e
// of a row of n output samples; the kernel ADDS the job's clipped samples to word 6 (the upload zeroes it).
template <bool S16>
__global__ __launch_bounds__(256) void wave_apply_kernel(const float* __restrict__ in, int* tab, const float* __restrict__ tab_in,
                                                         const float* __restrict__ tab_out, int fade_in, int fade_out, void* out) {
  __shared__ int clip_s;
  int* tb = tab + blockIdx.y * RS_TAB;
  const int count = tb[2], e0 = blockIdx.x * FN_TILE;
  if (e0 >= count) return;                                       // block-uniform
  const long in_off = tb[0], out_off = tb[1];
  const int i0 = tb[3], n = tb[4];
  const float g = __int_as_float(tb[5]);
  const int tid = threadIdx.x, e1 = count - e0 < FN_TILE ? count : e0 + FN_TILE;
  if (tid == 0) clip_s = 0;
  __syncthreads();
  int nclip = 0;
  for (int e = e0 + tid; e < e1; e += 256) {
    const float x = in[in_off + e];
    const float y = (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u ? x : 0.f;
    const int i = i0 + e, k = n - 1 - i;
    float v = y * g;
    if (i < fade_in) v *= tab_in[i];
    if (k < fade_out) v *= tab_out[k];
    if (S16) {
      float r = rintf(v * 32768.0f);
      if (r > 32767.f) { r = 32767.f; ++nclip; }
      if (r < -32768.f) { r = -32768.f; ++nclip; }
      static_cast<short*>(out)[out_off + e] = (short)(int)r;
    } else {
      nclip += fabsf(v) > 1.f ? 1 : 0;
      static_cast<float*>(out)[out_off + e] = v;
    }
  }
  if (nclip) atomicAdd(&clip_s, nclip);
  __syncthreads();
  if (tid == 0 && clip_s) atomicAdd(tb + 6, clip_s);
}

static long fn_win(const vx_ctx* c, int F) { return std::max<long>(wave_window(c->fn_window, VX_FINISH_WINDOW), F); }

// the measure pass (wave_stage.h)
int fn_measure(vx_ctx* c, const float* wav, int64_t wav_stride, const int32_t* lens, int batch, int F, std::vector<FnFrame>& table,
               std::vector<long>& f0, bool* resident, std::vector<long>& base) {
  std::vector<long> lo(batch, 0), hi(batch);
  f0.assign(batch + 1, 0);
  base.assign(batch, 0);
  for (int i = 0; i < batch; ++i) {
    hi[i] = lens[i];
    f0[i + 1] = f0[i] + fn_nframes(lens[i], F);
  }
  table.resize((size_t)f0[batch]);
  std::vector<FnJob> jobs;
  if (!fn_plan(lo.data(), hi.data(), batch, fn_win(c, F), RS_MAX_JOBS, F, &jobs)) FAIL(VX_EINVAL, "vx_finish: no frame fits an empty launch");   // win >= F rules it out
  *resident = jobs.empty() || jobs.back().launch == 0;
  const int stride = F | 1, fpt = std::max(1, std::min(256, FN_LDS / stride));
  FnFrame* ft = reinterpret_cast<FnFrame*>(c->rs_out);
  std::vector<int> tab;
  return wave_launches(c, jobs, [&](size_t j0, size_t j1) -> int {
    tab.clear();
    long max_f = 0;
    for (size_t k = j0; k < j1; ++k) {
      const FnJob& j = jobs[k];
      for (long v : {j.off, j.cnt, j.f_off, 0L, 0L, 0L, 0L, 0L}) tab.push_back((int)v);
      max_f = std::max(max_f, fn_nframes(j.cnt, F));
      if (j.s_lo == 0) base[j.row] = j.off;
      H2D(c->rs_in + j.off, wav + (long)j.row * wav_stride + j.s_lo, (size_t)j.cnt * sizeof(float));
    }
    H2D(c->rs_meta, tab.data(), tab.size() * sizeof(int));
    const dim3 grid((unsigned)((max_f + fpt - 1) / fpt), (unsigned)(j1 - j0));
    hipLaunchKernelGGL(wave_frames_kernel, grid, dim3(256), 0, c->stream, c->rs_in, c->rs_meta, ft, F, stride, fpt);
    for (size_t k = j0; k < j1; ++k) {
      const FnJob& j = jobs[k];
      D2H(table.data() + f0[j.row] + j.s_lo / F, ft + j.f_off, (size_t)fn_nframes(j.cnt, F) * sizeof(FnFrame));
    }
    return VX_OK;
  });
}

// the two device fade tables, rebuilt when a length changes
static int fn_fades(vx_ctx* c, int fade_in, int fade_out) {
  if (!fade_in && !fade_out) return VX_OK;
  if (!c->fn_fade)
    if (int e = dev_alloc(c, &c->fn_fade, (size_t)2 * FN_FADE_CAP, false)) return e;
  const int want[2] = {fade_in, fade_out};
  std::vector<float> t;
  for (int k = 0; k < 2; ++k) {
    if (!want[k] || c->fn_fade_n[k] == want[k]) continue;
    fn_fade_table(want[k], t);
    H2D(c->fn_fade + (size_t)k * FN_FADE_CAP, t.data(), t.size() * sizeof(float));
    c->fn_fade_n[k] = want[k];
  }
  return VX_OK;
}

// the apply pass (wave_stage.h)
int fn_apply(vx_ctx* c, const float* wav, int64_t wav_stride, int batch, const vx_finish_opts& o, bool resident, const std::vector<long>& base,
             void* out, int64_t out_stride, vx_wave_info* info, const float* src) {
  if (int e = fn_fades(c, o.fade_in, o.fade_out)) return e;
  const float* in = resident && src ? src : c->rs_in;
  const bool s16 = o.format == VX_PCM_S16;
  const size_t es = s16 ? sizeof(short) : sizeof(float);
  std::vector<long> lo(batch), hi(batch);
  for (int i = 0; i < batch; ++i) { lo[i] = info[i].begin; hi[i] = info[i].end; }
  std::vector<FnJob> jobs;
  if (!fn_plan(lo.data(), hi.data(), batch, fn_win(c, 1), RS_MAX_JOBS, 0, &jobs)) FAIL(VX_EINVAL, "vx_finish: no sample fits an empty launch");
  const float* tab_in = c->fn_fade;
  const float* tab_out = c->fn_fade ? c->fn_fade + FN_FADE_CAP : nullptr;
  std::vector<int> tab, back;
  return wave_launches(c, jobs, [&](size_t j0, size_t j1) -> int {
    tab.clear();
    long max_cnt = 0;
    for (size_t k = j0; k < j1; ++k) {
      const FnJob& j = jobs[k];
      const vx_wave_info& w = info[j.row];
      int gbits;
      memcpy(&gbits, &w.gain, sizeof gbits);
      const long in_off = resident ? base[j.row] + j.s_lo : j.off;
      for (long v : {in_off, j.off, j.cnt, j.s_lo - (long)w.begin, (long)w.end - (long)w.begin, (long)gbits, 0L, 0L}) tab.push_back((int)v);
      max_cnt = std::max(max_cnt, j.cnt);
      if (!resident) H2D(c->rs_in + j.off, wav + (long)j.row * wav_stride + j.s_lo, (size_t)j.cnt * sizeof(float));
    }
    H2D(c->rs_meta, tab.data(), tab.size() * sizeof(int));
    const dim3 grid((unsigned)((max_cnt + FN_TILE - 1) / FN_TILE), (unsigned)(j1 - j0));
    if (s16)
      hipLaunchKernelGGL(wave_apply_kernel<true>, grid, dim3(256), 0, c->stream, in, c->rs_meta, tab_in, tab_out, o.fade_in, o.fade_out,
                         (void*)c->rs_out);
    else
      hipLaunchKernelGGL(wave_apply_kernel<false>, grid, dim3(256), 0, c->stream, in, c->rs_meta, tab_in, tab_out, o.fade_in, o.fade_out,
                         (void*)c->rs_out);
    for (size_t k = j0; k < j1; ++k) {
      const FnJob& j = jobs[k];
      D2H(static_cast<char*>(out) + ((long)j.row * out_stride + (j.s_lo - info[j.row].begin)) * es,
          reinterpret_cast<const char*>(c->rs_out) + j.off * es, (size_t)j.cnt * es);
    }
    back.resize(tab.size());
    D2H(back.data(), c->rs_meta, back.size() * sizeof(int));
    return VX_OK;
  }, [&](size_t j0, size_t j1) -> int {
    for (size_t k = j0; k < j1; ++k) info[jobs[k].row].clipped += back[(k - j0) * RS_TAB + 6];
    return VX_OK;
  });
}

// The limiter over every kept span [w.begin, w.end) as a row of its own at the gain w.gain, then -- with an output -- the apply pass at
// gain 1 over the limited samples (fades and format); w.clipped is that pass's.  Resident rows stay on the device in between: the
// limited samples lie in the upper half of rs_out.  Without an output the detector alone runs.
static int fn_limited(vx_ctx* c, const char* who, const float* wav, int64_t wav_stride, int batch, const vx_finish_opts& o, float ceiling_db,
                      const vx_limit_opts& lim, bool resident, const std::vector<long>& base, void* out, int64_t out_stride,
                      std::vector<vx_wave_info>& w, vx_limit_info* lw) {
  const size_t n = (size_t)batch;
  if (c->lm_window) resident = false;
  std::vector<long> kept, len(n), sbase(n, 0);
  std::vector<float> gs(n);
  std::vector<const float*> src(n);
  std::vector<float*> dst(n, nullptr);
  long stride = 1;
  for (size_t i = 0; i < n; ++i) stride = std::max<long>(stride, w[i].end - w[i].begin);
  std::vector<float> limited;                                      // the limited spans on the host when the call does not fit one launch
  if (out && !resident) limited.resize(n * (size_t)stride);
  for (size_t i = 0; i < n; ++i) {
    src[i] = wav + (long)i * wav_stride + w[i].begin;
    if (!limited.empty()) dst[i] = limited.data() + i * (size_t)stride;
    len[i] = w[i].end - w[i].begin;
    gs[i] = w[i].gain;
    if (resident) sbase[i] = base[i] + w[i].begin;
  }
  if (int e = lm_run(c, who, src.data(), len.data(), batch, gs.data(), lm_ceiling(ceiling_db), lim.lookahead, lim.oversample, resident, sbase,
                     out && !resident ? dst.data() : nullptr, nullptr, nullptr, out && resident, &kept, lw))
    return e;
  if (!out) return VX_OK;
  std::vector<vx_wave_info> a(w);
  for (size_t i = 0; i < n; ++i) a[i].gain = 1.f;
  if (resident) {
    for (size_t i = 0; i < n; ++i) kept[i] -= w[i].begin;          // row i's limited sample `begin` lies at rs_out + kept[i]
    if (int e = fn_apply(c, wav, wav_stride, batch, o, true, kept, out, out_stride, a.data(), c->rs_out)) return e;
  } else {
    for (size_t i = 0; i < n; ++i) { a[i].end -= a[i].begin; a[i].begin = 0; }
    if (int e = fn_apply(c, limited.data(), stride, batch, o, false, kept, out, out_stride, a.data(), nullptr)) return e;
  }
  for (size_t i = 0; i < n; ++i) w[i].clipped = a[i].clipped;
  return VX_OK;
}

// The output stage behind the entries' pointer checks (wave_stage.h).  What the three entries differ in is decided by lo and lim alone:
//   checks      vx_finish names a struct of the wrong size without its own name in front and checks its rows behind its options (the
//               two others have checked theirs in front of their pointers); a loudness target refuses a level_mode
//   allocation  rs_buffers; with lo the step tables (ln_buffers), with lim the limiter's (lm_buffers)
//   gain        fn_reduce's level; with lo ln_gain under the sample peak; with lim lm_gain, the limiter, and the apply pass at gain 1
//   residency   rows that went through ONE frames launch stay in rs_in for the later passes, unless a pass has a development window set
int fn_pipeline(vx_ctx* c, const char* who, const float* wav, int64_t wav_stride, const int32_t* lens, int batch, const vx_finish_opts& o,
                const vx_loudness_opts* lo, const vx_limit_opts* lim, void* out, int64_t out_stride, int32_t* out_lens, vx_wave_info* info,
                vx_loudness_info* linfo, vx_limit_info* liminfo) {
  if (!lo) CHECK_STRUCT(o, vx_finish_opts);
  else {
    CHECK_STRUCT_OF(who, o, vx_finish_opts);
    CHECK_STRUCT_OF(who, *lo, vx_loudness_opts);
  }
  char why[160];
  if (fn_check_opts(o, why, sizeof why)) FAIL(VX_EINVAL, "%s: %s", who, why);
  if (lo) {
    if (o.level_mode != VX_LEVEL_NONE) FAIL(VX_EINVAL, "%s: level_mode %d is not VX_LEVEL_NONE: the loudness target sets the level", who, o.level_mode);
    if (ln_check_opts(*lo, why, sizeof why)) FAIL(VX_EINVAL, "%s: %s", who, why);
  }
  if (lim)
    if (int e = lm_check(c, who, lim, 1.f, lo->ceiling_db)) return e;
  if (!lo)
    if (int e = wave_check_rows(c, who, wav, wav_stride, lens, batch)) return e;
  if (out)
    if (int e = wave_check_out_stride(c, who, lens, batch, out_stride, " (its untrimmed length)")) return e;
  const int S = lo ? ln_step(lo->sample_rate) : 0;
  if (lo && c->ln_window && c->ln_window < 3L * S)
    FAIL(VX_EINVAL, "%s: the launch window of %ld samples (vx_dev_loudness_window) is below 3 S = %d at sample_rate %d", who, c->ln_window, 3 * S,
         lo->sample_rate);
  HIPCHK(hipSetDevice(c->dev));
  if (int e = lo ? ln_buffers(c) : rs_buffers(c)) return e;
  if (lim)
    if (int e = lm_buffers(c, lim->oversample)) return e;
  const size_t n = (size_t)batch;
  // frames pass -> span, peak and the level gain
  std::vector<FnFrame> table;
  std::vector<long> f0, base;
  bool resident = false;
  if (int e = fn_measure(c, wav, wav_stride, lens, batch, o.frame, table, f0, &resident, base)) return e;
  const double thr2 = fn_thr2(o.silence_db);
  std::vector<vx_wave_info> w(n);
  for (size_t i = 0; i < n; ++i) fn_reduce(table.data() + f0[i], lens[i], o, thr2, &w[i]);
  std::vector<vx_loudness_info> li(lo ? n : 0);
  std::vector<vx_limit_info> lw(lim ? n : 0);
  if (lo) {
    // steps pass over the kept spans -> gain; the limiter takes the ceiling's place in it
    std::vector<long> b(n), e(n), z0;
    for (size_t i = 0; i < n; ++i) { b[i] = w[i].begin; e[i] = w[i].end; }
    if (c->ln_window) resident = false;
    std::vector<double> z;
    std::vector<int> nonf;
    if (int err = ln_steps(c, who, wav, wav_stride, b.data(), e.data(), batch, lo->sample_rate, resident, base, z, z0, nonf)) return err;
    for (size_t i = 0; i < n; ++i) {
      ln_reduce(z.data() + z0[i], e[i] - b[i], S, nonf[i], &li[i]);
      w[i].gain = lim ? lm_gain(li[i].loudness, lo->target_lufs, o.max_gain_db)
                      : ln_gain(li[i].loudness, lo->target_lufs, lo->ceiling_db, o.max_gain_db, w[i].peak);
    }
  }
  if (lim) {
    if (int e = fn_limited(c, who, wav, wav_stride, batch, o, lo->ceiling_db, *lim, resident, base, out, out_stride, w, lw.data())) return e;
  } else if (out) {
    if (int e = fn_apply(c, wav, wav_stride, batch, o, resident, base, out, out_stride, w.data(), nullptr)) return e;
  }
  for (size_t i = 0; i < n; ++i) {
    info[i] = w[i];
    if (lo) linfo[i] = li[i];
    if (lim) liminfo[i] = lw[i];
    if (out_lens) out_lens[i] = w[i].end - w[i].begin;
  }
  return VX_OK;
}

}  // namespace vxe

extern "C" {

int vx_finish(vx_ctx* c, const float* wav, int64_t wav_stride, const int32_t* lens, int32_t batch, const vx_finish_opts* o, void* out,
              int64_t out_stride, int32_t* out_lens, vx_wave_info* info) {
  using namespace vxe;
  if (!c) return VX_EINVAL;
  if (!wav) FAIL(VX_EINVAL, "vx_finish: wav is NULL");
  if (!lens) FAIL(VX_EINVAL, "vx_finish: lens is NULL");
  if (!o) FAIL(VX_EINVAL, "vx_finish: o is NULL");
  if (!info) FAIL(VX_EINVAL, "vx_finish: info is NULL");
  if (out && !out_lens) FAIL(VX_EINVAL, "vx_finish: out is given without out_lens");
  if (batch <= 0) FAIL(VX_EINVAL, "vx_finish: batch %d below 1", batch);
  return fn_pipeline(c, "vx_finish", wav, wav_stride, lens, batch, *o, nullptr, nullptr, out, out_stride, out_lens, info, nullptr, nullptr);
}

int vx_dev_finish_frames(vx_ctx* c, const float* wav, int32_t len, int32_t frame, double* e, float* p, int32_t* z) {
  using namespace vxe;
  if (!c) return VX_EINVAL;
  if (!wav) FAIL(VX_EINVAL, "vx_dev_finish_frames: wav is NULL");
  if (!e || !p || !z) FAIL(VX_EINVAL, "vx_dev_finish_frames: e, p or z is NULL");
  if (len < 0) FAIL(VX_EINVAL, "vx_dev_finish_frames: len %d below 0", len);
  if (frame < FN_FRAME_MIN || frame > FN_FRAME_MAX) FAIL(VX_EINVAL, "vx_dev_finish_frames: frame %d outside %d .. %d", frame, FN_FRAME_MIN, FN_FRAME_MAX);
  HIPCHK(hipSetDevice(c->dev));
  if (int err = rs_buffers(c)) return err;
  std::vector<FnFrame> table;
  std::vector<long> f0, base;
  bool resident = false;
  if (int err = fn_measure(c, wav, len, &len, 1, frame, table, f0, &resident, base)) return err;
  for (size_t f = 0; f < table.size(); ++f) { e[f] = table[f].e; p[f] = table[f].p; z[f] = table[f].z; }
  return VX_OK;
}

int vx_dev_finish_window(vx_ctx* c, int32_t input_samples) {
  return vxe::wave_set_window(c, &vx_ctx::fn_window, "vx_dev_finish_window", "input_samples", input_samples, VX_DEV_FINISH_WINDOW_MIN,
                              VX_FINISH_WINDOW);
}

}  // extern "C"
