// What the waveform translation units share (resample.hip, finish.hip, stretch.hip, loudness.hip, limit.hip, f0.hip, psola.hip,
// denoise.hip, retime.hip): the launch buffers, the checks of a ragged batch of rows, the development windows, the launch-group driver, and the
// passes of the output stage that vx_finish, vx_finish_loud and vx_finish_limited run in turn.  Not part of the public C ABI.
#pragma once

#include "engine_ctx.h"
#include "finish_host.h"

namespace vxe {

// resample.hip: the launch buffers of the waveform entries, allocated by the first call that needs them and shared by all of them (a
// context is single-threaded): rs_in RS_IN_CAP floats, rs_out RS_OUT_CAP floats, rs_meta RS_MAX_JOBS records of RS_TAB ints
constexpr int RS_TAB = 8;                  // ints of a job record
constexpr int RS_MAX_JOBS = 4096;          // jobs per launch (grid.y)
constexpr long RS_IN_CAP = VX_RESAMPLE_WINDOW;          // input samples per launch, default
constexpr long RS_OUT_CAP = 2 * RS_IN_CAP;              // output samples per launch
int rs_buffers(vx_ctx* c);
// stretch.hip: the tables of a WSOLA walk (vx_stretch, vx_retime: ws_walk.h), shared like the launch buffers: st_fade, the crossfade
// table of hop H, rebuilt when the hop changes, and st_pos / st_cost, the positions and winning costs of one launch's frames
constexpr long ST_FRAME_CAP = 1L << 18;    // frames per launch
int ws_tables(vx_ctx* c, int H);

// resample.hip: wav, lens and batch of an entry (NULL, batch below 1), then every lens[i] against 0 .. wav_stride
int wave_check_rows(vx_ctx* c, const char* who, const float* wav, int64_t wav_stride, const int32_t* lens, int batch);
// ... and every lens[i] against out_stride; note: what the entry says behind "row %d" ("" or " (its untrimmed length)")
int wave_check_out_stride(vx_ctx* c, const char* who, const int32_t* lens, int batch, int64_t out_stride, const char* note);

// the samples per launch of a stage: its development window when one is set, else its default
inline long wave_window(long field, long dflt) { return field ? field : dflt; }
// resample.hip: the body of every vx_dev_*_window entry: 0 or lo .. hi into the stage's field; arg: the entry's name of the argument
int wave_set_window(vx_ctx* c, long vx_ctx::*field, const char* who, const char* arg, int32_t samples, long lo, long hi);

// CHECK_STRUCT with the entry's name in front
#define CHECK_STRUCT_OF(who, v, T)                                                                                                    \
  do {                                                                                                                                \
    if ((v).struct_size != sizeof(T))                                                                                                 \
      FAIL(VX_EINVAL, "%s: " #T ".struct_size is %u, this library expects %zu (ABI version %d)", who, (v).struct_size, sizeof(T), VX_ABI_VERSION); \
  } while (0)

// One launch per group of jobs.  A plan (the *_plan of a *_host.h) orders its jobs by their .launch; stage(j0, j1) packs the table of
// the jobs [j0, j1) of one launch, uploads, launches and queues what comes back; the driver syncs the stream behind it and checks the
// launch; done(j0, j1) then reads what came back.  The first error ends the walk.
template <typename Job, typename Stage, typename Done>
int wave_launches(vx_ctx* c, const std::vector<Job>& jobs, Stage stage, Done done) {
  for (size_t j0 = 0, j1; j0 < jobs.size(); j0 = j1) {
    for (j1 = j0 + 1; j1 < jobs.size() && jobs[j1].launch == jobs[j0].launch;) ++j1;
    if (int e = stage(j0, j1)) return e;
    SYNC();
    HIPCHK(hipGetLastError());
    if (int e = done(j0, j1)) return e;
  }
  return VX_OK;
}
template <typename Job, typename Stage>
int wave_launches(vx_ctx* c, const std::vector<Job>& jobs, Stage stage) {
  return wave_launches(c, jobs, stage, [](size_t, size_t) { return VX_OK; });
}

// ---- the passes of the output stage (finish.hip: fn_pipeline runs them in turn) ------------------------------------------------------
// finish.hip, the frames pass: the frame table of every row, row i at table[f0[i] ..).  resident: the whole batch went through ONE
// launch, and row i's samples still lie at rs_in + base[i]
int fn_measure(vx_ctx* c, const float* wav, int64_t wav_stride, const int32_t* lens, int batch, int F, std::vector<FnFrame>& table,
               std::vector<long>& f0, bool* resident, std::vector<long>& base);
// finish.hip, the apply pass.  src (with resident): the device buffer the rows lie in, row i's sample 0 at src + base[i]; nullptr: rs_in
int fn_apply(vx_ctx* c, const float* wav, int64_t wav_stride, int batch, const vx_finish_opts& o, bool resident, const std::vector<long>& base,
             void* out, int64_t out_stride, vx_wave_info* info, const float* src);
// loudness.hip: rs_buffers and the step tables; the steps pass over the spans [lo[i], hi[i]) of the rows
int ln_buffers(vx_ctx* c);
int ln_steps(vx_ctx* c, const char* who, const float* wav, int64_t wav_stride, const long* lo, const long* hi, int batch, int rate,
             bool resident, const std::vector<long>& base, std::vector<double>& z, std::vector<long>& z0, std::vector<int>& nonf);
// limit.hip: the check of the limiter's options, rs_buffers and the limiter's tables at oversampling n, the limiter over rows
int lm_check(vx_ctx* c, const char* who, const vx_limit_opts* o, float pre_gain, float ceiling_db);
int lm_buffers(vx_ctx* c, int n);
int lm_run(vx_ctx* c, const char* who, const float* const* src, const long* len, int batch, const float* gs, float cc, int Wn, int n, bool resident,
           const std::vector<long>& base, float* const* dst, float* const* dP, float* const* dG, bool keep, std::vector<long>* kept,
           vx_limit_info* info);
// finish.hip: the output stage behind the entries' pointer checks.  lo, lim NULL: vx_finish; lim NULL: vx_finish_loud; both:
// vx_finish_limited (linfo / liminfo with them)
int fn_pipeline(vx_ctx* c, const char* who, const float* wav, int64_t wav_stride, const int32_t* lens, int batch, const vx_finish_opts& o,
                const vx_loudness_opts* lo, const vx_limit_opts* lim, void* out, int64_t out_stride, int32_t* out_lens, vx_wave_info* info,
                vx_loudness_info* linfo, vx_limit_info* liminfo);

}  // namespace vxe
