// The spectral noise suppression (vx_denoise, include/vallex_hip.h): short-time Fourier analysis of mono fp32 rows (frame 512, hop 128,
// square-root Hann on both sides), a noise profile from the quietest full frames, a floored subtraction gain on a five-frame power
// average, overlap-add.
//
// Three kernels with plain host code between them.  denoise_power_kernel transforms one frame per workgroup and writes its power
// P[t][0 .. 256] and its energy E[t].  The host (denoise_host.h: dn_select) chooses the K quietest full frames of every row.
// denoise_profile_kernel averages their power, one lane per bin in ascending t.  denoise_synth_kernel writes one hop of 128 outputs per
// workgroup: it transforms the four frames that cover the hop AGAIN (the same function on the same words gives the same bits, so no
// spectrum is kept: 8 KB per frame, 270 MB for a full window, against 4x the forward transforms), forms the gain from the stored P,
// runs the inverse network and adds the four windowed frames in ascending t.  The contract -- the order of every addition inside the
// network, the gain, every rounding -- is in the header; denoise_host.h has a sequential reference.
//
// Arithmetic (the contract the tests rest on): IEEE double, contraction off for the whole file, no atomics, no inline assembly.  Every
// word is produced by one lane from words that do not depend on the launch, so the bits depend neither on the batch, the window nor
// the workgroup a frame lands in.
//
// The network in LDS.  256 lanes, one butterfly each per stage, nine stages, one barrier between stages (a lane touches only its own
// i0 and i1 within a stage).  LDS banking (ds_read_b64: the two 32-lane halves of a wave, bank = dword address mod 64, i.e. 32 banks of
// doubles; ds_write_b64: groups of 16 lanes, 16 banks of doubles): in a stage with h < 32 the i0 of 32 consecutive lanes are the 32
// indices of a 64-block whose bit log2(h) is clear -- laid out linearly, lanes l and l + 16 meet on a bank in every such stage (2-way).
// The arrays are therefore stored at dn_phys(i) = i ^ (15 if bit 4 of i) ^ (16 if bit 5 of i): two indices of a 64-block then share a
// read bank only if they differ in ALL of bits 0 .. 4, and two of a 32-block a write bank only if they differ in all of bits 0 .. 3, and
// no stage puts such a pair into one group; runs of 16 / 32 consecutive indices (h >= 16 / 32) stay a permutation of the banks.  The
// twiddles are kept in the order the stages read them (tc[h + p] = c[p 256 / h]): consecutive p read consecutive words, equal p
// broadcast -- the table c[q] itself would be read at a stride of 256 / h doubles (8-way at h = 32).
// LDS: 4 x 4 KiB (re, im, the two twiddle tables) + 2 KiB (gains or powers) = 18.1 KiB a workgroup: 8 workgroups fit a CU's 160 KiB
// and fill its 32 wave slots.
#include "wave_stage.h"
#include "denoise_host.h"

#include "../../include/vallex_hip_dev.h"

#pragma clang fp contract(off)

namespace vxe {

constexpr int DN_TAB = 8;                                            // ints of a job record
constexpr long DN_FCAP = VX_DENOISE_WINDOW / DN_H + 3L * DN_MAX_JOBS; // frames of a launch, at most (denoise_host.h: dn_frame_cap)
// dn_buf, in doubles: the window, the stage twiddles, E, the profiles of a launch's rows, the chosen frames (ints), P
constexpr long DN_W_AT = 0, DN_TC_AT = DN_N, DN_TS_AT = 2 * DN_N, DN_E_AT = 3 * DN_N;
constexpr long DN_NZ_AT = DN_E_AT + DN_FCAP, DN_SEL_AT = DN_NZ_AT + (long)DN_MAX_JOBS * DN_B;
constexpr long DN_P_AT = DN_SEL_AT + (DN_FCAP + 1) / 2, DN_BUF = DN_P_AT + DN_FCAP * DN_B;
// the gains of vx_dev_denoise_table: doubles in rs_out behind the output samples
constexpr long DN_GAIN_AT = VX_DENOISE_WINDOW, DN_GAIN_CAP = (RS_OUT_CAP - DN_GAIN_AT) / 2;
static_assert(VX_DENOISE_WINDOW <= RS_IN_CAP && DN_GAIN_AT % 2 == 0, "vx_denoise stages its samples in the resampler's launch buffers");
static_assert(DN_MAX_JOBS * DN_TAB <= RS_MAX_JOBS * RS_TAB, "the job records of a launch fit rs_meta");
static_assert((VX_DEV_DENOISE_TABLE_MAX / DN_H + 4L) * DN_B <= DN_GAIN_CAP, "the gains of the longest dev row fit behind the samples");
static_assert(VX_DEV_DENOISE_WINDOW_MIN >= DN_N && VX_DEV_DENOISE_WINDOW_MIN <= VX_DENOISE_WINDOW, "window bounds of the dev header");
static_assert(4L * DN_N * VX_DEV_DENOISE_FFT_MAX * sizeof(double) <= (size_t)RS_IN_CAP * sizeof(float), "the dev frames fit rs_in / rs_out");

__device__ __forceinline__ float dn_clean(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u ? x : 0.f; }
__device__ __forceinline__ int dn_phys(int i) { return i ^ (((i >> 4) & 1) * 15) ^ (((i >> 5) & 1) * 16); }
__device__ __forceinline__ int dn_rev(int i) { return (int)(__brev((unsigned)i) >> 23); }

struct DnLds {
  double re[DN_N], im[DN_N], tc[DN_N], ts[DN_N];
  double aux[DN_B + 7];                                              // the powers (power kernel) or the gains (synthesis) of a frame
};

__device__ __forceinline__ void dn_load_twiddles(DnLds& s, const double* __restrict__ buf, int tid) {
  s.tc[tid] = buf[DN_TC_AT + tid]; s.tc[tid + 256] = buf[DN_TC_AT + tid + 256];
  s.ts[tid] = buf[DN_TS_AT + tid]; s.ts[tid + 256] = buf[DN_TS_AT + tid + 256];
}

// the nine stages on s.re / s.im (bit-reversed order already, at dn_phys); synchronises before the first stage and after the last
__device__ __forceinline__ void dn_network(DnLds& s, bool inverse, int tid) {
#pragma unroll 1
  for (int h = 1; h < DN_N; h <<= 1) {
    __syncthreads();
    const int p = tid & (h - 1), i0 = ((tid - p) << 1) + p;
    const int a0 = dn_phys(i0), a1 = dn_phys(i0 + h);
    const double cq = s.tc[h + p], sv = s.ts[h + p], sq = inverse ? -sv : sv;
    const double r1 = s.re[a1], m1 = s.im[a1];
    const double tr = cq * r1 - sq * m1, ti = cq * m1 + sq * r1;
    const double ar = s.re[a0], ai = s.im[a0];
    s.re[a0] = ar + tr; s.im[a0] = ai + ti;
    s.re[a1] = ar - tr; s.im[a1] = ai - ti;
  }
  __syncthreads();
}

// frame t of a row, windowed, into s.re / s.im in bit-reversed order
__device__ __forceinline__ void dn_load_frame(DnLds& s, const float* __restrict__ x, long L, long t, const double* __restrict__ w, int tid) {
#pragma unroll
  for (int e = tid; e < DN_N; e += 256) {
    const int n = dn_rev(e);
    const long i = (t - 3) * DN_H + n;
    const float v = i >= 0 && i < L ? dn_clean(x[i]) : 0.f;
    s.re[dn_phys(e)] = (double)v * w[n];
    s.im[dn_phys(e)] = 0.0;
  }
}

// the gain of bin k of frame t: P the row's power table [T][257], Nz its profile
__device__ __forceinline__ double dn_gain(const double* __restrict__ P, long T, long t, int k, const double* __restrict__ Nz, double alpha,
                                          double fl) {
  auto at = [&](long q) { return P[(q < 0 ? 0 : q > T - 1 ? T - 1 : q) * DN_B + k]; };
  const double S = ((((at(t - 2) + at(t - 1)) + at(t)) + at(t + 1)) + at(t + 2)) / 5.0;
  const double g = S > 0.0 ? 1.0 - (alpha * Nz[k]) / S : fl;
  return g > fl ? g : fl;
}

// the last job whose word `field` is <= b (the words ascend with the job)
__device__ __forceinline__ int dn_job_of(const int* __restrict__ tab, int njobs, int field, int b) {
  int jl = 0, jh = njobs - 1;
  while (jl < jh) {
    const int m = (jl + jh + 1) >> 1;
    if (tab[m * DN_TAB + field] <= b) jl = m; else jh = m - 1;
  }
  return jl;
}

// tab [njobs][DN_TAB]:
//   0 in_off  first float of the row in `in` (and of its outputs in `out`);  1 L  samples of the row
//   2 f_off   first frame of the row in P and E;  3 T  its frames;  4 h_off  first synthesis workgroup of the row
//   5 K       chosen frames;  6 sel_off  the first of them in the list
__global__ __launch_bounds__(256) void denoise_power_kernel(const float* __restrict__ in, const int* __restrict__ tab, int njobs,
                                                            double* __restrict__ buf) {
  __shared__ DnLds s;
  const int tid = threadIdx.x;
  const int* tb = tab + dn_job_of(tab, njobs, 2, (int)blockIdx.x) * DN_TAB;
  const long L = tb[1], t = (long)blockIdx.x - tb[2];
  dn_load_twiddles(s, buf, tid);
  dn_load_frame(s, in + tb[0], L, t, buf + DN_W_AT, tid);
  dn_network(s, false, tid);
  double* P = buf + DN_P_AT + (long)blockIdx.x * DN_B;
  for (int k = tid; k < DN_B; k += 256) {
    const double r = s.re[dn_phys(k)], m = s.im[dn_phys(k)];
    const double p = r * r + m * m;
    s.aux[k] = p;
    P[k] = p;
  }
  __syncthreads();
  if (tid == 0) {
    double e = 0.0;
    for (int k = 0; k < DN_B; ++k) e = e + s.aux[k];
    buf[DN_E_AT + blockIdx.x] = e;
  }
}

__global__ __launch_bounds__(256) void denoise_profile_kernel(const int* __restrict__ tab, double* __restrict__ buf) {
  const int* tb = tab + blockIdx.x * DN_TAB;
  const int K = tb[5];
  const int* sel = reinterpret_cast<const int*>(buf + DN_SEL_AT) + tb[6];
  const double* P = buf + DN_P_AT + (long)tb[2] * DN_B;
  for (int k = threadIdx.x; k < DN_B; k += 256) {
    double a = 0.0;
    for (int i = 0; i < K; ++i) a = a + P[(long)sel[i] * DN_B + k];
    buf[DN_NZ_AT + (long)blockIdx.x * DN_B + k] = K > 0 ? a / (double)K : 0.0;
  }
}

__global__ __launch_bounds__(256) void denoise_synth_kernel(const float* __restrict__ in, const int* __restrict__ tab, int njobs,
                                                            const double* __restrict__ buf, float* __restrict__ out, double alpha, double fl) {
  __shared__ DnLds s;
  const int tid = threadIdx.x;
  const int job = dn_job_of(tab, njobs, 4, (int)blockIdx.x);
  const int* tb = tab + job * DN_TAB;
  const long L = tb[1], T = tb[3], u = (long)blockIdx.x - tb[4];
  const float* x = in + tb[0];
  const double* w = buf + DN_W_AT;
  const double* P = buf + DN_P_AT + (long)tb[2] * DN_B;
  const double* Nz = buf + DN_NZ_AT + (long)job * DN_B;
  dn_load_twiddles(s, buf, tid);
  double acc = 0.0;
#pragma unroll 1
  for (long t = u; t < u + 4; ++t) {                                 // the four frames of the hop, in ascending t
    dn_load_frame(s, x, L, t, w, tid);
    dn_network(s, false, tid);
    for (int k = tid; k < DN_B; k += 256) s.aux[k] = dn_gain(P, T, t, k, Nz, alpha, fl);
    __syncthreads();
    double vr[2], vi[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int e = tid + 256 * q;
      const double g = s.aux[e <= DN_N / 2 ? e : DN_N - e];
      vr[q] = s.re[dn_phys(e)] * g;
      vi[q] = s.im[dn_phys(e)] * g;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int a = dn_phys(dn_rev(tid + 256 * q));
      s.re[a] = vr[q];
      s.im[a] = vi[q];
    }
    dn_network(s, true, tid);
    if (tid < DN_H) {
      const int n = (int)(u + 3 - t) * DN_H + tid;
      acc = acc + (s.re[dn_phys(n)] * (1.0 / DN_N)) * w[n];
    }
    __syncthreads();                                                 // the next frame overwrites re / im
  }
  const long i = u * DN_H + tid;
  if (tid < DN_H && i < L) out[tb[0] + i] = (float)(0.5 * acc);
}

// vx_dev_denoise_table: the gains of one row, from the function the synthesis kernel runs
__global__ __launch_bounds__(256) void denoise_gain_kernel(const int* __restrict__ tab, const double* __restrict__ buf, double* __restrict__ gain,
                                                           double alpha, double fl) {
  const long T = tab[3], t = blockIdx.x;
  for (int k = threadIdx.x; k < DN_B; k += 256)
    gain[t * DN_B + k] = dn_gain(buf + DN_P_AT + (long)tab[2] * DN_B, T, t, k, buf + DN_NZ_AT, alpha, fl);
}

// vx_dev_denoise_fft: the network on caller frames, src / dst [nframes][2][512]
__global__ __launch_bounds__(256) void denoise_fft_kernel(const double* __restrict__ src, const double* __restrict__ buf, int inverse,
                                                          double* __restrict__ dst) {
  __shared__ DnLds s;
  const int tid = threadIdx.x;
  const double* f = src + (long)blockIdx.x * 2 * DN_N;
  double* d = dst + (long)blockIdx.x * 2 * DN_N;
  dn_load_twiddles(s, buf, tid);
  for (int e = tid; e < DN_N; e += 256) {
    s.re[dn_phys(e)] = f[dn_rev(e)];
    s.im[dn_phys(e)] = f[DN_N + dn_rev(e)];
  }
  dn_network(s, inverse != 0, tid);
  const double sc = inverse ? 1.0 / DN_N : 1.0;
  for (int e = tid; e < DN_N; e += 256) {
    d[e] = s.re[dn_phys(e)] * sc;
    d[DN_N + e] = s.im[dn_phys(e)] * sc;
  }
}

__global__ void denoise_div_kernel(const double* __restrict__ a, const double* __restrict__ b, int n, double* __restrict__ q) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) q[i] = a[i] / b[i];
}

// rs_buffers, and the stage's own allocation with the tables in it
static int dn_buffers(vx_ctx* c) {
  if (int e = rs_buffers(c)) return e;
  if (!c->dn_buf) {
    double* p = nullptr;
    if (int e = dev_alloc(c, &p, (size_t)DN_BUF, false)) return e;
    std::vector<double> t(2 * DN_N), st(3 * DN_N);
    dn_tables(t.data());
    memcpy(st.data(), t.data(), DN_N * sizeof(double));
    dn_stage_tables(t.data(), st.data() + DN_TC_AT, st.data() + DN_TS_AT);
    H2D(p + DN_W_AT, st.data(), st.size() * sizeof(double));
    SYNC();
    c->dn_buf = p;
  }
  return VX_OK;
}

// every check of vx_denoise behind the pointers: options, lengths, strides, the profile
static int dn_check(vx_ctx* c, const char* who, const int32_t* lens, int batch, const vx_denoise_opts* o, const double* psd, int64_t out_stride) {
  CHECK_STRUCT(*o, vx_denoise_opts);
  char why[160];
  if (dn_check_opts(*o, why, sizeof why)) FAIL(VX_EINVAL, "%s: %s", who, why);
  const long win = wave_window(c->dn_window, VX_DENOISE_WINDOW);
  for (int i = 0; i < batch; ++i)
    if (lens[i] > win)
      FAIL(VX_EINVAL, "%s: lens[%d] = %ld above the window of %ld samples (VX_DENOISE_WINDOW): a row is not cut", who, i, (long)lens[i], win);
  if (int e = wave_check_out_stride(c, who, lens, batch, out_stride, "")) return e;
  if (psd && !dn_psd_ok(psd)) FAIL(VX_EINVAL, "%s: noise_psd holds a word that is not finite or below 0", who);
  return VX_OK;
}

// The general path, launch by launch: power, the choice of the frames on the host, profile, synthesis.
// tP / tE / tsel / tgain: one row only (vx_dev_denoise_table).
static int dn_run(vx_ctx* c, const char* who, const float* wav, int64_t wav_stride, const int32_t* lens, int batch, const vx_denoise_opts& o,
                  const double* psd, float* out, int64_t out_stride, double* psd_out, vx_denoise_info* info, double* tP, double* tE,
                  int32_t* tsel, long tsel_cap, int32_t* n_sel, double* tgain) {
  const long win = wave_window(c->dn_window, VX_DENOISE_WINDOW);
  std::vector<DnJob> jobs;
  if (!dn_plan(lens, batch, win, dn_frame_cap(win), DN_MAX_JOBS, &jobs))
    FAIL(VX_EINVAL, "%s: a row in lens is above the window of %ld samples (vx_dev_denoise_window)", who, win);
  HIPCHK(hipSetDevice(c->dev));
  if (int e = dn_buffers(c)) return e;
  double* buf = c->dn_buf;
  int* dsel = reinterpret_cast<int*>(buf + DN_SEL_AT);
  double* dgain = reinterpret_cast<double*>(c->rs_out + DN_GAIN_AT);
  std::vector<vx_denoise_info> rinfo((size_t)batch);
  std::vector<int> tab;
  std::vector<double> E;
  std::vector<int32_t> sel, sel_all;
  for (size_t j0 = 0; j0 < jobs.size();) {
    size_t j1 = j0;
    while (j1 < jobs.size() && jobs[j1].launch == jobs[j0].launch) ++j1;
    const int nj = (int)(j1 - j0);
    const DnJob& last = jobs[j1 - 1];
    const long frames = last.f_off + dn_frames(lens[last.row]), hops = last.h_off + dn_hops(lens[last.row]);
    tab.clear();
    for (size_t k = j0; k < j1; ++k) {
      const DnJob& j = jobs[k];
      const long L = lens[j.row];
      if (L > 0) H2D(c->rs_in + j.in_off, wav + (long)j.row * wav_stride, (size_t)L * sizeof(float));
      for (long v : {j.in_off, L, j.f_off, dn_frames(L), j.h_off, 0L, 0L, 0L}) tab.push_back((int)v);
    }
    H2D(c->rs_meta, tab.data(), tab.size() * sizeof(int));
    hipLaunchKernelGGL(denoise_power_kernel, dim3((unsigned)frames), dim3(256), 0, c->stream, c->rs_in, c->rs_meta, nj, buf);
    E.resize((size_t)frames);
    D2H(E.data(), buf + DN_E_AT, (size_t)frames * sizeof(double));
    SYNC();
    HIPCHK(hipGetLastError());
    sel_all.clear();
    for (size_t k = j0; k < j1; ++k) {                               // the noise frames of every row
      const DnJob& j = jobs[k];
      const long L = lens[j.row], F = dn_full(L), K = psd ? 0 : dn_k(o, F);
      dn_select(E.data() + j.f_off, L, K, &sel);
      if (tsel && (long)sel.size() > tsel_cap) FAIL(VX_EINVAL, "%s: sel_cap %ld below the %zu chosen frames of the row", who, tsel_cap, sel.size());
      tab[(k - j0) * DN_TAB + 5] = (int)sel.size();
      tab[(k - j0) * DN_TAB + 6] = (int)sel_all.size();
      sel_all.insert(sel_all.end(), sel.begin(), sel.end());
      rinfo[(size_t)j.row] = {(int32_t)dn_frames(L), (int32_t)F, (int32_t)sel.size(), dn_nonfinite(wav + (long)j.row * wav_stride, L)};
      if (psd) H2D(buf + DN_NZ_AT + (long)(k - j0) * DN_B, psd, DN_B * sizeof(double));
    }
    if (!psd) {
      H2D(c->rs_meta, tab.data(), tab.size() * sizeof(int));
      if (!sel_all.empty()) H2D(dsel, sel_all.data(), sel_all.size() * sizeof(int32_t));
      hipLaunchKernelGGL(denoise_profile_kernel, dim3((unsigned)nj), dim3(256), 0, c->stream, c->rs_meta, buf);
    }
    if (hops > 0)
      hipLaunchKernelGGL(denoise_synth_kernel, dim3((unsigned)hops), dim3(256), 0, c->stream, c->rs_in, c->rs_meta, nj, buf, c->rs_out,
                         (double)o.alpha, (double)o.floor);
    for (size_t k = j0; k < j1; ++k) {
      const DnJob& j = jobs[k];
      if (lens[j.row] > 0) D2H(out + (long)j.row * out_stride, c->rs_out + j.in_off, (size_t)lens[j.row] * sizeof(float));
      if (psd_out) D2H(psd_out + (long)j.row * DN_B, buf + DN_NZ_AT + (long)(k - j0) * DN_B, DN_B * sizeof(double));
    }
    if (tP) {                                                        // one row, one launch
      hipLaunchKernelGGL(denoise_gain_kernel, dim3((unsigned)frames), dim3(256), 0, c->stream, c->rs_meta, buf, dgain, (double)o.alpha,
                         (double)o.floor);
      D2H(tP, buf + DN_P_AT, (size_t)frames * DN_B * sizeof(double));
      D2H(tgain, dgain, (size_t)frames * DN_B * sizeof(double));
      memcpy(tE, E.data(), (size_t)frames * sizeof(double));
      if (!sel_all.empty()) memcpy(tsel, sel_all.data(), sel_all.size() * sizeof(int32_t));
      *n_sel = (int32_t)sel_all.size();
    }
    SYNC();
    HIPCHK(hipGetLastError());
    j0 = j1;
  }
  for (int i = 0; i < batch; ++i) info[i] = rinfo[(size_t)i];
  return VX_OK;
}

}  // namespace vxe

extern "C" {

int vx_denoise_tables(double t[1024]) {
  if (!t) return VX_EINVAL;
  vxe::dn_tables(t);
  return VX_OK;
}

int vx_denoise(vx_ctx* c, const float* wav, int64_t wav_stride, const int32_t* lens, int32_t batch, const vx_denoise_opts* o,
               const double* noise_psd, float* out, int64_t out_stride, double* psd_out, vx_denoise_info* info) {
  using namespace vxe;
  if (!c) return VX_EINVAL;
  if (int e = wave_check_rows(c, "vx_denoise", wav, wav_stride, lens, batch)) return e;
  if (!o) FAIL(VX_EINVAL, "vx_denoise: o is NULL");
  if (!out) FAIL(VX_EINVAL, "vx_denoise: out is NULL");
  if (!info) FAIL(VX_EINVAL, "vx_denoise: info is NULL");
  if (int e = dn_check(c, "vx_denoise", lens, batch, o, noise_psd, out_stride)) return e;
  return dn_run(c, "vx_denoise", wav, wav_stride, lens, batch, *o, noise_psd, out, out_stride, psd_out, info, nullptr, nullptr, nullptr, 0,
                nullptr, nullptr);
}

int vx_dev_denoise_table(vx_ctx* c, const float* wav, int32_t len, const vx_denoise_opts* o, const double* noise_psd, double* P, double* E,
                         int32_t* sel, int32_t sel_cap, int32_t* n_sel, double* gain) {
  using namespace vxe;
  if (!c) return VX_EINVAL;
  if (!wav) FAIL(VX_EINVAL, "vx_dev_denoise_table: wav is NULL");
  if (!o) FAIL(VX_EINVAL, "vx_dev_denoise_table: o is NULL");
  if (!P || !E || !sel || !n_sel || !gain) FAIL(VX_EINVAL, "vx_dev_denoise_table: P, E, sel, n_sel or gain is NULL");
  if (len < 0 || len > VX_DEV_DENOISE_TABLE_MAX) FAIL(VX_EINVAL, "vx_dev_denoise_table: len %d outside 0 .. %d", len, VX_DEV_DENOISE_TABLE_MAX);
  if (sel_cap < 0) FAIL(VX_EINVAL, "vx_dev_denoise_table: sel_cap %d below 0", sel_cap);
  const int64_t big = 0x7fffffffL;
  if (int e = dn_check(c, "vx_dev_denoise_table", &len, 1, o, noise_psd, big)) return e;
  std::vector<float> y((size_t)len + 1);
  vx_denoise_info info;
  return dn_run(c, "vx_dev_denoise_table", wav, len, &len, 1, *o, noise_psd, y.data(), big, nullptr, &info, P, E, sel, sel_cap, n_sel, gain);
}

int vx_dev_denoise_fft(vx_ctx* c, const double* re, const double* im, int32_t nframes, int32_t inverse, double* out_re, double* out_im) {
  using namespace vxe;
  if (!c) return VX_EINVAL;
  if (!re || !im || !out_re || !out_im) FAIL(VX_EINVAL, "vx_dev_denoise_fft: re, im, out_re or out_im is NULL");
  if (nframes < 1 || nframes > VX_DEV_DENOISE_FFT_MAX)
    FAIL(VX_EINVAL, "vx_dev_denoise_fft: nframes %d outside 1 .. %d", nframes, VX_DEV_DENOISE_FFT_MAX);
  if (inverse != 0 && inverse != 1) FAIL(VX_EINVAL, "vx_dev_denoise_fft: inverse %d is not 0 or 1", inverse);
  HIPCHK(hipSetDevice(c->dev));
  if (int e = dn_buffers(c)) return e;
  double* src = reinterpret_cast<double*>(c->rs_in);
  double* dst = reinterpret_cast<double*>(c->rs_out);
  for (int f = 0; f < nframes; ++f) {
    H2D(src + (long)f * 2 * DN_N, re + (long)f * DN_N, DN_N * sizeof(double));
    H2D(src + (long)f * 2 * DN_N + DN_N, im + (long)f * DN_N, DN_N * sizeof(double));
  }
  hipLaunchKernelGGL(denoise_fft_kernel, dim3((unsigned)nframes), dim3(256), 0, c->stream, src, c->dn_buf, inverse, dst);
  for (int f = 0; f < nframes; ++f) {
    D2H(out_re + (long)f * DN_N, dst + (long)f * 2 * DN_N, DN_N * sizeof(double));
    D2H(out_im + (long)f * DN_N, dst + (long)f * 2 * DN_N + DN_N, DN_N * sizeof(double));
  }
  SYNC();
  HIPCHK(hipGetLastError());
  return VX_OK;
}

int vx_dev_denoise_window(vx_ctx* c, int32_t samples) {
  return vxe::wave_set_window(c, &vx_ctx::dn_window, "vx_dev_denoise_window", "samples", samples, VX_DEV_DENOISE_WINDOW_MIN, VX_DENOISE_WINDOW);
}

int vx_dev_denoise_div(vx_ctx* c, const double* a, const double* b, int32_t n, double* q) {
  using namespace vxe;
  if (!c) return VX_EINVAL;
  if (!a || !b || !q) FAIL(VX_EINVAL, "vx_dev_denoise_div: a, b or q is NULL");
  if (n < 1 || n > 65536) FAIL(VX_EINVAL, "vx_dev_denoise_div: n %d outside 1 .. 65536", n);
  HIPCHK(hipSetDevice(c->dev));
  if (int e = dn_buffers(c)) return e;
  double* da = reinterpret_cast<double*>(c->rs_in);
  double* dq = reinterpret_cast<double*>(c->rs_out);
  H2D(da, a, (size_t)n * sizeof(double));
  H2D(da + n, b, (size_t)n * sizeof(double));
  hipLaunchKernelGGL(denoise_div_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, da, da + n, n, dq);
  D2H(q, dq, (size_t)n * sizeof(double));
  SYNC();
  HIPCHK(hipGetLastError());
  return VX_OK;
}

}  // extern "C"
