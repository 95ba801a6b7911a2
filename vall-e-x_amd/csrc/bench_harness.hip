// Measurement and kernel-development entries (include/vallex_hip_dev.h): per-class HIP-event profiling, back-to-back kernel
// replays on the live decode state, stand-alone GEMM / attention micro-benchmarks.  Never on the product path.
#include "../../include/vallex_hip_dev.h"
#include "engine_ctx.h"

namespace {

// Kernel-development aid (VX_BENCH_CLOCK=1 in vx_bench_gemm): one wave that sits next to the kernel under test for `ref_ticks` of
// the constant 100 MHz counter and reports how many shader-clock ticks (s_memtime) went by -> the clock the chip actually
// holds under that load.  Bounded by the real-time counter, so it always terminates.
__global__ void clock_probe_kernel(unsigned long long* out, unsigned long long ref_ticks) {
  const unsigned long long r0 = __builtin_amdgcn_s_memrealtime(), c0 = __builtin_readcyclecounter();
  while (__builtin_amdgcn_s_memrealtime() - r0 < ref_ticks) __builtin_amdgcn_s_sleep(16);
  if (threadIdx.x == 0) {
    out[0] = __builtin_readcyclecounter() - c0;
    out[1] = __builtin_amdgcn_s_memrealtime() - r0;
  }
}


}  // namespace

extern "C" {

int vx_prof_enable(vx_ctx* c, int32_t on) {
  if (!c) return VX_EINVAL;
  c->prof_on = on;
  return VX_OK;
}

int vx_prof_reset(vx_ctx* c) {
  if (!c) return VX_EINVAL;
  for (auto& p : c->prof) { p.used = 0; p.bytes = 0; }
  return VX_OK;
}

int vx_prof_get(vx_ctx* c, int32_t which, double* total_ms, int64_t* launches, double* algo_bytes) {
  if (!c || which < 0 || which > 5) return VX_EINVAL;
  HIPCHK(hipSetDevice(c->dev));
  SYNC();
  ProfClass& p = c->prof[which];
  double tot = 0;
  for (size_t i = 0; i + 1 < p.used; i += 2) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, p.ev[i], p.ev[i + 1]));
    tot += ms;
  }
  if (total_ms) *total_ms = tot;
  if (launches) *launches = (int64_t)(p.used / 2);
  if (algo_bytes) *algo_bytes = p.bytes;
  return VX_OK;
}

// Back-to-back replays of ONE decode kernel on the live state of the last AR run, bracketed by a single HIP event
// pair on the engine stream (GPU-bound: no host gaps inside the interval).  which 0: dec_attn of layer 0 with every
// row's context set to prefill_len + gen_offset; which 1: the five weight-streaming GEMMs of a step's layer 0
// (+ predict layer), reported per launch.
int vx_bench_kernel(vx_ctx* c, int32_t which, int32_t reps, int32_t gen_offset, double* avg_us, double* algo_bytes) {
  if (!c || reps <= 0 || !avg_us || !algo_bytes) return VX_EINVAL;
  if (c->cur_batch <= 0) FAIL(VX_ESTATE, "no AR run to replay");
  HIPCHK(hipSetDevice(c->dev));
  const int nb = c->cur_batch;
  hipEvent_t e0, e1;
  HIPCHK(hipEventCreate(&e0));
  HIPCHK(hipEventCreate(&e1));
  double bytes = 0;
  int launches = 0;
  if (which == 0) {
    std::vector<int> ctx(nb), one(nb, 1);
    for (int i = 0; i < nb; ++i) {
      ctx[i] = std::min(c->h_L[i] + std::max(gen_offset, 1), c->Tmax - 1);
      bytes += (double)ctx[i] * 2.0 * D_MODEL * 4.0;
    }
    if (c->fuse_out && c->nsplit == 1) bytes += (double)D_MODEL * D_MODEL * 4.0;     // + W_o, streamed once (fused out_proj)
    // the replay's contexts go into the per-slot view dec_attn reads (the row order of the last prefill is kept)
    std::vector<int> meta(4 * nb);
    D2H(meta.data(), c->slot_meta, meta.size() * sizeof(int));
    SYNC();
    for (int y = 0; y < nb; ++y) { meta[4 * y + 1] = ctx[meta[4 * y]]; meta[4 * y + 2] = 1; }
    H2D(c->slot_meta, meta.data(), meta.size() * sizeof(int));
    H2D(c->ctx_len, ctx.data(), nb * sizeof(int));
    H2D(c->active, one.data(), nb * sizeof(int));
    SYNC();
    // rotate over the layers' KV arenas like the real step does: the working set (NL x ~178 MB at batch 32) is far beyond
    // the 256 MiB Infinity Cache, so no launch is served from it
    const size_t cache_layer = (size_t)c->mbr * N_HEAD * c->Tmax * D_HEAD;
    auto attn_l = [&](int r) {
      const int l = r % c->NL;
      const bool fused = c->fuse_out && (c->nsplit == 1 || c->split_fused);
      // slab counts of the product's in_proj (84 = 8 slabs of q, 4 of k / v: skinny_qkv_bal_kernel)
      launch_dec_attn(c->p_qkv, c->qkv_bal ? 84 : SK_QKV, c->ar[l].in_b, c->kc + l * cache_layer, c->vc + l * cache_layer, c->Tmax,
                      c->slot_meta, c->xp_att, c->part_o, c->part_ml, c->nsplit, nb, fused ? c->ar[l].out_wh : nullptr, c->p_oh,
                      c->stream);
    };
    for (int w = 0; w < 3; ++w) attn_l(w);
    HIPCHK(hipEventRecord(e0, c->stream));
    for (int r = 0; r < reps; ++r) attn_l(r);
    HIPCHK(hipEventRecord(e1, c->stream));
    launches = reps;
  } else if (which == 1) {
    const LayerW& L = c->ar[0];
    auto seq = [&]() {
      if (c->qkv_bal) launch_skinny_qkv_balanced(L.in_wp, c->xp, c->p_qkv, c->stream);      // the in_proj the decode step runs
      // (write-through result stores, as in the 32-row step: decode.hip store_result)
      else launch_skinny_gemm(L.in_wp, c->xp, c->p_qkv, 3 * D_MODEL, D_MODEL, SK_QKV, c->stream, true);
      launch_skinny_gemm(L.out_wp, c->xp_att, c->p_o, D_MODEL, D_MODEL, SK_OUT, c->stream, true);
      launch_linear1(c, L.l1_wp, c->xp, L.l1_b, c->xp4, c->stream);
      launch_skinny_gemm_kmap(L.l2_wp, c->xp4, c->p_o, D_MODEL, D_FF, SK_L2, c->stream, true, c->l2_kmap);
    };
    seq();
    HIPCHK(hipEventRecord(e0, c->stream));
    for (int r = 0; r < reps; ++r) seq();
    HIPCHK(hipEventRecord(e1, c->stream));
    launches = reps * 4;
    bytes = 12.0 * D_MODEL * D_MODEL * 4.0 / 4.0;     // per launch: a layer's 12 d^2 weights over its 4 GEMMs
  } else if (which == 2) {
    // cache-retention probe: the SAME weight-streaming GEMM (layer 0 QKV, 12.6 MB) back to back -- what a launch costs when
    // its weights were read a moment ago (memory-side cache hits) instead of coming cold from HBM (which 1)
    const LayerW& L = c->ar[0];
    auto one = [&]() { launch_skinny_gemm(L.in_wp, c->xp, c->p_qkv, 3 * D_MODEL, D_MODEL, SK_QKV, c->stream); };
    one();
    HIPCHK(hipEventRecord(e0, c->stream));
    for (int r = 0; r < reps; ++r) one();
    HIPCHK(hipEventRecord(e1, c->stream));
    launches = reps;
    bytes = 3.0 * D_MODEL * D_MODEL * 4.0;
#ifdef VX_DEV_PROBES
  } else if (which == 3 || which == 4) {
    // development timeline (tools/step_timeline.py): `reps` graph replays of a ONE-layer (which 3) or the whole (which 4) decode step (QKV | attention |
    // reduce+LN | linear1 | linear2 | reduce+LN | predict | sampler) on the live state; the kernels stamp the wall clock
    // (decode.hip) and the caller fetches the stamps of the last replay with vx_dev_stamps.
    vx_sampling sp{};
    sp.struct_size = sizeof(vx_sampling); sp.top_k = 10; sp.temperature = 1.0f; sp.seed = 1; sp.force_eos_at = -1; sp.best_of = 1;
    SampleArgs sa = make_sample_args(c, &sp, 1, nullptr);
    const int nl_keep = c->NL;
    if (which == 3) c->NL = 1;      // which 4: the whole step; the stamps that remain are the LAST layer's, whose weights the other
                                    // layers' 500 MB have pushed out of every cache since the previous replay
    hipGraph_t g = nullptr;
    hipGraphExec_t ge = nullptr;
    HIPCHK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    ar_step_launches(c, &sa);
    HIPCHK(hipStreamEndCapture(c->stream, &g));
    c->NL = nl_keep;
    HIPCHK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
    (void)hipGraphDestroy(g);
    for (int w = 0; w < 3; ++w) HIPCHK(hipGraphLaunch(ge, c->stream));
    SYNC();
    dev_clear_stamps();
    HIPCHK(hipEventRecord(e0, c->stream));
    for (int r = 0; r < reps; ++r) HIPCHK(hipGraphLaunch(ge, c->stream));
    HIPCHK(hipEventRecord(e1, c->stream));
    SYNC();
    (void)hipGraphExecDestroy(ge);
    launches = reps;
    bytes = 0;
#endif
  } else {
    FAIL(VX_EINVAL, "which must be 0, 1 or 2");
  }
  HIPCHK(hipEventSynchronize(e1));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  *avg_us = (double)ms * 1e3 / launches;
  *algo_bytes = bytes;
  HIPCHK(hipGetLastError());
  return VX_OK;
}

#ifdef VX_DEV_PROBES
extern "C" int vx_dev_stamps(unsigned long long* out) { dev_read_stamps(out); return VX_OK; }
extern "C" int vx_dev_wave_stamps(unsigned long long* out) { vx::dev_read_wave_stamps(out); return VX_OK; }
extern "C" int vx_dev_gemm_stamps(unsigned long long* out) { dev_read_gemm_stamps(out); return VX_OK; }
#endif

// Stand-alone GEMM micro-benchmark on scratch buffers (kernel development aid; never on the product path):
// kernel 0 = gemm_f32 (3 / 4 / 5: its register-staged / LDS-DMA 256 x 128 / LDS-DMA 128 x 128 kernel forced), 1 = gemm_bf16x3,
// 2 = gemm_bf16x3_dma, 6 = gemm_f16x2 (the default of the model path);
// 11-13 / 21-24 = timing probes of the bf16x3 kernels (VX_DEV_PROBES builds only).  Reports the average launch time and the max abs
// difference of the first and last 256 output rows against the fp32-MFMA kernel.
static int bench_gemm_impl(vx_ctx* c, int32_t M, int32_t N, int32_t K, int32_t kernel, int32_t reps, double* avg_us,
                           double* max_abs_diff, double* clock_mhz) {
  if (!c || M <= 0 || N <= 0 || K <= 0 || K % 32 || N % 4 || reps <= 0 || !avg_us || !max_abs_diff) return VX_EINVAL;
#ifndef VX_DEV_PROBES
  if (kernel < 0 || (kernel > 10 && kernel != 14 && kernel != 15))
    FAIL(VX_EINVAL, "kernel must be 0 .. 10, 14 or 15 (probes and the priority variants 12 / 13 need a VX_DEV_PROBES build)");
#endif
  HIPCHK(hipSetDevice(c->dev));
  float *A = nullptr, *Wt = nullptr, *C0 = nullptr, *C1 = nullptr;
  unsigned short *A3 = nullptr, *W3 = nullptr;
  auto cleanup = [&]() { for (void* p : {(void*)A, (void*)Wt, (void*)C0, (void*)C1, (void*)A3, (void*)W3}) if (p) (void)hipFree(p); };
  hipError_t he;
#define TRY(x) if ((he = (x)) != hipSuccess) { cleanup(); c->err = std::string(#x) + ": " + hipGetErrorString(he); return VX_EHIP; }
  TRY(hipMalloc((void**)&A, (size_t)M * K * 4));
  TRY(hipMalloc((void**)&Wt, (size_t)N * K * 4));
  TRY(hipMalloc((void**)&C0, (size_t)M * N * 4));
  TRY(hipMalloc((void**)&C1, (size_t)M * N * 4));
  TRY(hipMalloc((void**)&A3, (size_t)3 * h2_plane(M, K, H2_TILE_A) * 2));
  TRY(hipMalloc((void**)&W3, (size_t)3 * h2_plane(N, K, H2_TILE_W) * 2));
  TRY(hipMemset(A3, 0, (size_t)3 * h2_plane(M, K, H2_TILE_A) * 2));
  TRY(hipMemset(W3, 0, (size_t)3 * h2_plane(N, K, H2_TILE_W) * 2));
  {
    std::vector<float> h((size_t)std::max(M, N) * K);
    unsigned long long st = 0x9E3779B97F4A7C15ull;
    // VX_BENCH_GEMM_DATA (kernel-development aid): what the operands look like to the matrix pipe.  unset / "random": uniform in
    // [-1, 1) (heads and tails both busy);  "zero_tail": the same values rounded to 10 significant bits -> every fp16 tail plane is
    // exactly zero (the tail x head products toggle nothing);  "zero": all operands zero;  "const": every element 0.5.  Same
    // launches, same bytes moved: a kernel that gets faster on quieter operands is bound by power, not by its schedule.
    const char* dm = getenv("VX_BENCH_GEMM_DATA");
    const int data_mode = !dm ? 0 : (!strcmp(dm, "zero_tail") ? 1 : (!strcmp(dm, "zero") ? 2 : (!strcmp(dm, "const") ? 3 : 0)));
    auto fill = [&](size_t n) {
      for (size_t i = 0; i < n; ++i) {
        st = st * 6364136223846793005ull + 1442695040888963407ull;
        float v = (float)((st >> 40) & 0xFFFFFF) / 8388608.0f - 1.0f;
        if (data_mode == 1) { int ex; const float mant = frexpf(v, &ex); v = ldexpf(rintf(mant * 1024.0f) / 1024.0f, ex); }
        else if (data_mode == 2) v = 0.0f;
        else if (data_mode == 3) v = 0.5f;
        h[i] = v;
      }
    };
    fill((size_t)M * K);
    H2D(A, h.data(), (size_t)M * K * 4);
    fill((size_t)N * K);
    H2D(Wt, h.data(), (size_t)N * K * 4);
  }
  GemmArgs g0{};
  g0.A = A; g0.lda = K; g0.W = Wt; g0.ldw = K; g0.C = C0; g0.ldc = N; g0.M = M; g0.N = N; g0.K = K; g0.act = ACT_NONE;
  launch_gemm_f32(g0, c->stream, 1);                                     // the comparison baseline: the register-staged fp32 kernel
  if ((kernel >= 6 && kernel <= 13) || kernel == 15 || kernel >= 61) {   // fp16 head / tail planes
    launch_split2h(A, K, M, K, nullptr, A3, h2_plane(M, K, H2_TILE_A), H2_TILE_A, nullptr, H2_ACT_SCALE, c->stream);
    launch_split2h(Wt, K, N, K, nullptr, W3, h2_plane(N, K, H2_TILE_W), H2_TILE_W, nullptr, 16384.0f, c->stream);   // |w| < 1
  } else {
    launch_split3(A, K, M, K, nullptr, A3, (long)M * K, c->stream);
    launch_split3(Wt, K, N, K, nullptr, W3, (long)N * K, c->stream);
  }
  GemmX3Args gx{};
  const bool h2 = (kernel >= 6 && kernel <= 13) || kernel == 15 || kernel >= 61;
  gx.A = A3; gx.a_plane = h2 ? h2_plane(M, K, H2_TILE_A) : (long)M * K; gx.W = W3; gx.w_plane = h2 ? h2_plane(N, K, H2_TILE_W) : (long)N * K; gx.C = C1; gx.ldc = N; gx.M = M; gx.N = N; gx.K = K;
  gx.act = ACT_NONE;
  gx.descale = ldexpf(1.0f, -(H2_ACT_SHIFT + 14));
  GemmArgs g1 = g0;
  g1.C = C1;
  // VX_BENCH_GEMM_WALK="<gm>[,c]" (read at EVERY call of the harness, unlike the launchers' VX_GEMM_WALK): tile-order A/B inside one
  // process, interleaved (tools/gemm_walk_sweep.py ab); -1 = the order the kernels had before round 6 (8 row tiles deep, row-fastest)
  if (const char* we = getenv("VX_BENCH_GEMM_WALK")) {
    const int gm = atoi(we);
    const char* comma = strchr(we, ',');
    const int wk = gm == -1 ? 8 : ((gm >= 1 && gm <= 255) ? (gm | ((comma && comma[1] == 'c') ? 256 : 0)) : 0);
    gx.walk = wk;
    g1.walk = wk;
  }
  auto run = [&]() {
    if (kernel == 0) launch_gemm_f32(g1, c->stream);                       // fp32 MFMA, the product's choice of kernel
    else if (kernel >= 3 && kernel <= 5) launch_gemm_f32(g1, c->stream, kernel - 2);   // 3 register-staged / 4 LDS-DMA 256 x 128 / 5 LDS-DMA 128 x 128
    else if (kernel == 14) launch_gemm_f32(g1, c->stream, 4);                          // LDS-DMA 256 x 256
    else if (kernel == 1) launch_gemm_bf16x3(gx, c->stream);
    else if (kernel == 2) launch_gemm_bf16x3_dma(gx, c->stream);
    else if (kernel == 6) launch_gemm_f16x2(gx, c->stream);              // the product's choice of tile
    else if (kernel == 7) launch_gemm_f16x2(gx, c->stream, 128);
    else if (kernel == 8) launch_gemm_f16x2(gx, c->stream, 256);          // 256 x 256 tiles on the 8-wave kernel (64 x 128 per wave)
    else if (kernel == 15) launch_gemm_f16x2(gx, c->stream, 257);         // 256 x 256 tiles on the 4-wave kernel (128 x 128 per wave)
    else if (kernel == 9) launch_gemm_f16x2(gx, c->stream, -128);         // 128 x 128 tiles (the short-row-set kernel) forced
    else if (kernel == 10) launch_gemm_f16x2(gx, c->stream, -129);        // ... with two LDS stages forced (A/B of the four-stage ring)
#ifdef VX_DEV_PROBES
    else if (kernel == 12 || kernel == 13) {                            // 256 x 256 tiles with wave priority: static for waves 4-7 / per k16 step
      GemmX3Args gp = gx;
      gp.dev_variant = kernel - 11;
      launch_gemm_f16x2(gp, c->stream, 256);
    }
    else if (kernel >= 61) launch_gemm_f16x2_probe(gx, kernel - 60, c->stream);         // 61-64: probes of the f16x2 kernel
    else if (kernel >= 21) launch_gemm_bf16x3_dma_probe(gx, kernel - 20, c->stream);   // 21-24: probes of the DMA kernel
    else launch_gemm_bf16x3_probe(gx, kernel - 10, c->stream);      // 11 / 12 / 13: timing probes
#endif
  };
  run();
  // VX_BENCH_CLOCK=1: sample the shader clock on a second stream while the timed launches run (power / clock ceiling check)
  const char* want_clock = getenv("VX_BENCH_CLOCK");
  hipStream_t s2 = nullptr;
  unsigned long long* d_clk = nullptr;
  if (clock_mhz) *clock_mhz = 0.0;
  if (clock_mhz || (want_clock && want_clock[0] == '1')) {
    TRY(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking));
    TRY(hipMalloc((void**)&d_clk, 16));
    SYNC();
  }
  hipEvent_t e0, e1;
  TRY(hipEventCreate(&e0));
  TRY(hipEventCreate(&e1));
  TRY(hipEventRecord(e0, c->stream));
  run();                                                           // the probe starts once the device is busy
  if (s2) hipLaunchKernelGGL(clock_probe_kernel, dim3(1), dim3(64), 0, s2, d_clk, 100ull * 2000ull);   // 2 ms at 100 MHz
  for (int r = 1; r < reps; ++r) run();
  TRY(hipEventRecord(e1, c->stream));
  TRY(hipEventSynchronize(e1));
  float ms = 0;
  TRY(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  *avg_us = (double)ms * 1e3 / reps;
  if (s2) {
    unsigned long long hclk[2] = {0, 0};
    TRY(hipStreamSynchronize(s2));
    D2H(hclk, d_clk, 16); SYNC();
    const double mhz = hclk[1] ? (double)hclk[0] / ((double)hclk[1] / 100.0) : 0.0;
    if (clock_mhz) *clock_mhz = mhz;
    else
      fprintf(stderr, "[vx_bench_gemm] kernel %d M=%d N=%d K=%d: shader clock while running = %.0f MHz (%llu ticks in %.3f ms)\n", kernel,
              M, N, K, mhz, hclk[0], (double)hclk[1] / 1e5);
    (void)hipFree(d_clk);
    (void)hipStreamDestroy(s2);
  }
  // every output row against the register-staged fp32 kernel (round 6: interior tiles, the XCD remap and the tile-walk grouping are
  // compared too, not only the first and the last 256 rows), in chunks through the pinned ring
  double md = 0;
  {
    const int chunk = std::max(1, std::min(M, (int)((16u << 20) / ((size_t)N * 4))));
    std::vector<float> h0((size_t)chunk * N), h1((size_t)chunk * N);
    for (int r0 = 0; r0 < M; r0 += chunk) {
      const size_t n = (size_t)std::min(chunk, M - r0) * N;
      D2H(h0.data(), C0 + (size_t)r0 * N, n * 4);
      D2H(h1.data(), C1 + (size_t)r0 * N, n * 4);
      SYNC();
      for (size_t i = 0; i < n; ++i) {
        const double d = (double)fabsf(h0[i] - h1[i]);
        md = d > md || d != d ? (d != d ? 1e30 : d) : md;        // a NaN on either side is a mismatch, not a silent pass
      }
    }
  }
  *max_abs_diff = md;
#undef TRY
  cleanup();
  HIPCHK(hipGetLastError());
  return VX_OK;
}

int vx_bench_gemm(vx_ctx* c, int32_t M, int32_t N, int32_t K, int32_t kernel, int32_t reps, double* avg_us,
                  double* max_abs_diff) {
  return bench_gemm_impl(c, M, N, K, kernel, reps, avg_us, max_abs_diff, nullptr);
}

int vx_bench_gemm_clock(vx_ctx* c, int32_t M, int32_t N, int32_t K, int32_t kernel, int32_t reps, double* avg_us,
                        double* max_abs_diff, double* clock_mhz) {
  if (!clock_mhz) return VX_EINVAL;
  return bench_gemm_impl(c, M, N, K, kernel, reps, avg_us, max_abs_diff, clock_mhz);
}

// kernel-development aid: time attn_full (variant 0) or one of its probes (1 no staging, 2 no MFMA, 3 no softmax) on
// random q|k|v for `batch` sequences of length `len`, unmasked (NAR) or prefix-LM with prefix = len/3 (causal != 0).
int vx_bench_attn(vx_ctx* c, int32_t batch, int32_t len, int32_t causal, int32_t variant, int32_t reps, double* avg_us,
                  double* max_diff) {
  // variant: 0 fp32 kernel, 1-3 its probes; 10 bf16x3 kernel, 11-13 its probes.  max_diff (optional) = max |out - out of
  // the fp32 kernel| for the product variants (0 / 10), -1 for probes.
  if (!c || batch <= 0 || len <= 0 || reps <= 0 || !avg_us) return VX_EINVAL;
  HIPCHK(hipSetDevice(c->dev));
  const long M = (long)batch * len;
  float *qkv = nullptr, *out = nullptr, *ref = nullptr;
  int* meta = nullptr;
  auto cleanup = [&]() { for (void* p : {(void*)qkv, (void*)out, (void*)ref, (void*)meta}) if (p) (void)hipFree(p); };
  hipError_t he;
#define TRY(x) if ((he = (x)) != hipSuccess) { cleanup(); c->err = std::string(#x) + ": " + hipGetErrorString(he); return VX_EHIP; }
  TRY(hipMalloc((void**)&qkv, (size_t)M * 3 * D_MODEL * 4));
  TRY(hipMalloc((void**)&out, (size_t)M * D_MODEL * 4));
  TRY(hipMalloc((void**)&ref, (size_t)M * D_MODEL * 4));
  TRY(hipMalloc((void**)&meta, (size_t)3 * batch * 4));
  {
    std::vector<float> h((size_t)M * 3 * D_MODEL);
    unsigned long long st = 0x9E3779B97F4A7C15ull;
    for (auto& v : h) { st = st * 6364136223846793005ull + 1442695040888963407ull; v = (float)((st >> 40) & 0xFFFFFF) / 8388608.0f - 1.0f; }
    // Q columns x4: scores of a few units instead of ~0.3, so the softmax is not nearly uniform
    for (long r = 0; r < M; ++r) for (int k = 0; k < D_MODEL; ++k) h[(size_t)r * 3 * D_MODEL + k] *= 4.0f;
    H2D(qkv, h.data(), h.size() * 4);
    std::vector<int> m(3 * batch);
    for (int i = 0; i < batch; ++i) { m[i] = i * len; m[batch + i] = len; m[2 * batch + i] = len / 3; }
    H2D(meta, m.data(), m.size() * 4);
  }
  const int* pre = causal ? meta + 2 * batch : nullptr;
  auto run = [&]() {
    if (variant == 0) launch_attn_full(qkv, out, meta, meta + batch, pre, batch, len, c->stream);
    else if (variant == 8 || variant == 9)          // 8 / 9: the fp32 kernel with two / three LDS buffers forced (round-6 A/B)
      launch_attn_full(qkv, out, meta, meta + batch, pre, batch, len, c->stream, nullptr, nullptr, variant - 6);
#ifdef VX_DEV_PROBES
    else if (variant < 10) launch_attn_full_probe(qkv, out, meta, meta + batch, pre, batch, len, variant, c->stream);
#else
    else if (variant < 10) return;
#endif
    else if (variant >= 20 && variant <= 23)      // 20: the product's f16x2 kernel; 21-23: its wave-priority variants (tools builds)
      launch_attn_full_h2(qkv, out, meta, meta + batch, pre, batch, len, c->stream, nullptr, 0, nullptr, variant - 20);
    else launch_attn_full_x3(qkv, out, meta, meta + batch, pre, batch, len, variant - 10, c->stream);
  };
  run();
  hipEvent_t e0, e1;
  TRY(hipEventCreate(&e0));
  TRY(hipEventCreate(&e1));
  TRY(hipEventRecord(e0, c->stream));
  for (int r = 0; r < reps; ++r) run();
  TRY(hipEventRecord(e1, c->stream));
  TRY(hipEventSynchronize(e1));
  float ms = 0;
  TRY(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  *avg_us = (double)ms * 1e3 / reps;
  if (max_diff) {
    *max_diff = -1.0;
    if (variant == 0 || variant == 8 || variant == 9 || variant == 10 || (variant >= 20 && variant <= 23)) {
      launch_attn_full(qkv, ref, meta, meta + batch, pre, batch, len, c->stream, nullptr, nullptr, 2);      // reference: the two-buffer fp32 kernel
      SYNC();
      std::vector<float> ho((size_t)M * D_MODEL), hr((size_t)M * D_MODEL);
      D2H(ho.data(), out, ho.size() * 4); SYNC();
      D2H(hr.data(), ref, hr.size() * 4); SYNC();
      double md = 0;
      for (size_t i = 0; i < ho.size(); ++i) {
        const double d = std::fabs((double)ho[i] - (double)hr[i]);
        md = (d > md || d != d) ? (d != d ? 1e30 : d) : md;
      }
      *max_diff = md;
    }
  }
#undef TRY
  cleanup();
  HIPCHK(hipGetLastError());
  return VX_OK;
}


// Epilogue cross-check of the two f16x2 GEMM kernels (round 6, ADVICE): the four-wave 128 x 128 kernel (gemm_f16x2_w128_kernel, every
// 256 x 256 tile of the product) against the eight-wave kernel on the SAME operand planes, with the epilogue branches the plain
// micro-benchmark never reaches:  mode 0 = bias + ReLU + out_planes (linear1: the result leaves as the next GEMM's A planes);
// mode 1 = bias + residual read through resid_rows (the trimmed out_proj of the last NAR layer) on whatever ragged M was asked for;
// mode 2 = bias + residual, rows in place (out_proj / linear2).  Both kernels accumulate an output element in the same order, so
// every fp32 result and every plane half-word must be IDENTICAL: returns the number of differing 32-bit words of C (modes 1, 2) or
// 16-bit words of the planes (mode 0), and how many words were compared.
int vx_bench_gemm_epilogue(vx_ctx* c, int32_t M, int32_t N, int32_t K, int32_t mode, int64_t* differing, int64_t* compared) {
  // mode + 10: the eight-wave template on 128 x 128 tiles (the prefill / trimmed-layer instance) against the four-wave kernel
  const bool small_tiles = mode >= 10;
  if (small_tiles) mode -= 10;
  if (!c || M <= 0 || N <= 0 || K < 64 || K % 32 || N % 256 || mode < 0 || mode > 2 || !differing || !compared) return VX_EINVAL;
  HIPCHK(hipSetDevice(c->dev));
  const long a_pl = h2_plane(M, K, H2_TILE_A), w_pl = h2_plane(N, K, H2_TILE_W), o_pl = h2_plane(M, N, H2_TILE_A);
  float *A = nullptr, *Wt = nullptr, *bias = nullptr, *resid = nullptr, *C0 = nullptr, *C1 = nullptr;
  unsigned short *A3 = nullptr, *W3 = nullptr, *P0 = nullptr, *P1 = nullptr;
  int *rows = nullptr, *flag = nullptr;
  const int RR = M + 77;                                    // rows of the residual source (mode 1 reads it through a row map)
  auto cleanup = [&]() {
    for (void* p : {(void*)A, (void*)Wt, (void*)bias, (void*)resid, (void*)C0, (void*)C1, (void*)A3, (void*)W3, (void*)P0, (void*)P1, (void*)rows,
                    (void*)flag})
      if (p) (void)hipFree(p);
  };
  hipError_t he;
#define TRY(x) if ((he = (x)) != hipSuccess) { cleanup(); c->err = std::string(#x) + ": " + hipGetErrorString(he); return VX_EHIP; }
  TRY(hipMalloc((void**)&A, (size_t)M * K * 4));
  TRY(hipMalloc((void**)&Wt, (size_t)N * K * 4));
  TRY(hipMalloc((void**)&bias, (size_t)N * 4));
  TRY(hipMalloc((void**)&resid, (size_t)RR * N * 4));
  TRY(hipMalloc((void**)&C0, (size_t)M * N * 4));
  TRY(hipMalloc((void**)&C1, (size_t)M * N * 4));
  TRY(hipMalloc((void**)&A3, (size_t)2 * a_pl * 2));
  TRY(hipMalloc((void**)&W3, (size_t)2 * w_pl * 2));
  TRY(hipMalloc((void**)&P0, (size_t)2 * o_pl * 2));
  TRY(hipMalloc((void**)&P1, (size_t)2 * o_pl * 2));
  TRY(hipMalloc((void**)&rows, (size_t)M * 4));
  TRY(hipMalloc((void**)&flag, 4));
  TRY(hipMemsetAsync(A3, 0, (size_t)2 * a_pl * 2, c->stream));
  TRY(hipMemsetAsync(W3, 0, (size_t)2 * w_pl * 2, c->stream));
  TRY(hipMemsetAsync(P0, 0, (size_t)2 * o_pl * 2, c->stream));
  TRY(hipMemsetAsync(P1, 0, (size_t)2 * o_pl * 2, c->stream));
  TRY(hipMemsetAsync(C0, 0, (size_t)M * N * 4, c->stream));
  TRY(hipMemsetAsync(C1, 0, (size_t)M * N * 4, c->stream));
  TRY(hipMemsetAsync(flag, 0, 4, c->stream));
  {
    unsigned long long st = 0x2545F4914F6CDD1Dull;
    auto rnd = [&]() { st = st * 6364136223846793005ull + 1442695040888963407ull; return (float)((st >> 40) & 0xFFFFFF) / 8388608.0f - 1.0f; };
    std::vector<float> h((size_t)std::max<long>((long)std::max(M, N) * K, (long)RR * N));
    for (size_t i = 0; i < (size_t)M * K; ++i) h[i] = rnd();
    H2D(A, h.data(), (size_t)M * K * 4);
    for (size_t i = 0; i < (size_t)N * K; ++i) h[i] = rnd();
    H2D(Wt, h.data(), (size_t)N * K * 4);
    for (size_t i = 0; i < (size_t)N; ++i) h[i] = rnd();
    H2D(bias, h.data(), (size_t)N * 4);
    for (size_t i = 0; i < (size_t)RR * N; ++i) h[i] = 3.0f * rnd();
    H2D(resid, h.data(), (size_t)RR * N * 4);
    std::vector<int> rm(M);
    for (int i = 0; i < M; ++i) rm[i] = (int)(((long)i * 7919 + 13) % RR);       // a scattered, non-monotonic row map
    H2D(rows, rm.data(), (size_t)M * 4);
  }
  launch_split2h(A, K, M, K, nullptr, A3, a_pl, H2_TILE_A, nullptr, H2_ACT_SCALE, c->stream);
  launch_split2h(Wt, K, N, K, nullptr, W3, w_pl, H2_TILE_W, nullptr, 16384.0f, c->stream);
  GemmX3Args g{};
  g.A = A3; g.a_plane = a_pl; g.W = W3; g.w_plane = w_pl; g.bias = bias; g.M = M; g.N = N; g.K = K; g.ldc = N;
  g.descale = ldexpf(1.0f, -(H2_ACT_SHIFT + 14)); g.range_flag = flag;
  if (mode == 0) { g.act = ACT_RELU; g.out_plane = o_pl; }
  else { g.act = ACT_NONE; g.resid = resid; g.ldr = N; if (mode == 1) g.resid_rows = rows; }
  GemmX3Args g0 = g, g1 = g;
  if (mode == 0) { g0.out_planes = P0; g1.out_planes = P1; } else { g0.C = C0; g1.C = C1; }
  launch_gemm_f16x2(g0, c->stream, small_tiles ? -128 : 256);        // eight-wave template: 128 x 128 tiles / 256 x 256 tiles (64 x 128 per wave)
  launch_gemm_f16x2(g1, c->stream, 257);        // four waves of 128 x 128
  SYNC();
  TRY(hipGetLastError());
  int64_t bad = 0, total = 0;
  if (mode == 0) {
    // the planes are tile-major with pad rows inside the last row tile: compare the whole allocation (pads were zeroed on both sides)
    const size_t words = (size_t)2 * o_pl, chunk = (size_t)8 << 20;
    std::vector<unsigned short> h0(chunk), h1(chunk);
    for (size_t o = 0; o < words; o += chunk) {
      const size_t n = std::min(chunk, words - o);
      D2H(h0.data(), P0 + o, n * 2);
      D2H(h1.data(), P1 + o, n * 2);
      SYNC();
      for (size_t i = 0; i < n; ++i) bad += h0[i] != h1[i];
      total += (int64_t)n;
    }
  } else {
    const size_t words = (size_t)M * N, chunk = (size_t)4 << 20;
    std::vector<unsigned> h0(chunk), h1(chunk);
    for (size_t o = 0; o < words; o += chunk) {
      const size_t n = std::min(chunk, words - o);
      D2H(h0.data(), C0 + o, n * 4);
      D2H(h1.data(), C1 + o, n * 4);
      SYNC();
      for (size_t i = 0; i < n; ++i) bad += h0[i] != h1[i];
      total += (int64_t)n;
    }
  }
#undef TRY
  cleanup();
  *differing = bad;
  *compared = total;
  return VX_OK;
}

// ---- correctness entries: the product samplers / attention kernels on caller-chosen operands (no timing) ----------------------
// vx_dev_sample: case i runs in decode row i % 32 of launch i / 32 (the partials are laid out [splitk][32][npad], so the row matters).
// Every launch gets private scratch state pre-filled with the sentinels; only the fused embedding reads the context (the finalized
// AR audio embedding, position alpha, positional table and norm1 of layer 0).
// ffilt / ifilt / hist null: vx_dev_sample; else vx_dev_sample_filtered (kernel 1 only: the launch gets a row_flt record per row and
// every case's generated tokens in its gen row)
static int dev_sample_run(vx_ctx* c, int32_t n, const int32_t* cfg, const float* fcfg, const float* ffilt, const int32_t* ifilt,
                          const int32_t* hist, int32_t hist_stride, const float* partial, float* logits, int32_t* state,
                          float* sum_logp, float* emb_h, float* emb_xp) {
  if (!c) return VX_EINVAL;
  if (n <= 0 || !cfg || !fcfg || !partial || !logits || !state || !sum_logp || !emb_h || !emb_xp) FAIL(VX_EINVAL, "vx_dev_sample: null argument or n <= 0");
  if (!c->finalized) FAIL(VX_ESTATE, "vx_dev_sample: weights not finalized");
  constexpr int GS_MAX = 4096, NG_MAX = 4096, NC = VX_DEV_SAMPLE_CFG, NS = VX_DEV_SAMPLE_STATE;
  for (int i = 0; i < n; ++i) {
    const int32_t* k = cfg + (size_t)i * NC;
    const float T = fcfg[3 * i], u = fcfg[3 * i + 1];
    if ((k[0] != 0 && k[0] != 1) || (k[1] != 1 && k[1] != 2 && k[1] != 4) || (k[4] != 0 && k[4] != 1) || k[5] < 0 || k[5] > NG_MAX || k[6] < 0 ||
        k[6] + 1 >= c->pe_rows || k[8] < 0 || k[9] < 1 || k[9] > GS_MAX || !(T > 0.0f) || !(T < 3.0e38f) || !(u >= 0.0f) || !(u < 1.0f))
      FAIL(VX_EINVAL, "vx_dev_sample: case %d out of range (kernel 0/1, splitk 1/2/4, active 0/1, 0 <= n_gen <= %d, 0 <= cur_pos < %d, "
           "text_len >= 0, 1 <= gen_stride <= %d, temperature > 0, 0 <= u < 1)", i, NG_MAX, c->pe_rows - 1, GS_MAX);
    const int32_t* k0 = cfg + (size_t)(i / MB) * MB * NC;      // first case of the launch: the launch constants must agree
    const float T0 = fcfg[3 * (i / MB) * MB];
    if (k[0] != k0[0] || k[1] != k0[1] || k[9] != k0[9] ||
        (k[0] == 0 && (k[2] != k0[2] || k[3] != k0[3] || memcmp(&T, &T0, 4) != 0)))
      FAIL(VX_EINVAL, "vx_dev_sample: case %d differs from the first case of its launch in a launch constant (kernel, splitk, gen_stride; "
           "kernel 0 also top_k, temperature, force_eos_at)", i);
  }
  HIPCHK(hipSetDevice(c->dev));
  // scratch: one float block and one int block, both sized for the largest launch
  int ng_top = 0;
  for (int i = 0; i < n; ++i) ng_top = std::max(ng_top, cfg[(size_t)i * NC + 5]);
  const size_t f_part = 0, f_u = f_part + (size_t)4 * MB * PRED_NPAD, f_slp = f_u + (size_t)(ng_top + 1) * MB, f_lg = f_slp + MB,
               fh = f_lg + (size_t)MB * AR_LOGITS, fxp = fh + (size_t)MB * D_MODEL, fend = fxp + (size_t)MB * D_MODEL;
  static_assert((MB * AR_LOGITS) % 4 == 0 && (MB * PRED_NPAD) % 4 == 0, "emb_h / emb_xp take 16-byte vector stores");
  enum { I_ACT = 0, I_NGEN = MB, I_TOK = 2 * MB, I_POS = 3 * MB, I_CTX = 4 * MB, I_TLEN = 5 * MB, I_SLOT = 6 * MB, I_NACT = 7 * MB, I_META = 7 * MB + 4,
         I_SMP = I_META + 4 * MB, I_FLT = I_SMP + 4 * MB, I_GEN = I_FLT + 4 * MB };
  const size_t i_end = I_GEN + (size_t)MB * GS_MAX;
  float* df = nullptr;
  int* di = nullptr;
  auto cleanup = [&]() { if (df) (void)hipFree(df); if (di) (void)hipFree(di); };
  hipError_t he;
#define TRY(x) if ((he = (x)) != hipSuccess) { cleanup(); c->err = std::string(#x) + ": " + hipGetErrorString(he); return VX_EHIP; }
#define TRYX(x) do { if (int _e = (x)) { cleanup(); return _e; } } while (0)
  TRY(hipMalloc((void**)&df, fend * 4));
  TRY(hipMalloc((void**)&di, i_end * 4));
  const float* emb_tab = W(c, "ar_audio_embedding.word_embeddings.weight");
  const float* emb_alpha = W(c, "ar_audio_position.alpha");
  if (!emb_tab || !emb_alpha || c->ar.empty()) { cleanup(); FAIL(VX_ESTATE, "vx_dev_sample: the context has no AR embedding / layer 0"); }
  std::vector<float> hf(fend);
  std::vector<int> hi;
  for (int l0 = 0; l0 < n; l0 += MB) {
    const int nr = std::min(MB, n - l0);
    const int32_t* k0 = cfg + (size_t)l0 * NC;
    const int kernel = k0[0], splitk = k0[1], gs = k0[9];
    std::fill(hf.begin(), hf.end(), VX_DEV_SENTINEL_F);
    hi.assign(I_GEN + (size_t)MB * gs, VX_DEV_SENTINEL_I);
    int nact = 0;
    for (int b = 0; b < MB; ++b) {
      const int slot = (7 * b + 3) % MB;                        // a permutation of the launch slots: slot != row
      hi[I_SLOT + b] = slot;
      hi[I_ACT + b] = 0;                                         // rows without a case: inactive
      hi[I_NGEN + b] = hi[I_POS + b] = hi[I_CTX + b] = hi[I_TLEN + b] = 0;
      hi[I_META + 4 * slot] = b; hi[I_META + 4 * slot + 1] = 0; hi[I_META + 4 * slot + 2] = 0;
      hi[I_SMP + 4 * b] = 1; hi[I_SMP + 4 * b + 1] = 0x3F800000; hi[I_SMP + 4 * b + 2] = -1; hi[I_SMP + 4 * b + 3] = 0;
      hi[I_FLT + 4 * b] = hi[I_FLT + 4 * b + 1] = 0x3F800000; hi[I_FLT + 4 * b + 2] = hi[I_FLT + 4 * b + 3] = 0;
      hf[f_slp + b] = 0.f;
      for (int ks = 0; ks < 4; ++ks) for (int j = 0; j < PRED_NPAD; ++j) hf[f_part + ((size_t)ks * MB + b) * PRED_NPAD + j] = 0.f;
      if (b >= nr) continue;
      const int32_t* k = k0 + (size_t)b * NC;
      const float* f = fcfg + 3 * (size_t)(l0 + b);
      hi[I_ACT + b] = k[4]; hi[I_NGEN + b] = k[5]; hi[I_POS + b] = k[6]; hi[I_CTX + b] = k[7]; hi[I_TLEN + b] = k[8];
      hi[I_META + 4 * slot + 1] = k[7]; hi[I_META + 4 * slot + 2] = k[4];
      hi[I_SMP + 4 * b] = k[2]; memcpy(&hi[I_SMP + 4 * b + 1], &f[0], 4); hi[I_SMP + 4 * b + 2] = k[3];
      if (ffilt) {
        memcpy(&hi[I_FLT + 4 * b], ffilt + 2 * (size_t)(l0 + b), 8);
        hi[I_FLT + 4 * b + 2] = ifilt[2 * (size_t)(l0 + b)]; hi[I_FLT + 4 * b + 3] = ifilt[2 * (size_t)(l0 + b) + 1];
        const int nh = std::min(k[5], gs);
        if (nh) memcpy(&hi[I_GEN + (size_t)b * gs], hist + (size_t)(l0 + b) * hist_stride, (size_t)nh * 4);
      }
      hf[f_u + (size_t)k[5] * MB + b] = f[1];
      hf[f_slp + b] = f[2];
      nact += k[4];
      for (int ks = 0; ks < splitk; ++ks)
        memcpy(&hf[f_part + ((size_t)ks * MB + b) * PRED_NPAD], partial + ((size_t)(l0 + b) * 4 + ks) * AR_LOGITS, AR_LOGITS * 4);
    }
    hi[I_NACT] = nact;
    TRYX(xfer_h2d(c, df, hf.data(), fend * 4));
    TRYX(xfer_h2d(c, di, hi.data(), hi.size() * 4));
    bool ok;
    if (kernel == 0) {
      SampleArgs a{};
      a.partial = df + f_part; a.splitk = splitk; a.npad = PRED_NPAD;
      a.top_k = k0[2]; a.temperature = fcfg[3 * (size_t)l0]; a.force_eos_at = k0[3];
      a.uniforms = df + f_u; a.uniforms_stride = MB; a.seed_dev = c->seed_dev; a.commit = 1;
      a.cur_tok = di + I_TOK; a.cur_pos = di + I_POS; a.ctx_len = di + I_CTX; a.n_gen = di + I_NGEN; a.active = di + I_ACT;
      a.n_active = di + I_NACT; a.text_len = di + I_TLEN; a.slot_meta = di + I_META; a.slot_of = di + I_SLOT;
      a.gen = di + I_GEN; a.gen_stride = gs; a.logits_out = df + f_lg; a.sum_logp = df + f_slp; a.batch = MB;
      a.emb_tab = emb_tab; a.emb_alpha = emb_alpha; a.pe = c->pe; a.ln_g = c->ar[0].n1_w; a.ln_b = c->ar[0].n1_b;
      a.emb_h = df + fh; a.emb_xp = df + fxp; a.wt = 1;
      ok = launch_dec_sample(a, c->stream);
    } else {
      ServeSampleArgs a{};
      a.partial = df + f_part; a.splitk = splitk; a.npad = PRED_NPAD; a.row_smp = di + I_SMP;
      a.row_flt = ffilt ? di + I_FLT : nullptr;
      a.uniforms = df + f_u; a.uniforms_stride = MB;
      a.cur_tok = di + I_TOK; a.cur_pos = di + I_POS; a.ctx_len = di + I_CTX; a.n_gen = di + I_NGEN; a.active = di + I_ACT;
      a.n_active = di + I_NACT; a.text_len = di + I_TLEN; a.slot_meta = di + I_META; a.slot_of = di + I_SLOT;
      a.gen = di + I_GEN; a.gen_stride = gs; a.sum_logp = df + f_slp; a.batch = MB;
      a.emb_tab = emb_tab; a.emb_alpha = emb_alpha; a.pe = c->pe; a.ln_g = c->ar[0].n1_w; a.ln_b = c->ar[0].n1_b;
      a.emb_h = df + fh; a.emb_xp = df + fxp; a.wt = 1;
      ok = launch_serve_sample(a, c->stream);
    }
    if (!ok) { cleanup(); FAIL(VX_EINVAL, "vx_dev_sample: split-K factor not compiled in"); }
    std::vector<float> of(fend);
    std::vector<int> oi(hi.size());
    TRYX(xfer_d2h(c, of.data(), df, fend * 4));
    TRYX(xfer_d2h(c, oi.data(), di, oi.size() * 4));
    TRYX(xfer_sync(c));
    TRY(hipGetLastError());
    for (int b = 0; b < nr; ++b) {
      const size_t i = (size_t)l0 + b;
      const int slot = (7 * b + 3) % MB, ng0 = k0[(size_t)b * NC + 5];
      int32_t* st = state + i * NS;
      st[0] = oi[I_ACT + b]; st[1] = oi[I_NGEN + b]; st[2] = oi[I_TOK + b]; st[3] = oi[I_POS + b]; st[4] = oi[I_CTX + b];
      for (int w = 0; w < 4; ++w) st[5 + w] = oi[I_META + 4 * slot + w];
      st[9] = ng0 < gs ? oi[I_GEN + (size_t)b * gs + ng0] : VX_DEV_SENTINEL_I;
      st[10] = oi[I_NACT];
      st[11] = slot;
      sum_logp[i] = of[f_slp + b];
      memcpy(logits + i * AR_LOGITS, &of[f_lg + (size_t)b * AR_LOGITS], AR_LOGITS * 4);
      memcpy(emb_h + i * D_MODEL, &of[fh + (size_t)b * D_MODEL], D_MODEL * 4);
      // the packed-x image (decode.hip ln_pack_row): float4 column c4 of decode row b lives at ((c4 >> 1) * 64 + b + 32 * (c4 & 1)) * 4
      for (int c4 = 0; c4 < D_MODEL / 4; ++c4)
        memcpy(emb_xp + i * D_MODEL + 4 * c4, &of[fxp + (((size_t)(c4 >> 1) * 64) + b + 32 * (c4 & 1)) * 4], 16);
    }
  }
#undef TRY
#undef TRYX
  cleanup();
  return VX_OK;
}

int vx_dev_sample(vx_ctx* c, int32_t n, const int32_t* cfg, const float* fcfg, const float* partial, float* logits, int32_t* state,
                  float* sum_logp, float* emb_h, float* emb_xp) {
  return dev_sample_run(c, n, cfg, fcfg, nullptr, nullptr, nullptr, 0, partial, logits, state, sum_logp, emb_h, emb_xp);
}

int vx_dev_sample_filtered(vx_ctx* c, int32_t n, const int32_t* cfg, const float* fcfg, const float* ffilt, const int32_t* ifilt,
                           const int32_t* hist, int32_t hist_stride, const float* partial, float* logits, int32_t* state,
                           float* sum_logp, float* emb_h, float* emb_xp) {
  if (!c) return VX_EINVAL;
  if (n <= 0 || !cfg || !ffilt || !ifilt || hist_stride < 0) FAIL(VX_EINVAL, "vx_dev_sample_filtered: null argument, n <= 0 or hist_stride < 0");
  for (int i = 0; i < n; ++i) {
    const int32_t* k = cfg + (size_t)i * VX_DEV_SAMPLE_CFG;
    const float tp = ffilt[2 * i], rp = ffilt[2 * i + 1];
    if (k[0] != 1) FAIL(VX_EINVAL, "vx_dev_sample_filtered: case %d: kernel must be 1 (serve_sample_kernel)", i);
    if (!(tp > 0.0f) || !(tp <= 1.0f) || !(rp > 0.0f) || !(rp < 3.0e38f) || ifilt[2 * i] < 0 || ifilt[2 * i + 1] < 0)
      FAIL(VX_EINVAL, "vx_dev_sample_filtered: case %d out of range (0 < top_p <= 1, repetition_penalty > 0 and finite, "
           "repetition_window >= 0, min_frames >= 0)", i);
    const int nh = k[5] < k[9] ? k[5] : k[9];
    if (nh > 0 && (!hist || nh > hist_stride))
      FAIL(VX_EINVAL, "vx_dev_sample_filtered: case %d has %d generated tokens, hist holds %d per case", i, nh, hist_stride);
  }
  return dev_sample_run(c, n, cfg, fcfg, ffilt, ifilt, hist, hist_stride, partial, logits, state, sum_logp, emb_h, emb_xp);
}

// vx_dev_attn: one launch of a full-sequence attention kernel on the caller's packed q|k|v rows; seq_off / c_off are derived here.
int vx_dev_attn(vx_ctx* c, int32_t variant, int32_t planes, int32_t batch, const float* qkv, const int32_t* seq_len,
                const int32_t* prefix_len, const int32_t* q_first, float* out, int64_t out_rows, int32_t* range_flag) {
  if (!c) return VX_EINVAL;
  if (!qkv || !seq_len || !out || batch <= 0 || batch > 256) FAIL(VX_EINVAL, "vx_dev_attn: null argument or batch outside 1 .. 256");
  if ((variant != 0 && variant != 10 && variant != 20) || (planes != 0 && planes != 1) || (planes && variant == 0))
    FAIL(VX_EINVAL, "vx_dev_attn: variant must be 0, 10 or 20; planes 0 or 1 (1: variants 10 and 20)");
  if (q_first && !((variant == 0 && !planes) || (variant == 20 && planes)))
    FAIL(VX_EINVAL, "vx_dev_attn: q_first goes with variant 0 (fp32 rows) or variant 20 with planes: the launchers that trim");
  std::vector<int> meta(5 * (size_t)batch, 0);          // seq_off | seq_len | prefix_len | q_first | c_off
  long M = 0, rows = 0;
  int max_len = 0;
  for (int b = 0; b < batch; ++b) {
    const int len = seq_len[b];
    if (len <= 0 || len > 65536 || (prefix_len && (prefix_len[b] < 0 || prefix_len[b] > len)) || (q_first && (q_first[b] < 0 || q_first[b] > len)))
      FAIL(VX_EINVAL, "vx_dev_attn: sequence %d: 1 <= len <= 65536, 0 <= prefix_len <= len, 0 <= q_first <= len", b);
    meta[b] = (int)M; meta[batch + b] = len;
    meta[2 * batch + b] = prefix_len ? prefix_len[b] : 0;
    meta[3 * batch + b] = q_first ? q_first[b] : 0;
    meta[4 * batch + b] = (int)rows;
    M += len; rows += len - (q_first ? q_first[b] : 0);
    max_len = std::max(max_len, len);
    if (M > (1 << 20)) FAIL(VX_EINVAL, "vx_dev_attn: more than 2^20 rows");
  }
  if (out_rows < rows || out_rows > rows + 4096) FAIL(VX_EINVAL, "vx_dev_attn: out_rows must be %ld .. %ld", rows, rows + 4096);
  HIPCHK(hipSetDevice(c->dev));
  const long pstride = h2_plane(out_rows, D_MODEL, H2_TILE_A);
  float *dq = nullptr, *dout = nullptr;
  unsigned short* dpl = nullptr;
  int* dmeta = nullptr;
  auto cleanup = [&]() { for (void* p : {(void*)dq, (void*)dout, (void*)dpl, (void*)dmeta}) if (p) (void)hipFree(p); };
  hipError_t he;
#define TRY(x) if ((he = (x)) != hipSuccess) { cleanup(); c->err = std::string(#x) + ": " + hipGetErrorString(he); return VX_EHIP; }
#define TRYX(x) do { if (int _e = (x)) { cleanup(); return _e; } } while (0)
  TRY(hipMalloc((void**)&dq, (size_t)M * 3 * D_MODEL * 4));
  TRY(hipMalloc((void**)&dmeta, (meta.size() + 4) * 4));
  meta.resize(meta.size() + 4, 0);                                 // + the range flag, zero
  int* dflag = dmeta + 5 * (size_t)batch;
  TRYX(xfer_h2d(c, dq, qkv, (size_t)M * 3 * D_MODEL * 4));
  TRYX(xfer_h2d(c, dmeta, meta.data(), meta.size() * 4));
  if (planes) {
    TRY(hipMalloc((void**)&dpl, (size_t)2 * pstride * 2));
    std::vector<unsigned short> fill((size_t)2 * pstride, VX_DEV_SENTINEL_H);
    TRYX(xfer_h2d(c, dpl, fill.data(), fill.size() * 2));
  } else {
    TRY(hipMalloc((void**)&dout, (size_t)out_rows * D_MODEL * 4));
    std::vector<float> fill((size_t)out_rows * D_MODEL, VX_DEV_SENTINEL_F);
    TRYX(xfer_h2d(c, dout, fill.data(), fill.size() * 4));
  }
  const int *d_off = dmeta, *d_len = dmeta + batch, *d_pre = prefix_len ? dmeta + 2 * batch : nullptr,
            *d_qf = q_first ? dmeta + 3 * batch : nullptr, *d_co = q_first ? dmeta + 4 * batch : nullptr;
  if (variant == 0) launch_attn_full(dq, dout, d_off, d_len, d_pre, batch, max_len, c->stream, d_qf, d_co);
  else if (variant == 10) launch_attn_full_x3(dq, dout, d_off, d_len, d_pre, batch, max_len, 0, c->stream, dpl, pstride);
  else launch_attn_full_h2(dq, dout, d_off, d_len, d_pre, batch, max_len, c->stream, dpl, pstride, dflag, -1, d_qf, d_co);
  int flag = 0;
  std::vector<unsigned short> hp(planes ? (size_t)2 * pstride : 0);
  if (!planes) TRYX(xfer_d2h(c, out, dout, (size_t)out_rows * D_MODEL * 4));
  else TRYX(xfer_d2h(c, hp.data(), dpl, hp.size() * 2));
  TRYX(xfer_d2h(c, &flag, dflag, 4));
  TRYX(xfer_sync(c));
  if (planes) {
    // f16x2 A planes of out_proj (vx_common.h): tile-major [rows / 256][K / 32][256][32], x * 2^5 = head + tail
    for (long r = 0; r < out_rows; ++r)
      for (int col = 0; col < D_MODEL; ++col) {
        const size_t idx = ((((size_t)(r >> 8) * (D_MODEL / 32)) + (col >> 5)) * 256 + (r & 255)) * 32 + (col & 31);
        const unsigned short hh = hp[idx], tt = hp[idx + pstride];
        _Float16 fh_, ft_;
        memcpy(&fh_, &hh, 2); memcpy(&ft_, &tt, 2);
        out[(size_t)r * D_MODEL + col] = (hh == VX_DEV_SENTINEL_H && tt == VX_DEV_SENTINEL_H) ? VX_DEV_SENTINEL_F
                                                                                               : ((float)fh_ + (float)ft_) * (1.0f / H2_ACT_SCALE);
      }
  }
  TRY(hipGetLastError());
  if (range_flag) *range_flag = flag;
#undef TRY
#undef TRYX
  cleanup();
  return VX_OK;
}

// vx_dev_gemm_levers: the request-order / block-mapping switches of the decode GEMMs (weights.hip), in the header's order
int vx_dev_gemm_levers(vx_ctx* c, int32_t* out, int32_t n) {
  if (!c) return VX_EINVAL;
  if (!out || n < VX_DEV_GEMM_LEVERS) FAIL(VX_EINVAL, "vx_dev_gemm_levers: out must hold %d words", VX_DEV_GEMM_LEVERS);
  if (!c->finalized) FAIL(VX_ESTATE, "vx_dev_gemm_levers: weights not finalized");
  out[0] = c->l2_kmap;
  out[1] = c->l1_interleave;
  return VX_OK;
}

// vx_dev_switches: the kernel-selection fields finalize_weights read (weights.hip), in the order include/vallex_hip_dev.h documents
int vx_dev_switches(vx_ctx* c, int32_t* out, int32_t n) {
  if (!c) return VX_EINVAL;
  if (!out || n < VX_DEV_SWITCHES) FAIL(VX_EINVAL, "vx_dev_switches: out must hold %d words", VX_DEV_SWITCHES);
  if (!c->finalized) FAIL(VX_ESTATE, "vx_dev_switches: weights not finalized");
  const int32_t v[VX_DEV_SWITCHES] = {c->sb_fuse, c->sb_qkv_rows, c->sb_qkv_nsplit, c->qkv_bal, c->fuse_out, c->fuse_split, c->att_nsplit_force,
                                      c->balance_rows, c->nar_trim, c->graph_multi, c->gemm_mode, c->attn_x3, c->attn_h2, c->Tmax};
  memcpy(out, v, sizeof v);
  return VX_OK;
}

// vx_dev_dec_attn: the attention block of ONE decode step of layer 0 on caller-chosen operands -- the launch sequence of ar_step_launches
// from the attention launch to the launch behind which the out_proj result exists, with the geometry decode_geometry picks for `nrows`
// under the context's switches (every chain of ar_step_launches: sb_qkv, the small-batch chain without the fused QKV, and the general one).
// Everything the launches touch is private scratch pre-filled with the sentinels (the K / V arena included: [nrows slots][16][Tmax][64]);
// the context only lends its layer-0 weights and its geometry switches, and the four geometry fields decode_geometry sets are put
// back, so the decode state of the context is not touched.
int vx_dev_dec_attn(vx_ctx* c, int32_t nrows, int32_t Tmax, int32_t qkv_balanced, int32_t skp, const int32_t* ctx_len,
                    const int32_t* active, const int32_t* slot_order, float* kc, float* vc, const float* qkv, const float* x_in,
                    const float* resid, float* out, float* xp_att, float* part_ml, int32_t* geom) {
  if (!c) return VX_EINVAL;
  if (!ctx_len || !active || !slot_order || !kc || !vc || !out || !xp_att || !part_ml || !geom)
    FAIL(VX_EINVAL, "vx_dev_dec_attn: null argument");
  if (c->serve) FAIL(VX_ESTATE, "vx_dev_dec_attn: a serving session is open on this context (vx_serve_close it first)");
  if (!c->finalized || c->ar.empty()) FAIL(VX_ESTATE, "vx_dev_dec_attn: weights not finalized");
  if (nrows < 1 || nrows > MB) FAIL(VX_EINVAL, "vx_dev_dec_attn: nrows must be 1 .. %d", MB);
  if (Tmax < DEC_ATTN_TILE || Tmax > 4096) FAIL(VX_EINVAL, "vx_dev_dec_attn: Tmax must be %d .. 4096", DEC_ATTN_TILE);
  if (skp != 0 && skp != SK_L2) FAIL(VX_EINVAL, "vx_dev_dec_attn: skp must be 0 or %d", SK_L2);
  bool identity = true;
  {
    unsigned seen = 0;
    for (int y = 0; y < nrows; ++y) {
      const int r = slot_order[y];
      if (r < 0 || r >= nrows || (seen >> r & 1u)) FAIL(VX_EINVAL, "vx_dev_dec_attn: slot_order is not a permutation of 0 .. %d", nrows - 1);
      seen |= 1u << r;
      identity = identity && r == y;
    }
  }
  if (nrows <= SB_ROWS && !identity) FAIL(VX_EINVAL, "vx_dev_dec_attn: up to %d rows the slot order must be the identity", SB_ROWS);
  for (int r = 0; r < nrows; ++r) {
    if (ctx_len[r] < 1 || ctx_len[r] > Tmax) FAIL(VX_EINVAL, "vx_dev_dec_attn: row %d: the context (%d) must be 1 .. Tmax = %d", r, ctx_len[r], Tmax);
    if (active[r] != 0 && active[r] != 1) FAIL(VX_EINVAL, "vx_dev_dec_attn: row %d: active must be 0 or 1", r);
  }
  // the product's own rule; the context's geometry fields are put back below (a later ar_prefill / vx_serve_open sets its own anyway)
  const int k_nsplit = c->nsplit;
  const bool k_sf = c->split_fused, k_sbc = c->sb_chain, k_sbq = c->sb_qkv;
  decode_geometry(c, nrows, identity);
  const int nsplit = c->nsplit;
  const bool split_fused = c->split_fused, sb_chain = c->sb_chain, sb_qkv = c->sb_qkv;
  c->nsplit = k_nsplit; c->split_fused = k_sf; c->sb_chain = k_sbc; c->sb_qkv = k_sbq;
  geom[0] = nsplit; geom[1] = sb_qkv; geom[2] = split_fused; geom[3] = sb_chain;
  const bool sb_plain = sb_chain && !sb_qkv;                              // QKV GEMM | dec_attn partials | out_proj with the combine as prologue
  const bool fused = !sb_chain && c->fuse_out && (nsplit == 1 || split_fused);
  if (sb_qkv ? !x_in : (!qkv || (!resid && !sb_plain)))
    FAIL(VX_EINVAL, "vx_dev_dec_attn: %s", sb_qkv ? "this chain reads x_in" : sb_plain ? "this chain reads qkv" : "this chain reads qkv and resid");
  if (sb_plain && qkv_balanced) FAIL(VX_EINVAL, "vx_dev_dec_attn: the small-batch chain without the fused QKV reads four in_proj slabs, not the balanced layout");
  const LayerW& L = c->ar[0];
  if (fused && !L.out_wh) FAIL(VX_ESTATE, "vx_dev_dec_attn: the context has no head-major W_o");
  if ((split_fused && nsplit > 4) || nsplit > 16) FAIL(VX_ESTATE, "vx_dev_dec_attn: %d context splits exceed the scratch slabs", nsplit);
  HIPCHK(hipSetDevice(c->dev));

  constexpr int d = D_MODEL, NP = 3 * D_MODEL, NPART = 17;                 // NPART: partials per (row, head) of the scratch, >= nsplit + 1
  const size_t stream_w = (size_t)N_HEAD * Tmax * D_HEAD, arena = (size_t)nrows * stream_w;
  const size_t f_qkv = 0, f_xp = f_qkv + (size_t)SK_QKV_BAL_Q * MB * NP, f_xpa = f_xp + (size_t)MB * d, f_po = f_xpa + (size_t)MB * d,
               f_poh = f_po + (size_t)SK_L2 * MB * d, f_pto = f_poh + (size_t)4 * N_HEAD * MB * d, f_pml = f_pto + (size_t)MB * N_HEAD * NPART * D_HEAD,
               f_qkn = f_pml + (size_t)MB * N_HEAD * NPART * 2, f_dh = f_qkn + (size_t)MB * N_HEAD * 2 * D_HEAD, f_dh2 = f_dh + (size_t)MB * d,
               fend = f_dh2 + (size_t)MB * d;
  static_assert(SK_OUT <= SK_L2 && SK_QKV <= SK_QKV_BAL_Q, "p_o / p_qkv scratch is sized by the larger slab count");
  float *dk = nullptr, *dv = nullptr, *df = nullptr;
  int* di = nullptr;                                                       // slot_meta [MB][4] | active [MB]
  auto cleanup = [&]() { for (void* p : {(void*)dk, (void*)dv, (void*)df, (void*)di}) if (p) (void)hipFree(p); };
  hipError_t he;
#define TRY(x) if ((he = (x)) != hipSuccess) { cleanup(); c->err = std::string(#x) + ": " + hipGetErrorString(he); return VX_EHIP; }
#define TRYX(x) do { if (int _e = (x)) { cleanup(); return _e; } } while (0)
  TRY(hipMalloc((void**)&dk, arena * 4));
  TRY(hipMalloc((void**)&dv, arena * 4));
  TRY(hipMalloc((void**)&df, fend * 4));
  TRY(hipMalloc((void**)&di, (size_t)5 * MB * 4));
  std::vector<int> slot_of(nrows);
  for (int y = 0; y < nrows; ++y) slot_of[slot_order[y]] = y;
  {
    std::vector<float> hf(fend, VX_DEV_SENTINEL_F);
    for (int r = 0; r < nrows; ++r) {
      if (!sb_qkv) {
        const int slabs = qkv_balanced ? SK_QKV_BAL_Q : SK_QKV;
        for (int ks = 0; ks < slabs; ++ks) memcpy(&hf[f_qkv + ((size_t)ks * MB + r) * NP], qkv + ((size_t)ks * nrows + r) * NP, NP * 4);
        if (resid) memcpy(&hf[f_dh + (size_t)r * d], resid + (size_t)r * d, d * 4);
      } else if (skp == 0) {
        // the packed-x image (decode.hip ln_pack_row): float4 column c4 of row r at ((c4 >> 1) * 64 + r + 32 * (c4 & 1)) * 4
        for (int c4 = 0; c4 < d / 4; ++c4) memcpy(&hf[f_xp + (((size_t)(c4 >> 1) * 64) + r + 32 * (c4 & 1)) * 4], x_in + (size_t)r * d + 4 * c4, 16);
      } else {
        for (int ks = 0; ks < SK_L2; ++ks) memcpy(&hf[f_po + ((size_t)ks * MB + r) * d], x_in + ((size_t)ks * nrows + r) * d, d * 4);
        memcpy(&hf[f_dh + (size_t)r * d], x_in + ((size_t)SK_L2 * nrows + r) * d, d * 4);
      }
    }
    std::vector<int> hi(5 * MB, 0);
    for (int y = 0; y < nrows; ++y) {
      const int r = slot_order[y];
      hi[4 * y] = r; hi[4 * y + 1] = ctx_len[r]; hi[4 * y + 2] = active[r];
      hi[4 * MB + r] = active[r];
    }
    TRYX(xfer_h2d(c, df, hf.data(), fend * 4));
    TRYX(xfer_h2d(c, di, hi.data(), hi.size() * 4));
    for (int r = 0; r < nrows; ++r) {
      TRYX(xfer_h2d(c, dk + (size_t)slot_of[r] * stream_w, kc + (size_t)r * stream_w, stream_w * 4));
      TRYX(xfer_h2d(c, dv + (size_t)slot_of[r] * stream_w, vc + (size_t)r * stream_w, stream_w * 4));
    }
  }
  const int* d_meta = di;
  const int* d_active = di + 4 * MB;
  float *p_qkv = df + f_qkv, *xp = df + f_xp, *xpa = df + f_xpa, *p_o = df + f_po, *p_oh = df + f_poh, *pt_o = df + f_pto, *pt_ml = df + f_pml,
        *qk_new = df + f_qkn, *dh = df + f_dh, *dh2 = df + f_dh2;
  hipStream_t st = c->stream;
  bool ok = true;
  if (sb_qkv) {
    ok = launch_dec_attn_qkv(L.in_w, L.in_b, dk, dv, Tmax, d_meta, pt_o, pt_ml, qk_new, nsplit, nrows, skp ? p_o : nullptr, skp,
                             skp ? L.l2_b : nullptr, dh, dh2, L.n1_w, L.n1_b, xp, st);
    ok = ok && launch_skinny_gemm_sb_combine(L.out_wp, p_o, D_MODEL, SK_OUT, pt_o, pt_ml, nsplit + 1, nrows, st, qk_new);
  } else if (sb_plain) {
    // the engine's layer-0 sequence of this chain behind its QKV GEMM (ar_step_launches): the unfused kernel's nsplit partials, no qk_new
    ok = launch_dec_attn(p_qkv, SK_QKV, L.in_b, dk, dv, Tmax, d_meta, xpa, pt_o, pt_ml, nsplit, nrows, nullptr, p_oh, st);
    ok = ok && launch_skinny_gemm_sb_combine(L.out_wp, p_o, D_MODEL, SK_OUT, pt_o, pt_ml, nsplit, nrows, st, nullptr);
  } else if (!launch_dec_attn(p_qkv, qkv_balanced ? SK_QKV_BALANCED : SK_QKV, L.in_b, dk, dv, Tmax, d_meta, xpa, pt_o, pt_ml, nsplit, nrows,
                              fused ? L.out_wh : nullptr, p_oh, st)) {
    ok = false;
  } else if (fused && nsplit > 1) {
    ok = launch_dec_reduce_ln_split(p_oh, pt_ml, nsplit, L.out_b, dh, dh, L.n2_w, L.n2_b, xp, nrows, st);
  } else if (fused) {
    launch_dec_reduce_ln_pack(p_oh, N_HEAD, D_MODEL, L.out_b, dh, dh, L.n2_w, L.n2_b, xp, nrows, st);
  } else {
    if (nsplit > 1) launch_dec_attn_combine(pt_o, pt_ml, nsplit, d_active, xpa, nrows, st);
    launch_skinny_gemm(L.out_wp, xpa, p_o, D_MODEL, D_MODEL, SK_OUT, st, true);
    launch_dec_reduce_ln_pack(p_o, SK_OUT, D_MODEL, L.out_b, dh, dh, L.n2_w, L.n2_b, xp, nrows, st);
  }
  if (!ok) {
    (void)hipStreamSynchronize(st);
    cleanup();
    FAIL(VX_EINVAL, "vx_dev_dec_attn: a launcher refused this configuration (%d rows, %d splits)", nrows, nsplit);
  }
  std::vector<float> of(fend);
  TRYX(xfer_d2h(c, of.data(), df, fend * 4));
  for (int r = 0; r < nrows; ++r) {
    TRYX(xfer_d2h(c, kc + (size_t)r * stream_w, dk + (size_t)slot_of[r] * stream_w, stream_w * 4));
    TRYX(xfer_d2h(c, vc + (size_t)r * stream_w, dv + (size_t)slot_of[r] * stream_w, stream_w * 4));
  }
  TRYX(xfer_sync(c));
  TRY(hipGetLastError());
  // outputs, indexed by row.  out [SK_OUT][nrows][1024]: the out_proj slabs of the small-batch chains; the other chains: out[0] = h
  const int np = sb_qkv ? nsplit + 1 : nsplit;
  for (size_t i = 0; i < (size_t)SK_OUT * nrows * d; ++i) out[i] = VX_DEV_SENTINEL_F;
  for (size_t i = 0; i < (size_t)nrows * N_HEAD * NPART * 2; ++i) part_ml[i] = VX_DEV_SENTINEL_F;
  for (int r = 0; r < nrows; ++r) {
    if (sb_chain)
      for (int ks = 0; ks < SK_OUT; ++ks) memcpy(out + ((size_t)ks * nrows + r) * d, &of[f_po + ((size_t)ks * MB + r) * d], d * 4);
    else memcpy(out + (size_t)r * d, &of[f_dh + (size_t)r * d], d * 4);
    for (int c4 = 0; c4 < d / 4; ++c4) memcpy(xp_att + (size_t)r * d + 4 * c4, &of[f_xpa + (((size_t)(c4 >> 1) * 64) + r + 32 * (c4 & 1)) * 4], 16);
    for (int h = 0; h < N_HEAD; ++h)
      memcpy(part_ml + ((size_t)(r * N_HEAD + h) * NPART) * 2, &of[f_pml + ((size_t)(r * N_HEAD + h) * np) * 2], (size_t)np * 2 * 4);
  }
#undef TRY
#undef TRYX
  cleanup();
  return VX_OK;
}

// vx_dev_dec_op: ONE launch of the other half of ar_step_launches -- the skinny GEMMs, linear1, the reduce + LayerNorm kernels, their
// small-batch consumers and the teacher-forced embedding -- through the product launcher, on caller-chosen activations.  The weights
// are the context's own device images (in_wp / out_wp / l1_wp / l2_wp / pred_wp, biases, norms): what pack_weight_kernel and
// pack_weight16_kernel wrote at load time is what the launch reads.  Split counts and the write-through rule are the engine's.
// Everything the launch reads or writes besides the weights is private scratch pre-filled with the sentinel.
int vx_dev_dec_op(vx_ctx* c, int32_t op, int32_t variant, int32_t layer, int32_t nrows, const int32_t* tok, const int32_t* pos,
                  const float* x, const float* slabs, float* resid, float* out, float* h, float* xp) {
  if (!c) return VX_EINVAL;
  if (c->serve) FAIL(VX_ESTATE, "vx_dev_dec_op: a serving session is open on this context (vx_serve_close it first)");
  if (!c->finalized || c->ar.empty()) FAIL(VX_ESTATE, "vx_dev_dec_op: weights not finalized");
  if (op < VX_DEV_OP_EMBED || op > VX_DEV_OP_SB_LINEAR1) FAIL(VX_EINVAL, "vx_dev_dec_op: unknown op %d", op);
  if (nrows < 1 || nrows > MB) FAIL(VX_EINVAL, "vx_dev_dec_op: nrows must be 1 .. %d", MB);
  const int NL = (int)c->ar.size();
  if (layer < 0 || layer >= NL) FAIL(VX_EINVAL, "vx_dev_dec_op: layer must be 0 .. %d", NL - 1);
  const bool sb = op == VX_DEV_OP_SB_LN_GEMM || op == VX_DEV_OP_SB_LINEAR1;
  if (sb && nrows > SB_ROWS) FAIL(VX_EINVAL, "vx_dev_dec_op: the small-batch ops take at most %d rows", SB_ROWS);
  const LayerW& L = c->ar[layer];
  const float *fin_g = W(c, "ar_decoder.norm.weight"), *fin_b = W(c, "ar_decoder.norm.bias");
  const float* emb_tab = W(c, "ar_audio_embedding.word_embeddings.weight");
  const float* emb_alpha = W(c, "ar_audio_position.alpha");
  if (!fin_g || !fin_b || !emb_tab || !emb_alpha || !c->pred_wp || !c->pe) FAIL(VX_ESTATE, "vx_dev_dec_op: the context has no AR decoder");
  constexpr int d = D_MODEL;
  // the GEMM role: weight image, padded columns, K, K slices of the output
  const float* wp = nullptr;
  int Npad = 0, K = d, sk = 0;
  if (op == VX_DEV_OP_GEMM || op == VX_DEV_OP_SB_LN_GEMM) {
    if (variant == VX_DEV_W_IN) { wp = L.in_wp; Npad = 3 * d; sk = SK_QKV; }
    else if (variant == VX_DEV_W_OUT) { wp = L.out_wp; Npad = d; sk = SK_OUT; }
    else if (variant == VX_DEV_W_L2) { wp = L.l2_wp; Npad = d; K = D_FF; sk = SK_L2; }
    else if (variant == VX_DEV_W_PRED) { wp = c->pred_wp; Npad = PRED_NPAD; sk = SK_PRED; }
    else FAIL(VX_EINVAL, "vx_dev_dec_op: unknown weight %d (0 in_proj, 1 out_proj, 2 linear2, 3 predict)", variant);
    if (op == VX_DEV_OP_SB_LN_GEMM) {
      if (variant != VX_DEV_W_IN && variant != VX_DEV_W_PRED) FAIL(VX_EINVAL, "vx_dev_dec_op: sb_ln_gemm runs in_proj or predict");
      if (variant == VX_DEV_W_IN && layer == 0) FAIL(VX_EINVAL, "vx_dev_dec_op: in_proj of layer 0 has no linear2 slabs in front of it");
      if (variant == VX_DEV_W_PRED && layer != NL - 1) FAIL(VX_EINVAL, "vx_dev_dec_op: predict follows the last layer (%d)", NL - 1);
    }
  } else if (op == VX_DEV_OP_REDUCE_LN) {
    if (variant != 0 && variant != SK_OUT && variant != SK_L2 && variant != N_HEAD)
      FAIL(VX_EINVAL, "vx_dev_dec_op: reduce_ln takes 0, %d, %d or %d slabs", SK_OUT, SK_L2, N_HEAD);
  } else if (variant != 0) {
    FAIL(VX_EINVAL, "vx_dev_dec_op: op %d has no variant %d", op, variant);
  }
  if (op == VX_DEV_OP_QKV_BAL) { wp = L.in_wp; Npad = 3 * d; sk = SK_QKV_BAL_Q; }
  if (op == VX_DEV_OP_LINEAR1 || op == VX_DEV_OP_SB_LINEAR1) wp = L.l1_wp;
  const int sk_in = op == VX_DEV_OP_REDUCE_LN ? variant : op == VX_DEV_OP_SB_LN_GEMM ? SK_L2 : op == VX_DEV_OP_SB_LINEAR1 ? SK_OUT : 0;
  const bool reads_x = op == VX_DEV_OP_GEMM || op == VX_DEV_OP_QKV_BAL || op == VX_DEV_OP_LINEAR1;
  const bool reads_resid = op == VX_DEV_OP_REDUCE_LN || sb;
  const bool writes_out = op != VX_DEV_OP_EMBED && op != VX_DEV_OP_REDUCE_LN;
  const bool writes_h = op == VX_DEV_OP_EMBED || reads_resid;
  const bool writes_xp = op == VX_DEV_OP_EMBED || op == VX_DEV_OP_REDUCE_LN;
  if ((op == VX_DEV_OP_EMBED && (!tok || !pos)) || (reads_x && !x) || (sk_in && !slabs) || (reads_resid && !resid) || (writes_out && !out) ||
      (writes_h && !h) || (writes_xp && !xp))
    FAIL(VX_EINVAL, "vx_dev_dec_op: op %d: null argument", op);
  if (wp == nullptr && (reads_x || sb)) FAIL(VX_ESTATE, "vx_dev_dec_op: the context has no packed image of this weight");
  if (op == VX_DEV_OP_EMBED) {
    const auto it = c->w.find("ar_audio_embedding.word_embeddings.weight");
    const long emb_rows = it->second.shape.empty() ? 0 : (long)it->second.shape[0];
    for (int r = 0; r < nrows; ++r)
      if (tok[r] < 0 || tok[r] >= emb_rows || pos[r] < 0 || pos[r] >= c->pe_rows)
        FAIL(VX_EINVAL, "vx_dev_dec_op: row %d: tok must be 0 .. %ld, pos 0 .. %d", r, emb_rows - 1, c->pe_rows - 1);
  }
  HIPCHK(hipSetDevice(c->dev));

  static_assert(SK_OUT <= N_HEAD && SK_L2 <= N_HEAD, "the slab scratch holds N_HEAD slabs");
  static_assert(SK_QKV_BAL_Q * 3 * D_MODEL >= D_FF && SK_QKV_BAL_Q * 3 * D_MODEL >= SK_L2 * D_MODEL && SK_QKV_BAL_Q * 3 * D_MODEL >= SK_PRED * PRED_NPAD &&
                SK_QKV_BAL_Q >= SK_QKV, "the output scratch is sized by the balanced in_proj");
  const size_t f_x = 0, f_sl = f_x + (size_t)MB * D_FF, f_out = f_sl + (size_t)N_HEAD * MB * d, f_dh = f_out + (size_t)SK_QKV_BAL_Q * MB * 3 * d,
               f_dh2 = f_dh + (size_t)MB * d, f_xp = f_dh2 + (size_t)MB * d, fend = f_xp + (size_t)MB * d;
  float* df = nullptr;
  int* di = nullptr;                                                       // tok [MB] | pos [MB]
  auto cleanup = [&]() { if (df) (void)hipFree(df); if (di) (void)hipFree(di); };
  hipError_t he;
#define TRY(x) if ((he = (x)) != hipSuccess) { cleanup(); c->err = std::string(#x) + ": " + hipGetErrorString(he); return VX_EHIP; }
#define TRYX(x) do { if (int _e = (x)) { cleanup(); return _e; } } while (0)
  TRY(hipMalloc((void**)&df, fend * 4));
  TRY(hipMalloc((void**)&di, (size_t)2 * MB * 4));
  {
    std::vector<float> hf(fend, VX_DEV_SENTINEL_F);
    std::vector<int> hi(2 * MB, 0);
    if (reads_x) dev_pack_image(&hf[f_x], x, K);
    if (sk_in) memcpy(&hf[f_sl], slabs, (size_t)sk_in * MB * d * 4);
    if (reads_resid) memcpy(&hf[f_dh], resid, (size_t)nrows * d * 4);
    if (op == VX_DEV_OP_EMBED) for (int r = 0; r < nrows; ++r) { hi[r] = tok[r]; hi[MB + r] = pos[r]; }
    TRYX(xfer_h2d(c, df, hf.data(), fend * 4));
    TRYX(xfer_h2d(c, di, hi.data(), hi.size() * 4));
  }
  float *dx = df + f_x, *dsl = df + f_sl, *dout = df + f_out, *dh = df + f_dh, *dh2 = df + f_dh2, *dxp = df + f_xp;
  hipStream_t st = c->stream;
  const bool last = layer + 1 == NL;
  bool ok = true;
  switch (op) {
    case VX_DEV_OP_EMBED:
      launch_dec_embed_ln_pack(di, di + MB, emb_tab, emb_alpha, c->pe, dh, c->ar[0].n1_w, c->ar[0].n1_b, dxp, nrows, st);
      break;
    case VX_DEV_OP_GEMM:
      // as the engine launches it: linear2 of the 5 .. 32-row chain takes the context's block mapping
      launch_skinny_gemm_kmap(wp, dx, dout, Npad, K, sk, st, nrows > SB_ROWS, nrows > SB_ROWS && variant == VX_DEV_W_L2 && c->l2_kmap);
      break;
    case VX_DEV_OP_QKV_BAL:
      launch_skinny_qkv_balanced(wp, dx, dout, st);
      break;
    case VX_DEV_OP_LINEAR1:
      launch_linear1(c, wp, dx, L.l1_b, dout, st);
      break;
    case VX_DEV_OP_REDUCE_LN:
      // the engine's four uses: behind out_proj (4 slabs, or 16 head slabs of the fused dec_attn) with norm2, behind linear2 with the
      // next layer's norm1 or the final norm, and the final norm alone in front of the first logits (no slabs, no bias, no h); in place
      if (variant == 0) launch_dec_reduce_ln_pack(nullptr, 0, D_MODEL, nullptr, dh, nullptr, fin_g, fin_b, dxp, nrows, st);
      else if (variant == SK_L2)
        launch_dec_reduce_ln_pack(dsl, SK_L2, D_MODEL, L.l2_b, dh, dh, last ? fin_g : c->ar[layer + 1].n1_w, last ? fin_b : c->ar[layer + 1].n1_b, dxp,
                                  nrows, st);
      else launch_dec_reduce_ln_pack(dsl, variant, D_MODEL, L.out_b, dh, dh, L.n2_w, L.n2_b, dxp, nrows, st);
      break;
    case VX_DEV_OP_SB_LN_GEMM:
      // (the engine hands predict a null h_out; here both weights get one, so that the prologue's slab sum is seen)
      if (variant == VX_DEV_W_PRED) ok = launch_skinny_gemm_sb_ln(wp, dout, Npad, sk, dsl, SK_L2, L.l2_b, dh, dh2, fin_g, fin_b, nrows, st);
      else ok = launch_skinny_gemm_sb_ln(wp, dout, Npad, sk, dsl, SK_L2, c->ar[layer - 1].l2_b, dh, dh2, L.n1_w, L.n1_b, nrows, st);
      break;
    default:
      ok = launch_skinny16_sb_ln(wp, L.l1_b, dout, D_FF, dsl, SK_OUT, L.out_b, dh, dh2, L.n2_w, L.n2_b, nrows, st);
      break;
  }
  if (!ok) {
    (void)hipStreamSynchronize(st);
    cleanup();
    FAIL(VX_EINVAL, "vx_dev_dec_op: a launcher refused this configuration (op %d, %d rows)", op, nrows);
  }
  const bool image_out = op == VX_DEV_OP_LINEAR1 || op == VX_DEV_OP_SB_LINEAR1;
  const size_t n_out = !writes_out ? 0 : image_out ? (size_t)MB * D_FF : (size_t)sk * MB * Npad;
  std::vector<float> o_out(image_out ? n_out : 0), o_xp(writes_xp ? (size_t)MB * d : 0);
  if (n_out) TRYX(xfer_d2h(c, image_out ? o_out.data() : out, dout, n_out * 4));
  // h: the reduce kernel works in place as in the engine (dh); the small-batch consumers write the other buffer of the dh / dh2
  // pair; reduce_ln without slabs is handed no h at all, and the caller gets the buffer nothing was stored to
  const bool h_apart = sb || (op == VX_DEV_OP_REDUCE_LN && variant == 0);
  if (writes_h) TRYX(xfer_d2h(c, h, h_apart ? dh2 : dh, (size_t)nrows * d * 4));
  if (writes_xp) TRYX(xfer_d2h(c, o_xp.data(), dxp, o_xp.size() * 4));
  if (reads_resid) TRYX(xfer_d2h(c, resid, dh, (size_t)nrows * d * 4));      // what the residual buffer holds behind the launch
  TRYX(xfer_sync(c));
  TRY(hipGetLastError());
  if (image_out) dev_unpack_image(out, o_out.data(), D_FF);
  if (writes_xp) dev_unpack_image(xp, o_xp.data(), d);
#undef TRY
#undef TRYX
  cleanup();
  return VX_OK;
}

// un-tile one f16x2 plane pair (tile-major [rows / 256][K / 32][256][32], vx_common.h) into [2][rows256][K] row-major half-words
static void dev_untile_planes(uint16_t* dst, const std::vector<unsigned short>& src, long pstride, long rows256, int K) {
  for (int p = 0; p < 2; ++p)
    for (long r = 0; r < rows256; ++r)
      for (int kt = 0; kt < K / 32; ++kt)
        memcpy(dst + ((size_t)p * rows256 + r) * K + (size_t)kt * 32,
               &src[(size_t)p * pstride + ((((size_t)(r >> 8) * (K / 32)) + kt) * 256 + (r & 255)) * 32], 64);
}

// vx_dev_gemm: ONE full-sequence GEMM through a product launcher (launch_gemm_f32 / launch_gemm_f16x2 / launch_gemm_bf16x3[_dma]) on
// caller operands, with the operand preparation of proj(): launch_split2h at H2_ACT_SCALE with the gather for A, the loader's
// absmax -> shift -> launch_split2h for W (or the context's own load-time planes), descale = 2^-(5 + shift).  Everything is private
// scratch: outputs pre-filled with the sentinels, the plane buffers too (the pad rows of a last tile are finite garbage).
int vx_dev_gemm(vx_ctx* c, int32_t kernel, int32_t flags, int32_t M, int32_t N, int32_t K, const float* A, int32_t rowsA, int32_t lda,
                const int32_t* gather, const float* Wt, int32_t w_src, int32_t w_layer, int32_t w_shift, const float* bias,
                const float* resid, int32_t rowsR, int32_t ldr, const int32_t* resid_rows, const float* colscale, int32_t act, float* Cout,
                int32_t rowsC, uint16_t* planes, uint16_t* a_planes, int32_t* info) {
  if (!c) return VX_EINVAL;
  if (c->serve) FAIL(VX_ESTATE, "vx_dev_gemm: a serving session is open on this context (vx_serve_close it first)");
  constexpr int CAP = 4096, LD_CAP = 8192;
  const bool f32k = kernel >= 0 && kernel <= 4, h2k = kernel >= 10 && kernel <= 15, x3k = kernel == 20 || kernel == 21;
  if (!f32k && !h2k && !x3k) FAIL(VX_EINVAL, "vx_dev_gemm: kernel must be 0 .. 4 (fp32), 10 .. 15 (f16x2) or 20, 21 (bf16x3)");
  if (!A || !info || M < 1 || M > CAP || N < 4 || N > CAP || N % 4 || K < 32 || K > CAP || K % 32)
    FAIL(VX_EINVAL, "vx_dev_gemm: null argument, or M, N, K outside 1 .. %d with N %% 4 == 0 and K %% 32 == 0", CAP);
  if (lda < K || lda > LD_CAP || lda % 4 || rowsA < 1 || rowsA > 2 * CAP || (!gather && rowsA < M))
    FAIL(VX_EINVAL, "vx_dev_gemm: K <= lda <= %d with lda %% 4 == 0; 1 <= rowsA <= %d, rowsA >= M without a gather", LD_CAP, 2 * CAP);
  if (gather) for (int m = 0; m < M; ++m) if (gather[m] < 0 || gather[m] >= rowsA) FAIL(VX_EINVAL, "vx_dev_gemm: gather[%d] outside A", m);
  if (flags & ~(VX_DEV_GEMM_OUT_PLANES | VX_DEV_GEMM_INPLACE)) FAIL(VX_EINVAL, "vx_dev_gemm: unknown flag");
  const bool out_pl = flags & VX_DEV_GEMM_OUT_PLANES, inplace = flags & VX_DEV_GEMM_INPLACE;
  if (act < ACT_NONE || act > ACT_ELU || (!f32k && (colscale || act > ACT_RELU)))
    FAIL(VX_EINVAL, "vx_dev_gemm: act must be 0 .. 3; colscale, GELU and ELU are the fp32 kernels'");
  if (x3k && (gather || bias || resid || resid_rows || colscale || act || flags))
    FAIL(VX_EINVAL, "vx_dev_gemm: the bf16x3 kernels run with the plain epilogue here");
  if (resid) {
    if (ldr < N || ldr > LD_CAP || ldr % 4 || rowsR < 1 || rowsR > 2 * CAP || (!resid_rows && rowsR < M))
      FAIL(VX_EINVAL, "vx_dev_gemm: N <= ldr <= %d with ldr %% 4 == 0; 1 <= rowsR <= %d, rowsR >= M without resid_rows", LD_CAP, 2 * CAP);
    if (resid_rows) for (int m = 0; m < M; ++m) if (resid_rows[m] < 0 || resid_rows[m] >= rowsR) FAIL(VX_EINVAL, "vx_dev_gemm: resid_rows[%d] outside resid", m);
  } else if (resid_rows || inplace) FAIL(VX_EINVAL, "vx_dev_gemm: resid_rows / the in-place flag without resid");
  if (inplace && (resid_rows || ldr != N || out_pl)) FAIL(VX_EINVAL, "vx_dev_gemm: in place: ldr == N, no resid_rows, no out_planes");
  if (out_pl && (!h2k || N % 256 || !planes)) FAIL(VX_EINVAL, "vx_dev_gemm: out_planes: an f16x2 kernel, N %% 256 == 0 and a planes buffer");
  if (!out_pl && (!Cout || planes)) FAIL(VX_EINVAL, "vx_dev_gemm: C is null (or planes given) without the out_planes flag");
  if (Cout && (rowsC < M || rowsC > M + 64)) FAIL(VX_EINVAL, "vx_dev_gemm: rowsC must be M .. M + 64");
  if (a_planes && !h2k) FAIL(VX_EINVAL, "vx_dev_gemm: a_planes goes with the f16x2 kernels");
  const unsigned short* ctx_w3 = nullptr;
  int shift = -1;
  if (w_src != 0) {
    if (!h2k || Wt || w_src < 1 || w_src > 8) FAIL(VX_EINVAL, "vx_dev_gemm: w_src 1 .. 8 goes with an f16x2 kernel and a null W");
    if (!c->finalized || c->gemm_mode != 0) FAIL(VX_ESTATE, "vx_dev_gemm: the context holds no f16x2 weight planes");
    const std::vector<LayerW>& st = w_src <= 4 ? c->ar : c->nar;
    if (w_layer < 0 || w_layer >= (int)st.size()) FAIL(VX_EINVAL, "vx_dev_gemm: w_layer must be 0 .. %d", (int)st.size() - 1);
    const LayerW& L = st[w_layer];
    const int which = (w_src - 1) & 3;
    ctx_w3 = which == 0 ? L.in_w3 : which == 1 ? L.out_w3 : which == 2 ? L.l1_w3 : L.l2_w3;
    const int wn = which == 0 ? 3 * D_MODEL : which == 2 ? D_FF : D_MODEL, wk = which == 3 ? D_FF : D_MODEL;
    if (N != wn || K != wk) FAIL(VX_EINVAL, "vx_dev_gemm: this weight is [%d][%d]", wn, wk);
    const auto it = c->w_shift.find(ctx_w3);
    if (!ctx_w3 || it == c->w_shift.end()) FAIL(VX_ESTATE, "vx_dev_gemm: the context has no planes of this weight");
    shift = it->second;
  } else {
    if (!Wt) FAIL(VX_EINVAL, "vx_dev_gemm: W is null");
    if (w_shift < -1 || w_shift > 24) FAIL(VX_EINVAL, "vx_dev_gemm: w_shift must be -1 (the loader's rule) or 0 .. 24");
  }
  HIPCHK(hipSetDevice(c->dev));

  const long M256 = (M + 255) / 256 * 256;
  const long a_pl = h2k ? h2_plane(M, K, H2_TILE_A) : (long)M * K, w_pl = h2k ? h2_plane(N, K, H2_TILE_W) : (long)N * K;
  const long o_pl = h2_plane(M, N, H2_TILE_A);
  const int P = h2k ? 2 : 3;
  float *dA = nullptr, *dW = nullptr, *dbias = nullptr, *dcs = nullptr, *dres = nullptr, *dC = nullptr;
  unsigned short *dA3 = nullptr, *dW3 = nullptr, *dP = nullptr;
  int* di = nullptr;                                                  // range flag | absmax bits | gather [M] | resid_rows [M]
  auto cleanup = [&]() {
    for (void* p : {(void*)dA, (void*)dW, (void*)dbias, (void*)dcs, (void*)dres, (void*)dC, (void*)dA3, (void*)dW3, (void*)dP, (void*)di})
      if (p) (void)hipFree(p);
  };
  hipError_t he;
  // an error return drains the ring first: a queued xfer_d2h must not be delivered into host buffers that are gone by then
#define TRY(x) if ((he = (x)) != hipSuccess) { (void)xfer_sync(c); cleanup(); c->err = std::string(#x) + ": " + hipGetErrorString(he); return VX_EHIP; }
#define TRYX(x) do { if (int _e = (x)) { const std::string _m = c->err; (void)xfer_sync(c); c->err = _m; cleanup(); return _e; } } while (0)
  TRY(hipMalloc((void**)&dA, (size_t)rowsA * lda * 4));
  TRYX(xfer_h2d(c, dA, A, (size_t)rowsA * lda * 4));
  if (Wt) {
    TRY(hipMalloc((void**)&dW, (size_t)N * K * 4));
    TRYX(xfer_h2d(c, dW, Wt, (size_t)N * K * 4));
  }
  if (bias) { TRY(hipMalloc((void**)&dbias, (size_t)N * 4)); TRYX(xfer_h2d(c, dbias, bias, (size_t)N * 4)); }
  if (colscale) { TRY(hipMalloc((void**)&dcs, (size_t)N * 4)); TRYX(xfer_h2d(c, dcs, colscale, (size_t)N * 4)); }
  if (resid && !inplace) { TRY(hipMalloc((void**)&dres, (size_t)rowsR * ldr * 4)); TRYX(xfer_h2d(c, dres, resid, (size_t)rowsR * ldr * 4)); }
  {
    std::vector<int> hi(2 + 2 * (size_t)M, 0);
    if (gather) memcpy(&hi[2], gather, (size_t)M * 4);
    if (resid_rows) memcpy(&hi[2 + M], resid_rows, (size_t)M * 4);
    TRY(hipMalloc((void**)&di, hi.size() * 4));
    TRYX(xfer_h2d(c, di, hi.data(), hi.size() * 4));
  }
  int* dflag = di;
  const int *dgather = gather ? di + 2 : nullptr, *drr = resid_rows ? di + 2 + M : nullptr;
  if (Cout) {
    TRY(hipMalloc((void**)&dC, (size_t)rowsC * N * 4));
    std::vector<float> fill((size_t)rowsC * N, VX_DEV_SENTINEL_F);
    if (inplace) memcpy(fill.data(), resid, (size_t)M * N * 4);      // ldr == N: the residual rows are the output rows
    TRYX(xfer_h2d(c, dC, fill.data(), fill.size() * 4));
  }
  if (!f32k) {
    TRY(hipMalloc((void**)&dA3, (size_t)P * a_pl * 2));
    std::vector<unsigned short> fill((size_t)P * std::max(a_pl, std::max(w_pl, o_pl)), VX_DEV_SENTINEL_H);
    TRYX(xfer_h2d(c, dA3, fill.data(), (size_t)P * a_pl * 2));
    if (!ctx_w3) {
      TRY(hipMalloc((void**)&dW3, (size_t)P * w_pl * 2));
      TRYX(xfer_h2d(c, dW3, fill.data(), (size_t)P * w_pl * 2));
    }
    if (out_pl) {
      TRY(hipMalloc((void**)&dP, (size_t)2 * o_pl * 2));
      TRYX(xfer_h2d(c, dP, fill.data(), (size_t)2 * o_pl * 2));
    }
  }
  hipStream_t st = c->stream;
  if (f32k) {
    GemmArgs g{};
    g.A = dA; g.lda = lda; g.W = dW; g.ldw = K; g.bias = dbias; g.resid = inplace ? dC : dres; g.ldr = ldr; g.colscale = dcs;
    g.C = dC; g.ldc = N; g.M = M; g.N = N; g.K = K; g.act = act; g.row_gather = dgather; g.resid_rows = drr;
    launch_gemm_f32(g, st, kernel);
  } else {
    if (h2k) {
      launch_split2h(dA, lda, M, K, dgather, dA3, a_pl, H2_TILE_A, dflag, H2_ACT_SCALE, st);          // as proj()
      if (!ctx_w3) {
        if (w_shift >= 0) shift = w_shift;
        else {                                                                                        // as the loader (weights.hip)
          unsigned bits = 0;
          launch_absmax(dW, (long)N * K, reinterpret_cast<unsigned*>(di + 1), st);
          TRYX(xfer_d2h(c, &bits, di + 1, 4));
          TRYX(xfer_sync(c));
          float mx;
          memcpy(&mx, &bits, sizeof mx);
          shift = h2_weight_shift(mx);
        }
        launch_split2h(dW, K, N, K, nullptr, dW3, w_pl, H2_TILE_W, dflag, ldexpf(1.0f, shift), st);
      }
    } else {
      launch_split3(dA, lda, M, K, nullptr, dA3, a_pl, st);
      launch_split3(dW, K, N, K, nullptr, dW3, w_pl, st);
    }
    GemmX3Args g{};
    g.A = dA3; g.a_plane = a_pl; g.W = ctx_w3 ? ctx_w3 : dW3; g.w_plane = w_pl; g.bias = dbias; g.resid = inplace ? dC : dres; g.ldr = ldr;
    g.C = dC; g.ldc = N; g.M = M; g.N = N; g.K = K; g.act = act;
    g.out_planes = out_pl ? dP : nullptr; g.out_plane = out_pl ? o_pl : 0; g.range_flag = dflag; g.resid_rows = drr;
    if (h2k) g.descale = ldexpf(1.0f, -(H2_ACT_SHIFT + shift));
    static const int tn_of[6] = {0, 128, 256, 257, -128, -129};
    if (h2k) launch_gemm_f16x2(g, st, tn_of[kernel - 10]);
    else if (kernel == 20) launch_gemm_bf16x3(g, st);
    else launch_gemm_bf16x3_dma(g, st);
  }
  int flag = 0;
  std::vector<unsigned short> hp(out_pl ? (size_t)2 * o_pl : 0), hap(a_planes ? (size_t)2 * a_pl : 0);
  if (Cout) TRYX(xfer_d2h(c, Cout, dC, (size_t)rowsC * N * 4));
  if (out_pl) TRYX(xfer_d2h(c, hp.data(), dP, hp.size() * 2));
  if (a_planes) TRYX(xfer_d2h(c, hap.data(), dA3, hap.size() * 2));
  TRYX(xfer_d2h(c, &flag, dflag, 4));
  TRYX(xfer_sync(c));
  TRY(hipGetLastError());
  if (out_pl) dev_untile_planes(planes, hp, o_pl, M256, N);
  if (a_planes) dev_untile_planes(a_planes, hap, a_pl, M256, K);
  info[0] = flag; info[1] = h2k ? shift : -1; info[2] = 0;
#undef TRY
#undef TRYX
  cleanup();
  return VX_OK;
}

// vx_dev_layernorm: ONE launch_layernorm on caller rows (private scratch, outputs pre-filled with the sentinels).
int vx_dev_layernorm(vx_ctx* c, int32_t rows, int32_t C, int32_t ldx, const float* x, const float* g, const float* b, const float* ada_w,
                     const float* ada_b, float* y, int32_t rowsY, uint16_t* planes, int32_t* range_flag) {
  if (!c) return VX_EINVAL;
  if (c->serve) FAIL(VX_ESTATE, "vx_dev_layernorm: a serving session is open on this context (vx_serve_close it first)");
  if (!x || rows < 1 || rows > 4096 || (C != 1024 && C != 384) || ldx < C || ldx > 8192 || ldx % 4)
    FAIL(VX_EINVAL, "vx_dev_layernorm: null x, rows outside 1 .. 4096, C not 1024 / 384, or ldx outside C .. 8192 with ldx %% 4 == 0");
  if (!g != !b || !ada_w != !ada_b) FAIL(VX_EINVAL, "vx_dev_layernorm: g / b and ada_w / ada_b come in pairs");
  if (planes && C != 1024) FAIL(VX_EINVAL, "vx_dev_layernorm: planes go with C = 1024");
  if (!y && !planes) FAIL(VX_EINVAL, "vx_dev_layernorm: neither y nor planes");
  if (y && (rowsY < rows || rowsY > rows + 64)) FAIL(VX_EINVAL, "vx_dev_layernorm: rowsY must be rows .. rows + 64");
  HIPCHK(hipSetDevice(c->dev));
  const long R256 = (rows + 255) / 256 * 256, pstride = h2_plane(rows, C, H2_TILE_A);
  float *dx = nullptr, *dv = nullptr, *dy = nullptr;                // dv: g | b | ada_w | ada_b
  unsigned short* dpl = nullptr;
  int* dflag = nullptr;
  auto cleanup = [&]() { for (void* p : {(void*)dx, (void*)dv, (void*)dy, (void*)dpl, (void*)dflag}) if (p) (void)hipFree(p); };
  hipError_t he;
  // an error return drains the ring first: a queued xfer_d2h must not be delivered into host buffers that are gone by then
#define TRY(x) if ((he = (x)) != hipSuccess) { (void)xfer_sync(c); cleanup(); c->err = std::string(#x) + ": " + hipGetErrorString(he); return VX_EHIP; }
#define TRYX(x) do { if (int _e = (x)) { const std::string _m = c->err; (void)xfer_sync(c); c->err = _m; cleanup(); return _e; } } while (0)
  TRY(hipMalloc((void**)&dx, (size_t)rows * ldx * 4));
  TRYX(xfer_h2d(c, dx, x, (size_t)rows * ldx * 4));
  TRY(hipMalloc((void**)&dv, (size_t)4 * C * 4));
  const float* hv[4] = {g, b, ada_w, ada_b};
  for (int i = 0; i < 4; ++i) if (hv[i]) TRYX(xfer_h2d(c, dv + (size_t)i * C, hv[i], (size_t)C * 4));
  TRY(hipMalloc((void**)&dflag, 4));
  const int zero = 0;
  TRYX(xfer_h2d(c, dflag, &zero, 4));
  if (y) {
    TRY(hipMalloc((void**)&dy, (size_t)rowsY * C * 4));
    std::vector<float> fill((size_t)rowsY * C, VX_DEV_SENTINEL_F);
    TRYX(xfer_h2d(c, dy, fill.data(), fill.size() * 4));
  }
  if (planes) {
    TRY(hipMalloc((void**)&dpl, (size_t)2 * pstride * 2));
    std::vector<unsigned short> fill((size_t)2 * pstride, VX_DEV_SENTINEL_H);
    TRYX(xfer_h2d(c, dpl, fill.data(), fill.size() * 2));
  }
  launch_layernorm(dx, ldx, dy, C, rows, C, LN_EPS, g ? dv : nullptr, b ? dv + C : nullptr, ada_w ? dv + 2 * C : nullptr,
                   ada_b ? dv + 3 * C : nullptr, c->stream, dpl, pstride, dflag);
  int flag = 0;
  std::vector<unsigned short> hp(planes ? (size_t)2 * pstride : 0);
  if (y) TRYX(xfer_d2h(c, y, dy, (size_t)rowsY * C * 4));
  if (planes) TRYX(xfer_d2h(c, hp.data(), dpl, hp.size() * 2));
  TRYX(xfer_d2h(c, &flag, dflag, 4));
  TRYX(xfer_sync(c));
  TRY(hipGetLastError());
  if (planes) dev_untile_planes(planes, hp, pstride, R256, C);
  if (range_flag) *range_flag = flag;
#undef TRY
#undef TRYX
  cleanup();
  return VX_OK;
}

}  // extern "C"
