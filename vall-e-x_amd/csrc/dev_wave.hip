// vx_dev_wave_op (include/vallex_hip_dev.h): ONE launch of a glue kernel of the waveform half -- the Vocos head (vocos.hip) and the
// EnCodec decoder / encoder (encodec.hip) -- through its product launcher on caller-chosen operands.  Host pointers in and out through
// the context's pinned ring; everything the launch touches is private scratch of the call, every output pre-filled with a sentinel.
// Never on the product path.
#include "../../include/vallex_hip_dev.h"
#include "engine_ctx.h"

extern "C" {

int vx_dev_wave_op(vx_ctx* c, int32_t op, const int32_t* dims, const float* a, const float* b, const float* w, const float* bias,
                   const int32_t* ia, const int32_t* ib, float* out, float* out2, float* out3, int64_t* codes, int32_t* geom) {
  if (!c) return VX_EINVAL;
  if (c->serve) FAIL(VX_ESTATE, "vx_dev_wave_op: a serving session is open on this context (vx_serve_close it first)");
  if (!c->finalized) FAIL(VX_ESTATE, "vx_dev_wave_op: weights not finalized");
  if (op < VX_DEV_WAVE_CODEBOOK_SUM || op > VX_DEV_WAVE_TABLES) FAIL(VX_EINVAL, "vx_dev_wave_op: unknown op %d", op);
  constexpr int ROWS_CAP = 4096, EXTRA_CAP = 64, SAMPLES_CAP = 65536, STRIDE_CAP = 1 << 20;
  constexpr long ELEMS_CAP = 1L << 24;             // elements of one buffer of the call
  constexpr int VC_NBP = 1408, VC_KP = 1312, VC_NF = 1280, HOP = 320, HD = 512;
  if (op == VX_DEV_WAVE_TABLES) {
    if (!out && !out2 && !out3) FAIL(VX_EINVAL, "vx_dev_wave_op: tables: no table asked for");
    if ((out || out2) && !c->has_vocos) FAIL(VX_ESTATE, "vx_dev_wave_op: tables: Vocos weights not loaded");
    if (out3 && !c->has_encodec_enc) FAIL(VX_ESTATE, "vx_dev_wave_op: tables: EnCodec encoder weights not loaded");
    HIPCHK(hipSetDevice(c->dev));
    if (out) D2H(out, c->vc_dft, (size_t)VC_NF * VC_KP * 4);
    if (out2) D2H(out2, c->vc_win2, (size_t)VC_NF * 4);
    if (out3) D2H(out3, c->en_e2, (size_t)N_Q * 1024 * 4);
    SYNC();
    return VX_OK;
  }
  if (!dims) FAIL(VX_EINVAL, "vx_dev_wave_op: null dims");
  // ---- the documented domain of every op; nothing is launched (or allocated) before all of it holds ----
  const bool seq_op = op == VX_DEV_WAVE_OVERLAP_ADD || op == VX_DEV_WAVE_IM2COL_SEQ || op == VX_DEV_WAVE_LSTM_CELL || op == VX_DEV_WAVE_FINAL_CONV;
  const bool row_op = op == VX_DEV_WAVE_IM2COL7 || op == VX_DEV_WAVE_DWCONV7;
  int max_len = 0;
  if (seq_op) {
    // dims[0] = batch, dims[2] = frames the packed operand holds: every sequence lies inside it
    const int batch = dims[0], frames = dims[2];
    if (batch < 1 || batch > MB) FAIL(VX_EINVAL, "vx_dev_wave_op: batch must be 1 .. %d", MB);
    if (frames < 1 || frames > ROWS_CAP) FAIL(VX_EINVAL, "vx_dev_wave_op: frames must be 1 .. %d", ROWS_CAP);
    if (!ia || !ib) FAIL(VX_EINVAL, "vx_dev_wave_op: null seq_off / seq_len");
    for (int i = 0; i < batch; ++i) {
      if (ia[i] < 0 || ib[i] < 0 || (long)ia[i] + ib[i] > frames)
        FAIL(VX_EINVAL, "vx_dev_wave_op: sequence %d (offset %d, length %d) leaves the %d frames of the operand", i, ia[i], ib[i], frames);
      max_len = std::max(max_len, ib[i]);
    }
  }
  if (row_op) {
    const int rows = dims[0];
    if (rows < 1 || rows > ROWS_CAP) FAIL(VX_EINVAL, "vx_dev_wave_op: rows must be 1 .. %d", ROWS_CAP);
    if (!ia || !ib) FAIL(VX_EINVAL, "vx_dev_wave_op: null row_t / row_len");
    for (int r = 0; r < rows; ++r)       // row r is frame row_t[r] of a sequence of row_len[r] frames that lies inside the operand
      if (ib[r] < 1 || ia[r] < 0 || ia[r] >= ib[r] || r - ia[r] < 0 || (long)r - ia[r] + ib[r] > rows)
        FAIL(VX_EINVAL, "vx_dev_wave_op: row %d (frame %d of %d) belongs to a sequence that leaves the %d rows of the operand", r, ia[r], ib[r], rows);
  }
  const auto extra_ok = [](int e) { return e >= 0 && e <= EXTRA_CAP; };
  long n_a = 0, n_b = 0, n_w = 0, n_bias = 0, n_ia = 0, n_ib = 0, n_out = 0, n_out2 = 0, n_out3 = 0, n_codes = 0;   // element counts
  EncPadGeom pg{};
  switch (op) {
    case VX_DEV_WAVE_CODEBOOK_SUM: {
      const int rows = dims[0];
      if (rows < 1 || rows > ROWS_CAP || !extra_ok(dims[1])) FAIL(VX_EINVAL, "vx_dev_wave_op: codebook_sum: rows 1 .. %d, extra 0 .. %d", ROWS_CAP, EXTRA_CAP);
      if (!ia || !a || !out) FAIL(VX_EINVAL, "vx_dev_wave_op: codebook_sum: null codes, codebook or feat");
      for (long i = 0; i < (long)rows * N_Q; ++i)
        if (ia[i] < 0 || ia[i] >= AUDIO_VOCAB) FAIL(VX_EINVAL, "vx_dev_wave_op: codebook_sum: code %d outside 0 .. 1023", ia[i]);
      n_ia = (long)rows * N_Q; n_a = (long)N_Q * 1024 * 128; n_out = (long)(rows + dims[1]) * 128;
      break;
    }
    case VX_DEV_WAVE_IM2COL7:
      if (!extra_ok(dims[1]) || !a || !out) FAIL(VX_EINVAL, "vx_dev_wave_op: im2col7: extra 0 .. %d, x and out not null", EXTRA_CAP);
      n_ia = n_ib = dims[0]; n_a = (long)dims[0] * 128; n_out = (long)(dims[0] + dims[1]) * 896;
      break;
    case VX_DEV_WAVE_DWCONV7:
      if (!extra_ok(dims[1]) || (dims[2] != 384 && dims[2] != 512) || !a || !w || !bias || !out)
        FAIL(VX_EINVAL, "vx_dev_wave_op: dwconv7: extra 0 .. %d, C 384 or 512, x, w, bias and out not null", EXTRA_CAP);
      n_ia = n_ib = dims[0]; n_a = (long)dims[0] * dims[2]; n_w = (long)dims[2] * 7; n_bias = dims[2]; n_out = (long)(dims[0] + dims[1]) * dims[2];
      break;
    case VX_DEV_WAVE_ISTFT_PREP:
      if (dims[0] < 1 || dims[0] > ROWS_CAP || !extra_ok(dims[1]) || !a || !out)
        FAIL(VX_EINVAL, "vx_dev_wave_op: istft_prep: rows 1 .. %d, extra 0 .. %d, o and reim not null", ROWS_CAP, EXTRA_CAP);
      n_a = (long)dims[0] * VC_NBP; n_out = (long)(dims[0] + dims[1]) * VC_KP;
      break;
    case VX_DEV_WAVE_OVERLAP_ADD: {
      const int stride = dims[3];
      if (!c->has_vocos) FAIL(VX_ESTATE, "vx_dev_wave_op: overlap_add: Vocos weights not loaded (the window table is the context's)");
      if (!extra_ok(dims[1]) || !a || !out || stride < 0 || stride > STRIDE_CAP || (stride && (long)max_len * HOP > stride))
        FAIL(VX_EINVAL, "vx_dev_wave_op: overlap_add: extra 0 .. %d, frames and audio not null, audio_stride 0 or >= 320 x the longest sequence", EXTRA_CAP);
      n_ia = n_ib = dims[0]; n_a = (long)dims[2] * VC_NF; n_out = (stride ? (long)dims[0] * stride : (long)dims[2] * HOP) + dims[1];
      break;
    }
    case VX_DEV_WAVE_IM2COL_SEQ: {
      const int C = dims[3], k = dims[4], mode = dims[5], elu = dims[6], R = dims[7];
      if (!extra_ok(dims[1]) || !a || !out) FAIL(VX_EINVAL, "vx_dev_wave_op: im2col_seq: extra 0 .. %d, x and out not null", EXTRA_CAP);
      if (C < 4 || C > 512 || C % 4 || (mode != 0 && mode != 1) || (mode == 0 ? (k < 1 || k > 7) : k != 2) || (elu != 0 && elu != 1) || R < 1 || R > 320)
        FAIL(VX_EINVAL, "vx_dev_wave_op: im2col_seq: C 4 .. 512 with C %% 4 == 0; mode 0 with k 1 .. 7 or mode 1 with k 2; elu 0 | 1; R 1 .. 320");
      n_ia = n_ib = dims[0]; n_a = (long)dims[2] * R * C; n_out = ((long)dims[2] * R + dims[1]) * k * C;
      break;
    }
    case VX_DEV_WAVE_LSTM_CELL: {
      const int splitk = dims[1], t = dims[3];
      if ((splitk != 1 && splitk != 2) || t < 0 || t >= ROWS_CAP || !extra_ok(dims[4]) || !a || !b || !out || !out2 || !out3)
        FAIL(VX_EINVAL, "vx_dev_wave_op: lstm_cell: splitk 1 | 2, t 0 .. %d, extra 0 .. %d, part, xg, cstate, h and y not null", ROWS_CAP - 1, EXTRA_CAP);
      n_ia = n_ib = dims[0]; n_a = (long)2 * MB * 4 * HD; n_b = (long)dims[2] * 4 * HD; n_w = w ? (long)dims[2] * HD : 0;
      n_out = n_out2 = (long)MB * HD; n_out3 = (long)(dims[2] + dims[4]) * HD;
      break;
    }
    case VX_DEV_WAVE_FINAL_CONV: {
      const int R = dims[3], stride = dims[4];
      if (!extra_ok(dims[1]) || !a || !w || !bias || !out || R < 1 || R > 320 || stride < 1 || stride > STRIDE_CAP || (long)max_len * R > stride)
        FAIL(VX_EINVAL, "vx_dev_wave_op: final_conv: extra 0 .. %d, x, w, bias, audio not null, R 1 .. 320, audio_stride >= R x the longest sequence", EXTRA_CAP);
      n_ia = n_ib = dims[0]; n_a = (long)dims[2] * R * 32; n_w = 32 * 7; n_bias = 1; n_out = (long)dims[0] * stride + dims[1];
      break;
    }
    case VX_DEV_WAVE_ENC_FIRST_CONV:
      if (dims[0] < 1 || dims[0] > SAMPLES_CAP || !extra_ok(dims[1]) || !a || !w || !bias || !out)
        FAIL(VX_EINVAL, "vx_dev_wave_op: enc_first_conv: L 1 .. %d, extra 0 .. %d, wav, w, bias, out not null", SAMPLES_CAP, EXTRA_CAP);
      n_a = dims[0]; n_w = 32 * 7; n_bias = 32; n_out = (long)(dims[0] + dims[1]) * 32;
      break;
    case VX_DEV_WAVE_ENC_PAD_ELU: {
      const int Lc = dims[0], C = dims[2], r = dims[3];
      if (Lc < 1 || Lc > SAMPLES_CAP || C < 4 || C > 512 || C % 4 || r < 1 || r > 16 || !a || !out || !geom)
        FAIL(VX_EINVAL, "vx_dev_wave_op: enc_pad_elu: Lc 1 .. %d, C 4 .. 512 with C %% 4 == 0, r 1 .. 16, x, out, geom not null", SAMPLES_CAP);
      pg = enc_pad_geom(Lc, r);
      if (dims[1] < pg.rows || dims[1] > pg.rows + EXTRA_CAP)
        FAIL(VX_EINVAL, "vx_dev_wave_op: enc_pad_elu: out must hold rows .. rows + %d rows, rows = %ld here", EXTRA_CAP, pg.rows);
      n_a = (long)Lc * C; n_out = (long)dims[1] * C;
      break;
    }
    default: {                                     // VX_DEV_WAVE_RVQ_SELECT
      if (dims[0] < 1 || dims[0] > ROWS_CAP || !extra_ok(dims[1]) || dims[2] < 0 || dims[2] >= N_Q || !a || !b || !w || !bias || !out || !codes)
        FAIL(VX_EINVAL, "vx_dev_wave_op: rvq_select: rows 1 .. %d, extra 0 .. %d, q 0 .. 7, resid, scores, e2, codebook, out, codes not null", ROWS_CAP, EXTRA_CAP);
      n_a = (long)dims[0] * 128; n_b = (long)dims[0] * 1024; n_w = 1024; n_bias = (long)1024 * 128;
      n_out = (long)(dims[0] + dims[1]) * 128; n_codes = (long)(dims[0] + dims[1]) * N_Q;
      break;
    }
  }
  if (n_a > ELEMS_CAP || n_out > ELEMS_CAP) FAIL(VX_EINVAL, "vx_dev_wave_op: an operand of more than 2^24 elements");
  HIPCHK(hipSetDevice(c->dev));

  std::vector<void*> allocs;
  auto cleanup = [&]() { for (void* p : allocs) (void)hipFree(p); };
  hipError_t he;
  // an error return drains the ring first: a queued xfer_d2h must not be delivered into host buffers that are gone by then
#define TRY(x) if ((he = (x)) != hipSuccess) { (void)xfer_sync(c); cleanup(); c->err = std::string(#x) + ": " + hipGetErrorString(he); return VX_EHIP; }
#define TRYX(x) do { if (int _e = (x)) { const std::string _m = c->err; (void)xfer_sync(c); c->err = _m; cleanup(); return _e; } } while (0)
  // device copy of a host operand (n elements of 4 bytes; null for n == 0)
  auto upload = [&](const void* h, long n, void** d) -> int {
    *d = nullptr;
    if (n <= 0) return VX_OK;
    HIPCHK(hipMalloc(d, (size_t)n * 4));
    allocs.push_back(*d);
    return xfer_h2d(c, *d, h, (size_t)n * 4);
  };
  // device output of n floats: the sentinel everywhere, then the first n_init elements of `init` (an in / out operand)
  auto output = [&](long n, const float* init, long n_init, float** d) -> int {
    *d = nullptr;
    if (n <= 0) return VX_OK;
    std::vector<float> fill((size_t)n, VX_DEV_SENTINEL_F);
    if (init) memcpy(fill.data(), init, (size_t)n_init * 4);
    return upload(fill.data(), n, reinterpret_cast<void**>(d));
  };
  float *da = nullptr, *db = nullptr, *dw = nullptr, *dbias = nullptr, *dout = nullptr, *dout2 = nullptr, *dout3 = nullptr;
  int *dia = nullptr, *dib = nullptr;
  long long* dcodes = nullptr;
  TRYX(upload(a, n_a, reinterpret_cast<void**>(&da)));
  TRYX(upload(b, n_b, reinterpret_cast<void**>(&db)));
  TRYX(upload(w, n_w, reinterpret_cast<void**>(&dw)));
  TRYX(upload(bias, n_bias, reinterpret_cast<void**>(&dbias)));
  TRYX(upload(ia, n_ia, reinterpret_cast<void**>(&dia)));
  TRYX(upload(ib, n_ib, reinterpret_cast<void**>(&dib)));
  std::vector<float> himg;                        // LSTM_CELL: the packed-x image of the caller's h rows
  if (op == VX_DEV_WAVE_LSTM_CELL) {
    himg.assign((size_t)MB * HD, 0.f);
    dev_pack_image(himg.data(), out2, HD);
    TRYX(output(n_out, out, n_out, &dout));                              // cstate, in and out
    TRYX(output(n_out2, himg.data(), n_out2, &dout2));
    TRYX(output(n_out3, nullptr, 0, &dout3));
  } else if (op == VX_DEV_WAVE_RVQ_SELECT) {
    TRYX(output(n_out, a, n_a, &dout));                                  // the residual rows, updated in place
    std::vector<long long> fill((size_t)n_codes, VX_DEV_SENTINEL_L);
    TRY(hipMalloc((void**)&dcodes, fill.size() * 8));
    allocs.push_back(dcodes);
    TRYX(xfer_h2d(c, dcodes, fill.data(), fill.size() * 8));
  } else {
    TRYX(output(n_out, nullptr, 0, &dout));
  }
  hipStream_t st = c->stream;
  switch (op) {
    case VX_DEV_WAVE_CODEBOOK_SUM: launch_codebook_sum(dia, da, dout, dims[0], st); break;
    case VX_DEV_WAVE_IM2COL7: launch_im2col7(da, 128, dia, dib, dout, dims[0], st); break;
    case VX_DEV_WAVE_DWCONV7: launch_dwconv7(da, dw, dbias, dia, dib, dout, dims[0], dims[2], st); break;
    case VX_DEV_WAVE_ISTFT_PREP: launch_istft_prep(da, VC_NBP, dout, VC_KP, dims[0], st); break;
    case VX_DEV_WAVE_OVERLAP_ADD: launch_overlap_add(da, VC_NF, dia, dib, c->vc_win2, dout, dims[3], dims[0], max_len, st); break;
    case VX_DEV_WAVE_IM2COL_SEQ:
      launch_im2col_seq(da, dims[3], dims[4], dims[5], dims[6], dia, dib, dims[7], dout, dims[4] * dims[3], dims[0], (long)max_len * dims[7], st);
      break;
    case VX_DEV_WAVE_LSTM_CELL: launch_lstm_cell(da, dims[1], db, dia, dib, dims[3], dout, dout2, dout3, dw, dims[0], st); break;
    case VX_DEV_WAVE_FINAL_CONV: launch_final_conv(da, dw, dbias, dia, dib, dims[3], dout, dims[4], dims[0], (long)max_len * dims[3], st); break;
    case VX_DEV_WAVE_ENC_FIRST_CONV: launch_enc_first_conv(da, dims[0], dw, dbias, dout, st); break;
    case VX_DEV_WAVE_ENC_PAD_ELU: launch_enc_pad_elu(da, dims[0], pg.Le, dims[2], dims[3], pg.rows, dout, st); break;
    default: launch_rvq_select(dout, db, dw, dbias, dcodes, dims[2], dims[0], st); break;
  }
  if (op == VX_DEV_WAVE_LSTM_CELL) {
    TRYX(xfer_d2h(c, out, dout, (size_t)n_out * 4));
    TRYX(xfer_d2h(c, himg.data(), dout2, (size_t)n_out2 * 4));
    TRYX(xfer_d2h(c, out3, dout3, (size_t)n_out3 * 4));
  } else {
    TRYX(xfer_d2h(c, out, dout, (size_t)n_out * 4));
    if (dcodes) TRYX(xfer_d2h(c, codes, dcodes, (size_t)n_codes * 8));
  }
  TRYX(xfer_sync(c));
  TRY(hipGetLastError());
  if (op == VX_DEV_WAVE_LSTM_CELL) dev_unpack_image(out2, himg.data(), HD);
  if (op == VX_DEV_WAVE_ENC_PAD_ELU) { geom[0] = (int32_t)pg.rows; geom[1] = (int32_t)pg.Le; geom[2] = (int32_t)pg.n_out; }
#undef TRY
#undef TRYX
  cleanup();
  return VX_OK;
}

}  // extern "C"
