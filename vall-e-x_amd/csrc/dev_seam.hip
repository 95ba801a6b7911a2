// vx_dev_seam_op (include/vallex_hip_dev.h): ONE launch of a kernel of the seams between the phases -- the embedding gathers, the NAR
// arg-max, the prefill -> decode K / V hand-over and the AdaLN GEMV (rows.hip), the best_of fan-out (beams.hip), the admission kernels
// of the continuous schedule and the serving session (admit.hip, serve.hip) and teacher forcing (decode.hip) -- through its product
// launcher on caller-chosen operands.  Host pointers in and out through the context's pinned ring; everything the launch touches is
// private scratch of the call, every output pre-filled with a sentinel; every index the kernel will form is checked here first.
// Never on the product path.
#include "../../include/vallex_hip_dev.h"
#include "engine_ctx.h"

#include <set>

extern "C" {

int vx_dev_seam_op(vx_ctx* c, int32_t op, const int32_t* dims, const float* fa, const float* fb, const float* fc, const float* fd,
                   const int32_t* ia, const int32_t* ib, const int32_t* ic, const int32_t* id, float* out, float* out2, float* out3,
                   int32_t* iout) {
  if (!c) return VX_EINVAL;
  if (c->serve) FAIL(VX_ESTATE, "vx_dev_seam_op: a serving session is open on this context (vx_serve_close it first)");
  if (!c->finalized) FAIL(VX_ESTATE, "vx_dev_seam_op: weights not finalized");
  if (op < VX_DEV_SEAM_EMBED_ROWS || op > VX_DEV_SEAM_TABLES) FAIL(VX_EINVAL, "vx_dev_seam_op: unknown op %d", op);
  constexpr int ROWS_CAP = 4096, EXTRA_CAP = 64, COLS_CAP = 8192;
  constexpr long ELEMS_CAP = 1L << 24;             // elements of one buffer of the call
  constexpr int D = D_MODEL;
  if (op == VX_DEV_SEAM_TABLES) {
    const int nnorm = 2 * c->NL + 1;
    if (!out && !out2 && !iout) FAIL(VX_EINVAL, "vx_dev_seam_op: tables: nothing asked for");
    HIPCHK(hipSetDevice(c->dev));
    if (out) D2H(out, c->pe, (size_t)c->pe_rows * D * 4);
    if (out2) D2H(out2, c->ada, (size_t)(N_Q - 1) * nnorm * 2 * D * 4);
    if (out || out2) SYNC();
    if (iout) { iout[0] = c->pe_rows; iout[1] = c->NL; iout[2] = nnorm; }
    return VX_OK;
  }
  if (!dims) FAIL(VX_EINVAL, "vx_dev_seam_op: null dims");
  // ---- the documented domain of every op; nothing is launched (or allocated) before all of it holds ----
  const int extra = dims[1];
  if (extra < 0 || extra > EXTRA_CAP) FAIL(VX_EINVAL, "vx_dev_seam_op: extra must be 0 .. %d", EXTRA_CAP);
  const auto in_range = [](const int32_t* v, long n, long lo, long hi) {      // every v[i] in [lo, hi)
    for (long i = 0; i < n; ++i)
      if (v[i] < lo || v[i] >= hi) return false;
    return true;
  };
  const auto distinct = [](const int32_t* v, long n, long stride) {          // v[0], v[stride], ... are pairwise different
    std::set<int32_t> seen;
    for (long i = 0; i < n; ++i)
      if (!seen.insert(v[i * stride]).second) return false;
    return true;
  };
  const auto dim_ok = [&](int i, int lo, int hi) { return dims[i] >= lo && dims[i] <= hi; };
  // element counts: inputs fa .. fd, ia .. id; outputs (total words, of which the first *_init come from the caller: in / out operands)
  long n_fa = 0, n_fb = 0, n_fc = 0, n_fd = 0, n_ia = 0, n_ib = 0, n_ic = 0, n_id = 0;
  long n_out = 0, n_out2 = 0, n_out3 = 0, n_iout = 0, i_out = 0, i_out2 = 0, i_out3 = 0, i_iout = 0;
  const bool state_op = op == VX_DEV_SEAM_ADMIT_ROWS || op == VX_DEV_SEAM_ADMIT_MASK || op == VX_DEV_SEAM_SERVE_UNIFORMS ||
                        op == VX_DEV_SEAM_SERVE_CANCEL || op == VX_DEV_SEAM_FORCE_TOKEN;
  int gen_stride = 0, max_steps = 0;
  if (state_op) {
    // the decode state block: every array a state kernel may read or write, VX_DEV_SEAM_ST_* words, then gen [32][gen_stride]
    gen_stride = dims[2];
    if (gen_stride < 1 || gen_stride > ROWS_CAP) FAIL(VX_EINVAL, "vx_dev_seam_op: gen_stride must be 1 .. %d", ROWS_CAP);
    if (!iout) FAIL(VX_EINVAL, "vx_dev_seam_op: null state block");
    const int32_t* so = iout + VX_DEV_SEAM_ST_SLOT_OF;
    if (!in_range(so, MB, 0, MB) || !distinct(so, MB, 1)) FAIL(VX_EINVAL, "vx_dev_seam_op: slot_of must be a permutation of 0 .. 31");
    i_iout = VX_DEV_SEAM_ST_GEN + (long)MB * gen_stride;
    n_iout = i_iout + extra;
  }
  switch (op) {
    case VX_DEV_SEAM_EMBED_ROWS: {
      const int rows = dims[0], out_rows = dims[2], rowsA = dims[3], rowsB = dims[4], pe_rows = dims[5];
      if (!dim_ok(0, 1, ROWS_CAP) || !dim_ok(2, 1, ROWS_CAP) || !dim_ok(3, 1, ROWS_CAP) || !dim_ok(4, 0, ROWS_CAP) || !dim_ok(5, 1, ROWS_CAP))
        FAIL(VX_EINVAL, "vx_dev_seam_op: embed_rows: rows, out_rows, rowsA, pe_rows 1 .. %d, rowsB 0 .. %d", ROWS_CAP, ROWS_CAP);
      if (!fa || !fc || !fd || !ia || !ic || !out) FAIL(VX_EINVAL, "vx_dev_seam_op: embed_rows: null tabA, alpha, pe, idA, pos or out");
      if ((fb != nullptr) != (ib != nullptr) || (fb != nullptr) != (rowsB > 0))
        FAIL(VX_EINVAL, "vx_dev_seam_op: embed_rows: tabB, idB and rowsB > 0 come together or not at all");
      if (!in_range(ia, rows, 0, rowsA)) FAIL(VX_EINVAL, "vx_dev_seam_op: embed_rows: an idA outside tabA");
      if (ib && !in_range(ib, rows, -1, rowsB)) FAIL(VX_EINVAL, "vx_dev_seam_op: embed_rows: an idB outside -1 .. rowsB - 1");
      if (!in_range(ic, rows, 0, pe_rows)) FAIL(VX_EINVAL, "vx_dev_seam_op: embed_rows: a pos outside the pe table");
      if (id ? !in_range(id, rows, 0, out_rows) || !distinct(id, rows, 1) : rows > out_rows)
        FAIL(VX_EINVAL, "vx_dev_seam_op: embed_rows: dst outside out, a duplicate in dst, or out_rows < rows without dst");
      n_fa = (long)rowsA * D; n_fb = (long)rowsB * D; n_fc = 1; n_fd = (long)pe_rows * D;
      n_ia = rows; n_ib = ib ? rows : 0; n_ic = rows; n_id = id ? rows : 0; n_out = (long)(out_rows + extra) * D;
      break;
    }
    case VX_DEV_SEAM_NAR_YEMB_INIT: {
      const int rows = dims[0], tab_rows = dims[2];
      if (!dim_ok(0, 1, ROWS_CAP) || !dim_ok(2, 1, 1024)) FAIL(VX_EINVAL, "vx_dev_seam_op: nar_yemb_init: rows 1 .. %d, tab_rows 1 .. 1024", ROWS_CAP);
      if (!fa || !ia || !ib || !out) FAIL(VX_EINVAL, "vx_dev_seam_op: nar_yemb_init: null tabs, codes, nj or out");
      if (!in_range(ia, (long)rows * N_Q, 0, tab_rows)) FAIL(VX_EINVAL, "vx_dev_seam_op: nar_yemb_init: a code outside the tables");
      if (!in_range(ib, rows, 1, N_Q + 1)) FAIL(VX_EINVAL, "vx_dev_seam_op: nar_yemb_init: nj must be 1 .. 8");
      n_fa = (long)N_Q * tab_rows * D; n_ia = (long)rows * N_Q; n_ib = rows; n_out = (long)(rows + extra) * D;
      break;
    }
    case VX_DEV_SEAM_ADD_PE_SCATTER: {
      const int rows = dims[0], out_rows = dims[2], pe_rows = dims[3];
      if (!dim_ok(0, 1, ROWS_CAP) || !dim_ok(2, 1, ROWS_CAP) || !dim_ok(3, 1, ROWS_CAP))
        FAIL(VX_EINVAL, "vx_dev_seam_op: add_pe_scatter: rows, out_rows, pe_rows 1 .. %d", ROWS_CAP);
      if (!fa || !fc || !fd || !ic || !id || !out) FAIL(VX_EINVAL, "vx_dev_seam_op: add_pe_scatter: null yemb, alpha, pe, pos, dst or out");
      if (!in_range(ic, rows, 0, pe_rows)) FAIL(VX_EINVAL, "vx_dev_seam_op: add_pe_scatter: a pos outside the pe table");
      if (!in_range(id, rows, 0, out_rows) || !distinct(id, rows, 1)) FAIL(VX_EINVAL, "vx_dev_seam_op: add_pe_scatter: dst outside out or a duplicate in dst");
      n_fa = (long)rows * D; n_fc = 1; n_fd = (long)pe_rows * D; n_ic = rows; n_id = rows; n_out = (long)(out_rows + extra) * D;
      break;
    }
    case VX_DEV_SEAM_EMBED_ACCUM: {
      const int n = dims[0], yrows = dims[2], tab_rows = dims[3];
      if (!dim_ok(0, 1, ROWS_CAP) || !dim_ok(2, 1, ROWS_CAP) || !dim_ok(3, 1, ROWS_CAP))
        FAIL(VX_EINVAL, "vx_dev_seam_op: embed_accum: n, yrows, tab_rows 1 .. %d", ROWS_CAP);
      if (!fa || !ia || !id || !out) FAIL(VX_EINVAL, "vx_dev_seam_op: embed_accum: null tab, tok, rowidx or yemb");
      if (!in_range(ia, n, 0, tab_rows)) FAIL(VX_EINVAL, "vx_dev_seam_op: embed_accum: a tok outside the table");
      if (!in_range(id, n, 0, yrows) || !distinct(id, n, 1)) FAIL(VX_EINVAL, "vx_dev_seam_op: embed_accum: rowidx outside yemb or a duplicate in rowidx");
      n_fa = (long)tab_rows * D; n_ia = n; n_id = n; i_out = (long)yrows * D; n_out = (long)(yrows + extra) * D;
      break;
    }
    case VX_DEV_SEAM_ARGMAX_ROWS: {
      if (!dim_ok(0, 1, ROWS_CAP) || !dim_ok(2, 1, COLS_CAP) || dims[3] < dims[2] || dims[3] > COLS_CAP)
        FAIL(VX_EINVAL, "vx_dev_seam_op: argmax_rows: rows 1 .. %d, N 1 .. %d, N <= ldx <= %d", ROWS_CAP, COLS_CAP, COLS_CAP);
      if (!fa || !iout) FAIL(VX_EINVAL, "vx_dev_seam_op: argmax_rows: null x or idx");
      n_fa = (long)dims[0] * dims[3]; n_iout = dims[0] + extra;
      break;
    }
    case VX_DEV_SEAM_KV_SCATTER: {
      const int M = dims[0], Tmax = dims[2], slots = dims[3];
      if (!dim_ok(0, 1, ROWS_CAP) || !dim_ok(2, 1, ROWS_CAP) || !dim_ok(3, 1, MB)) FAIL(VX_EINVAL, "vx_dev_seam_op: kv_scatter: M, Tmax 1 .. %d, slots 1 .. 32", ROWS_CAP);
      if (!fa || !ia || !ib || !out || !out2) FAIL(VX_EINVAL, "vx_dev_seam_op: kv_scatter: null qkv, row_b, row_t, kc or vc");
      if (!in_range(ia, M, 0, slots) || !in_range(ib, M, 0, Tmax)) FAIL(VX_EINVAL, "vx_dev_seam_op: kv_scatter: a row_b outside the slots or a row_t outside Tmax");
      std::set<long> seen;
      for (int r = 0; r < M; ++r)
        if (!seen.insert((long)ia[r] * Tmax + ib[r]).second) FAIL(VX_EINVAL, "vx_dev_seam_op: kv_scatter: two rows with one (row_b, row_t)");
      n_fa = (long)M * 3 * D; n_ia = n_ib = M; n_out = n_out2 = ((long)slots * N_HEAD * Tmax + extra) * D_HEAD;
      break;
    }
    case VX_DEV_SEAM_GEMV: {
      if (!dim_ok(0, 1, ROWS_CAP) || !dim_ok(2, 4, ROWS_CAP) || dims[2] % 4) FAIL(VX_EINVAL, "vx_dev_seam_op: gemv: N 1 .. %d, K 4 .. %d with K %% 4 == 0", ROWS_CAP, ROWS_CAP);
      if (!fa || !fb || !out) FAIL(VX_EINVAL, "vx_dev_seam_op: gemv: null W, e or out");
      n_fa = (long)dims[0] * dims[2]; n_fb = dims[2]; n_fc = fc ? dims[0] : 0; n_out = dims[0] + extra;
      break;
    }
    case VX_DEV_SEAM_BEAM_FANOUT: {
      const int layers = dims[0], Tmax = dims[2], slots = dims[3], npairs = dims[4], nrows = dims[5], hrows = dims[6];
      if (!dim_ok(0, 1, 64) || !dim_ok(2, 1, ROWS_CAP) || !dim_ok(3, 1, MB) || !dim_ok(4, 0, MB) || !dim_ok(5, 0, MB) || !dim_ok(6, 0, ROWS_CAP) || npairs + nrows < 1)
        FAIL(VX_EINVAL, "vx_dev_seam_op: beam_fanout: layers 1 .. 64, Tmax 1 .. %d, slots 1 .. 32, pairs and rows 0 .. 32 and not both 0, hrows 0 .. %d", ROWS_CAP, ROWS_CAP);
      if (npairs && (!ia || !out || !out2)) FAIL(VX_EINVAL, "vx_dev_seam_op: beam_fanout: pairs without a pair table, kc or vc");
      if (nrows && (!ib || !fa || !out3 || hrows < 1)) FAIL(VX_EINVAL, "vx_dev_seam_op: beam_fanout: rows without hsrc_row, hsrc or dh");
      std::set<int> dsts;
      for (int p = 0; p < npairs; ++p) {
        const int s = ia[3 * p], d = ia[3 * p + 1], len = ia[3 * p + 2];
        if (s < 0 || s >= slots || d < 0 || d >= slots || s == d || len < 0 || len > Tmax)
          FAIL(VX_EINVAL, "vx_dev_seam_op: beam_fanout: pair %d (%d -> %d, %d rows) leaves the %d slots of %d rows", p, s, d, len, slots, Tmax);
        if (!dsts.insert(d).second) FAIL(VX_EINVAL, "vx_dev_seam_op: beam_fanout: slot %d is the destination of two pairs", d);
      }
      for (int p = 0; p < npairs; ++p)
        if (dsts.count(ia[3 * p])) FAIL(VX_EINVAL, "vx_dev_seam_op: beam_fanout: slot %d is a source and a destination (a chained pair)", ia[3 * p]);
      if (nrows && !in_range(ib, nrows, 0, hrows)) FAIL(VX_EINVAL, "vx_dev_seam_op: beam_fanout: an hsrc_row outside hsrc");
      n_ia = 3L * npairs; n_ib = nrows; n_fa = nrows ? (long)hrows * D : 0;
      if (out) { i_out = (long)layers * slots * N_HEAD * Tmax * D_HEAD; n_out = i_out + (long)extra * D_HEAD; }
      if (out2) { i_out2 = (long)layers * slots * N_HEAD * Tmax * D_HEAD; n_out2 = i_out2 + (long)extra * D_HEAD; }
      if (out3) n_out3 = (long)(nrows + extra) * D;
      break;
    }
    case VX_DEV_SEAM_ADMIT_ROWS: {
      const int n = dims[0], hrows = dims[3];
      if (!dim_ok(0, 1, MB) || !dim_ok(3, 1, ROWS_CAP)) FAIL(VX_EINVAL, "vx_dev_seam_op: admit_rows: n 1 .. 32, hrows 1 .. %d", ROWS_CAP);
      if (!ia || !fa || !out3) FAIL(VX_EINVAL, "vx_dev_seam_op: admit_rows: null tab, hsrc or hres");
      for (int i = 0; i < n; ++i)
        if (ia[5 * i] < 0 || ia[5 * i] >= MB || ia[5 * i + 4] < 0 || ia[5 * i + 4] >= hrows)
          FAIL(VX_EINVAL, "vx_dev_seam_op: admit_rows: entry %d: decode row %d outside 0 .. 31 or hsrc row %d outside hsrc", i, ia[5 * i], ia[5 * i + 4]);
      if (!distinct(ia, n, 5)) FAIL(VX_EINVAL, "vx_dev_seam_op: admit_rows: a decode row admitted twice");
      n_ia = 5L * n; n_fa = (long)hrows * D; i_out3 = (long)MB * D; n_out3 = (long)(MB + extra) * D;
      break;
    }
    case VX_DEV_SEAM_ADMIT_MASK:
      if (!dim_ok(0, 1, MB) || !dim_ok(3, 0, 1) || !ia) FAIL(VX_EINVAL, "vx_dev_seam_op: admit_mask: nrows 1 .. 32, phase 0 | 1, admitted not null");
      n_ia = dims[0];
      break;
    case VX_DEV_SEAM_ADMIT_UNIFORMS: {
      const int n = dims[0], steps = dims[2], ncols = dims[3], usteps = dims[4];
      if (!dim_ok(0, 1, MB) || !dim_ok(4, 1, ROWS_CAP) || steps < 1 || steps > usteps || !dim_ok(3, 1, MB))
        FAIL(VX_EINVAL, "vx_dev_seam_op: admit_uniforms: n 1 .. 32, usteps 1 .. %d, steps 1 .. usteps, ncols 1 .. 32", ROWS_CAP);
      if (!ia || !out) FAIL(VX_EINVAL, "vx_dev_seam_op: admit_uniforms: null pairs or u");
      for (int i = 0; i < n; ++i)
        if (ia[2 * i] < 0 || ia[2 * i] >= ncols || ia[2 * i + 1] < 0) FAIL(VX_EINVAL, "vx_dev_seam_op: admit_uniforms: pair %d: column outside u or a negative caller row", i);
      if (!distinct(ia, n, 2)) FAIL(VX_EINVAL, "vx_dev_seam_op: admit_uniforms: a column named twice");
      n_ia = 2L * n; n_fa = fa ? (long)n * steps : 0; i_out = (long)usteps * ncols; n_out = i_out + extra;
      break;
    }
    case VX_DEV_SEAM_SERVE_UNIFORMS: {
      const int n = dims[0], ncols = dims[3], usteps = dims[4], nstaged = dims[5];
      if (!dim_ok(0, 1, MB) || !dim_ok(3, 1, MB) || !dim_ok(4, 1, ROWS_CAP) || nstaged < 0 || nstaged > ELEMS_CAP || (nstaged > 0) != (fa != nullptr))
        FAIL(VX_EINVAL, "vx_dev_seam_op: serve_uniforms: n, ncols 1 .. 32, usteps 1 .. %d, nstaged > 0 with staged draws only", ROWS_CAP);
      if (!ia || !out || !out2) FAIL(VX_EINVAL, "vx_dev_seam_op: serve_uniforms: null tab, u or sum_logp");
      for (int i = 0; i < n; ++i) {
        const int32_t* e = ia + SERVE_UTAB * i;
        if (e[0] < 0 || e[0] >= ncols || e[1] < 0 || e[3] < 0 || e[3] > usteps || e[2] < -1 || (e[2] >= 0 && (long)e[2] + e[3] > nstaged))
          FAIL(VX_EINVAL, "vx_dev_seam_op: serve_uniforms: entry %d: decode row outside u, a negative beam, draws outside 0 .. usteps or staged draws outside `staged`", i);
        max_steps = std::max(max_steps, e[3]);
      }
      if (!distinct(ia, n, SERVE_UTAB)) FAIL(VX_EINVAL, "vx_dev_seam_op: serve_uniforms: a decode row named twice");
      n_ia = (long)SERVE_UTAB * n; n_fa = nstaged; i_out = (long)usteps * ncols; n_out = i_out + extra; i_out2 = MB; n_out2 = MB + extra;
      break;
    }
    case VX_DEV_SEAM_SERVE_CANCEL:
      if (!dim_ok(0, 1, MB)) FAIL(VX_EINVAL, "vx_dev_seam_op: serve_cancel: nrows 1 .. 32");
      break;
    default: {                                     // VX_DEV_SEAM_FORCE_TOKEN
      if (!dim_ok(0, 1, MB) || !ia) FAIL(VX_EINVAL, "vx_dev_seam_op: force_token: batch 1 .. 32, tok not null");
      for (int b = 0; b < dims[0]; ++b)
        if (iout[VX_DEV_SEAM_ST_N_GEN + b] < 0) FAIL(VX_EINVAL, "vx_dev_seam_op: force_token: n_gen[%d] is negative", b);
      n_ia = dims[0];
      break;
    }
  }
  for (long n : {n_fa, n_fb, n_fd, n_out, n_out2, n_out3, n_iout})
    if (n > ELEMS_CAP) FAIL(VX_EINVAL, "vx_dev_seam_op: an operand of more than 2^24 elements");
  HIPCHK(hipSetDevice(c->dev));

  std::vector<void*> allocs;
  auto cleanup = [&]() { for (void* p : allocs) (void)hipFree(p); };
  hipError_t he;
  // an error return drains the ring first: a queued xfer_d2h must not be delivered into host buffers that are gone by then
#define TRY(x) if ((he = (x)) != hipSuccess) { (void)xfer_sync(c); cleanup(); c->err = std::string(#x) + ": " + hipGetErrorString(he); return VX_EHIP; }
#define TRYX(x) do { if (int _e = (x)) { const std::string _m = c->err; (void)xfer_sync(c); c->err = _m; cleanup(); return _e; } } while (0)
  // device copy of a host operand (n words of 4 bytes; null for n == 0)
  auto upload = [&](const void* h, long n, void* dp) -> int {
    void** d = reinterpret_cast<void**>(dp);
    *d = nullptr;
    if (n <= 0) return VX_OK;
    HIPCHK(hipMalloc(d, (size_t)n * 4));
    allocs.push_back(*d);
    return xfer_h2d(c, *d, h, (size_t)n * 4);
  };
  // device output of n words: the sentinel everywhere, then the first n_init words of `init` (an in / out operand)
  auto output = [&](long n, const void* init, long n_init, uint32_t sentinel, void* dp) -> int {
    if (n <= 0) { *reinterpret_cast<void**>(dp) = nullptr; return VX_OK; }
    std::vector<uint32_t> fill((size_t)n, sentinel);
    if (n_init) memcpy(fill.data(), init, (size_t)n_init * 4);
    return upload(fill.data(), n, dp);
  };
  const float sent_f = VX_DEV_SENTINEL_F;
  const int32_t sent_i = VX_DEV_SENTINEL_I;
  uint32_t sf, si;
  memcpy(&sf, &sent_f, 4);
  memcpy(&si, &sent_i, 4);
  float *dfa = nullptr, *dfb = nullptr, *dfc = nullptr, *dfd = nullptr, *dout = nullptr, *dout2 = nullptr, *dout3 = nullptr;
  int *dia = nullptr, *dib = nullptr, *dic = nullptr, *did = nullptr, *diout = nullptr;
  const float** dtabs = nullptr;
  TRYX(upload(fa, n_fa, &dfa));
  TRYX(upload(fb, n_fb, &dfb));
  TRYX(upload(fc, n_fc, &dfc));
  TRYX(upload(fd, n_fd, &dfd));
  TRYX(upload(ia, n_ia, &dia));
  TRYX(upload(ib, n_ib, &dib));
  TRYX(upload(ic, n_ic, &dic));
  TRYX(upload(id, n_id, &did));
  TRYX(output(n_out, out, i_out, sf, &dout));
  TRYX(output(n_out2, out2, i_out2, sf, &dout2));
  TRYX(output(n_out3, out3, i_out3, sf, &dout3));
  TRYX(output(n_iout, iout, i_iout, si, &diout));
  if (op == VX_DEV_SEAM_NAR_YEMB_INIT) {           // the device array of the 8 table pointers, as the loader builds it
    const float* tabs[N_Q];
    for (int j = 0; j < N_Q; ++j) tabs[j] = dfa + (long)j * dims[2] * D;
    TRY(hipMalloc((void**)&dtabs, sizeof tabs));
    allocs.push_back((void*)dtabs);
    TRYX(xfer_h2d(c, (void*)dtabs, tabs, sizeof tabs));
  }
  int* const st = diout;                           // the state block of a state op
  hipStream_t s = c->stream;
  switch (op) {
    case VX_DEV_SEAM_EMBED_ROWS: launch_embed_rows(dout, did, dfa, dia, dfb, dib, dfc, dfd, dic, dims[0], s); break;
    case VX_DEV_SEAM_NAR_YEMB_INIT: launch_nar_yemb_init(dout, dtabs, dia, dib, dims[0], s); break;
    case VX_DEV_SEAM_ADD_PE_SCATTER: launch_add_pe_scatter(dout, did, dfa, dfc, dfd, dic, dims[0], s); break;
    case VX_DEV_SEAM_EMBED_ACCUM: launch_embed_accum(dout, did, dfa, dia, dims[0], s); break;
    case VX_DEV_SEAM_ARGMAX_ROWS: launch_argmax_rows(dfa, dims[3], dims[0], dims[2], diout, s); break;
    case VX_DEV_SEAM_KV_SCATTER: launch_kv_scatter(dfa, dia, dib, dims[0], dout, dout2, dims[2], s); break;
    case VX_DEV_SEAM_GEMV: launch_gemv(dfa, dfb, dfc, dout, dims[0], dims[2], s); break;
    case VX_DEV_SEAM_BEAM_FANOUT:
      launch_beam_fanout(dout, dout2, (long)dims[3] * N_HEAD * dims[2] * D_HEAD, dims[0], dims[2], dia, dims[4], dfa, dib, dout3, dims[5], s);
      break;
    case VX_DEV_SEAM_ADMIT_ROWS:
      launch_admit_rows(dia, dims[0], dfa, dout3, st + VX_DEV_SEAM_ST_CUR_TOK, st + VX_DEV_SEAM_ST_CUR_POS, st + VX_DEV_SEAM_ST_CTX_LEN,
                        st + VX_DEV_SEAM_ST_N_GEN, st + VX_DEV_SEAM_ST_TEXT_LEN, st + VX_DEV_SEAM_ST_SLOT_META, st + VX_DEV_SEAM_ST_SLOT_OF, s);
      break;
    case VX_DEV_SEAM_ADMIT_MASK:
      launch_admit_mask(dims[3], dia, st + VX_DEV_SEAM_ST_SAVED, dims[0], st + VX_DEV_SEAM_ST_ACTIVE, st + VX_DEV_SEAM_ST_SLOT_META,
                        st + VX_DEV_SEAM_ST_SLOT_OF, st + VX_DEV_SEAM_ST_N_ACTIVE, s);
      break;
    case VX_DEV_SEAM_ADMIT_UNIFORMS:
      launch_admit_uniforms(dia, dims[0], dfa, dims[2], (unsigned long long)(uint32_t)dims[5] | ((unsigned long long)(uint32_t)dims[6] << 32), dout,
                            dims[3], s);
      break;
    case VX_DEV_SEAM_SERVE_UNIFORMS:
      launch_serve_uniforms(dia, dims[0], max_steps, dfa, dout, dims[3], dout2, st + VX_DEV_SEAM_ST_ROW_SMP, st + VX_DEV_SEAM_ST_ROW_FLT, s);
      break;
    case VX_DEV_SEAM_SERVE_CANCEL:
      launch_serve_cancel((unsigned)dims[3], dims[0], st + VX_DEV_SEAM_ST_ACTIVE, st + VX_DEV_SEAM_ST_SLOT_META, st + VX_DEV_SEAM_ST_SLOT_OF,
                          st + VX_DEV_SEAM_ST_N_ACTIVE, s);
      break;
    default:
      launch_dec_force_token(dia, st + VX_DEV_SEAM_ST_CUR_TOK, st + VX_DEV_SEAM_ST_CUR_POS, st + VX_DEV_SEAM_ST_CTX_LEN, st + VX_DEV_SEAM_ST_N_GEN,
                             st + VX_DEV_SEAM_ST_GEN, gen_stride, st + VX_DEV_SEAM_ST_ACTIVE, dims[0], st + VX_DEV_SEAM_ST_SLOT_META,
                             st + VX_DEV_SEAM_ST_SLOT_OF, s);
      break;
  }
  if (dout) TRYX(xfer_d2h(c, out, dout, (size_t)n_out * 4));
  if (dout2) TRYX(xfer_d2h(c, out2, dout2, (size_t)n_out2 * 4));
  if (dout3) TRYX(xfer_d2h(c, out3, dout3, (size_t)n_out3 * 4));
  if (diout) TRYX(xfer_d2h(c, iout, diout, (size_t)n_iout * 4));
  TRYX(xfer_sync(c));
  TRY(hipGetLastError());
#undef TRY
#undef TRYX
  cleanup();
  return VX_OK;
}

}  // extern "C"
