// Engine: context, weight ingest, arenas, launch sequences and the C ABI (include/vallex_hip.h).
// Host-side counterpart of VALLE.inference (models/vallex.py:458-686) + the Vocos call of
// utils/generation.py:148-150; every hot op is a hand-written gfx950 kernel from the sibling .hip files.
#include "engine_ctx.h"

#include <deque>
#include <memory>

namespace {
// the message of a failed vx_create (no context to hang it on): per thread, contexts are created from several host threads
// (bench.py --contexts) and vx_last_error(NULL) must not read a string another thread is assigning
thread_local std::string g_create_err;
}  // namespace

namespace vxe {

const float* W(vx_ctx* c, const std::string& name) {
  auto it = c->w.find(name);
  return it == c->w.end() ? nullptr : it->second.d;
}

// ---- pinned transfer ring (engine_ctx.h: PinRing) ----------------------------------------------------------
static int ring_slot(vx_ctx* c, size_t n, char** slot) {
  PinRing& r = c->ring;
  if (!r.base) FAIL(VX_ESTATE, "the context has no pinned transfer ring");
  const size_t a = (n + 255) & ~(size_t)255;
  if (r.head + a > r.cap) if (int e = xfer_sync(c)) return e;
  *slot = r.base + r.head;
  r.head += a;
  return VX_OK;
}

int xfer_h2d(vx_ctx* c, void* dst_dev, const void* src_host, size_t bytes) {
  const char* s = static_cast<const char*>(src_host);
  char* d = static_cast<char*>(dst_dev);
  while (bytes) {
    const size_t n = std::min(bytes, XFER_CHUNK);
    char* slot = nullptr;
    if (int e = ring_slot(c, n, &slot)) return e;
    memcpy(slot, s, n);
    HIPCHK(hipMemcpyAsync(d, slot, n, hipMemcpyHostToDevice, c->stream));
    s += n; d += n; bytes -= n;
  }
  return VX_OK;
}

int xfer_d2h(vx_ctx* c, void* dst_host, const void* src_dev, size_t bytes) {
  char* d = static_cast<char*>(dst_host);
  const char* s = static_cast<const char*>(src_dev);
  while (bytes) {
    const size_t n = std::min(bytes, XFER_CHUNK);
    char* slot = nullptr;
    if (int e = ring_slot(c, n, &slot)) return e;
    HIPCHK(hipMemcpyAsync(slot, s, n, hipMemcpyDeviceToHost, c->stream));
    c->ring.pend.push_back({d, slot, n});
    s += n; d += n; bytes -= n;
  }
  return VX_OK;
}

int xfer_sync(vx_ctx* c) {
  const hipError_t e = hipStreamSynchronize(c->stream);
  PinRing& r = c->ring;
  if (e == hipSuccess) {
    size_t total = 0;
    for (const PinRing::Pend& p : r.pend) total += p.n;
    if (total < ((size_t)4 << 20)) {
      for (const PinRing::Pend& p : r.pend) memcpy(p.dst, p.src, p.n);
    } else {
      // a large delivery (the audio of a batch: 24.6 MB for 32 x 8 s) is cut into ~1 MiB pieces and copied by four host threads: one
      // thread moves ~10 GB/s out of the ring, i.e. 2.5 ms behind a Vocos pass whose GEMMs take 4 ms
      struct Piece { char* dst; const char* src; size_t n; };
      std::vector<Piece> pieces;
      for (const PinRing::Pend& p : r.pend)
        for (size_t o = 0; o < p.n; o += (size_t)1 << 20)
          pieces.push_back({static_cast<char*>(p.dst) + o, p.src + o, std::min((size_t)1 << 20, p.n - o)});
      constexpr int NT = 4;
      std::thread th[NT - 1];
      auto work = [&pieces](int k) { for (size_t i = k; i < pieces.size(); i += NT) memcpy(pieces[i].dst, pieces[i].src, pieces[i].n); };
      bool started[NT - 1] = {};
      for (int k = 1; k < NT; ++k) {
        try { th[k - 1] = std::thread(work, k); started[k - 1] = true; }
        catch (...) {}                                  // no thread to be had: this share is copied here, below (nothing crosses the C ABI)
      }
      work(0);
      for (int k = 1; k < NT; ++k) {
        if (started[k - 1]) th[k - 1].join();
        else work(k);
      }
    }
  }
  r.pend.clear();
  r.head = 0;
  HIPCHK(e);
  return VX_OK;
}

// ---- int metadata upload ---------------------------------------------------------------------------------
int upload_meta(vx_ctx* c) {
  if ((long)c->hmeta.size() > c->imeta_cap) FAIL(VX_EINVAL, "row metadata overflow (%zu > %ld)", c->hmeta.size(), c->imeta_cap);
  H2D(c->imeta, c->hmeta.data(), c->hmeta.size() * sizeof(int));      // staged: the host vector is free for the next call
  return VX_OK;
}

int tap_store(vx_ctx* c, const std::string& name, const float* src, size_t n) {
  if (!c->cfg.debug_taps) return VX_OK;
  Tensor& t = c->taps[name];
  if (t.n < n) {
    void* q = nullptr;
    HIPCHK(hipMalloc(&q, n * sizeof(float)));
    c->allocs.push_back(q);
    t.d = reinterpret_cast<float*>(q);
  }
  t.n = n;
  HIPCHK(hipMemcpyAsync(t.d, src, n * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  return VX_OK;
}

// ---- dense helpers -----------------------------------------------------------------------------------------
void gemm(vx_ctx* c, const float* A, int lda, const float* Wt, int ldw, const float* bias, const float* resid, int ldr,
          const float* colscale, float* C, int ldc, long M, int N, int K, int act, const int* gather, int cls, const int* resid_rows) {
  GemmArgs g{};
  g.A = A; g.lda = lda; g.W = Wt; g.ldw = ldw; g.bias = bias; g.resid = resid; g.ldr = ldr; g.colscale = colscale;
  g.C = C; g.ldc = ldc; g.M = (int)M; g.N = N; g.K = K; g.act = act; g.row_gather = gather; g.resid_rows = resid_rows;
  ProfScope ps(c, cls);               // class 2 = transformer projections (proj), 4 = the fp32 GEMMs of Vocos / EnCodec
  if (c->prof_on) c->prof[cls].bytes += 2.0 * (double)M * N * K;      // flops for this class
  launch_gemm_f32(g, c->stream);
}

// transformer projection (F.linear of modules/activation.py:144,166, modules/transformer.py:371-373, models/vallex.py:677)
// f16x2 mode extras: `a_pre` = A operand already in plane form (skip the split pass); `out_pl` = write the result as the next
// GEMM's A planes (K = N) instead of fp32 rows (C may then be null).
void proj(vx_ctx* c, const float* A, int lda, const float* Wf, const unsigned short* W3, const float* bias,
          const float* resid, int ldr, float* C, int ldc, long M, int N, int K, int act, const int* gather,
          const unsigned short* a_pre, unsigned short* out_pl, const int* resid_rows) {
  if (c->gemm_mode == 2 || !W3) {
    gemm(c, A, lda, Wf, K, bias, resid, ldr, nullptr, C, ldc, M, N, K, act, gather, 2, resid_rows);
    return;
  }
  const long a_plane = c->gemm_mode == 0 ? h2_plane(M, K, H2_TILE_A) : (long)M * K;
  if (!a_pre) {
    if (c->gemm_mode == 0) launch_split2h(A, lda, M, K, gather, c->fa3, a_plane, H2_TILE_A, c->range_flag, H2_ACT_SCALE, c->stream);
    else launch_split3(A, lda, M, K, gather, c->fa3, a_plane, c->stream);
  }
  GemmX3Args g{};
  g.A = a_pre ? a_pre : c->fa3; g.a_plane = a_plane; g.W = W3; g.w_plane = c->gemm_mode == 0 ? h2_plane(N, K, H2_TILE_W) : (long)N * K;
  g.bias = bias; g.resid = resid; g.ldr = ldr;
  g.colscale = nullptr; g.C = C; g.ldc = ldc; g.M = (int)M; g.N = N; g.K = K; g.act = act;
  g.out_planes = out_pl; g.out_plane = out_pl ? h2_plane(M, N, H2_TILE_A) : 0; g.range_flag = c->range_flag;
  g.resid_rows = resid_rows;                     // f16x2 kernel only (the one mode that trims rows)
  if (c->gemm_mode == 0) g.descale = ldexpf(1.0f, -(H2_ACT_SHIFT + c->w_shift.at(W3)));
  ProfScope ps(c, 2);
  if (c->prof_on) c->prof[2].bytes += 2.0 * (double)M * N * K;
  if (c->gemm_mode == 0) launch_gemm_f16x2(g, c->stream);
  else if (M >= 1024) launch_gemm_bf16x3_dma(g, c->stream);        // 256-row tiles: not for short row sets
  else launch_gemm_bf16x3(g, c->stream);
}

// Row trimming of the LAST decoder layer of a NAR stage (f16x2 mode, and since round 6 the reference-arithmetic fp32 mode): only the generated frames of every sequence reach a predict
// layer (models/vallex.py:672-679), so behind the K / V projection -- which attention needs for ALL rows -- the layer only has to
// produce those rows: attention queries, out_proj, norm2 and the FFN run on the Mc = sum T_b compacted rows.  Every op of the
// block treats rows independently, so each kept row goes through exactly the arithmetic it would see untrimmed: same ids, same
// logits, bit for bit.  The compacted residual stream lives in c->fxn (f16x2 mode: unused otherwise) or in the QKV buffer (fp32 mode).
// (struct Trim: engine_ctx.h -- the teacher-forced scoring passes of score.hip trim the same way)

// one pre-norm block on packed rows (modules/transformer.py:296-302 / :337-347) -- shared by AR prefill and NAR
int full_layer(vx_ctx* c, const LayerW& L, long M, const int* seq_off, const int* seq_len, const int* prefix_len,
               int batch, int max_len, const float* ada1, const float* ada2, float* kcl, float* vcl,
               const int* row_b, const int* row_t, double attn_flops, const Trim* tr) {
  // f16x2 mode: every producer of a GEMM operand (the two LayerNorms, the attention, linear1's epilogue) writes the operand
  // planes itself -- no fp32 round trip of the normalised / attended / hidden activations and no split pass on any edge.
  const bool pl = c->gemm_mode == 0;
  const long pl1024 = h2_plane(M, D_MODEL, H2_TILE_A);
  launch_layernorm(c->fx, D_MODEL, pl ? nullptr : c->fxn, D_MODEL, (int)M, D_MODEL, LN_EPS, L.n1_w, L.n1_b, ada1,
                   ada1 ? ada1 + D_MODEL : nullptr, c->stream, pl ? c->fa3 : nullptr, pl1024, c->range_flag);
  proj(c, c->fxn, D_MODEL, L.in_w, L.in_w3, L.in_b, nullptr, 0, c->fqkv, 3 * D_MODEL, M, 3 * D_MODEL, D_MODEL, ACT_NONE, nullptr,
       pl ? c->fa3 : nullptr);
  if (kcl) launch_kv_scatter(c->fqkv, row_b, row_t, (int)M, kcl, vcl, c->Tmax, c->stream);
  const bool att_pl = pl && c->attn_x3;
  if (tr && !pl) {
    // reference arithmetic (fp32 projections + fp32 attention, round 6): the same trimming on fp32 rows.  The compacted residual
    // stream lives in the QKV buffer, which is free once the attention has read it (stream order); fatt / fxn / fffn hold the
    // compacted attention output, normalised rows and hidden activations.  gemm_f32 reads the residual of out_proj through the row
    // map (GemmArgs.resid_rows); every kept row goes through the arithmetic it would see untrimmed.
    float* xc = c->fqkv;
    {
      ProfScope ps(c, 3);
      if (c->prof_on) c->prof[3].bytes += tr->attn_flops;
      launch_attn_full(c->fqkv, c->fatt, seq_off, seq_len, prefix_len, batch, max_len, c->stream, tr->q_first, tr->c_off);
    }
    proj(c, c->fatt, D_MODEL, L.out_w, L.out_w3, L.out_b, c->fx, D_MODEL, xc, D_MODEL, tr->Mc, D_MODEL, D_MODEL, ACT_NONE, nullptr, nullptr,
         nullptr, tr->rows);
    launch_layernorm(xc, D_MODEL, c->fxn, D_MODEL, (int)tr->Mc, D_MODEL, LN_EPS, L.n2_w, L.n2_b, ada2, ada2 ? ada2 + D_MODEL : nullptr,
                     c->stream);
    proj(c, c->fxn, D_MODEL, L.l1_w, L.l1_w3, L.l1_b, nullptr, 0, c->fffn, D_FF, tr->Mc, D_FF, D_MODEL, ACT_RELU);
    proj(c, c->fffn, D_FF, L.l2_w, L.l2_w3, L.l2_b, xc, D_MODEL, xc, D_MODEL, tr->Mc, D_MODEL, D_FF, ACT_NONE);
    return VX_OK;
  }
  if (tr) {                                        // f16x2 projections + f16x2 attention
    const long plc = h2_plane(tr->Mc, D_MODEL, H2_TILE_A);
    {
      ProfScope ps(c, 3);
      if (c->prof_on) c->prof[3].bytes += tr->attn_flops;
      launch_attn_full_h2(c->fqkv, nullptr, seq_off, seq_len, prefix_len, batch, max_len, c->stream, c->fa3, plc, c->range_flag, -1,
                          tr->q_first, tr->c_off);
    }
    // x' = x[kept rows] + out_proj(attention): residual read through the row map, result compacted in fxn
    proj(c, nullptr, D_MODEL, L.out_w, L.out_w3, L.out_b, c->fx, D_MODEL, c->fxn, D_MODEL, tr->Mc, D_MODEL, D_MODEL, ACT_NONE, nullptr,
         c->fa3, nullptr, tr->rows);
    launch_layernorm(c->fxn, D_MODEL, nullptr, D_MODEL, (int)tr->Mc, D_MODEL, LN_EPS, L.n2_w, L.n2_b, ada2, ada2 ? ada2 + D_MODEL : nullptr,
                     c->stream, c->fa3, plc, c->range_flag);
    proj(c, nullptr, D_MODEL, L.l1_w, L.l1_w3, L.l1_b, nullptr, 0, nullptr, D_FF, tr->Mc, D_FF, D_MODEL, ACT_RELU, nullptr, c->fa3, c->fa3b);
    proj(c, nullptr, D_FF, L.l2_w, L.l2_w3, L.l2_b, c->fxn, D_MODEL, c->fxn, D_MODEL, tr->Mc, D_MODEL, D_FF, ACT_NONE, nullptr, c->fa3b);
    return VX_OK;
  }
  {
    ProfScope ps(c, 3);
    if (c->prof_on) c->prof[3].bytes += attn_flops;
    if (c->attn_x3 && c->attn_h2)
      launch_attn_full_h2(c->fqkv, att_pl ? nullptr : c->fatt, seq_off, seq_len, prefix_len, batch, max_len, c->stream,
                          att_pl ? c->fa3 : nullptr, pl1024, c->range_flag);
    else if (c->attn_x3)
      launch_attn_full_x3(c->fqkv, att_pl ? nullptr : c->fatt, seq_off, seq_len, prefix_len, batch, max_len, 0, c->stream,
                          att_pl ? c->fa3 : nullptr, pl1024);
    else launch_attn_full(c->fqkv, c->fatt, seq_off, seq_len, prefix_len, batch, max_len, c->stream);
  }
  proj(c, c->fatt, D_MODEL, L.out_w, L.out_w3, L.out_b, c->fx, D_MODEL, c->fx, D_MODEL, M, D_MODEL, D_MODEL, ACT_NONE, nullptr,
       att_pl ? c->fa3 : nullptr);
  launch_layernorm(c->fx, D_MODEL, pl ? nullptr : c->fxn, D_MODEL, (int)M, D_MODEL, LN_EPS, L.n2_w, L.n2_b, ada2,
                   ada2 ? ada2 + D_MODEL : nullptr, c->stream, pl ? c->fa3 : nullptr, pl1024, c->range_flag);
  if (pl) {
    // linear1's epilogue writes relu(x W1^T + b1) directly as linear2's A planes
    proj(c, nullptr, D_MODEL, L.l1_w, L.l1_w3, L.l1_b, nullptr, 0, nullptr, D_FF, M, D_FF, D_MODEL, ACT_RELU, nullptr, c->fa3, c->fa3b);
    proj(c, nullptr, D_FF, L.l2_w, L.l2_w3, L.l2_b, c->fx, D_MODEL, c->fx, D_MODEL, M, D_MODEL, D_FF, ACT_NONE, nullptr, c->fa3b);
  } else {
    proj(c, c->fxn, D_MODEL, L.l1_w, L.l1_w3, L.l1_b, nullptr, 0, c->fffn, D_FF, M, D_FF, D_MODEL, ACT_RELU);
    proj(c, c->fffn, D_FF, L.l2_w, L.l2_w3, L.l2_b, c->fx, D_MODEL, c->fx, D_MODEL, M, D_MODEL, D_FF, ACT_NONE);
  }
  return VX_OK;
}

// ---- f16x2 range guard ---------------------------------------------------------------------------------------------
// The f16x2 kernels need every scaled operand to fit fp16: |LayerNorm / attention / ReLU'd FFN activation| < 2047, |q|/8, |k|,
// |v| < 2047 (vx_common.h).  The reference puts no bound on any of them (fp32 throughout: modules/transformer.py:371-373,
// modules/activation.py:144-166), and trained transformers are known for massive activations.  The producers of the operand
// planes raise `range_flag`; it is read at a host sync the phase has anyway (no extra round trip in the common case) and a
// raised flag RE-RUNS THE PHASE on the exact-fp32 kernels (gemm_f32 / attn_full: the reference's own arithmetic, fp32 weights
// are resident, the two extra activation buffers are allocated on first use) -- the call never fails and never returns
// non-finite garbage because of the reduced-operand format.  vx_last_fallbacks() reports how often that happened.
bool range_guarded(const vx_ctx* c) { return c->gemm_mode == 0 || (c->attn_x3 && c->attn_h2); }


int ensure_f32_buffers(vx_ctx* c) {
  const long M = c->Mmax + 128;
  if (!c->fatt) if (int e = dev_alloc(c, &c->fatt, (size_t)M * D_MODEL)) return e;
  if (!c->fffn) if (int e = dev_alloc(c, &c->fffn, (size_t)M * D_FF)) return e;
  return VX_OK;
}

// synchronous read-and-clear (paths without a sync of their own: vx_finalize_weights, the vx_ar_prefill test seam)
int take_range_flag(vx_ctx* c, bool* raised) {
  *raised = false;
  if (!range_guarded(c)) return VX_OK;
  int flag = 0;
  D2H(&flag, c->range_flag, sizeof(int));
  SYNC();
  if (flag) HIPCHK(hipMemsetAsync(c->range_flag, 0, sizeof(int), c->stream));
  *raised = flag != 0;
  return VX_OK;
}

int check_batch(vx_ctx* c, const vx_batch* b, int max_rows) {
  if (!c->finalized) FAIL(VX_ESTATE, "weights not finalized");
  if (!b) FAIL(VX_EINVAL, "null batch");
  if (b->struct_size != sizeof(vx_batch))
    FAIL(VX_EINVAL, "vx_batch.struct_size is %u, this library expects %zu (ABI version %d)", b->struct_size, sizeof(vx_batch), VX_ABI_VERSION);
  if (b->batch <= 0 || b->batch > max_rows) FAIL(VX_EINVAL, "batch must be in 1..%d", max_rows);
  for (int i = 0; i < b->batch; ++i) {
    const int S = b->text_lens[i], Tp = b->prompt_lens[i];
    if (S <= 0) FAIL(VX_EINVAL, "x_lens must be > 0 (models/vallex.py:493)");       // assert torch.all(x_lens > 0)
    if (S > c->cfg.max_text || S > b->text_stride) FAIL(VX_EINVAL, "row %d: text length %d exceeds max_text", i, S);
    if (Tp < 0 || Tp > c->cfg.max_prompt || Tp > b->prompt_stride)
      FAIL(VX_EINVAL, "row %d: prompt length %d exceeds max_prompt", i, Tp);
    for (int s = 0; s < S; ++s) {
      const int id = b->text_ids[(long)i * b->text_stride + s], lg = b->text_lang[(long)i * b->text_stride + s];
      if (id < 0 || id >= 2048) FAIL(VX_EINVAL, "row %d: text id %d out of range", i, id);
      if (lg < -1 || lg > 2) FAIL(VX_EINVAL, "row %d: language id %d out of range", i, lg);   // -1: no language embedding
    }
    for (int t = 0; t < Tp * N_Q; ++t) {
      const int v = b->prompt_codes[(long)i * b->prompt_stride * N_Q + t];
      if (v < 0 || v >= AUDIO_VOCAB) FAIL(VX_EINVAL, "row %d: prompt code %d out of range", i, v);
    }
  }
  return VX_OK;
}

// ---- AR prefill (models/vallex.py:497-562, first ar_decoder.infer call) ------------------------------------
// The full-sequence part of a prefill (tables, embeddings, the prefix-LM layers that fill the KV arena) is shared by the first fill
// of a decode batch (ar_prefill) and by the admission of waiting rows into a running one (continuous schedule, admit_rows below).
// prefill_tables builds the sequence tables of caller rows r0 .. r0+nb-1 into `mb`; row_b (the arena slot of every packed row) is
// left as PREFILL row indices: the caller maps them to slots and adds them (o_rb) before upload_meta.
int prefill_tables(vx_ctx* c, const vx_batch* b, int r0, int nb, PrefillPlan& p, MetaBuilder& mb) {
  p.nb = nb;
  p.seq_off.assign(nb, 0); p.seq_len.assign(nb, 0); p.S_.assign(nb, 0);
  std::vector<int> dst_t, id_t, lang_t, pos_t, dst_a, id_a, pos_a, row_t;
  p.row_b.clear();
  long M = 0;
  int max_len = 0;
  for (int i = 0; i < nb; ++i) {
    const int r = r0 + i, S = b->text_lens[r], Tp = b->prompt_lens[r];
    p.seq_off[i] = (int)M; p.seq_len[i] = S + 1 + Tp; p.S_[i] = S;
    max_len = std::max(max_len, p.seq_len[i]);
    for (int s = 0; s < S; ++s) {
      dst_t.push_back((int)M + s);
      id_t.push_back(b->text_ids[(long)r * b->text_stride + s]);
      lang_t.push_back(b->text_lang[(long)r * b->text_stride + s]);
      pos_t.push_back(s);
    }
    for (int t = 0; t <= Tp; ++t) {                       // BOS then prompt codebook 0 (models/vallex.py:515-517)
      dst_a.push_back((int)M + S + t);
      id_a.push_back(t == 0 ? BOS_ID : b->prompt_codes[((long)r * b->prompt_stride + (t - 1)) * N_Q]);
      pos_a.push_back(t);
    }
    for (int t = 0; t < p.seq_len[i]; ++t) { p.row_b.push_back(i); row_t.push_back(t); }
    M += p.seq_len[i];
  }
  if (M > c->Mmax) FAIL(VX_EINVAL, "prefill rows %ld exceed arena %ld", M, c->Mmax);
  p.M = M; p.max_len = max_len;
  p.n_t = (int)dst_t.size(); p.n_a = (int)dst_a.size();
  p.o_off = mb.add(p.seq_off); p.o_len = mb.add(p.seq_len); p.o_S = mb.add(p.S_); p.o_dt = mb.add(dst_t); p.o_it = mb.add(id_t);
  p.o_lt = mb.add(lang_t); p.o_pt = mb.add(pos_t); p.o_da = mb.add(dst_a); p.o_ia = mb.add(id_a); p.o_pa = mb.add(pos_a);
  p.o_rt = mb.add(row_t);
  // Row trimming of the LAST prefill layer (round 6; struct Trim): the decode only continues from the last row of every sequence
  // (models/vallex.py:568: the logits of the newest position), so behind the K / V projection -- the cache needs every row -- the last
  // layer runs its attention queries, out_proj and FFN on nb rows instead of M.
  std::vector<int> tq_first(nb), tc_off(nb), t_rows(nb);
  p.trim_flops = 0;
  for (int i = 0; i < nb; ++i) {
    tq_first[i] = p.seq_len[i] - 1; tc_off[i] = i; t_rows[i] = p.seq_off[i] + p.seq_len[i] - 1;
    p.trim_flops += 4.0 * p.seq_len[i] * D_MODEL;
  }
  p.o_tq = mb.add(tq_first); p.o_tc = mb.add(tc_off); p.o_tr = mb.add(t_rows);
  p.trim_h2 = c->gemm_mode == 0 && c->attn_x3 && c->attn_h2;
  const bool trim_f32 = c->gemm_mode == 2 && !c->attn_x3;
  p.trim = c->nar_trim && (p.trim_h2 || trim_f32) && !c->cfg.debug_taps;      // the same switch as the NAR stages (VX_NAR_TRIM)
  return VX_OK;
}

// embeddings + the prefix-LM layers (K / V into the arena slots of p.row_b); the last row of every sequence is then row
// p.hrow(i) of prefill_hsrc(c, p)
int prefill_layers(vx_ctx* c, const PrefillPlan& p, const MetaBuilder& mb) {
  const int NL = c->NL, nb = p.nb;
  launch_embed_rows(c->fx, mb.dev(p.o_dt), W(c, "ar_text_embedding.word_embeddings.weight"), mb.dev(p.o_it),
                    W(c, "ar_language_embedding.word_embeddings.weight"), mb.dev(p.o_lt), W(c, "ar_text_position.alpha"),
                    c->pe, mb.dev(p.o_pt), p.n_t, c->stream);
  launch_embed_rows(c->fx, mb.dev(p.o_da), W(c, "ar_audio_embedding.word_embeddings.weight"), mb.dev(p.o_ia), nullptr,
                    nullptr, W(c, "ar_audio_position.alpha"), c->pe, mb.dev(p.o_pa), p.n_a, c->stream);
  if (int e = tap_store(c, "ar_prefill_in", c->fx, (size_t)p.M * D_MODEL)) return e;

  double attn_flops = 0;
  for (int i = 0; i < nb; ++i) attn_flops += 4.0 * p.seq_len[i] * (double)p.seq_len[i] * D_MODEL;
  const size_t cache_layer = (size_t)c->mbr * N_HEAD * c->Tmax * D_HEAD;
  const Trim tr{nb, mb.dev(p.o_tq), mb.dev(p.o_tc), mb.dev(p.o_tr), p.trim_flops};
  for (int l = 0; l < NL; ++l) {
    if (int e = full_layer(c, c->ar[l], p.M, mb.dev(p.o_off), mb.dev(p.o_len), mb.dev(p.o_S), nb, p.max_len, nullptr, nullptr,
                           c->kc + l * cache_layer, c->vc + l * cache_layer, mb.dev(p.o_rb), mb.dev(p.o_rt), attn_flops,
                           (p.trim && l == NL - 1) ? &tr : nullptr))
      return e;
    if (c->cfg.debug_taps) {
      char nm[64];
      snprintf(nm, sizeof nm, "ar_layer_out.%d", l);
      if (int e = tap_store(c, nm, c->fx, (size_t)p.M * D_MODEL)) return e;
    }
  }
  return VX_OK;
}

// the buffer that holds the last row of every sequence behind prefill_layers (trimmed: the last layer left exactly those rows,
// compacted, in the buffer full_layer uses for the compacted residual stream: fxn in f16x2 mode, the QKV buffer in fp32 mode)
const float* prefill_hsrc(const vx_ctx* c, const PrefillPlan& p) { return p.trim ? (p.trim_h2 ? c->fxn : c->fqkv) : c->fx; }

// Decode geometry of a decode batch of nrows rows: context splits of dec_attn, chain choice (host state only; the first fill of a
// decode batch sets it through ar_prefill, a serving session once for its nd free rows, serve_setup).  `identity`: the launch slot
// order is the identity (slot == row).
void decode_geometry(vx_ctx* c, int nrows, bool identity) {
  // enough (row, head, split) 8-wave workgroups to put >= 2 on every CU; one split (no combine launch) from 32 rows up
  c->nsplit = std::max(1, std::min(16, 512 / (nrows * N_HEAD)));
  // 5 .. 16 rows: ONE 8-wave workgroup per CU (256 / (rows x 16) splits, at least 2) -- round 6 sweep at 5 / 8 / 12 / 16 rows x contexts
  // ~500 / ~1300 (profiles/r06_sb_sweep2.txt): 5 rows 6 -> 3 splits -3.5 %, 8 rows 4 -> 2 splits -3 % / -0.6 % of the AR phase, 12 and 16 rows
  // stay at 2; one split (the fused out_proj) only pays from 17 rows up
  if (nrows > SB_ROWS && nrows <= 16) c->nsplit = std::max(2, 256 / (nrows * N_HEAD));
  // 8 .. 16 rows (round 6, profiles/r06_fuse_split_sweep.txt): out_proj folded into dec_attn WITH context splits -- the combine moves behind the
  // head's W_o slice (decode.hip dec_attn_kernel<true, *, true>, dec_reduce_ln_split_kernel), two launches per layer fewer.  The fused
  // kernel runs two rows per 16-wave workgroup: as many splits (<= 4) as keep 16 heads x row pairs x splits inside ONE round of the 256 CUs
  // (8 rows: 4, 9 .. 10: 3, 11 .. 16: 2; AR phase -2.7 % at 8 rows / context ~1000, -7 % at 10 rows, -5.5 % at 12, -4.6 % at 16).  5 .. 7 rows:
  // too few workgroups either way, the unfused chain stays (5 rows: 297 vs 299 ms, 6 rows: 302 vs 302).
  c->split_fused = false;
  if (c->fuse_out && c->fuse_split == 1 && nrows >= 8 && nrows <= 16) {
    const int ns = std::min(4, 256 / (N_HEAD * ((nrows + 1) / 2)));
    if (ns >= 2) { c->nsplit = ns; c->split_fused = true; }
  }
  if (c->att_nsplit_force > 0) {                                      // measurement switches (tools/gpu_call.sh sb_sweep, tools/fuse_split_sweep.sh)
    c->nsplit = c->att_nsplit_force;
    c->split_fused = c->fuse_out && c->fuse_split != 0 && nrows > SB_ROWS && c->nsplit >= 2 && c->nsplit <= 4;
  }
  // the small-batch chain compiles the split counts in (decode.hip): taken only for a combination that is instantiated.  Its fused
  // attention relies on slot == row, i.e. on the identity launch order (<= SB_ROWS rows are never balanced; best_of: the beams of
  // row i are decode rows i*beams + j in that order) -- passed by the caller (ar_prefill checks its slot order, it does not assume it
  // from its `balance` rule)
  c->sb_chain = false;
  c->sb_qkv = false;
  if (c->sb_fuse && nrows <= SB_ROWS && identity) {
    const int ns = nrows <= 2 ? 16 : 8;
    if (sb_chain_supported(SK_L2, SK_OUT, ns, nrows)) { c->nsplit = ns; c->sb_chain = true; }
    // ... with norm1 + QKV inside the attention launch for the smallest batches (VX_SB_QKV=<max rows>; its split count is tunable)
    if (c->sb_chain && nrows <= c->sb_qkv_rows) {
      // the fused kernel holds one 8-wave workgroup per CU: 16 heads x rows x splits workgroups must fit the 256 CUs in ONE round,
      // and every workgroup of a head re-reads the head's q slice through L2 -- few splits win (profiles/r04_sb_qkv_ab.log)
      // one row: 16 splits = 256 workgroups (round 6 sweep, profiles/r06_sb_sweep.txt: equal to 8 at contexts ~400 / ~800, -2 % of the AR
      // phase at ~1300 -- the context share of a workgroup halves while the q slice it re-reads through L2 stays)
      const int fit[5] = {0, 16, 8, 4, 4};
      const int ns2 = c->sb_qkv_nsplit > 0 ? c->sb_qkv_nsplit : fit[nrows];
      // dec_attn_qkv_kernel addresses the KV arena and its partials by batch ROW and returns when slot_meta[slot].row != row
      // (decode.hip): the launch order is the identity (`identity`, above)
      if (sb_qkv_chain_supported(SK_L2, SK_OUT, ns2, nrows)) { c->nsplit = ns2; c->sb_qkv = true; }
    }
  }
}

// First fill of a decode batch: the prefill of caller rows r0 .. r0+nb-1 plus the decode state and geometry that only the first
// fill sets up (slot order, context splits, chain choice, cur_batch).
// beams > 1: best_of.  The reference repeats the prompt N times and runs N identical prefills (models/vallex.py:525-527); here
// every one of the nb rows is prefilled once and decode row i*beams + j (j < beams) continues from prefill row i: its KV cache
// and residual row are fanned out to the beams (beams.hip), which then sample independently.
int ar_prefill(vx_ctx* c, const vx_batch* b, int r0, int nb, int beams = 1) {
  const int NL = c->NL;
  const int nrows = nb * beams;                      // decode rows after this call
  PrefillPlan p;
  MetaBuilder mb(c);
  if (int e = prefill_tables(c, b, r0, nb, p, mb)) return e;
  const std::vector<int>&seq_off = p.seq_off, &seq_len = p.seq_len, &S_ = p.S_;
  if (nrows > c->mbr) FAIL(VX_EINVAL, "%d decode rows exceed the micro-batch (%d)", nrows, c->mbr);
  c->h_L.resize(nrows);
  for (int i = 0; i < nrows; ++i) c->h_L[i] = seq_len[i / beams];
  // decode state
  std::vector<int> st_pos(nrows), st_ctx(nrows), st_zero(nrows, 0), st_one(nrows, 1), st_S(nrows);
  for (int i = 0; i < nrows; ++i) {
    const int j = i / beams;                                      // the prefill row decode row i continues from
    st_pos[i] = b->prompt_lens[r0 + j]; st_ctx[i] = seq_len[j]; st_S[i] = S_[j];
  }
  // dec_attn launch order (decode.hip): rows by context length, the longest ceil(nb/2) first (descending), then the rest
  // ascending, so launch slots y and y + nb/2 -- which share a CU or a workgroup -- hold a long and a short context.  The
  // order of the contexts never changes during generation (every active row grows by one per step).  A row's beams have equal
  // contexts: the stable sort keeps them adjacent (nothing below relies on it: the fan-out reads every beam's slot from st_slot).
  // (The continuous schedule admits new rows into the slots of finished ones: there the pairing holds only for the first fill.)
  std::vector<int> by_len(nrows), st_ord(nrows);
  for (int i = 0; i < nrows; ++i) by_len[i] = i;
  // (<= SB_ROWS rows: batch order -- the fused small-batch attention relies on slot == row, and there is nothing to balance)
  const bool balance = c->balance_rows && nrows > SB_ROWS;
  if (balance) std::stable_sort(by_len.begin(), by_len.end(), [&](int a, int b2) { return st_ctx[a] > st_ctx[b2]; });
  if (!balance) st_ord = by_len;                                  // batch order (also VX_BALANCE_ROWS=0)
  else {
    const int first = (nrows + 1) / 2;
    for (int y = 0; y < first; ++y) st_ord[y] = by_len[y];
    for (int y = first; y < nrows; ++y) st_ord[y] = by_len[nrows - 1 - (y - first)];
  }
  std::vector<int> st_meta(4 * nrows, 0), st_slot(nrows);
  for (int y = 0; y < nrows; ++y) {
    st_meta[4 * y] = st_ord[y]; st_meta[4 * y + 1] = st_ctx[st_ord[y]]; st_meta[4 * y + 2] = 1;
    st_slot[st_ord[y]] = y;
  }
  // The KV arena is indexed by LAUNCH SLOT, not by batch row: dec_attn knows the address of its K / V stream from its block id
  // alone and requests the first tile before the slot record (row, context, active) has arrived (decode.hip).  The prefill
  // scatters every sequence's K / V into the arena row of its slot; best_of: prefill row i into the slot of decode row i*beams,
  // and the fan-out (beams.hip) copies it to the slots of decode rows i*beams + 1 .. i*beams + beams-1.
  for (int& rb : p.row_b) rb = st_slot[rb * beams];
  p.o_rb = mb.add(p.row_b);
  const long o_sp = mb.add(st_pos), o_sc = mb.add(st_ctx), o_z = mb.add(st_zero), o_1 = mb.add(st_one), o_sS = mb.add(st_S),
             o_meta = mb.add(st_meta), o_slot = mb.add(st_slot);
  const bool trim = p.trim;
  // best_of fan-out tables (beams.hip): (slot of decode row i*beams, slot of decode row i*beams + j, seq_len[i]) per copy, and the
  // row of the prefill's last-row buffer every decode row's residual comes from (trimmed: compacted row i, else packed row)
  long o_fp = 0, o_fr = 0;
  if (beams > 1) {
    std::vector<int> fpairs, frow(nrows);
    for (int i = 0; i < nb; ++i) {
      if (seq_len[i] > c->Tmax) FAIL(VX_EINVAL, "row %d: %d cached rows exceed the arena (%d)", r0 + i, seq_len[i], c->Tmax);
      for (int j = 1; j < beams; ++j) fpairs.insert(fpairs.end(), {st_slot[i * beams], st_slot[i * beams + j], seq_len[i]});
      for (int j = 0; j < beams; ++j) frow[i * beams + j] = p.hrow(i);
    }
    o_fp = mb.add(fpairs); o_fr = mb.add(frow);
  }
  if (int e = upload_meta(c)) return e;
  const size_t ib = nrows * sizeof(int);
  HIPCHK(hipMemcpyAsync(c->cur_pos, mb.dev(o_sp), ib, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->ctx_len, mb.dev(o_sc), ib, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->n_gen, mb.dev(o_z), ib, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->cur_tok, mb.dev(o_z), ib, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->active, mb.dev(o_1), ib, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->text_len, mb.dev(o_sS), ib, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->slot_meta, mb.dev(o_meta), 4 * ib, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->slot_of, mb.dev(o_slot), ib, hipMemcpyDeviceToDevice, c->stream));
  H2D(c->n_active, &nrows, sizeof(int));
  c->cur_batch = nrows;
  bool identity = true;
  for (int y = 0; y < nrows; ++y) identity = identity && st_ord[y] == y;
  decode_geometry(c, nrows, identity);

  if (int e = prefill_layers(c, p, mb)) return e;
  // last row of every sequence -> decode residual stream h[b]
  const float* hsrc = prefill_hsrc(c, p);
  const size_t cache_layer = (size_t)c->mbr * N_HEAD * c->Tmax * D_HEAD;
  if (beams > 1)      // best_of: every decode row's residual row + the other beams' K / V, one launch
    launch_beam_fanout(c->kc, c->vc, (long)cache_layer, NL, c->Tmax, mb.dev(o_fp), nb * (beams - 1), hsrc, mb.dev(o_fr), c->dh, nrows,
                       c->stream);
  else if (trim)
    HIPCHK(hipMemcpyAsync(c->dh, hsrc, (size_t)nb * D_MODEL * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  else
    for (int i = 0; i < nb; ++i)
      HIPCHK(hipMemcpyAsync(c->dh + (size_t)i * D_MODEL, c->fx + ((size_t)seq_off[i] + seq_len[i] - 1) * D_MODEL,
                            D_MODEL * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  // final norm + ar_predict_layer on every decode row (models/vallex.py:568; the predict GEMM's 32-column block costs the same for
  // 1 or 32 rows, so the beams compute their logits instead of copying them)
  launch_dec_reduce_ln_pack(nullptr, 0, D_MODEL, nullptr, c->dh, nullptr, W(c, "ar_decoder.norm.weight"),
                            W(c, "ar_decoder.norm.bias"), c->xp, nrows, c->stream);
  launch_skinny_gemm(c->pred_wp, c->xp, c->p_logits, PRED_NPAD, D_MODEL, SK_PRED, c->stream);
  return VX_OK;
}

SampleArgs make_sample_args(vx_ctx* c, const vx_sampling* s, int commit, float* logits_out) {
  SampleArgs a{};
  a.partial = c->p_logits; a.splitk = SK_PRED; a.npad = PRED_NPAD;
  a.top_k = s ? s->top_k : 1;
  a.temperature = s ? s->temperature : 1.0f;
  a.uniforms = (s && s->uniforms) ? c->d_uniforms : nullptr;
  a.uniforms_stride = c->cur_batch;
  a.seed_dev = c->seed_dev;
  a.force_eos_at = s ? s->force_eos_at : -1;
  a.commit = commit;
  a.cur_tok = c->cur_tok; a.cur_pos = c->cur_pos; a.ctx_len = c->ctx_len; a.n_gen = c->n_gen; a.active = c->active;
  a.n_active = c->n_active; a.slot_meta = c->slot_meta; a.slot_of = c->slot_of;
  a.text_len = c->text_len; a.gen = c->gen; a.gen_stride = c->gen_stride; a.logits_out = logits_out;
  a.sum_logp = (s && s->best_of > 1) ? c->sum_logp : nullptr;
  a.batch = c->cur_batch;
  if (commit) {      // the sampler also embeds the committed token and applies norm1 of layer 0 (start of the next step)
    a.emb_tab = W(c, "ar_audio_embedding.word_embeddings.weight"); a.emb_alpha = W(c, "ar_audio_position.alpha");
    a.pe = c->pe; a.ln_g = c->ar[0].n1_w; a.ln_b = c->ar[0].n1_b; a.emb_h = c->dh; a.emb_xp = c->xp;
    a.wt = c->sb_chain ? 0 : 1;
  }
  return a;
}

// ---- one cached decode step (models/vallex.py:552-571 with kv_cache set) --------------------------------------
void ar_step_launches(vx_ctx* c, const SampleArgs* sa, const ServeSampleArgs* rsa) {
  const int nb = c->cur_batch, NL = c->NL;
  hipStream_t st = c->stream;
  const size_t cache_layer = (size_t)c->mbr * N_HEAD * c->Tmax * D_HEAD;
  // sampling mode: the previous dec_sample already embedded the token and applied norm1 of layer 0; the teacher-forced
  // mode (sa == null, rsa == null: vx_ar_step) has to do it here
  if (!sa && !rsa)
    launch_dec_embed_ln_pack(c->cur_tok, c->cur_pos, W(c, "ar_audio_embedding.word_embeddings.weight"),
                             W(c, "ar_audio_position.alpha"), c->pe, c->dh, c->ar[0].n1_w, c->ar[0].n1_b, c->xp, nb, st);
  if (c->sb_chain) {
    // small batch (BASELINE config 2: one utterance): 5 launches per layer -- QKV | dec_attn partials | out_proj | linear1 | linear2 --
    // every reduce + residual + LayerNorm and the context-split combine run in the prologue of the GEMM that consumes them
    // (decode.hip: skinny_gemm_sb_kernel, skinny16_sb_kernel).  The residual stream alternates between dh and dh2.
    float *hr = c->dh, *hw = c->dh2;            // the sampler / embed kernel left h in dh
    for (int l = 0; l < NL; ++l) {
      const LayerW& L = c->ar[l];
      if (c->sb_qkv) {
        // 4 launches per layer: norm1 + QKV run inside the split attention launch (decode.hip: dec_attn_qkv_kernel), which hands
        // nsplit + 1 partials per (row, head) to the out_proj prologue
        {
          ProfScope ps(c, 0);
          LAUNCH(launch_dec_attn_qkv(L.in_w, L.in_b, c->kc + l * cache_layer, c->vc + l * cache_layer, c->Tmax, c->slot_meta, c->part_o,
                                     c->part_ml, c->qk_new, c->nsplit, nb, l ? c->p_o : nullptr, l ? SK_L2 : 0,
                                     l ? c->ar[l - 1].l2_b : nullptr, hr, hw, L.n1_w, L.n1_b, c->xp, st));
          if (l) std::swap(hr, hw);
        }
        {
          ProfScope ps(c, 1);
          LAUNCH(launch_skinny_gemm_sb_combine(L.out_wp, c->p_o, D_MODEL, SK_OUT, c->part_o, c->part_ml, c->nsplit + 1, nb, st, c->qk_new));
        }
      } else {
      {
        ProfScope ps(c, 1);
        if (l == 0) launch_skinny_gemm(L.in_wp, c->xp, c->p_qkv, 3 * D_MODEL, D_MODEL, SK_QKV, st);      // xp = norm1(h) from the sampler
        else {
          LAUNCH(launch_skinny_gemm_sb_ln(L.in_wp, c->p_qkv, 3 * D_MODEL, SK_QKV, c->p_o, SK_L2, c->ar[l - 1].l2_b, hr, hw, L.n1_w, L.n1_b, nb, st));
          std::swap(hr, hw);
        }
      }
      {
        ProfScope ps(c, 0);
        LAUNCH(launch_dec_attn(c->p_qkv, SK_QKV, L.in_b, c->kc + l * cache_layer, c->vc + l * cache_layer, c->Tmax, c->slot_meta,
                        c->xp_att, c->part_o, c->part_ml, c->nsplit, nb, nullptr, c->p_oh, st));
      }
      { ProfScope ps(c, 1); LAUNCH(launch_skinny_gemm_sb_combine(L.out_wp, c->p_o, D_MODEL, SK_OUT, c->part_o, c->part_ml, c->nsplit, nb, st)); }
      }
      {
        ProfScope ps(c, 1);
        LAUNCH(launch_skinny16_sb_ln(L.l1_wp, L.l1_b, c->xp4, D_FF, c->p_o, SK_OUT, L.out_b, hr, hw, L.n2_w, L.n2_b, nb, st));
        std::swap(hr, hw);
      }
      { ProfScope ps(c, 1); launch_skinny_gemm(L.l2_wp, c->xp4, c->p_o, D_MODEL, D_FF, SK_L2, st); }
    }
    {
      ProfScope ps(c, 1);
      LAUNCH(launch_skinny_gemm_sb_ln(c->pred_wp, c->p_logits, PRED_NPAD, SK_PRED, c->p_o, SK_L2, c->ar[NL - 1].l2_b, hr, nullptr,
                               W(c, "ar_decoder.norm.weight"), W(c, "ar_decoder.norm.bias"), nb, st));
    }
    if (rsa) LAUNCH(launch_serve_sample(*rsa, st));
    else if (sa) LAUNCH(launch_dec_sample(*sa, st));
    return;
  }
  for (int l = 0; l < NL; ++l) {
    const LayerW& L = c->ar[l];
    {
      ProfScope ps(c, 1);
      if (c->qkv_bal) launch_skinny_qkv_balanced(L.in_wp, c->xp, c->p_qkv, st);
      else launch_skinny_gemm(L.in_wp, c->xp, c->p_qkv, 3 * D_MODEL, D_MODEL, SK_QKV, st, true);
    }
    // out_proj inside dec_attn: one context split (17 .. 32 rows), or 2 .. 4 splits with the combine moved behind W_o (8 .. 16 rows, round 6)
    const bool fused = c->fuse_out && (c->nsplit == 1 || c->split_fused);
    {
      ProfScope ps(c, 0);
      LAUNCH(launch_dec_attn(c->p_qkv, c->qkv_bal ? SK_QKV_BALANCED : SK_QKV, L.in_b, c->kc + l * cache_layer, c->vc + l * cache_layer, c->Tmax, c->slot_meta,
                      c->xp_att, c->part_o, c->part_ml, c->nsplit, nb, fused ? L.out_wh : nullptr, c->p_oh, st));
    }
    if (fused && c->nsplit > 1) {
      LAUNCH(launch_dec_reduce_ln_split(c->p_oh, c->part_ml, c->nsplit, L.out_b, c->dh, c->dh, L.n2_w, L.n2_b, c->xp, nb, st));
    } else if (fused) {
      launch_dec_reduce_ln_pack(c->p_oh, N_HEAD, D_MODEL, L.out_b, c->dh, c->dh, L.n2_w, L.n2_b, c->xp, nb, st);
    } else {
      if (c->nsplit > 1) launch_dec_attn_combine(c->part_o, c->part_ml, c->nsplit, c->active, c->xp_att, nb, st);
      { ProfScope ps(c, 1); launch_skinny_gemm(L.out_wp, c->xp_att, c->p_o, D_MODEL, D_MODEL, SK_OUT, st, true); }
      launch_dec_reduce_ln_pack(c->p_o, SK_OUT, D_MODEL, L.out_b, c->dh, c->dh, L.n2_w, L.n2_b, c->xp, nb, st);
    }
    { ProfScope ps(c, 1); launch_skinny16_relu_pack(L.l1_wp, c->xp, L.l1_b, c->xp4, D_FF, D_MODEL, st); }
    { ProfScope ps(c, 1); launch_skinny_gemm(L.l2_wp, c->xp4, c->p_o, D_MODEL, D_FF, SK_L2, st, true); }
    const float* ng = (l + 1 < NL) ? c->ar[l + 1].n1_w : W(c, "ar_decoder.norm.weight");
    const float* nbp = (l + 1 < NL) ? c->ar[l + 1].n1_b : W(c, "ar_decoder.norm.bias");
    launch_dec_reduce_ln_pack(c->p_o, SK_L2, D_MODEL, L.l2_b, c->dh, c->dh, ng, nbp, c->xp, nb, st);
  }
  { ProfScope ps(c, 1); launch_skinny_gemm(c->pred_wp, c->xp, c->p_logits, PRED_NPAD, D_MODEL, SK_PRED, st, true); }
  if (rsa) LAUNCH(launch_serve_sample(*rsa, st));
  else if (sa) LAUNCH(launch_dec_sample(*sa, st));
}

// the decode kernels compile these split counts in (decode.hip); retuning one without instantiating it must not reach a GPU
static_assert(SK_QKV == 4, "dec_attn_kernel<*, 4> sums four QKV slabs in its prologue");
static_assert(SK_OUT == 4, "skinny16_sb_kernel<4> / dec_reduce_ln_pack<4> are the instantiated out_proj consumers");
static_assert(SK_L2 == 8 || SK_L2 == 4, "skinny_gemm_sb_kernel<0, 8 | 4> are the instantiated linear2 consumers");
static_assert(SK_PRED == 4 || SK_PRED == 2 || SK_PRED == 1, "dec_sample_kernel<4 | 2 | 1>");

int launch_status(vx_ctx* c) {
  if (!c->launch_fail) return VX_OK;
  const char* what = c->launch_fail;
  c->launch_fail = nullptr;
  FAIL(VX_EINVAL, "kernel configuration not compiled into this library: %s", what);
}

// nsteps consecutive decode steps.  Graph mode keeps TWO instantiated graphs per signature: one step, and GRAPH_STEPS steps in one
// graph -- between two hipGraphLaunch calls the GPU idles for ~9 us (kernel traces, profiles/r04_gaps_*.csv: the gap behind every
// dec_sample launch), which a multi-step graph pays once per GRAPH_STEPS steps.  All step state (positions, lengths, flags, the
// sampler's counters) lives on the device, so a replay is position independent.
constexpr int GRAPH_STEPS = 4;
int ar_step_run(vx_ctx* c, const SampleArgs* sa, const std::string& sig, int nsteps = 1, const ServeSampleArgs* rsa = nullptr) {
  if (!c->cfg.use_graph || c->prof_on == 1 || (!sa && !rsa)) {
    for (int i = 0; i < nsteps; ++i) ar_step_launches(c, sa, rsa);
    HIPCHK(hipGetLastError());
    return launch_status(c);
  }
  if (c->graph_sig != sig) {
    for (hipGraphExec_t* ge : {&c->graph_exec, &c->graph_exec_n})
      if (*ge) { (void)hipGraphExecDestroy(*ge); *ge = nullptr; }
    c->graph_sig = sig;
  }
  hipGraphExec_t& ge = nsteps == 1 ? c->graph_exec : c->graph_exec_n;
  if (!ge) {
    hipGraph_t g = nullptr;
    HIPCHK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    for (int i = 0; i < nsteps; ++i) ar_step_launches(c, sa, rsa);
    HIPCHK(hipStreamEndCapture(c->stream, &g));
    if (int e = launch_status(c)) { (void)hipGraphDestroy(g); return e; }      // an incomplete step must never be replayed
    HIPCHK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
    (void)hipGraphDestroy(g);
  }
  HIPCHK(hipGraphLaunch(ge, c->stream));
  return VX_OK;
}

// ---- sticky fp32 fallback bookkeeping (engine_ctx.h) -----------------------------------------------------------
// does this phase go to the fp32 kernels directly?  In sticky mode yes, except every FB_STICKY_PROBE_EVERY-th phase (a probe on f16x2)
bool fb_direct(vx_ctx* c, bool sticky, int& age) {
  if (!sticky || !range_guarded(c)) return false;
  if (++age >= FB_STICKY_PROBE_EVERY) { age = 0; return false; }
  return true;
}
// outcome of a phase that RAN on f16x2: a raise counts towards sticky mode, a clean pass resets the count and leaves sticky mode
void fb_outcome(vx_ctx* c, bool raised, int& raises, bool& sticky, int& age) {
  if (!range_guarded(c)) return;
  if (!raised) { raises = 0; sticky = false; age = 0; return; }
  if (++raises >= FB_STICKY_AFTER && !sticky) { sticky = true; age = 0; ++c->sticky_engaged; }
}

// ---- AR generation for one micro-batch -----------------------------------------------------------------------
// caller rows r0 .. r0+nb-1, each decoded as `beams` rows (decode row i*beams + j: beam j of row r0 + i); `seed` is the sampler's
// seed for this micro-batch (unused with injected uniforms)
int ar_generate(vx_ctx* c, const vx_batch* b, const vx_sampling* s, int r0, int nb, std::vector<int>& n_gen,
                std::vector<int>& gen, int beams, unsigned long long seed) {
  const int nb_rows = nb;                            // rows of the caller's batch that this micro-batch prefills
  // a context whose prefills keep leaving the fp16 range runs them on the exact-fp32 kernels straight away (sticky fallback)
  const bool direct_f32 = fb_direct(c, c->sticky_prefill_f32, c->sticky_prefill_age);
  if (direct_f32) {
    ++c->st_fb_prefill; ++c->fb_total;
    if (int e = ensure_f32_buffers(c)) return e;
    F32Scope f32(c);
    if (int e = ar_prefill(c, b, r0, nb_rows, beams)) return e;
  } else if (int e = ar_prefill(c, b, r0, nb_rows, beams)) return e;
  const long ub = (long)b->batch * beams;            // columns of the caller's uniforms: [steps][batch x best_of]
  nb = nb_rows * beams;                              // decode rows from here on
  if (s->uniforms) {
    // slice [steps][batch x beams] -> [steps][nb] for this micro-batch: columns r0*beams .. (r0 + nb_rows)*beams
    // only the first gen_stride + 1 draws can ever be consumed (one per generated frame + the terminating sample)
    const long steps = std::min<long>(s->uniforms_steps, c->gen_stride + 1);
    if (steps * nb > c->uniforms_cap) FAIL(VX_EINVAL, "too many uniforms (%ld steps)", steps);
    std::vector<float> u((size_t)steps * nb);
    for (long t = 0; t < steps; ++t)
      for (int i = 0; i < nb; ++i) u[t * nb + i] = s->uniforms[t * ub + (long)r0 * beams + i];
    H2D(c->d_uniforms, u.data(), u.size() * sizeof(float));
    SYNC();
  }
  // the seed of the counter-based sampler lives in a device word: a new seed per call (the reference's contract, every call
  // draws from torch's generator) does not change the captured step graph
  H2D(c->seed_dev, &seed, sizeof seed);
  SampleArgs sa = make_sample_args(c, s, 1, nullptr);
  std::vector<int> act(nb);
  bool any = true, raised = false;
  // first token from the prefill logits; the host sync that tells whether anything is still active also brings the range
  // flag of the prefill back (f16x2 guard, see F32Scope)
  auto first_sample = [&]() -> int {
    int flag = 0;
    HIPCHK(hipMemsetAsync(c->sum_logp, 0, MB * sizeof(float), c->stream));
    LAUNCH(launch_dec_sample(sa, c->stream));
    if (int e = launch_status(c)) return e;
    D2H(act.data(), c->active, nb * sizeof(int));
    if (range_guarded(c) && !direct_f32) D2H(&flag, c->range_flag, sizeof(int));
    SYNC();
    raised = flag != 0;
    any = std::any_of(act.begin(), act.end(), [](int v) { return v != 0; });
    return VX_OK;
  };
  if (int e = first_sample()) return e;
  if (!direct_f32) fb_outcome(c, raised, c->fb_prefill_raises, c->sticky_prefill_f32, c->sticky_prefill_age);
  if (raised) {
    // an operand of the prefill left the fp16 range: the K/V cache, the residual row and the logits are not to be trusted.
    // Re-run the prefill on the exact-fp32 kernels (it resets the decode state) and sample the first token again.
    HIPCHK(hipMemsetAsync(c->range_flag, 0, sizeof(int), c->stream));
    ++c->st_fb_prefill; ++c->fb_total;
    if (int e = ensure_f32_buffers(c)) return e;
    {
      F32Scope f32(c);
      if (int e = ar_prefill(c, b, r0, nb_rows, beams)) return e;
      if (int e = first_sample()) return e;
    }
  }
  char sig[160];
  snprintf(sig, sizeof sig, "b%d ns%d c%d%d%d k%d t%a u%d f%d l%d", nb, c->nsplit, (int)c->sb_chain, (int)c->sb_qkv, (int)c->split_fused, sa.top_k, sa.temperature,
           sa.uniforms != nullptr, sa.force_eos_at, sa.sum_logp != nullptr);
  const int sync_every = s->sync_every > 0 ? s->sync_every : 8;
  // with a forced EOS every row is inactive after force_eos_at steps: do not run on to the next host poll
  const int hard_cap = s->force_eos_at >= 0 ? std::min(c->gen_stride + 2, s->force_eos_at) : c->gen_stride + 2;
  int steps = 0;
  // GRAPH_STEPS steps per graph launch while that neither crosses a host poll nor the cap (nsteps is 1 or GRAPH_STEPS: two graphs)
  const int gs = (c->graph_multi && sync_every % GRAPH_STEPS == 0) ? GRAPH_STEPS : 1;
  while (any && steps < hard_cap) {
    const int n = (steps % gs == 0 && steps + gs <= hard_cap) ? gs : 1;
    if (int e = ar_step_run(c, &sa, sig, n)) return e;
    steps += n;
    if (steps % sync_every == 0) {
      D2H(act.data(), c->active, nb * sizeof(int));
      SYNC();
      any = std::any_of(act.begin(), act.end(), [](int v) { return v != 0; });
    }
  }
  n_gen.resize(nb);
  gen.resize((size_t)nb * c->gen_stride);
  D2H(n_gen.data(), c->n_gen, nb * sizeof(int));
  D2H(gen.data(), c->gen, gen.size() * sizeof(int));
  SYNC();
  c->st_steps += steps;
  if (c->prof_on) {
    // algorithmic KV bytes: every decode step of an active row reads ctx rows of K and V in all layers
    for (int i = 0; i < nb; ++i)
      for (int t = 1; t <= n_gen[i]; ++t)
        c->prof[0].bytes += (double)c->NL * ((double)(c->h_L[i] + t) * 2.0 * D_MODEL * 4.0);
    c->prof[1].bytes += (double)steps * ((double)c->NL * 12.0 * D_MODEL * D_MODEL + (double)AR_LOGITS * D_MODEL) * 4.0;
  }
  return VX_OK;
}

// best_of selection of one row's N beams (models/vallex.py:583-594): sum(logp) / len^length_penalty with len = torch.sum(y != EOS) =
// BOS + prompt + frames; the first index wins ties; return_worst picks the lowest.  vx_infer and the serving session both call it.
static int select_beam(const float* slp, const int* n_gen, int N, int Tp, float length_penalty, bool return_worst) {
  int best = 0, worst = 0;
  double bv = 0, wv = 0;
  for (int j = 0; j < N; ++j) {
    const double len = 1.0 + Tp + n_gen[j];
    const double v = (double)(float)((float)slp[j] / powf((float)len, length_penalty));
    if (j == 0 || v > bv) { bv = v; best = j; }
    if (j == 0 || v < wv) { wv = v; worst = j; }
  }
  return return_worst ? worst : best;
}

// best_of: the sampler's seed of micro-batch k.  The counter-based sampler mixes (seed, decode row, step), so without this the beams
// of the first row of every micro-batch would draw the same streams.  Micro-batch 0 keeps the caller's seed: a batch-1 call (one
// micro-batch) draws exactly what it drew before batched best_of existed.
static unsigned long long beam_seed(unsigned long long seed, int k) {
  if (k == 0) return seed;
  unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (unsigned long long)k;      // splitmix64 of (seed, k)
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// ---- NAR: 7 stages (models/vallex.py:600-686, prefix_mode 1) ----------------------------------------------------
int nar_generate_once(vx_ctx* c, const vx_batch* b, int r0, int nb, const std::vector<int>& T, const int* codes0,
                      long codes0_stride, std::vector<int>& out_codes /* [7][sumT] */, long& sumT_out) {
  const int NL = c->NL;
  std::vector<int> seq_off(nb), seq_len(nb), dst_t, id_t, lang_t, pos_t, ycodes, ynj, ydst, ypos, gen_rows, gen_y, q_first(nb), c_off(nb);
  long M = 0, Y = 0, sumT = 0;
  int max_len = 0;
  double trim_attn_flops = 0;
  {      // the host builds ~0.3 M ints of row metadata while the GPU waits between the AR and the NAR phase: no reallocation on the way
    size_t nS = 0, nY = 0, nT = 0;
    for (int i = 0; i < nb; ++i) { nS += b->text_lens[r0 + i]; nY += b->prompt_lens[r0 + i] + T[i]; nT += T[i]; }
    for (auto* v : {&dst_t, &id_t, &lang_t, &pos_t}) v->reserve(nS);
    for (auto* v : {&ynj, &ydst, &ypos}) v->reserve(nY);
    ycodes.reserve(nY * N_Q);
    gen_rows.reserve(nT); gen_y.reserve(nT);
  }
  for (int i = 0; i < nb; ++i) {
    const int r = r0 + i, S = b->text_lens[r], Tp = b->prompt_lens[r];
    seq_off[i] = (int)M; seq_len[i] = S + Tp + T[i];
    q_first[i] = S + Tp; c_off[i] = (int)sumT;
    trim_attn_flops += 4.0 * T[i] * (double)seq_len[i] * D_MODEL;
    max_len = std::max(max_len, seq_len[i]);
    for (int s = 0; s < S; ++s) {
      dst_t.push_back((int)M + s);
      id_t.push_back(b->text_ids[(long)r * b->text_stride + s]);
      lang_t.push_back(b->text_lang[(long)r * b->text_stride + s]);
      pos_t.push_back(s);
    }
    for (int t = 0; t < Tp + T[i]; ++t) {
      if (t < Tp) {
        for (int j = 0; j < N_Q; ++j) ycodes.push_back(b->prompt_codes[((long)r * b->prompt_stride + t) * N_Q + j]);
        ynj.push_back(N_Q);
      } else {
        ycodes.push_back(codes0[(long)i * codes0_stride + (t - Tp)]);
        for (int j = 1; j < N_Q; ++j) ycodes.push_back(0);
        ynj.push_back(1);
        gen_rows.push_back((int)M + S + t);
        gen_y.push_back((int)Y + t);
      }
      ydst.push_back((int)M + S + t);
      ypos.push_back(t);
    }
    M += seq_len[i]; Y += Tp + T[i]; sumT += T[i];
  }
  sumT_out = sumT;
  out_codes.assign((size_t)(N_Q - 1) * sumT, 0);
  if (sumT == 0) return VX_OK;
  if (M > c->Mmax) FAIL(VX_EINVAL, "NAR rows %ld exceed arena %ld", M, c->Mmax);
  MetaBuilder mb(c);
  const long o_off = mb.add(seq_off), o_len = mb.add(seq_len), o_dt = mb.add(dst_t), o_it = mb.add(id_t),
             o_lt = mb.add(lang_t), o_pt = mb.add(pos_t), o_yc = mb.add(ycodes), o_nj = mb.add(ynj), o_yd = mb.add(ydst),
             o_yp = mb.add(ypos), o_gr = mb.add(gen_rows), o_gy = mb.add(gen_y), o_qf = mb.add(q_first), o_co = mb.add(c_off);
  std::vector<int> zeros((size_t)(N_Q - 1) * sumT, 0);
  const long o_samples = mb.add(zeros);
  if (int e = upload_meta(c)) return e;

  launch_nar_yemb_init(c->fyemb, c->nar_tabs_dev, mb.dev(o_yc), mb.dev(o_nj), (int)Y, c->stream);
  double attn_flops = 0;
  for (int i = 0; i < nb; ++i) attn_flops += 4.0 * seq_len[i] * (double)seq_len[i] * D_MODEL;
  const int nnorm = 2 * NL + 1;
  for (int st = 0; st < N_Q - 1; ++st) {
    launch_embed_rows(c->fx, mb.dev(o_dt), W(c, "nar_text_embedding.word_embeddings.weight"), mb.dev(o_it),
                      W(c, "nar_language_embedding.word_embeddings.weight"), mb.dev(o_lt),
                      W(c, "nar_text_position.alpha"), c->pe, mb.dev(o_pt), (int)dst_t.size(), c->stream);
    launch_add_pe_scatter(c->fx, mb.dev(o_yd), c->fyemb, W(c, "nar_audio_position.alpha"), c->pe, mb.dev(o_yp), (int)Y,
                          c->stream);
    const float* ada = c->ada + (size_t)st * nnorm * 2 * D_MODEL;
    // the last layer only has to produce the generated rows (struct Trim); the per-layer taps want every row
    // f16x2 projections + f16x2 attention, or the reference arithmetic (fp32 projections + fp32 attention); the mixed modes of the
    // VX_GEMM_* / VX_ATTN_* switches and bf16x3 run every row
    const bool trim_h2 = c->gemm_mode == 0 && c->attn_x3 && c->attn_h2, trim_f32 = c->gemm_mode == 2 && !c->attn_x3;
    const bool trim = c->nar_trim && (trim_h2 || trim_f32) && !c->cfg.debug_taps;
    const Trim tr{sumT, mb.dev(o_qf), mb.dev(o_co), mb.dev(o_gr), trim_attn_flops};
    for (int l = 0; l < NL; ++l) {
      if (int e = full_layer(c, c->nar[l], M, mb.dev(o_off), mb.dev(o_len), nullptr, nb, max_len,
                             ada + (size_t)(2 * l) * 2 * D_MODEL, ada + (size_t)(2 * l + 1) * 2 * D_MODEL, nullptr, nullptr,
                             nullptr, nullptr, attn_flops, (trim && l == NL - 1) ? &tr : nullptr))
        return e;
      if (c->cfg.debug_taps && st == 0) {
        char nm[64];
        snprintf(nm, sizeof nm, "nar_layer_out.%d", l);
        if (int e = tap_store(c, nm, c->fx, (size_t)M * D_MODEL)) return e;
      }
    }
    const float* adaf = ada + (size_t)(2 * NL) * 2 * D_MODEL;
    char nm[64];
    snprintf(nm, sizeof nm, "nar_predict_layers.%d.weight", st);
    if (trim && trim_f32) {
      // the compacted residual stream (in the QKV buffer, full_layer) holds exactly the rows the predict layer reads: no gather
      launch_layernorm(c->fqkv, D_MODEL, c->fxn, D_MODEL, (int)sumT, D_MODEL, LN_EPS, W(c, "nar_decoder.norm.norm.weight"),
                       W(c, "nar_decoder.norm.norm.bias"), adaf, adaf + D_MODEL, c->stream);
      proj(c, c->fxn, D_MODEL, W(c, nm), c->pred_w3[st], nullptr, nullptr, 0, c->flogits, AUDIO_VOCAB, sumT, AUDIO_VOCAB, D_MODEL, ACT_NONE);
    } else if (trim) {
      // the compacted residual stream (fxn) holds exactly the rows the predict layer reads: the final norm writes the GEMM's
      // operand planes itself (bit-identical to a split of its fp32 result), no gather, no split pass
      launch_layernorm(c->fxn, D_MODEL, nullptr, D_MODEL, (int)sumT, D_MODEL, LN_EPS, W(c, "nar_decoder.norm.norm.weight"),
                       W(c, "nar_decoder.norm.norm.bias"), adaf, adaf + D_MODEL, c->stream, c->fa3, h2_plane(sumT, D_MODEL, H2_TILE_A),
                       c->range_flag);
      proj(c, nullptr, D_MODEL, W(c, nm), c->pred_w3[st], nullptr, nullptr, 0, c->flogits, AUDIO_VOCAB, sumT, AUDIO_VOCAB, D_MODEL,
           ACT_NONE, nullptr, c->fa3);
    } else {
      launch_layernorm(c->fx, D_MODEL, c->fxn, D_MODEL, (int)M, D_MODEL, LN_EPS, W(c, "nar_decoder.norm.norm.weight"),
                       W(c, "nar_decoder.norm.norm.bias"), adaf, adaf + D_MODEL, c->stream);
      proj(c, c->fxn, D_MODEL, W(c, nm), c->pred_w3[st], nullptr, nullptr, 0, c->flogits, AUDIO_VOCAB, sumT, AUDIO_VOCAB, D_MODEL,
           ACT_NONE, mb.dev(o_gr));
    }
    if (c->cfg.debug_taps) {                             // "nar_logits0" .. "nar_logits6": every stage's logits of the generated rows
      snprintf(nm, sizeof nm, "nar_logits%d", st);
      if (int e = tap_store(c, nm, c->flogits, (size_t)sumT * AUDIO_VOCAB)) return e;
    }
    int* samples = c->imeta + o_samples + (long)st * sumT;
    launch_argmax_rows(c->flogits, AUDIO_VOCAB, (int)sumT, AUDIO_VOCAB, samples, c->stream);
    if (st == 0 && c->fb_nar_raises > 0 && range_guarded(c)) {
      // this context has left the fp16 range in a NAR phase before: look at the flag behind stage 0 already, so that an
      // out-of-range model does not pay six more f16x2 stages before the fp32 re-run (costs one host sync; never in the common case)
      int early = 0;
      D2H(&early, c->range_flag, sizeof(int));
      SYNC();
      if (early) {
        HIPCHK(hipMemsetAsync(c->range_flag, 0, sizeof(int), c->stream));
        return VX_RETRY_F32;
      }
    }
    if (st < N_Q - 2) {
      snprintf(nm, sizeof nm, "nar_audio_embeddings.%d.word_embeddings.weight", st + 1);
      launch_embed_accum(c->fyemb, mb.dev(o_gy), W(c, nm), samples, (int)sumT, c->stream);
    }
  }
  D2H(out_codes.data(), c->imeta + o_samples, out_codes.size() * sizeof(int));
  int flag = 0;                        // the range flag rides on the sync that brings the ids back
  if (range_guarded(c)) D2H(&flag, c->range_flag, sizeof(int));
  SYNC();
  if (flag) {
    HIPCHK(hipMemsetAsync(c->range_flag, 0, sizeof(int), c->stream));
    return VX_RETRY_F32;
  }
  return VX_OK;
}

int nar_generate(vx_ctx* c, const vx_batch* b, int r0, int nb, const std::vector<int>& T, const int* codes0,
                 long codes0_stride, std::vector<int>& out_codes /* [7][sumT] */, long& sumT_out) {
  int e = VX_RETRY_F32;
  const bool direct_f32 = fb_direct(c, c->sticky_nar_f32, c->sticky_nar_age);          // sticky fallback (engine_ctx.h)
  if (!direct_f32) {
    e = nar_generate_once(c, b, r0, nb, T, codes0, codes0_stride, out_codes, sumT_out);
    if (e == VX_OK || e == VX_RETRY_F32) fb_outcome(c, e == VX_RETRY_F32, c->fb_nar_raises, c->sticky_nar_f32, c->sticky_nar_age);
    if (e != VX_RETRY_F32) return e;
  }
  // an operand of one of the 7 stages left the fp16 range: the whole phase (again) on the exact-fp32 kernels (F32Scope)
  ++c->st_fb_nar; ++c->fb_total;
  if ((e = ensure_f32_buffers(c))) return e;
  F32Scope f32(c);
  return nar_generate_once(c, b, r0, nb, T, codes0, codes0_stride, out_codes, sumT_out);
}

// ---- continuous schedule (vx_infer_continuous) ---------------------------------------------------------------
// One decode batch of nd = min(mbr, batch) rows for the whole call: the first fill is ar_prefill of caller rows 0 .. nd-1 (it sets
// the geometry: slot order, context splits, chain choice -- fixed from then on, so the captured step graph never changes); at every
// host poll (every sync_every steps, and at the step where a row reaches its cap) the rows that stopped are harvested (n_gen + gen row to the host) and waiting caller rows, first come first served, are
// admitted into the freed decode rows: one prefill per admission round into the freed rows' KV slots, then the first sample of
// the admitted rows alone.  Harvested rows go through the NAR stages in groups of mbr (the rest once nothing is left to decode),
// between two decode steps: nar_generate only touches the full-sequence buffers.

// caller rows `rows` of b gathered into a batch of their own (prefill / NAR of a non-contiguous row set)
struct SubBatch {
  std::vector<int32_t> ids, lang, tl, pc, pl;
  vx_batch b{};
  SubBatch(const vx_batch* src, const std::vector<int>& rows) {
    const int n = (int)rows.size(), ts = src->text_stride, ps = src->prompt_stride;
    ids.resize((size_t)n * ts); lang.resize((size_t)n * ts); pc.resize((size_t)n * ps * N_Q); tl.resize(n); pl.resize(n);
    for (int i = 0; i < n; ++i) {
      const int r = rows[i];
      std::copy_n(src->text_ids + (long)r * ts, ts, ids.begin() + (size_t)i * ts);
      std::copy_n(src->text_lang + (long)r * ts, ts, lang.begin() + (size_t)i * ts);
      std::copy_n(src->prompt_codes + (long)r * ps * N_Q, (size_t)ps * N_Q, pc.begin() + (size_t)i * ps * N_Q);
      tl[i] = src->text_lens[r]; pl[i] = src->prompt_lens[r];
    }
    b = *src;
    b.batch = n; b.text_ids = ids.data(); b.text_lang = lang.data(); b.text_lens = tl.data();
    b.prompt_codes = pc.data(); b.prompt_lens = pl.data();
  }
};

// the sampler's draws of caller rows crow[i] into decode columns drow[i] of d_uniforms (launch_admit_uniforms); the tables go into
// the MetaBuilder of the phase, before its upload
struct UniformCols { long o_pairs = 0, o_staged = -1; int n = 0, steps = 0; };
static int uniform_cols(vx_ctx* c, const vx_batch* b, const vx_sampling* s, const std::vector<int>& drow, const std::vector<int>& crow,
                        MetaBuilder& mb, UniformCols& u) {
  // only the first gen_stride + 1 draws of a row can ever be consumed (one per generated frame + the terminating sample)
  u.n = (int)drow.size();
  u.steps = s->uniforms ? (int)std::min<long>(s->uniforms_steps, c->gen_stride + 1) : c->gen_stride + 1;
  if ((long)u.steps * c->cur_batch > c->uniforms_cap) FAIL(VX_EINVAL, "too many uniforms (%d steps)", u.steps);
  std::vector<int> pairs(2 * u.n);
  for (int i = 0; i < u.n; ++i) { pairs[2 * i] = drow[i]; pairs[2 * i + 1] = crow[i]; }
  u.o_pairs = mb.add(pairs);
  if (s->uniforms) {       // column r of the caller's [uniforms_steps][batch], staged as [n][steps] (float bits in the int tables)
    std::vector<int> st((size_t)u.n * u.steps);
    for (int i = 0; i < u.n; ++i)
      for (int t = 0; t < u.steps; ++t) memcpy(&st[(size_t)i * u.steps + t], &s->uniforms[(long)t * b->batch + crow[i]], sizeof(float));
    u.o_staged = mb.add(st);
  }
  return VX_OK;
}
static void uniform_cols_launch(vx_ctx* c, const vx_sampling* s, const UniformCols& u, const MetaBuilder& mb) {
  const float* staged = u.o_staged >= 0 ? reinterpret_cast<const float*>(mb.dev(u.o_staged)) : nullptr;
  launch_admit_uniforms(mb.dev(u.o_pairs), u.n, staged, u.steps, s->seed, c->d_uniforms, c->cur_batch, c->stream);
}

// admission of caller rows crow[i] (sub-batch sb, row i) into the free decode rows drow[i] of the running decode batch, up to and
// including their first sample.  The rows still decoding keep every piece of their state: the prefill scatters K / V into the
// admitted rows' slots only, its final norm + predict layer run on scratch copies (dh2 / xp_att: the step recomputes both before
// it reads them; the logits of rows that are not admitted are never read), and the sampler commits the admitted rows only.
static int admit_rows(vx_ctx* c, const vx_batch* b, const vx_sampling* s, const SampleArgs& sa, const std::vector<int>& drow,
                      const std::vector<int>& crow, const std::vector<int>& slot_of) {
  const int k = (int)drow.size(), nd = c->cur_batch;
  SubBatch sb(b, crow);
  PrefillPlan p;
  MetaBuilder mb(c);
  if (int e = prefill_tables(c, &sb.b, 0, k, p, mb)) return e;
  for (int& rb : p.row_b) rb = slot_of[drow[rb]];
  p.o_rb = mb.add(p.row_b);
  std::vector<int> tab(5 * k), adm(nd, 0), saved(nd, 0);
  for (int i = 0; i < k; ++i) {
    tab[5 * i] = drow[i]; tab[5 * i + 1] = sb.pl[i]; tab[5 * i + 2] = p.seq_len[i]; tab[5 * i + 3] = p.S_[i]; tab[5 * i + 4] = p.hrow(i);
    adm[drow[i]] = 1;
  }
  const long o_tab = mb.add(tab), o_adm = mb.add(adm), o_saved = mb.add(saved);
  UniformCols uc;
  if (int e = uniform_cols(c, b, s, drow, crow, mb, uc)) return e;
  if (int e = upload_meta(c)) return e;
  uniform_cols_launch(c, s, uc, mb);
  if (int e = prefill_layers(c, p, mb)) return e;
  launch_admit_rows(mb.dev(o_tab), k, prefill_hsrc(c, p), c->dh2, c->cur_tok, c->cur_pos, c->ctx_len, c->n_gen, c->text_len,
                    c->slot_meta, c->slot_of, c->stream);
  launch_dec_reduce_ln_pack(nullptr, 0, D_MODEL, nullptr, c->dh2, nullptr, W(c, "ar_decoder.norm.weight"),
                            W(c, "ar_decoder.norm.bias"), c->xp_att, nd, c->stream);
  launch_skinny_gemm(c->pred_wp, c->xp_att, c->p_logits, PRED_NPAD, D_MODEL, SK_PRED, c->stream);
  int* sv = c->imeta + o_saved;
  launch_admit_mask(0, mb.dev(o_adm), sv, nd, c->active, c->slot_meta, c->slot_of, c->n_active, c->stream);
  LAUNCH(launch_dec_sample(sa, c->stream));
  launch_admit_mask(1, mb.dev(o_adm), sv, nd, c->active, c->slot_meta, c->slot_of, c->n_active, c->stream);
  return launch_status(c);
}

int infer_continuous(vx_ctx* c, const vx_batch* b, const vx_sampling* s, vx_row_done_fn on_row, void* user, int64_t* out_codes,
                     int32_t out_stride, int32_t* out_lens) {
  const int B = b->batch, nd = std::min(c->mbr, B);
  hipEvent_t e0 = c->ev_t[0], e1 = c->ev_t[1], e2 = c->ev_t[2];
  HIPCHK(hipEventRecord(e0, c->stream));
  // per decode row: the caller row in it (-1: free), the step count at its admission and the step by which it has stopped at the
  // latest (the sampler stops a row at n_gen = min(16 S, gen_stride, force_eos_at))
  std::vector<int> occ(nd, -1), done_by(nd, 0), act(nd, 0), ng(nd, 0), slot_of(nd);
  std::vector<std::vector<int>> rowgen(B);           // first-codebook ids of every harvested row (D2H target: never reallocated)
  std::vector<int> pend;                             // harvested rows waiting for their NAR stages, in the order they completed
  int next = 0;                                      // first caller row not admitted yet
  long steps = 0;
  const int first_cap = s->force_eos_at >= 0 ? std::min(c->gen_stride, s->force_eos_at) : c->gen_stride;
  auto row_cap = [&](int r) { return std::min(first_cap, 16 * b->text_lens[r]); };
  auto cut_by_arena = [&](int n, int S) {
    return n >= c->gen_stride && c->gen_stride < 16 * S && !(s->force_eos_at >= 0 && s->force_eos_at <= c->gen_stride);
  };
  SampleArgs sa{};
  // one admission round (first fill or admission) with the f16x2 range guard of ar_generate: a raised flag re-runs the round,
  // prefill and first sample, on the exact-fp32 kernels; it counts in vx_last_fallbacks and towards sticky mode
  auto round = [&](const std::vector<int>& drow, const std::vector<int>& crow) -> int {
    const bool first = occ[0] < 0 && next == 0;
    bool raised = false;
    auto attempt = [&](bool read_flag) -> int {
      if (first) {
        if (int e = ar_prefill(c, b, 0, nd)) return e;
        sa = make_sample_args(c, s, 1, nullptr);
        sa.uniforms = c->d_uniforms;                 // every row draws from its own column, injected or counter-based
        MetaBuilder mb(c);
        UniformCols uc;
        if (int e = uniform_cols(c, b, s, drow, crow, mb, uc)) return e;
        if (int e = upload_meta(c)) return e;
        uniform_cols_launch(c, s, uc, mb);
        LAUNCH(launch_dec_sample(sa, c->stream));
        if (int e = launch_status(c)) return e;
        D2H(slot_of.data(), c->slot_of, nd * sizeof(int));
      } else if (int e = admit_rows(c, b, s, sa, drow, crow, slot_of)) return e;
      int flag = 0;
      D2H(act.data(), c->active, nd * sizeof(int));
      D2H(ng.data(), c->n_gen, nd * sizeof(int));
      if (read_flag) D2H(&flag, c->range_flag, sizeof(int));
      SYNC();
      raised = flag != 0;
      return VX_OK;
    };
    const bool direct_f32 = fb_direct(c, c->sticky_prefill_f32, c->sticky_prefill_age);
    if (direct_f32) {
      ++c->st_fb_prefill; ++c->fb_total;
      if (int e = ensure_f32_buffers(c)) return e;
      F32Scope f32(c);
      if (int e = attempt(false)) return e;
    } else {
      if (int e = attempt(range_guarded(c))) return e;
      fb_outcome(c, raised, c->fb_prefill_raises, c->sticky_prefill_f32, c->sticky_prefill_age);
      if (raised) {
        HIPCHK(hipMemsetAsync(c->range_flag, 0, sizeof(int), c->stream));
        ++c->st_fb_prefill; ++c->fb_total;
        if (int e = ensure_f32_buffers(c)) return e;
        F32Scope f32(c);
        if (int e = attempt(false)) return e;
      }
    }
    for (size_t i = 0; i < drow.size(); ++i) { occ[drow[i]] = crow[i]; done_by[drow[i]] = (int)steps + row_cap(crow[i]); }
    next += (int)crow.size();
    return VX_OK;
  };
  // NAR stages of the first n pending rows, then their codes to the caller
  auto nar_group = [&](int n) -> int {
    std::vector<int> rows(pend.begin(), pend.begin() + n), T(n), codes0((size_t)n * c->gen_stride, 0), oc;
    pend.erase(pend.begin(), pend.begin() + n);
    SYNC();                                          // the harvested gen rows have arrived
    for (int i = 0; i < n; ++i) {
      T[i] = (int)rowgen[rows[i]].size();
      std::copy(rowgen[rows[i]].begin(), rowgen[rows[i]].end(), codes0.begin() + (size_t)i * c->gen_stride);
    }
    SubBatch sb(b, rows);
    long sumT = 0;
    HIPCHK(hipEventRecord(e1, c->stream));
    if (int e = nar_generate(c, &sb.b, 0, n, T, codes0.data(), c->gen_stride, oc, sumT)) return e;
    HIPCHK(hipEventRecord(e2, c->stream));
    HIPCHK(hipEventSynchronize(e2));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e1, e2)); c->st_nar_ms += ms;
    long off = 0;
    for (int i = 0; i < n; ++i) {
      const int r = rows[i];
      out_lens[r] = T[i];
      c->st_frames += T[i];
      if (cut_by_arena(T[i], b->text_lens[r])) ++c->st_truncated;
      int64_t* o0 = out_codes + (long)r * out_stride * N_Q;
      for (int t = 0; t < T[i]; ++t) {
        int64_t* o = o0 + (long)t * N_Q;
        o[0] = codes0[(size_t)i * c->gen_stride + t];
        for (int st = 0; st < N_Q - 1; ++st) o[st + 1] = oc[(size_t)st * sumT + off + t];
      }
      off += T[i];
      if (on_row) on_row(user, r, o0, T[i]);
    }
    return VX_OK;
  };

  {
    std::vector<int> first(nd);
    for (int i = 0; i < nd; ++i) first[i] = i;
    if (int e = round(first, first)) return e;
  }
  char sig[160];
  snprintf(sig, sizeof sig, "b%d ns%d c%d%d%d k%d t%a u%d f%d l%d", nd, c->nsplit, (int)c->sb_chain, (int)c->sb_qkv, (int)c->split_fused, sa.top_k,
           sa.temperature, sa.uniforms != nullptr, sa.force_eos_at, sa.sum_logp != nullptr);
  const int sync_every = s->sync_every > 0 ? s->sync_every : 8;
  const int gs = (c->graph_multi && sync_every % GRAPH_STEPS == 0) ? GRAPH_STEPS : 1;
  for (;;) {
    // harvest: the rows that stopped hand their ids to the host (delivered at the next sync) and free their decode rows
    std::vector<int> freed;
    for (int d = 0; d < nd; ++d) {
      if (occ[d] < 0 || act[d]) continue;
      const int r = occ[d];
      if (ng[d] > out_stride) FAIL(VX_EINVAL, "out_stride %d too small for %d frames", out_stride, ng[d]);
      rowgen[r].assign(ng[d], 0);
      if (ng[d]) D2H(rowgen[r].data(), c->gen + (size_t)d * c->gen_stride, ng[d] * sizeof(int));
      pend.push_back(r);
      occ[d] = -1;
    }
    for (int d = 0; d < nd; ++d) if (occ[d] < 0) freed.push_back(d);
    // admission (policy: whenever a poll finds a free row), FIFO over the waiting caller rows
    if (next < B && !freed.empty()) {
      const int k = std::min<int>((int)freed.size(), B - next);
      std::vector<int> drow(freed.begin(), freed.begin() + k), crow(k);
      for (int i = 0; i < k; ++i) crow[i] = next + i;
      if (int e = round(drow, crow)) return e;
      continue;                                      // an admitted row may have stopped at its first sample
    }
    const bool live = std::any_of(occ.begin(), occ.end(), [](int r) { return r >= 0; });
    while ((int)pend.size() >= c->mbr || (!live && !pend.empty()))
      if (int e = nar_group(std::min<int>(c->mbr, (int)pend.size()))) return e;
    if (!live) break;
    // decode steps up to the next host poll, or up to the step by which a live row has stopped at the latest (its cap: that poll
    // is sure to free a row -- without it a row capped between two polls would leave its decode row idle until the next one)
    long soonest = (steps / sync_every + 1) * sync_every;
    for (int d = 0; d < nd; ++d) if (occ[d] >= 0) soonest = std::min<long>(soonest, done_by[d]);
    const long target = std::max(soonest, steps + 1);
    while (steps < target) {
      const int n = (steps % gs == 0 && steps + gs <= target) ? gs : 1;
      if (int e = ar_step_run(c, &sa, sig, n)) return e;
      steps += n;
    }
    D2H(act.data(), c->active, nd * sizeof(int));
    D2H(ng.data(), c->n_gen, nd * sizeof(int));
    SYNC();
  }
  HIPCHK(hipEventRecord(e1, c->stream));
  HIPCHK(hipEventSynchronize(e1));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, e0, e1));
  c->st_ar_ms = ms - c->st_nar_ms;
  c->st_steps = steps;
  return VX_OK;
}

// ---- serving session (vx_serve_*) ----------------------------------------------------------------------------------
// A decode batch of nd = min(max_batch, 32) rows that outlives any single call.  Requests are submitted at any time (host copies
// only); vx_serve_run admits them first come first served into free decode rows, decodes, harvests requests whose beams have all
// stopped, selects one beam per request and runs the NAR stages in groups.  Geometry (slot order, context splits, chain) is fixed
// at vx_serve_open for nd free rows (serve_setup), so the captured step graph never changes; every admission, the first included,
// goes through serve_admit.  DESIGN.md section 10.
struct ServeReq {
  int64_t id = 0;
  int N = 1;                                   // beams
  float length_penalty = 1.f;
  bool worst = false;
  unsigned long long seed = 0;
  int usteps = 0;                              // injected draws per beam (0: counter-based)
  int top_k = 1;                               // topk_sampling arguments of this request (vx_request_sampling, or the session's)
  float temperature = 1.f;
  int force_eos_at = -1;
  float top_p = 1.f, rep_penalty = 1.f;        // vx_request_filters (neutral: 1, 1, 0, 0)
  int rep_window = 0, min_frames = 0;
  std::vector<float> u;                        // [N][usteps]
  std::vector<int32_t> ids, lang, pc;          // text ids / language ids [S], prompt codes [Tp][8]
  int S = 0, Tp = 0;
  std::vector<int> rows;                       // decode row of every beam
  std::vector<std::vector<int>> gen;           // first-codebook ids of every harvested beam (D2H targets: never reallocated)
  std::vector<int> ng;                         // frames of every harvested beam
  std::vector<float> slp;                      // sum(logp) of every harvested beam
  int harvested = 0;
  // the step count at which the sampler has stopped every beam at the latest: min(16 S, gen_stride, force_eos_at)
  int cap(int gen_stride) const { return std::min(force_eos_at >= 0 ? std::min(gen_stride, force_eos_at) : gen_stride, 16 * S); }
};

// requests gathered into one vx_batch (prefill / NAR of a request group)
struct ReqBatch {
  std::vector<int32_t> ids, lang, tl, pc, pl;
  vx_batch b{};
  explicit ReqBatch(const std::vector<ServeReq*>& rq) {
    const int n = (int)rq.size();
    int ts = 1, ps = 1;
    for (const ServeReq* r : rq) { ts = std::max(ts, r->S); ps = std::max(ps, r->Tp); }
    ids.assign((size_t)n * ts, 0); lang.assign((size_t)n * ts, 0); pc.assign((size_t)n * ps * N_Q, 0); tl.resize(n); pl.resize(n);
    for (int i = 0; i < n; ++i) {
      const ServeReq* r = rq[i];
      std::copy(r->ids.begin(), r->ids.end(), ids.begin() + (size_t)i * ts);
      std::copy(r->lang.begin(), r->lang.end(), lang.begin() + (size_t)i * ts);
      std::copy(r->pc.begin(), r->pc.end(), pc.begin() + (size_t)i * ps * N_Q);
      tl[i] = r->S; pl[i] = r->Tp;
    }
    b.struct_size = sizeof(vx_batch); b.batch = n;
    b.text_ids = ids.data(); b.text_lang = lang.data(); b.text_stride = ts; b.text_lens = tl.data();
    b.prompt_codes = pc.data(); b.prompt_stride = ps; b.prompt_lens = pl.data();
  }
};

}  // namespace vxe

struct vx_serve {
  vx_ctx* c = nullptr;
  vx_sampling s{};                             // session-wide: top_k, temperature, force_eos_at, sync_every
  int nd = 0;
  int64_t next_id = 0;
  std::deque<std::unique_ptr<ServeReq>> waiting;
  std::vector<std::unique_ptr<ServeReq>> live;     // admitted, some beam still decoding
  std::vector<std::unique_ptr<ServeReq>> pend;     // every beam harvested, NAR stages pending (in the order they completed)
  std::vector<ServeReq*> occ;                  // per decode row: its request (null: free)
  std::vector<int> beam, done_by, act, ng, slot_of;
  long steps = 0;                              // decode steps since vx_serve_open
  ServeSampleArgs rsa{};                       // the per-row sampler of every step and admission (serve_sample.hip)
  std::string sig;
  bool running = false;                        // inside vx_serve_run (on_done): vx_serve_cancel refuses
};

namespace vxe {

// nd free decode rows: identity slot order, every row inactive (slot record {d, 1, 0}), n_active = 0, and the geometry of nd rows
static int serve_setup(vx_ctx* c, int nd) {
  std::vector<int> zero(nd, 0), one(nd, 1), meta(4 * nd, 0), slot(nd);
  for (int d = 0; d < nd; ++d) { meta[4 * d] = d; meta[4 * d + 1] = 1; slot[d] = d; }
  MetaBuilder mb(c);
  const long o_z = mb.add(zero), o_1 = mb.add(one), o_meta = mb.add(meta), o_slot = mb.add(slot);
  if (int e = upload_meta(c)) return e;
  const size_t ib = nd * sizeof(int);
  HIPCHK(hipMemcpyAsync(c->cur_pos, mb.dev(o_z), ib, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->ctx_len, mb.dev(o_1), ib, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->n_gen, mb.dev(o_z), ib, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->cur_tok, mb.dev(o_z), ib, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->active, mb.dev(o_z), ib, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->text_len, mb.dev(o_1), ib, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->slot_meta, mb.dev(o_meta), 4 * ib, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->slot_of, mb.dev(o_slot), ib, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemsetAsync(c->n_active, 0, sizeof(int), c->stream));
  c->cur_batch = nd;
  c->h_L.assign(nd, 0);
  decode_geometry(c, nd, true);
  SYNC();                                      // the staged tables are consumed before the next MetaBuilder reuses imeta
  return VX_OK;
}

// admission of requests rq (their beam rows assigned, rq[i]->rows) into free decode rows, up to and including their first sample.
// Each request is prefilled once, into the arena slot of its first beam row; the fan-out (beams.hip, pairs only) copies its K / V to
// the other beams' slots; every beam row gets its own admit_rows entry pointing at the request's prefill row, its own draws (keyed
// on (request seed, beam) or the request's injected column) and a zero sum_logp.  The rows still decoding keep every piece of their
// state, as in admit_rows.
static int serve_admit(vx_serve* v, const std::vector<ServeReq*>& rq) {
  vx_ctx* c = v->c;
  const int k = (int)rq.size(), nd = v->nd;
  ReqBatch rb(rq);
  PrefillPlan p;
  MetaBuilder mb(c);
  if (int e = prefill_tables(c, &rb.b, 0, k, p, mb)) return e;
  for (int& r : p.row_b) r = v->slot_of[rq[r]->rows[0]];
  p.o_rb = mb.add(p.row_b);
  std::vector<int> tab, adm(nd, 0), saved(nd, 0), pairs, staged, utab;
  const int cap_steps = c->gen_stride + 1;         // draws a row can ever consume: one per generated frame + the terminating one
  int max_steps = 1;
  for (int i = 0; i < k; ++i) {
    const ServeReq* r = rq[i];
    if (p.seq_len[i] > c->Tmax) FAIL(VX_EINVAL, "request %lld: %d cached rows exceed the arena (%d)", (long long)r->id, p.seq_len[i], c->Tmax);
    for (int j = 0; j < r->N; ++j) {
      const int d = r->rows[j];
      tab.insert(tab.end(), {d, r->Tp, p.seq_len[i], p.S_[i], p.hrow(i)});
      adm[d] = 1;
      if (j) pairs.insert(pairs.end(), {v->slot_of[r->rows[0]], v->slot_of[d], p.seq_len[i]});
    }
  }
  // injected draws first (their offsets go into the draw table), as float bits in the int tables
  std::vector<int> soff(k, -1);
  for (int i = 0; i < k; ++i) {
    const ServeReq* r = rq[i];
    if (!r->usteps) continue;
    soff[i] = (int)staged.size();
    const int st = std::min(r->usteps, cap_steps);
    for (int j = 0; j < r->N; ++j) {
      const size_t o = staged.size();
      staged.resize(o + st);
      memcpy(&staged[o], &r->u[(size_t)j * r->usteps], st * sizeof(float));
    }
  }
  const long o_st = staged.empty() ? 0 : mb.add(staged);
  for (int i = 0; i < k; ++i) {
    const ServeReq* r = rq[i];
    const int st = r->usteps ? std::min(r->usteps, cap_steps) : cap_steps;
    max_steps = std::max(max_steps, st);
    for (int j = 0; j < r->N; ++j)
      utab.insert(utab.end(), {r->rows[j], j, r->usteps ? (int)(o_st + soff[i] + (long)j * st) : -1, st, (int)(uint32_t)r->seed,
                               (int)(uint32_t)(r->seed >> 32), r->top_k, __builtin_bit_cast(int, r->temperature), r->force_eos_at,
                               __builtin_bit_cast(int, r->top_p), __builtin_bit_cast(int, r->rep_penalty), r->rep_window,
                               r->min_frames});
  }
  const int nbeam = (int)tab.size() / 5;
  if ((long)max_steps * nd > c->uniforms_cap) FAIL(VX_EINVAL, "too many uniforms (%d steps)", max_steps);
  const long o_tab = mb.add(tab), o_adm = mb.add(adm), o_saved = mb.add(saved), o_ut = mb.add(utab),
             o_fp = pairs.empty() ? 0 : mb.add(pairs);
  if (int e = upload_meta(c)) return e;
  launch_serve_uniforms(mb.dev(o_ut), nbeam, max_steps, reinterpret_cast<const float*>(c->imeta), c->d_uniforms, nd, c->sum_logp,
                        c->row_smp, c->row_flt, c->stream);
  if (int e = prefill_layers(c, p, mb)) return e;
  const float* hsrc = prefill_hsrc(c, p);
  if (!pairs.empty())
    launch_beam_fanout(c->kc, c->vc, (long)((size_t)c->mbr * N_HEAD * c->Tmax * D_HEAD), c->NL, c->Tmax, mb.dev(o_fp),
                       (int)pairs.size() / 3, hsrc, nullptr, c->dh, 0, c->stream);
  launch_admit_rows(mb.dev(o_tab), nbeam, hsrc, c->dh2, c->cur_tok, c->cur_pos, c->ctx_len, c->n_gen, c->text_len, c->slot_meta,
                    c->slot_of, c->stream);
  launch_dec_reduce_ln_pack(nullptr, 0, D_MODEL, nullptr, c->dh2, nullptr, W(c, "ar_decoder.norm.weight"),
                            W(c, "ar_decoder.norm.bias"), c->xp_att, nd, c->stream);
  launch_skinny_gemm(c->pred_wp, c->xp_att, c->p_logits, PRED_NPAD, D_MODEL, SK_PRED, c->stream);
  int* sv = c->imeta + o_saved;
  launch_admit_mask(0, mb.dev(o_adm), sv, nd, c->active, c->slot_meta, c->slot_of, c->n_active, c->stream);
  LAUNCH(launch_serve_sample(v->rsa, c->stream));
  launch_admit_mask(1, mb.dev(o_adm), sv, nd, c->active, c->slot_meta, c->slot_of, c->n_active, c->stream);
  return launch_status(c);
}

// one admission round with the f16x2 range guard of infer_continuous: a raised flag re-runs the round (prefill, fan-out, first
// sample) on the exact-fp32 kernels; it counts in vx_last_fallbacks and towards sticky mode
static int serve_round(vx_serve* v, const std::vector<ServeReq*>& rq) {
  vx_ctx* c = v->c;
  const int nd = v->nd;
  bool raised = false;
  auto attempt = [&](bool read_flag) -> int {
    if (int e = serve_admit(v, rq)) return e;
    int flag = 0;
    D2H(v->act.data(), c->active, nd * sizeof(int));
    D2H(v->ng.data(), c->n_gen, nd * sizeof(int));
    if (read_flag) D2H(&flag, c->range_flag, sizeof(int));
    SYNC();
    raised = flag != 0;
    return VX_OK;
  };
  if (fb_direct(c, c->sticky_prefill_f32, c->sticky_prefill_age)) {
    ++c->st_fb_prefill; ++c->fb_total;
    if (int e = ensure_f32_buffers(c)) return e;
    F32Scope f32(c);
    if (int e = attempt(false)) return e;
  } else {
    if (int e = attempt(range_guarded(c))) return e;
    fb_outcome(c, raised, c->fb_prefill_raises, c->sticky_prefill_f32, c->sticky_prefill_age);
    if (raised) {
      HIPCHK(hipMemsetAsync(c->range_flag, 0, sizeof(int), c->stream));
      ++c->st_fb_prefill; ++c->fb_total;
      if (int e = ensure_f32_buffers(c)) return e;
      F32Scope f32(c);
      if (int e = attempt(false)) return e;
    }
  }
  for (ServeReq* r : rq)
    for (int j = 0; j < r->N; ++j) {
      const int d = r->rows[j];
      v->occ[d] = r; v->beam[d] = j; v->done_by[d] = (int)v->steps + r->cap(c->gen_stride);
    }
  return VX_OK;
}

// NAR stages of the first n pending requests (each reduced to its selected beam), then their codes to the caller
static int serve_nar_group(vx_serve* v, int n, vx_serve_done_fn on_done, void* user) {
  vx_ctx* c = v->c;
  std::vector<std::unique_ptr<ServeReq>> grp;
  for (int i = 0; i < n; ++i) grp.push_back(std::move(v->pend[i]));
  v->pend.erase(v->pend.begin(), v->pend.begin() + n);
  SYNC();                                            // the harvested gen rows and sums have arrived
  std::vector<ServeReq*> rq(n);
  std::vector<int> T(n), codes0((size_t)n * c->gen_stride, 0), oc;
  for (int i = 0; i < n; ++i) {
    ServeReq* r = rq[i] = grp[i].get();
    const int pick = select_beam(r->slp.data(), r->ng.data(), r->N, r->Tp, r->length_penalty, r->worst);
    T[i] = r->ng[pick];
    std::copy(r->gen[pick].begin(), r->gen[pick].begin() + T[i], codes0.begin() + (size_t)i * c->gen_stride);
  }
  ReqBatch rb(rq);
  long sumT = 0;
  hipEvent_t e1 = c->ev_t[1], e2 = c->ev_t[2];
  HIPCHK(hipEventRecord(e1, c->stream));
  if (int e = nar_generate(c, &rb.b, 0, n, T, codes0.data(), c->gen_stride, oc, sumT)) return e;
  HIPCHK(hipEventRecord(e2, c->stream));
  HIPCHK(hipEventSynchronize(e2));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, e1, e2)); c->st_nar_ms += ms;
  long off = 0;
  std::vector<int64_t> out;
  for (int i = 0; i < n; ++i) {
    c->st_frames += T[i];
    const bool forced = rq[i]->force_eos_at >= 0 && rq[i]->force_eos_at <= c->gen_stride;     // the request's own cap
    if (T[i] >= c->gen_stride && c->gen_stride < 16 * rq[i]->S && !forced) ++c->st_truncated;
    out.assign((size_t)std::max(1, T[i]) * N_Q, 0);
    for (int t = 0; t < T[i]; ++t) {
      int64_t* o = out.data() + (size_t)t * N_Q;
      o[0] = codes0[(size_t)i * c->gen_stride + t];
      for (int st = 0; st < N_Q - 1; ++st) o[st + 1] = oc[(size_t)st * sumT + off + t];
    }
    off += T[i];
    if (on_done) on_done(user, rq[i]->id, out.data(), T[i]);
  }
  return VX_OK;
}

static int serve_run(vx_serve* v, int max_steps, vx_serve_done_fn on_done, void* user) {
  vx_ctx* c = v->c;
  const int nd = v->nd;
  hipEvent_t e0 = c->ev_t[0], e1 = c->ev_t[1];
  HIPCHK(hipEventRecord(e0, c->stream));
  const long start = v->steps;
  const int sync_every = v->s.sync_every > 0 ? v->s.sync_every : 8;
  const int gs = (c->graph_multi && sync_every % GRAPH_STEPS == 0) ? GRAPH_STEPS : 1;
  for (;;) {
    // harvest: the beam rows that stopped hand their ids and sums to the host (delivered at the next sync) and free their rows
    for (int d = 0; d < nd; ++d) {
      ServeReq* r = v->occ[d];
      if (!r || v->act[d]) continue;
      const int j = v->beam[d];
      r->ng[j] = v->ng[d];
      r->gen[j].assign(std::max(1, v->ng[d]), 0);
      if (v->ng[d]) D2H(r->gen[j].data(), c->gen + (size_t)d * c->gen_stride, v->ng[d] * sizeof(int));
      D2H(&r->slp[j], c->sum_logp + d, sizeof(float));
      v->occ[d] = nullptr;
      if (++r->harvested == r->N) {
        auto it = std::find_if(v->live.begin(), v->live.end(), [&](const std::unique_ptr<ServeReq>& q) { return q.get() == r; });
        v->pend.push_back(std::move(*it));
        v->live.erase(it);
      }
    }
    // admission, first come first served: the head waits for best_of free rows, a later request does not overtake it
    std::vector<int> freed;
    for (int d = 0; d < nd; ++d) if (!v->occ[d]) freed.push_back(d);
    std::vector<ServeReq*> rq;
    size_t used = 0;
    while (!v->waiting.empty() && (size_t)v->waiting.front()->N <= freed.size() - used) {
      std::unique_ptr<ServeReq> r = std::move(v->waiting.front());
      v->waiting.pop_front();
      r->rows.assign(freed.begin() + used, freed.begin() + used + r->N);
      used += r->N;
      r->gen.assign(r->N, {}); r->ng.assign(r->N, 0); r->slp.assign(r->N, 0.f); r->harvested = 0;
      rq.push_back(r.get());
      v->live.push_back(std::move(r));
    }
    if (!rq.empty()) {
      if (int e = serve_round(v, rq)) return e;
      continue;                                      // an admitted beam may have stopped at its first sample
    }
    const bool live = std::any_of(v->occ.begin(), v->occ.end(), [](const ServeReq* r) { return r != nullptr; });
    while ((int)v->pend.size() >= c->mbr)
      if (int e = serve_nar_group(v, c->mbr, on_done, user)) return e;
    if (!live || (max_steps > 0 && v->steps - start >= max_steps)) break;
    // decode steps up to the next host poll, or up to the step by which a live row has stopped at the latest (its cap)
    long soonest = (v->steps / sync_every + 1) * sync_every;
    for (int d = 0; d < nd; ++d) if (v->occ[d]) soonest = std::min<long>(soonest, v->done_by[d]);
    long target = std::max(soonest, v->steps + 1);
    if (max_steps > 0) target = std::min(target, start + max_steps);
    while (v->steps < target) {
      const int n = (v->steps % gs == 0 && v->steps + gs <= target) ? gs : 1;
      if (int e = ar_step_run(c, nullptr, v->sig, n, &v->rsa)) return e;
      v->steps += n;
    }
    D2H(v->act.data(), c->active, nd * sizeof(int));
    D2H(v->ng.data(), c->n_gen, nd * sizeof(int));
    SYNC();
  }
  // every request harvested during this call goes through its NAR stages before the call returns
  while (!v->pend.empty())
    if (int e = serve_nar_group(v, std::min<int>(c->mbr, (int)v->pend.size()), on_done, user)) return e;
  HIPCHK(hipEventRecord(e1, c->stream));
  HIPCHK(hipEventSynchronize(e1));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, e0, e1));
  c->st_ar_ms = ms - c->st_nar_ms;
  c->st_steps = v->steps - start;
  SYNC();                                            // beams harvested at the last poll of a request still decoding: delivered now
  return VX_OK;
}

// entry points that overwrite the decode state refuse to run while a serving session owns it
static int serve_busy(vx_ctx* c, const char* what) {
  if (!c->serve) return VX_OK;
  FAIL(VX_EINVAL, "%s: a serving session is open on this context (vx_serve_close it first)", what);
}

// vx_serve_submit / vx_serve_submit_ex / vx_serve_submit_filtered: smp null = the session's top_k / temperature / force_eos_at for
// every request; flt null = the neutral filters (top_p 1, repetition penalty 1, min_frames 0)
static int serve_submit(vx_serve* v, const vx_batch* b, const vx_request* req, const vx_request_sampling* smp,
                        const vx_request_filters* flt, int64_t* ids_out) {
  vx_ctx* c = v->c;
  if (int e = check_batch(c, b, 0x7fffffff)) return e;
  std::vector<vx_request_sampling> rs(b->batch, vx_request_sampling{sizeof(vx_request_sampling), v->s.top_k, v->s.temperature,
                                                                    v->s.force_eos_at});
  for (int i = 0; i < b->batch; ++i) {
    const vx_request& q = req[i];
    if (q.struct_size != sizeof(vx_request))
      FAIL(VX_EINVAL, "vx_request.struct_size is %u, this library expects %zu (ABI version %d)", q.struct_size, sizeof(vx_request), VX_ABI_VERSION);
    if (smp) {
      const vx_request_sampling& m = smp[i];
      if (m.struct_size != sizeof(vx_request_sampling))
        FAIL(VX_EINVAL, "vx_request_sampling.struct_size is %u, this library expects %zu (ABI version %d)", m.struct_size,
             sizeof(vx_request_sampling), VX_ABI_VERSION);
      if (!(m.temperature > 0.f) || !std::isfinite(m.temperature))
        FAIL(VX_EINVAL, "request %d: temperature must be > 0 and finite (got %g)", i, (double)m.temperature);
      if (m.force_eos_at < -1) FAIL(VX_EINVAL, "request %d: force_eos_at must be >= -1 (got %d)", i, m.force_eos_at);
      rs[i] = m;
    }
    if (flt) {
      const vx_request_filters& f = flt[i];
      if (f.struct_size != sizeof(vx_request_filters))
        FAIL(VX_EINVAL, "vx_request_filters.struct_size is %u, this library expects %zu (ABI version %d)", f.struct_size,
             sizeof(vx_request_filters), VX_ABI_VERSION);
      if (!std::isfinite(f.top_p) || !(f.top_p > 0.f) || !(f.top_p <= 1.f))
        FAIL(VX_EINVAL, "request %d: top_p must be in (0, 1] (got %g)", i, (double)f.top_p);
      if (!std::isfinite(f.repetition_penalty) || !(f.repetition_penalty > 0.f))
        FAIL(VX_EINVAL, "request %d: repetition_penalty must be > 0 and finite (got %g)", i, (double)f.repetition_penalty);
      if (f.repetition_window < 0) FAIL(VX_EINVAL, "request %d: repetition_window must be >= 0 (got %d)", i, f.repetition_window);
      if (f.min_frames < 0) FAIL(VX_EINVAL, "request %d: min_frames must be >= 0 (got %d)", i, f.min_frames);
    }
    const int N = std::max(1, q.best_of);
    if (N > v->nd) FAIL(VX_EINVAL, "request %d: best_of %d exceeds the session's %d decode rows", i, N, v->nd);
    if (b->text_lens[i] + 1 + b->prompt_lens[i] > c->Tmax) FAIL(VX_EINVAL, "request %d: the prompt does not fit the arena", i);
    if (q.uniforms) {
      // every draw the request can consume: one per generated frame + the terminating one (its own force_eos_at)
      const int f = rs[i].force_eos_at;
      const int need = std::min(f >= 0 ? std::min(c->gen_stride, f) : c->gen_stride, 16 * b->text_lens[i]) + 1;
      if (q.uniforms_steps < need) FAIL(VX_EINVAL, "request %d: %d uniforms steps, it can draw %d", i, q.uniforms_steps, need);
    }
  }
  std::vector<std::unique_ptr<ServeReq>> add;
  for (int i = 0; i < b->batch; ++i) {
    const vx_request& q = req[i];
    auto r = std::make_unique<ServeReq>();
    r->top_k = rs[i].top_k; r->temperature = rs[i].temperature; r->force_eos_at = rs[i].force_eos_at;
    if (flt) {
      r->top_p = flt[i].top_p; r->rep_penalty = flt[i].repetition_penalty;
      r->rep_window = flt[i].repetition_window; r->min_frames = flt[i].min_frames;
    }
    r->N = std::max(1, q.best_of);
    r->length_penalty = q.length_penalty;
    r->worst = q.return_worst != 0;
    r->seed = q.seed;
    r->S = b->text_lens[i]; r->Tp = b->prompt_lens[i];
    r->ids.assign(b->text_ids + (long)i * b->text_stride, b->text_ids + (long)i * b->text_stride + r->S);
    r->lang.assign(b->text_lang + (long)i * b->text_stride, b->text_lang + (long)i * b->text_stride + r->S);
    r->pc.assign(b->prompt_codes + (long)i * b->prompt_stride * N_Q, b->prompt_codes + ((long)i * b->prompt_stride + r->Tp) * N_Q);
    if (q.uniforms) {       // [uniforms_steps][N] -> [N][steps], only the draws that can be consumed
      r->usteps = std::min(q.uniforms_steps, c->gen_stride + 1);
      r->u.resize((size_t)r->N * r->usteps);
      for (int j = 0; j < r->N; ++j)
        for (int t = 0; t < r->usteps; ++t) r->u[(size_t)j * r->usteps + t] = q.uniforms[(long)t * r->N + j];
    }
    add.push_back(std::move(r));
  }
  for (int i = 0; i < b->batch; ++i) {
    add[i]->id = v->next_id++;
    if (ids_out) ids_out[i] = add[i]->id;
    v->waiting.push_back(std::move(add[i]));
  }
  return VX_OK;
}

// vx_serve_cancel: 0 unknown / delivered / cancelled, 1 waiting (removed), 2 decoding (its rows stop and are free)
static int serve_cancel(vx_serve* v, int64_t id, int* state) {
  vx_ctx* c = v->c;
  *state = 0;
  auto wi = std::find_if(v->waiting.begin(), v->waiting.end(), [&](const std::unique_ptr<ServeReq>& q) { return q->id == id; });
  if (wi != v->waiting.end()) {
    v->waiting.erase(wi);
    *state = 1;
    return VX_OK;
  }
  auto li = std::find_if(v->live.begin(), v->live.end(), [&](const std::unique_ptr<ServeReq>& q) { return q->id == id; });
  if (li == v->live.end()) return VX_OK;
  // its beam rows that are still occupied (a beam harvested earlier has freed its row already): inactive before the next step,
  // slot records and n_active corrected on the stream, free on the host; the harvest never looks at them again
  unsigned rows = 0;
  for (int d = 0; d < v->nd; ++d)
    if (v->occ[d] == li->get()) { rows |= 1u << d; v->occ[d] = nullptr; }
  if (rows) launch_serve_cancel(rows, v->nd, c->active, c->slot_meta, c->slot_of, c->n_active, c->stream);
  HIPCHK(hipGetLastError());
  SYNC();                                           // the rows are stopped before the call returns (cancel is rare: one sync)
  v->live.erase(li);
  *state = 2;
  return VX_OK;
}

}  // namespace vxe

// =================================================================================================================
// C ABI
// =================================================================================================================
extern "C" {

const char* vx_last_error(const vx_ctx* c) { return c ? c->err.c_str() : g_create_err.c_str(); }

int32_t vx_abi_version(void) { return VX_ABI_VERSION; }

int vx_create(int device_id, const vx_config* cfg, vx_ctx** out) {
  if (!cfg || !out) { g_create_err = "null argument"; return VX_EINVAL; }
  if (cfg->struct_size != sizeof(vx_config)) {
    g_create_err = "vx_config.struct_size is " + std::to_string(cfg->struct_size) + ", this library expects " +
                   std::to_string(sizeof(vx_config)) + " (ABI version " + std::to_string(VX_ABI_VERSION) + ")";
    return VX_EINVAL;
  }
  if (cfg->num_layers <= 0 || cfg->max_batch <= 0 || cfg->max_text <= 0 || cfg->max_prompt < 0 || cfg->max_new <= 0) {
    g_create_err = "invalid vx_config";
    return VX_EINVAL;
  }
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) {
    g_create_err = std::string("no HIP device available: ") + hipGetErrorString(e);
    return VX_EHIP;
  }
  if (device_id < 0 || device_id >= ndev) { g_create_err = "device_id out of range"; return VX_EINVAL; }
  vx_ctx* c = new vx_ctx();
  c->cfg = *cfg;
  c->dev = device_id;
  c->NL = cfg->num_layers;
  auto fail = [&](hipError_t err, const char* what) {
    g_create_err = std::string(what) + ": " + hipGetErrorString(err);
    delete c;
    return VX_EHIP;
  };
  if ((e = hipSetDevice(device_id)) != hipSuccess) return fail(e, "hipSetDevice");
  bool masked = false;
  for (uint32_t w : cfg->cu_mask) masked |= w != 0;
  if (masked) {      // a context that shares the GPU with others: its stream only dispatches to the CUs of cfg->cu_mask
    if ((e = hipExtStreamCreateWithCUMask(&c->stream, 8, cfg->cu_mask)) != hipSuccess)
      return fail(e, "hipExtStreamCreateWithCUMask");
  } else if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) return fail(e, "hipStreamCreate");
  for (auto& ev : c->ev_t)
    if ((e = hipEventCreate(&ev)) != hipSuccess) {
      for (auto& e2 : c->ev_t) if (e2) (void)hipEventDestroy(e2);
      (void)hipStreamDestroy(c->stream);
      return fail(e, "hipEventCreate");
    }
  // the pinned transfer ring (engine_ctx.h): 64 MiB unless VX_PIN_MB says otherwise (>= 2 chunks)
  {
    size_t mb = 64;
    if (const char* ev = getenv("VX_PIN_MB")) mb = (size_t)std::max(16, std::min(1024, atoi(ev)));
    void* q = nullptr;
    if ((e = hipHostMalloc(&q, mb << 20, hipHostMallocDefault)) != hipSuccess) {
      for (auto& e2 : c->ev_t) if (e2) (void)hipEventDestroy(e2);
      (void)hipStreamDestroy(c->stream);
      return fail(e, "hipHostMalloc (pinned transfer ring)");
    }
    c->ring.base = static_cast<char*>(q);
    c->ring.cap = mb << 20;
  }
  *out = c;
  return VX_OK;
}

void vx_destroy(vx_ctx* c) {
  if (!c) return;
  delete c->serve;                 // an open session goes with its context
  c->serve = nullptr;
  (void)hipSetDevice(c->dev);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->graph_exec) (void)hipGraphExecDestroy(c->graph_exec);
  if (c->graph_exec_n) (void)hipGraphExecDestroy(c->graph_exec_n);
  for (auto& p : c->prof) for (auto ev : p.ev) (void)hipEventDestroy(ev);
  for (auto ev : c->ev_t) if (ev) (void)hipEventDestroy(ev);
  for (void* p : c->allocs) (void)hipFree(p);
  for (auto& kv : c->w) (void)hipFree(kv.second.d);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  if (c->ring.base) (void)hipHostFree(c->ring.base);
  delete c;
}

int vx_synchronize(vx_ctx* c) {
  if (!c) return VX_EINVAL;
  HIPCHK(hipSetDevice(c->dev));
  SYNC();
  return VX_OK;
}

int vx_ar_prefill(vx_ctx* c, const vx_batch* b) {
  if (!c) return VX_EINVAL;
  if (int e = serve_busy(c, "vx_ar_prefill")) return e;
  HIPCHK(hipSetDevice(c->dev));
  if (int e = check_batch(c, b, c->mbr)) return e;
  c->st_fb_prefill = c->st_fb_nar = 0;
  bool raised = fb_direct(c, c->sticky_prefill_f32, c->sticky_prefill_age);
  if (!raised) {
    if (int e = ar_prefill(c, b, 0, b->batch)) return e;
    if (int e = take_range_flag(c, &raised)) return e;       // syncs when the mode is guarded
    fb_outcome(c, raised, c->fb_prefill_raises, c->sticky_prefill_f32, c->sticky_prefill_age);
  }
  if (raised) {
    ++c->st_fb_prefill; ++c->fb_total;
    if (int e = ensure_f32_buffers(c)) return e;
    F32Scope f32(c);
    if (int e = ar_prefill(c, b, 0, b->batch)) return e;
  }
  SYNC();                 // the seam returns with the prefill complete in every mode
  HIPCHK(hipGetLastError());
  return VX_OK;
}

int vx_ar_logits(vx_ctx* c, float* out) {
  if (!c || !out) return VX_EINVAL;
  if (c->cur_batch <= 0) FAIL(VX_ESTATE, "no prefill has run");
  HIPCHK(hipSetDevice(c->dev));
  SampleArgs sa = make_sample_args(c, nullptr, 0, c->d_logits);
  LAUNCH(launch_dec_sample(sa, c->stream));
  if (int e = launch_status(c)) return e;
  D2H(out, c->d_logits, (size_t)c->cur_batch * AR_LOGITS * sizeof(float));
  SYNC();
  return VX_OK;
}

int vx_ar_step(vx_ctx* c, const int32_t* tokens) {
  if (!c || !tokens) return VX_EINVAL;
  if (int e = serve_busy(c, "vx_ar_step")) return e;
  if (c->cur_batch <= 0) FAIL(VX_ESTATE, "no prefill has run");
  HIPCHK(hipSetDevice(c->dev));
  H2D(c->force_tok, tokens, c->cur_batch * sizeof(int));
  launch_dec_force_token(c->force_tok, c->cur_tok, c->cur_pos, c->ctx_len, c->n_gen, c->gen, c->gen_stride, c->active,
                         c->cur_batch, c->slot_meta, c->slot_of, c->stream);
  if (int e = ar_step_run(c, nullptr, "")) return e;
  SYNC();
  HIPCHK(hipGetLastError());
  return VX_OK;
}

int vx_nar(vx_ctx* c, const vx_batch* b, const int32_t* codes0, int32_t codes0_stride, const int32_t* lens,
           int64_t* out_codes, int32_t out_stride) {
  if (!c || !codes0 || !lens || !out_codes) return VX_EINVAL;
  if (int e = serve_busy(c, "vx_nar")) return e;
  HIPCHK(hipSetDevice(c->dev));
  if (int e = check_batch(c, b, c->mbr)) return e;
  std::vector<int> T(lens, lens + b->batch);
  for (int i = 0; i < b->batch; ++i) {
    if (T[i] < 0 || T[i] > c->cfg.max_new || T[i] > out_stride || T[i] > codes0_stride) FAIL(VX_EINVAL, "row %d: bad length %d", i, T[i]);
    for (int t = 0; t < T[i]; ++t) {                    // indexes nar_audio_embeddings.0 (1025 rows) on the device
      const int v = codes0[(long)i * codes0_stride + t];
      if (v < 0 || v > AUDIO_VOCAB) FAIL(VX_EINVAL, "row %d: first-codebook id %d out of range (0..1024)", i, v);
    }
  }
  std::vector<int> oc;
  long sumT = 0;
  c->st_fb_prefill = c->st_fb_nar = 0;
  if (int e = nar_generate(c, b, 0, b->batch, T, codes0, codes0_stride, oc, sumT)) return e;
  long off = 0;
  for (int i = 0; i < b->batch; ++i) {
    for (int t = 0; t < T[i]; ++t) {
      int64_t* o = out_codes + ((long)i * out_stride + t) * N_Q;
      o[0] = codes0[(long)i * codes0_stride + t];
      for (int st = 0; st < N_Q - 1; ++st) o[st + 1] = oc[(size_t)st * sumT + off + t];
    }
    off += T[i];
  }
  return VX_OK;
}

int vx_infer(vx_ctx* c, const vx_batch* b, const vx_sampling* s, int64_t* out_codes, int32_t out_stride,
             int32_t* out_lens) {
  if (!c || !s || !out_codes || !out_lens) return VX_EINVAL;
  if (int e = serve_busy(c, "vx_infer")) return e;
  HIPCHK(hipSetDevice(c->dev));
  if (s->struct_size != sizeof(vx_sampling))
    FAIL(VX_EINVAL, "vx_sampling.struct_size is %u, this library expects %zu (ABI version %d)", s->struct_size, sizeof(vx_sampling), VX_ABI_VERSION);
  if (int e = check_batch(c, b, c->cfg.max_batch)) return e;
  if (!(s->temperature > 0.f)) FAIL(VX_EINVAL, "temperature must be > 0");
  c->st_steps = 0; c->st_frames = 0; c->st_ar_ms = 0; c->st_nar_ms = 0; c->st_truncated = 0;
  c->st_fb_prefill = c->st_fb_nar = 0;
  // a row that fills the arena although neither EOS, the reference's 16*S cap nor a forced EOS ended it was cut short
  auto cut_by_arena = [&](int n, int S) {
    return n >= c->gen_stride && c->gen_stride < 16 * S && !(s->force_eos_at >= 0 && s->force_eos_at <= c->gen_stride);
  };
  hipEvent_t e0 = c->ev_t[0], e1 = c->ev_t[1], e2 = c->ev_t[2];      // owned by the context: nothing to leak on an early return
  if (s->best_of > 1) {
    // best-of-N beams of every row (models/vallex.py:491,525-527): each row is decoded as N beams that sample independently, beams
    // that emit EOS stop; per row, selection on sum(logp) / len^penalty (:583-594), then the NAR stages run on the chosen beams only
    // (:600).  A micro-batch holds R = mbr / N rows = R*N decode rows; row r's result is what a batch-1 call on that row alone
    // returns with the same draws (uniforms column r*N + j = beam j of row r).
    const int N = s->best_of;
    if (N > c->mbr) FAIL(VX_EINVAL, "best_of %d exceeds the micro-batch (%d)", N, c->mbr);
    const int R = c->mbr / N;
    for (int r0 = 0, k = 0; r0 < b->batch; r0 += R, ++k) {
      const int nb = std::min(R, b->batch - r0);
      std::vector<int> n_gen, gen, oc;
      HIPCHK(hipEventRecord(e0, c->stream));
      if (int e = ar_generate(c, b, s, r0, nb, n_gen, gen, N, beam_seed(s->seed, k))) return e;
      HIPCHK(hipEventRecord(e1, c->stream));
      std::vector<float> slp((size_t)nb * N);
      D2H(slp.data(), c->sum_logp, slp.size() * sizeof(float)); SYNC();
      std::vector<int> T(nb), codes0((size_t)nb * c->gen_stride);
      for (int i = 0; i < nb; ++i) {
        const int pick = i * N + select_beam(&slp[(size_t)i * N], &n_gen[(size_t)i * N], N, b->prompt_lens[r0 + i], s->length_penalty,
                                             s->return_worst != 0);
        T[i] = n_gen[pick];
        if (T[i] > out_stride) FAIL(VX_EINVAL, "out_stride %d too small for %d frames", out_stride, T[i]);
        std::copy_n(gen.begin() + (size_t)pick * c->gen_stride, c->gen_stride, codes0.begin() + (size_t)i * c->gen_stride);
      }
      long sumT = 0;
      if (int e = nar_generate(c, b, r0, nb, T, codes0.data(), c->gen_stride, oc, sumT)) return e;
      HIPCHK(hipEventRecord(e2, c->stream));
      HIPCHK(hipEventSynchronize(e2));
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, e0, e1)); c->st_ar_ms += ms;
      HIPCHK(hipEventElapsedTime(&ms, e1, e2)); c->st_nar_ms += ms;
      long off = 0;
      for (int i = 0; i < nb; ++i) {
        out_lens[r0 + i] = T[i];
        c->st_frames += T[i];
        if (cut_by_arena(T[i], b->text_lens[r0 + i])) ++c->st_truncated;
        for (int t = 0; t < T[i]; ++t) {
          int64_t* o = out_codes + ((long)(r0 + i) * out_stride + t) * N_Q;
          o[0] = codes0[(size_t)i * c->gen_stride + t];
          for (int st = 0; st < N_Q - 1; ++st) o[st + 1] = oc[(size_t)st * sumT + off + t];
        }
        off += T[i];
      }
    }
    return VX_OK;
  }
  for (int r0 = 0; r0 < b->batch; r0 += c->mbr) {
    const int nb = std::min(c->mbr, b->batch - r0);
    std::vector<int> n_gen, gen, oc;
    HIPCHK(hipEventRecord(e0, c->stream));
    if (int e = ar_generate(c, b, s, r0, nb, n_gen, gen, 1, s->seed)) return e;
    HIPCHK(hipEventRecord(e1, c->stream));
    for (int i = 0; i < nb; ++i)
      if (n_gen[i] > out_stride) FAIL(VX_EINVAL, "out_stride %d too small for %d frames", out_stride, n_gen[i]);
    long sumT = 0;
    if (int e = nar_generate(c, b, r0, nb, n_gen, gen.data(), c->gen_stride, oc, sumT)) return e;
    HIPCHK(hipEventRecord(e2, c->stream));
    HIPCHK(hipEventSynchronize(e2));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1)); c->st_ar_ms += ms;
    HIPCHK(hipEventElapsedTime(&ms, e1, e2)); c->st_nar_ms += ms;
    long off = 0;
    for (int i = 0; i < nb; ++i) {
      out_lens[r0 + i] = n_gen[i];
      c->st_frames += n_gen[i];
      if (cut_by_arena(n_gen[i], b->text_lens[r0 + i])) ++c->st_truncated;
      for (int t = 0; t < n_gen[i]; ++t) {
        int64_t* o = out_codes + ((long)(r0 + i) * out_stride + t) * N_Q;
        o[0] = gen[(size_t)i * c->gen_stride + t];
        for (int st = 0; st < N_Q - 1; ++st) o[st + 1] = oc[(size_t)st * sumT + off + t];
      }
      off += n_gen[i];
    }
  }
  return VX_OK;
}

int vx_infer_continuous(vx_ctx* c, const vx_batch* b, const vx_sampling* s, vx_row_done_fn on_row, void* user, int64_t* out_codes,
                        int32_t out_stride, int32_t* out_lens) {
  if (!c || !s || !out_codes || !out_lens) return VX_EINVAL;
  if (int e = serve_busy(c, "vx_infer_continuous")) return e;
  HIPCHK(hipSetDevice(c->dev));
  if (s->struct_size != sizeof(vx_sampling))
    FAIL(VX_EINVAL, "vx_sampling.struct_size is %u, this library expects %zu (ABI version %d)", s->struct_size, sizeof(vx_sampling), VX_ABI_VERSION);
  // any number of rows: the call holds device memory for its min(max_batch, 32) decode rows and one NAR group only
  if (int e = check_batch(c, b, 0x7fffffff)) return e;
  if (!(s->temperature > 0.f)) FAIL(VX_EINVAL, "temperature must be > 0");
  if (s->best_of > 1) FAIL(VX_EINVAL, "vx_infer_continuous does not run best_of > 1 (use vx_infer)");
  c->st_steps = 0; c->st_frames = 0; c->st_ar_ms = 0; c->st_nar_ms = 0; c->st_truncated = 0;
  c->st_fb_prefill = c->st_fb_nar = 0;
  return infer_continuous(c, b, s, on_row, user, out_codes, out_stride, out_lens);
}

int vx_serve_open(vx_ctx* c, const vx_sampling* s, vx_serve** out) {
  if (!c || !s || !out) return VX_EINVAL;
  HIPCHK(hipSetDevice(c->dev));
  if (!c->finalized) FAIL(VX_ESTATE, "weights not finalized");
  if (s->struct_size != sizeof(vx_sampling))
    FAIL(VX_EINVAL, "vx_sampling.struct_size is %u, this library expects %zu (ABI version %d)", s->struct_size, sizeof(vx_sampling), VX_ABI_VERSION);
  if (c->serve) FAIL(VX_EINVAL, "a serving session is already open on this context");
  if (!(s->temperature > 0.f)) FAIL(VX_EINVAL, "temperature must be > 0");
  if (s->best_of > 1 || s->seed != 0 || s->uniforms || (s->length_penalty != 0.f && s->length_penalty != 1.f) || s->return_worst)
    FAIL(VX_EINVAL, "vx_serve_open: best_of, seed, uniforms, length_penalty and return_worst are per request (vx_request)");
  auto* v = new vx_serve();
  v->c = c;
  v->s = *s;
  v->s.best_of = 1; v->s.length_penalty = 1.f;
  v->nd = c->mbr;
  v->occ.assign(v->nd, nullptr);
  v->beam.assign(v->nd, 0); v->done_by.assign(v->nd, 0); v->act.assign(v->nd, 0); v->ng.assign(v->nd, 0);
  v->slot_of.resize(v->nd);
  for (int d = 0; d < v->nd; ++d) v->slot_of[d] = d;
  // the per-row sampling records (allocated once per context, before any step graph of a session is captured)
  if (!c->row_smp) {
    if (int e = dev_alloc(c, &c->row_smp, 4 * MB)) { delete v; return e; }
  }
  if (!c->row_flt) {
    if (int e = dev_alloc(c, &c->row_flt, 4 * MB)) { delete v; return e; }
  }
  if (int e = serve_setup(c, v->nd)) { delete v; return e; }
  // the per-row sampler (serve_sample.hip) with dec_sample's buffers: every beam row draws from its own column of d_uniforms
  // (injected or counter-based) and accumulates sum_logp (best_of is per request); top_k / temperature / force_eos_at come from
  // row_smp, so they are not part of the graph signature
  const SampleArgs sa = make_sample_args(c, &v->s, 1, nullptr);
  ServeSampleArgs& r = v->rsa;
  r.partial = sa.partial; r.splitk = sa.splitk; r.npad = sa.npad;
  r.row_smp = c->row_smp;
  r.row_flt = c->row_flt;           // every admission writes its rows' records; no sample runs on a row before its admission
  r.uniforms = c->d_uniforms; r.uniforms_stride = sa.uniforms_stride;
  r.cur_tok = sa.cur_tok; r.cur_pos = sa.cur_pos; r.ctx_len = sa.ctx_len; r.n_gen = sa.n_gen; r.active = sa.active;
  r.n_active = sa.n_active; r.text_len = sa.text_len; r.slot_meta = sa.slot_meta; r.slot_of = sa.slot_of;
  r.gen = sa.gen; r.gen_stride = sa.gen_stride; r.sum_logp = c->sum_logp; r.batch = sa.batch;
  r.emb_tab = sa.emb_tab; r.emb_alpha = sa.emb_alpha; r.pe = sa.pe; r.ln_g = sa.ln_g; r.ln_b = sa.ln_b; r.emb_h = sa.emb_h;
  r.emb_xp = sa.emb_xp; r.wt = sa.wt;
  char sig[160];
  snprintf(sig, sizeof sig, "b%d ns%d c%d%d%d serve-rows u1 l1", v->nd, c->nsplit, (int)c->sb_chain, (int)c->sb_qkv, (int)c->split_fused);
  v->sig = sig;
  c->serve = v;
  *out = v;
  return VX_OK;
}

int vx_serve_submit(vx_serve* v, const vx_batch* b, const vx_request* req, int64_t* ids_out) {
  if (!v || !req) return VX_EINVAL;
  return serve_submit(v, b, req, nullptr, nullptr, ids_out);
}

int vx_serve_submit_ex(vx_serve* v, const vx_batch* b, const vx_request* req, const vx_request_sampling* smp, int64_t* ids_out) {
  if (!v || !req) return VX_EINVAL;
  return serve_submit(v, b, req, smp, nullptr, ids_out);
}

int vx_serve_submit_filtered(vx_serve* v, const vx_batch* b, const vx_request* req, const vx_request_sampling* smp,
                             const vx_request_filters* flt, int64_t* ids_out) {
  if (!v || !req) return VX_EINVAL;
  return serve_submit(v, b, req, smp, flt, ids_out);
}

int vx_serve_cancel(vx_serve* v, int64_t request_id, int32_t* state) {
  if (!v) return VX_EINVAL;
  vx_ctx* c = v->c;
  if (v->running) FAIL(VX_EINVAL, "vx_serve_cancel: called from inside vx_serve_run (on_done); cancel between two vx_serve_run calls");
  HIPCHK(hipSetDevice(c->dev));
  int st = 0;
  if (int e = serve_cancel(v, request_id, &st)) return e;
  if (state) *state = st;
  return VX_OK;
}

int vx_serve_run(vx_serve* v, int32_t max_steps, vx_serve_done_fn on_done, void* user, int32_t* live_requests,
                 int32_t* waiting_requests) {
  if (!v) return VX_EINVAL;
  vx_ctx* c = v->c;
  if (v->running) FAIL(VX_EINVAL, "vx_serve_run: called from inside vx_serve_run (on_done)");
  HIPCHK(hipSetDevice(c->dev));
  c->st_steps = 0; c->st_frames = 0; c->st_ar_ms = 0; c->st_nar_ms = 0; c->st_truncated = 0;
  c->st_fb_prefill = c->st_fb_nar = 0;
  v->running = true;
  const int rc = serve_run(v, max_steps, on_done, user);
  v->running = false;
  if (rc) return rc;
  if (live_requests) *live_requests = (int32_t)v->live.size();
  if (waiting_requests) *waiting_requests = (int32_t)v->waiting.size();
  return VX_OK;
}

int vx_serve_close(vx_serve* v) {
  if (!v) return VX_EINVAL;
  vx_ctx* c = v->c;
  HIPCHK(hipSetDevice(c->dev));
  SYNC();                                           // no copy in flight may target a request that is about to go
  c->serve = nullptr;
  delete v;
  // the next vx_infer sets its own geometry (ar_prefill); nothing of the session's decode state is read again
  return VX_OK;
}

int64_t vx_read_tap(vx_ctx* c, const char* name, float* dst, int64_t max_floats) {
  if (!c || !name || !dst) return VX_EINVAL;
  auto it = c->taps.find(name);
  if (it == c->taps.end()) {
    // not a tap: a tensor as vx_load_tensor stored it (read-back check of an upload, tools/verify_checkpoint.py)
    it = c->w.find(name);
    if (it == c->w.end()) FAIL(VX_ENOTFOUND, "no tap or loaded tensor '%s'", name);
  }
  const int64_t n = std::min<int64_t>((int64_t)it->second.n, max_floats);
  HIPCHK(hipSetDevice(c->dev));
  SYNC();
  D2H(dst, it->second.d, n * sizeof(float)); SYNC();
  return n;
}

int vx_last_fallbacks(vx_ctx* c, int32_t* prefill_phases, int32_t* nar_phases, int64_t* lifetime) {
  if (!c) return VX_EINVAL;
  if (prefill_phases) *prefill_phases = c->st_fb_prefill;
  if (nar_phases) *nar_phases = c->st_fb_nar;
  if (lifetime) *lifetime = c->fb_total;
  return VX_OK;
}

int vx_fallback_state(vx_ctx* c, int32_t* sticky_prefill, int32_t* sticky_nar, int64_t* times_engaged) {
  if (!c) return VX_EINVAL;
  if (sticky_prefill) *sticky_prefill = c->sticky_prefill_f32;
  if (sticky_nar) *sticky_nar = c->sticky_nar_f32;
  if (times_engaged) *times_engaged = c->sticky_engaged;
  return VX_OK;
}

int vx_fallback_reset(vx_ctx* c) {
  if (!c) return VX_EINVAL;
  c->fb_prefill_raises = c->fb_nar_raises = 0;
  c->sticky_prefill_f32 = c->sticky_nar_f32 = false;
  c->sticky_prefill_age = c->sticky_nar_age = 0;
  return VX_OK;
}

int vx_arith_mode(vx_ctx* c, int32_t* gemm_mode, int32_t* attn_mode) {
  if (!c) return VX_EINVAL;
  if (!c->finalized) FAIL(VX_ESTATE, "weights not finalized");
  if (gemm_mode) *gemm_mode = c->gemm_mode;
  if (attn_mode) *attn_mode = !c->attn_x3 ? 2 : (c->attn_h2 ? 0 : 1);
  return VX_OK;
}

int vx_last_truncated(vx_ctx* c, int32_t* rows) {
  if (!c || !rows) return VX_EINVAL;
  *rows = c->st_truncated;
  return VX_OK;
}

int vx_last_stats(vx_ctx* c, int64_t* ar_steps, int64_t* frames, double* ar_ms, double* nar_ms) {
  if (!c) return VX_EINVAL;
  if (ar_steps) *ar_steps = c->st_steps;
  if (frames) *frames = c->st_frames;
  if (ar_ms) *ar_ms = c->st_ar_ms;
  if (nar_ms) *nar_ms = c->st_nar_ms;
  return VX_OK;
}

}  // extern "C"
