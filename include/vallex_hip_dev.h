/* vallex_hip_dev.h -- measurement and kernel-development entries of libvallex_hip.so.
 *
 * NOT part of the drop-in boundary (include/vallex_hip.h): nothing here has a counterpart in the reference and the Python
 * mirrors of utils/generation.py / models/vallex.py never call these.  bench.py (roofline leg), tools/ and a few GPU tests do.
 * Kept in the same library so that the kernels that are timed are the kernels that ship.
 */
#ifndef VALLEX_HIP_DEV_H
#define VALLEX_HIP_DEV_H

#include "vallex_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- per-class event timing --------------------------------------------------------------------------------
 * HIP-event timing of kernel classes on the context's own stream (bench.py roofline leg).
 * which: 0 = dec_attn (KV streaming), 1 = skinny GEMMs, 2 = transformer projections (full-sequence GEMMs), 3 = full-seq
 * attention, 4 = the fp32 GEMMs of the Vocos / EnCodec heads, 5 = the LSTM recurrences of the EnCodec decoder (one event pair
 * per layer around its T dependent steps; `algo_bytes` of this class counts the steps).
 * vx_prof_enable(1) makes the AR step run un-graphed with an event pair around each launch of every class. */
int vx_prof_enable(vx_ctx* ctx, int32_t on);
int vx_prof_get(vx_ctx* ctx, int32_t which, double* total_ms, int64_t* launches, double* algo_bytes);
int vx_prof_reset(vx_ctx* ctx);
/* GPU-bound micro-replay of one decode kernel on the state the last AR run left behind: `reps` back-to-back launches
 * between ONE event pair (eager per-launch events pick up host launch gaps; events recorded inside a hipGraph cannot be
 * timed on ROCm 7.2).  which 0: dec_attn with every row at context prefill_len + gen_offset; which 1: the four
 * weight-streaming GEMMs of a layer.  avg_us = per launch; algo_bytes = algorithmic bytes per launch. */
int vx_bench_kernel(vx_ctx* ctx, int32_t which, int32_t reps, int32_t gen_offset, double* avg_us, double* algo_bytes);
/* kernel-development aid: time one full-sequence GEMM kernel (0 fp32 MFMA, 1 bf16x3) on scratch data and
 * report its max abs difference to the fp32-MFMA kernel.  Not used by the product path. */
int vx_bench_gemm(vx_ctx* ctx, int32_t M, int32_t N, int32_t K, int32_t kernel, int32_t reps, double* avg_us,
                  double* max_abs_diff);
int vx_bench_attn(vx_ctx* ctx, int32_t batch, int32_t len, int32_t causal, int32_t variant, int32_t reps, double* avg_us,
                  double* max_diff);
/* vx_bench_gemm + the shader clock the chip HOLDS while that kernel runs: a one-wave side kernel on a second stream counts
 * shader-clock ticks (s_memtime) over 2 ms of the constant 100 MHz counter (s_memrealtime) while the timed launches execute.
 * The MFMA peaks of the guide assume the 2.4 GHz boost clock; under the f16 matrix kernels this board holds less (power), and
 * bench.py reports the value measured in ITS run next to every MFMA-bound roofline fraction.  clock_mhz = 0 if the probe saw
 * no overlap (kernel too short). */
int vx_bench_gemm_clock(vx_ctx* ctx, int32_t M, int32_t N, int32_t K, int32_t kernel, int32_t reps, double* avg_us,
                        double* max_abs_diff, double* clock_mhz);

/* Epilogue cross-check of the two f16x2 GEMM kernels on the same operand planes (four waves of 128 x 128 against eight waves of
 * 64 x 128; bit-identical by construction): mode 0 = bias + ReLU + out_planes, 1 = bias + residual through resid_rows (ragged M),
 * 2 = bias + residual in place; mode + 10: the eight-wave template on 128 x 128 tiles instead of 256 x 256.  differing / compared =
 * 32-bit words of C (16-bit words of the planes in mode 0).  N % 256 == 0. */
int vx_bench_gemm_epilogue(vx_ctx* ctx, int32_t M, int32_t N, int32_t K, int32_t mode, int64_t* differing, int64_t* compared);

/* ---- correctness entries: product kernels on caller-chosen operands -------------------------------------------
 * Not timed.  Host pointers in and out, staged through the context's pinned ring, launched on the context's stream through the
 * product launchers.  Every output buffer is pre-filled with a sentinel, so the caller sees what a kernel did not write. */
#define VX_DEV_SENTINEL_I (-123456789)
#define VX_DEV_SENTINEL_F (-1.0e30f)
#define VX_DEV_SENTINEL_H 0xFBFF /* half-word fill of plane outputs (fp16 -65504); reported as VX_DEV_SENTINEL_F */
#define VX_DEV_SAMPLE_CFG 10
#define VX_DEV_SAMPLE_STATE 12
/* The decode sampler (kernel 0: dec_sample_kernel, 1: serve_sample_kernel) on n chosen cases; case i runs in decode row i % 32 of
 * launch i / 32, launch slot (7 row + 3) % 32.  Rows of a launch without a case are inactive.
 *   cfg   [n][10] = {kernel, splitk (1 | 2 | 4), top_k, force_eos_at, active, n_gen, cur_pos, ctx_len, text_len, gen_stride}
 *   fcfg  [n][3]  = {temperature, the draw u in [0, 1), incoming sum_logp}
 *   partial [n][4][1025]: the split-K addends of the logit row (the first `splitk` are read)
 * kernel, splitk and gen_stride are launch constants, and for kernel 0 so are top_k, temperature and force_eos_at: the cases of
 * one launch must agree on them (VX_EINVAL otherwise).
 *   logits [n][1025]: the reduced logits (kernel 0 writes them; kernel 1 leaves the sentinel)
 *   state  [n][12] = {active, n_gen, cur_tok, cur_pos, ctx_len, slot_meta[4 slot .. 4 slot + 3], gen[row][old n_gen], the launch's
 *                     n_active, slot}.  Before the launch cur_tok, gen and slot_meta word 3 hold the sentinel, slot_meta words 0 .. 2
 *                     = {row, ctx_len, active} and n_active = the number of active cases of the launch.
 *   sum_logp [n]; emb_h [n][1024]; emb_xp [n][1024] = the row's part of the packed-x image, un-packed.
 * The fused next-step embedding reads the context's finalized AR audio embedding, position alpha, positional table and norm1 of
 * layer 0. */
int vx_dev_sample(vx_ctx* ctx, int32_t n, const int32_t* cfg, const float* fcfg, const float* partial, float* logits, int32_t* state,
                  float* sum_logp, float* emb_h, float* emb_xp);
/* vx_dev_sample for kernel 1 only (cfg[i][0] must be 1), with the per-row filter record of the serving session's sampler:
 *   ffilt [n][2] = {top_p, repetition_penalty};  ifilt [n][2] = {repetition_window, min_frames}
 *   hist  [n][hist_stride] int32: the case's first min(n_gen, gen_stride) generated tokens, copied into its gen row before the
 *                                 launch (hist_stride >= that count for every case; hist may be NULL when all counts are 0)
 * Same sentinels and outputs (gen[row][old n_gen] is still reported from the slot the sample writes). */
int vx_dev_sample_filtered(vx_ctx* ctx, int32_t n, const int32_t* cfg, const float* fcfg, const float* ffilt, const int32_t* ifilt,
                           const int32_t* hist, int32_t hist_stride, const float* partial, float* logits, int32_t* state,
                           float* sum_logp, float* emb_h, float* emb_xp);
/* One launch of a full-sequence attention kernel: variant 0 fp32, 10 bf16x3, 20 f16x2; planes 1 (variants 10, 20): the output leaves
 * as the fp16 head / tail planes of out_proj, read back and returned as (head + tail) / 2^5.  qkv [sum seq_len][3072]; prefix_len
 * NULL: no mask; q_first (variant 0 with fp32 rows, variant 20 with planes) or NULL: only rows [q_first[b], seq_len[b]) of every
 * sequence are computed and stored compacted.  out [out_rows][1024], out_rows >= the rows stored (a few more rows show that
 * nothing is written behind them).  *range_flag = the f16x2 range flag after the launch (0 for the other variants). */
int vx_dev_attn(vx_ctx* ctx, int32_t variant, int32_t planes, int32_t batch, const float* qkv, const int32_t* seq_len,
                const int32_t* prefix_len, const int32_t* q_first, float* out, int64_t out_rows, int32_t* range_flag);
/* The kernel-selection fields a context read from its configuration and the environment when its weights were finalized, so that
 * a measurement or a test that sets a switch can show that the context took it.  out[0 .. 13], in this order:
 *    0 sb_fuse           VX_SB_FUSE (1; 0: no small-batch chain)       7 balance_rows  VX_BALANCE_ROWS (1)
 *    1 sb_qkv_rows       VX_SB_QKV (4: the fused QKV up to 4 rows)      8 nar_trim      VX_NAR_TRIM (1)
 *    2 sb_qkv_nsplit     VX_SB_QKV_NSPLIT (0: the rule's count)         9 graph_multi   VX_GRAPH_MULTI (1)
 *    3 qkv_bal           VX_QKV_BALANCED (1)                           10 gemm_mode     0 f16x2, 1 bf16x3 (VX_GEMM_X3), 2 fp32 (VX_GEMM_F32)
 *    4 fuse_out          VX_FUSE_OUT (1), 0 whenever Tmax < 128        11 attn_x3       0: exact-fp32 full-sequence attention (VX_ATTN_F32)
 *    5 fuse_split        VX_FUSE_SPLIT (1)                             12 attn_h2       0: bf16x3 full-sequence attention (VX_ATTN_X3)
 *    6 att_nsplit_force  VX_ATT_NSPLIT (0: the rule; at most 16)       13 Tmax          arena rows per (slot, head)
 * VX_EINVAL for a null out or n < 14 (VX_DEV_SWITCHES), VX_ESTATE before vx_finalize_weights. */
#define VX_DEV_SWITCHES 14
int vx_dev_switches(vx_ctx* ctx, int32_t* out, int32_t n);
/* The switches of the decode step's weight-streaming GEMMs (round 35), read like the fields above and reported apart from them
 * (the word count of vx_dev_switches is fixed).  Both choose WHERE a workgroup runs or in which order it requests its operands,
 * never what it computes: every output word is the same under either value.  out[0 .. 1]:
 *    0 l2_kmap        VX_L2_KMAP (1: linear2 of the 5 .. 32-row chain cuts its block id with the K slice fastest, one slice per XCD)
 *    1 l1_interleave  VX_L1_INTERLEAVE (1: linear1 requests w, x0, x1 per k-block; 0: all of x, then the weights)
 * VX_EINVAL for a null out or n < 2 (VX_DEV_GEMM_LEVERS), VX_ESTATE before vx_finalize_weights. */
#define VX_DEV_GEMM_LEVERS 2
int vx_dev_gemm_levers(vx_ctx* ctx, int32_t* out, int32_t n);
/* The attention block of ONE decode step on nrows (1 .. 32) chosen rows: the launches of the engine's step from the attention launch
 * to the launch behind which the out_proj result exists, with the chain and the context splits the engine's own rule picks for nrows
 * rows under the context's switches (reported in geom[4] = {nsplit, sb_qkv, split_fused, sb_chain}).  With the default switches:
 *   1 .. 4 rows        dec_attn_qkv (norm1 + in_proj + split attention) | out_proj GEMM with the combine as prologue
 *   5 .. 7 rows        dec_attn | dec_attn_combine | out_proj GEMM | reduce + LayerNorm
 *   8 .. 16 rows       dec_attn with out_proj folded in, context splits | reduce (weighs the slabs by e^(m_s - M) / L) + LayerNorm
 *   17 .. 32 rows      dec_attn with out_proj folded in, one split | reduce + LayerNorm
 * and under a switch whatever decode_geometry (engine.hip) makes of it, at any row count: the unfused chain with 1 .. 16 splits (one
 * split: no combine launch, no (m, l)), the split-fused one with 2 .. 4, the fused one, and
 *   1 .. 4 rows, sb_chain without sb_qkv (VX_SB_QKV below the row count, or a VX_SB_QKV_NSPLIT that is not instantiated):
 *                      dec_attn (unfused, 16 | 8 splits) | out_proj GEMM with the combine as prologue
 * A combination a launcher does not instantiate is VX_EINVAL ("a launcher refused this configuration"), nothing launched.
 * The weights are the context's layer 0 (in_proj, out_proj, norm1, norm2, and linear2's bias for skp 8); everything else is private
 * scratch of the call, pre-filled with the sentinel -- the K / V arena too, which has nrows slots of [16][Tmax][64] for a Tmax of the
 * caller's (128 .. 4096).  The context's decode state is not touched.
 *   ctx_len [nrows]: cached rows INCLUDING the new token (1 .. Tmax);  active [nrows]: 0 = a finished row
 *   slot_order [nrows]: slot_order[y] = the row in launch slot y, a permutation (the identity for nrows <= 4)
 *   kc, vc [nrows][16][Tmax][64], in and out, indexed by ROW (the entry moves row r's stream into its slot and back): the cached rows
 *       0 .. ctx - 2 and whatever the caller wants a reused slot to hold behind them; out: the whole stream after the launch
 *   qkv (the dec_attn chains, sb_chain without sb_qkv included): the in_proj split-K slabs [4][nrows][3072], or for qkv_balanced != 0
 *       [8][nrows][3072] with q in all eight and k, v in the first four (columns 1024 .. 3071 of slabs 4 .. 7 are not read); sb_chain
 *       without sb_qkv reads four slabs only, as the engine's QKV GEMM of that chain writes them: qkv_balanced != 0 is VX_EINVAL there
 *   x_in (the sb_qkv chain): skp 0: [nrows][1024], norm1(h) as the sampler leaves it (packed by the entry); skp 8: [9][nrows][1024],
 *       eight linear2 slabs and the residual row: x = norm1(resid + sum of the slabs + linear2 bias)
 *   resid [nrows][1024] (the dec_attn chains; sb_chain without sb_qkv does not read it and takes NULL): the residual rows the closing
 *       reduce + LayerNorm adds
 *   out [4][nrows][1024]: sb_chain, with or without sb_qkv: the four split-K slabs of out_proj (bias not added); the other chains: out[0] = h =
 *       resid + out_proj(attention) (every row: the reduce kernels do not look at the active flag), out[1 .. 3] keep the sentinel
 *   xp_att [nrows][1024]: the attention output in front of out_proj where a chain stores it (the unfused chain), un-packed
 *   part_ml [nrows][16][17][2]: (m, l) of partial s < nsplit of every (row, head) where the chain has context splits (nsplit >= 2, or
 *       sb_chain); the sb_qkv chain's partial `nsplit` (the new token's) has no (m, l): the consumer forms it
 * VX_ESTATE while a serving session is open; VX_EINVAL for Tmax < 128, a context beyond Tmax, a slot order that is no permutation. */
int vx_dev_dec_attn(vx_ctx* ctx, int32_t nrows, int32_t Tmax, int32_t qkv_balanced, int32_t skp, const int32_t* ctx_len,
                    const int32_t* active, const int32_t* slot_order, float* kc, float* vc, const float* qkv, const float* x_in,
                    const float* resid, float* out, float* xp_att, float* part_ml, int32_t* geom);
/* ONE launch of the rest of the decode step -- the skinny GEMMs, linear1, reduce + LayerNorm, their small-batch consumers, the
 * teacher-forced embedding -- through the product launcher on nrows (1 .. 32) chosen rows.  The weights are the context's own device
 * images of `layer` (in_wp, out_wp, l1_wp, l2_wp, pred_wp as the load-time pack kernels wrote them, the biases and the norms), the
 * split counts the engine's (4 K slices for in_proj, out_proj and predict, 8 for linear2 and the q columns of the balanced in_proj,
 * predict padded to 1056 columns), write-through result stores of the general GEMM on when nrows > 4 as in the engine.  Everything
 * else the launch reads or writes is private scratch pre-filled with VX_DEV_SENTINEL_F; the context's decode state is not touched.
 * Activation operands travel un-packed as the whole 32-row image [32][K] row-major (the entry packs and un-packs), so the caller
 * decides what rows nrows .. 31 hold; slabs travel as [slices][32][N] with all 32 rows.  Arguments an op does not use may be NULL.
 *   op                      variant                       reads                              writes
 *   EMBED (norm1, layer 0)  0                             tok, pos [nrows]                   h [nrows][1024], xp [32][1024]
 *   GEMM                    weight VX_DEV_W_*             x [32][K] (K 4096 for linear2)     out [4 | 8][32][3072 | 1024 | 1056]
 *   QKV_BAL                 0                             x [32][1024]                       out [8][32][3072] (k, v columns: slabs 0 .. 3)
 *   LINEAR1                 0                             x [32][1024]                       out [32][4096] = relu(x W1^T + b1), the image
 *   REDUCE_LN               slabs 0 | 4 | 8 | 16          slabs [variant][32][1024], resid   h, xp; resid = the buffer behind the launch
 *   SB_LN_GEMM (<= 4 rows)  VX_DEV_W_IN | VX_DEV_W_PRED   slabs [8][32][1024], resid         out (as GEMM), h, resid
 *   SB_LINEAR1 (<= 4 rows)  0                             slabs [4][32][1024], resid         out (as LINEAR1), h, resid
 * REDUCE_LN: h = resid + (sum of the slabs + bias), xp = LayerNorm(h); 4 and 16 slabs: out_proj's bias and norm2 of `layer`; 8:
 * linear2's bias of `layer` and norm1 of layer + 1, the final norm behind the last layer; 0: the final norm of resid alone, no bias,
 * and the kernel is handed no h (h returns the sentinel).  With slabs it works in place as in the engine: resid returns h.
 * SB_LN_GEMM: the GEMM whose prologue is REDUCE_LN 8 -- in_proj of `layer` >= 1 behind linear2 of layer - 1, or predict behind the
 * last layer; SB_LINEAR1: linear1 whose prologue is REDUCE_LN 4.  Both write h into the other buffer of the engine's dh / dh2 pair:
 * resid returns unchanged.  (The engine hands predict no h; the entry does.)
 * VX_EINVAL, nothing launched: an unknown op or variant, nrows outside 1 .. 32 (1 .. 4 for the small-batch ops), a layer the context
 * does not have, in_proj through SB_LN_GEMM at layer 0 or predict anywhere but behind the last layer, a tok outside the embedding
 * table or a pos outside the positional table.  VX_ESTATE while a serving session is open. */
#define VX_DEV_OP_EMBED 0
#define VX_DEV_OP_GEMM 1
#define VX_DEV_OP_QKV_BAL 2
#define VX_DEV_OP_LINEAR1 3
#define VX_DEV_OP_REDUCE_LN 4
#define VX_DEV_OP_SB_LN_GEMM 5
#define VX_DEV_OP_SB_LINEAR1 6
#define VX_DEV_W_IN 0
#define VX_DEV_W_OUT 1
#define VX_DEV_W_L2 2
#define VX_DEV_W_PRED 3
int vx_dev_dec_op(vx_ctx* ctx, int32_t op, int32_t variant, int32_t layer, int32_t nrows, const int32_t* tok, const int32_t* pos,
                  const float* x, const float* slabs, float* resid, float* out, float* h, float* xp);

/* ONE full-sequence GEMM through a product launcher on caller operands:
 *   C[m][n] = resid[rr(m)][n] + colscale[n] * act(sum_k A[ga(m)][k] W[n][k] + bias[n]),  m < M, n < N
 * with ga(m) = gather ? gather[m] : m and rr(m) = resid_rows ? resid_rows[m] : m.  M, N, K <= 4096; N % 4 == 0, K % 32 == 0.
 *   kernel   0 .. 4     launch_gemm_f32, variant `kernel` (0: the product's choice)
 *            10 .. 15   launch_gemm_f16x2 with tn = 0 (the product's choice), 128, 256, 257, -128, -129
 *            20, 21     launch_gemm_bf16x3, launch_gemm_bf16x3_dma: plain epilogue only (no gather, bias, resid, colscale, act)
 *   A [rowsA][lda] (lda >= K, lda % 4 == 0; rowsA >= M without gather); bias, colscale [N]; resid [rowsR][ldr] (ldr >= N, ldr % 4 == 0;
 *   rowsR >= M without resid_rows); gather, resid_rows [M].  act: 0 none, 1 ReLU, 2 GELU, 3 ELU.  colscale, GELU and ELU: kernels 0 .. 4.
 * f16x2: A is split by launch_split2h at the activation scale 2^5 (the gather applied there, as the engine does) into planes whose
 * pad rows behind M hold VX_DEV_SENTINEL_H (finite garbage the kernels must keep out of every stored element); W [N][K] is split at
 * 2^w_shift (0 .. 24), or for w_shift = -1 at the shift the loader's rule derives from max |w| (absmax kernel + h2_weight_shift);
 * descale = 2^-(5 + shift).  w_src != 0 (W must be NULL): the context's own load-time planes of layer w_layer with their recorded shift,
 * w_src 1 .. 4 = in_w3, out_w3, l1_w3, l2_w3 of the AR stack, 5 .. 8 of the NAR stack (N and K must be the weight's).
 *   flags & VX_DEV_GEMM_OUT_PLANES (f16x2, N % 256 == 0): the launch writes out_planes instead of fp32 rows; C may be NULL
 *   flags & VX_DEV_GEMM_INPLACE (ldr == N, no resid_rows): the launch runs with C == resid
 *   C [rowsC][N], M <= rowsC <= M + 64: rows the launch did not write hold VX_DEV_SENTINEL_F
 *   planes [2][roundup(M, 256)][N] (OUT_PLANES), a_planes [2][roundup(M, 256)][K] (f16x2, optional): head and tail plane, un-tiled, as
 *       fp16 bit patterns; words the launch did not write hold VX_DEV_SENTINEL_H
 *   info [3] = {the f16x2 range flag behind the launches, the weight shift used (-1: not f16x2), 0}
 * VX_EINVAL, nothing launched, for anything outside the above; VX_ESTATE while a serving session is open or when w_src asks for planes
 * the context does not hold. */
#define VX_DEV_GEMM_OUT_PLANES 1
#define VX_DEV_GEMM_INPLACE 2
int vx_dev_gemm(vx_ctx* ctx, int32_t kernel, int32_t flags, int32_t M, int32_t N, int32_t K, const float* A, int32_t rowsA, int32_t lda,
                const int32_t* gather, const float* W, int32_t w_src, int32_t w_layer, int32_t w_shift, const float* bias,
                const float* resid, int32_t rowsR, int32_t ldr, const int32_t* resid_rows, const float* colscale, int32_t act, float* C,
                int32_t rowsC, uint16_t* planes, uint16_t* a_planes, int32_t* info);
/* ONE launch_layernorm on caller rows: y = (LN(x) * g + b) * ada_w + ada_b with eps 1e-5; C = 1024 or 384; rows 1 .. 4096.
 *   x [rows][ldx] (ldx >= C, ldx % 4 == 0, ldx <= 8192); g, b [C] both or neither; ada_w, ada_b [C] both or neither
 *   y [rowsY][C], rows <= rowsY <= rows + 64, or NULL (C = 1024 with planes only): rows the launch did not write hold VX_DEV_SENTINEL_F
 *   planes [2][roundup(rows, 256)][1024] or NULL (C = 1024 only): the f16x2 planes the launch writes next to / instead of y, un-tiled
 *       fp16 bit patterns; words not written hold VX_DEV_SENTINEL_H.  *range_flag = the f16x2 range flag behind the launch.
 * VX_EINVAL, nothing launched, for anything outside the above; VX_ESTATE while a serving session is open. */
int vx_dev_layernorm(vx_ctx* ctx, int32_t rows, int32_t C, int32_t ldx, const float* x, const float* g, const float* b, const float* ada_w,
                     const float* ada_b, float* y, int32_t rowsY, uint16_t* planes, int32_t* range_flag);
/* ONE launch of score_rows_kernel (csrc/score.hip, the kernel behind vx_score) on caller rows:
 *   m = max_j l_j, s = sum_j expf(l_j - m), logp = (l_t - m) - logf(s), rank = #{j : l_j > l_t} over the columns j < ncols of row r,
 *   t = targets[r].  logits [rows][ld], ncols 1024 or 1025, ld >= ncols, ld % 4 == 0, ld <= 8192 (columns ncols .. ld-1 are padding
 *   and influence nothing); rows 1 .. 4096; targets [rows] in 0 .. ncols-1.
 *   logp, rank [rows_out], rows <= rows_out <= rows + 64: entries the launch did not write hold VX_DEV_SENTINEL_F / VX_DEV_SENTINEL_I.
 * VX_EINVAL, nothing launched, for anything outside the above; VX_ESTATE while a serving session is open. */
int vx_dev_score_rows(vx_ctx* ctx, int32_t rows, int32_t ncols, int32_t ld, const float* logits, const int32_t* targets,
                      float* logp, int32_t* rank, int32_t rows_out);
/* ONE launch of align_rows_kernel (csrc/align.hip, the kernel behind vx_align) on caller rows of one layer:
 *   out[out_off + t][s] += sum_h w[h] * softmax_j(0.125 * q_r,h . k_j,h)[s]  for t < n_rows, s < S, r = q_first + t, over the keys
 *   j = 0 .. r of the sequence (all text, causal audio: r >= S).  qkv [M][3072], packed rows: q in columns 0 .. 1023, k in
 *   1024 .. 2047, head h at h * 64; M 1 .. 8192.  tab [nseq][6] = {seq_off, seq_len, S, q_first, n_rows, out_off} per sequence,
 *   nseq 1 .. 32: the sequence inside [0, M), S >= 1, q_first >= S, n_rows >= 0, q_first + n_rows <= seq_len, the output rows
 *   [out_off, out_off + n_rows) inside [0, rows_out) and disjoint between sequences.  w [16] finite and >= 0; a head with
 *   w[h] == 0 is skipped (never read).  out [rows_out][ld_out] is IN / OUT, ld_out >= every S: the caller's contents go in, the
 *   reported elements come back increased, every other element as it was.  The kernel works on tiles of VX_DEV_ALIGN_ROW_TILE
 *   reported rows and VX_DEV_ALIGN_KEY_TILE keys.
 * VX_EINVAL, nothing launched, the message naming the field, for anything outside the above; VX_ESTATE while a serving session is
 * open. */
#define VX_DEV_ALIGN_ROW_TILE 32
#define VX_DEV_ALIGN_KEY_TILE 32
int vx_dev_align_rows(vx_ctx* ctx, int32_t M, int32_t nseq, const int32_t* tab, const float* qkv, const float* w, float* out,
                      int32_t rows_out, int32_t ld_out);

/* ONE launch of a glue kernel of the waveform half -- the Vocos head (csrc/vocos.hip) and the EnCodec decoder / encoder
 * (csrc/encodec.hip) -- through its product launcher on caller operands.  Everything the launch reads or writes is private scratch of
 * the call (the context's arenas are not touched); the only context state read is the window table of OVERLAP_ADD and what TABLES
 * returns.  Every output is pre-filled with VX_DEV_SENTINEL_F (codes: VX_DEV_SENTINEL_L), and holds `extra` (0 .. 64) more rows or
 * samples than the launch may write, so the caller sees both what was not written and that nothing was written behind the end.
 * dims is an int32 array whose meaning depends on op; arguments an op does not name may be NULL.  "rows" are 1 .. 4096.
 *
 *   CODEBOOK_SUM   dims {rows, extra}; ia = codes [rows][8], each 0 .. 1023; a = codebook [8192][128]
 *                  out = feat [rows + extra][128]: feat[r] = sum_q codebook[1024 q + codes[r][q]], fp32 adds in ascending q
 *   IM2COL7        dims {rows, extra}; a = x [rows][128]; ia = row_t, ib = row_len [rows]: row r is frame row_t[r] of a packed sequence of
 *                  row_len[r] frames (0 <= row_t < row_len, and the whole sequence lies inside the rows)
 *                  out [rows + extra][896]: out[r][128 tap + c] = x[r + tap - 3][c] inside the row's own sequence, 0 outside
 *   DWCONV7        dims {rows, extra, C}, C 384 | 512; a = x [rows][C], w [C][7], bias [C]; ia, ib as IM2COL7
 *                  out [rows + extra][C]: out[r][c] = bias[c] + sum_tap w[c][tap] x[r + tap - 3][c]
 *   ISTFT_PREP     dims {rows, extra}; a = o [rows][1408] (log-magnitudes 0 .. 640, phases 641 .. 1281, padding behind)
 *                  out = reim [rows + extra][1312]: min(expf(o[k]), 100) * (cosf(p), sinf(p)) at k and 641 + k, columns 1282 .. 1311 zero
 *   OVERLAP_ADD    dims {batch, extra, frames, audio_stride}; a = windowed frames [frames][1280]; ia = seq_off, ib = seq_len [batch]
 *                  (batch 1 .. 32; every sequence inside the frames); the hann^2 table is THE CONTEXT'S (Vocos weights loaded)
 *                  out = audio [batch x audio_stride + extra], or for audio_stride 0 (the product's: packed like the frames)
 *                  [320 frames + extra]: sample s of sequence b = (sum_f frames[f][s + 480 - 320 f]) / (sum_f win2[s + 480 - 320 f])
 *   IM2COL_SEQ     dims {batch, extra, frames, C, k, mode, elu, R}; a = x [frames R][C]; ia, ib as OVERLAP_ADD, in frames of R rows each
 *                  C 4 .. 512 with C % 4 == 0; mode 0 (causal Conv1d, reflect into the zero-extended input) with k 1 .. 7, mode 1
 *                  (ConvTranspose1d) with k = 2; elu 0 | 1; R 1 .. 320
 *                  out [frames R + extra][k C]
 *   LSTM_CELL      dims {batch, splitk, frames, t, extra}; splitk 1 | 2; a = part [2][32][2048] (slab 1 is not read for splitk 1);
 *                  b = xg [frames][2048]; w = skip [frames][512] or NULL; ia, ib as OVERLAP_ADD
 *                  out = cstate [32][512] and out2 = h [32][512], both in and out (h travels un-packed: the entry packs it into the
 *                  packed-x image of the recurrence GEMM and un-packs it again, so the caller decides what untouched sequences hold);
 *                  out3 = y [frames + extra][512].  Sequences with t >= seq_len[b] are finished: nothing of theirs is written.
 *   FINAL_CONV     dims {batch, extra, frames, R, audio_stride}; a = x [frames R][32], w [32][7], bias [1]; ia, ib as IM2COL_SEQ;
 *                  audio_stride >= R x the longest sequence;  out = audio [batch x audio_stride + extra]
 *   ENC_FIRST_CONV dims {L, extra}, L 1 .. 65536; a = wav [L], w [32][7], bias [32];  out [L + extra][32]
 *   ENC_PAD_ELU    dims {Lc, out_rows, C, r}, Lc 1 .. 65536, C as IM2COL_SEQ, r 1 .. 16; a = x [Lc][C]
 *                  out [out_rows][C], rows <= out_rows <= rows + 64; geom = {rows, Le, n_out}: the geometry comes from the host rule the
 *                  encoder itself uses (enc_pad_geom), so the rule is under test with the kernel
 *   RVQ_SELECT     dims {rows, extra, q}, q 0 .. 7; a = resid [rows][128], b = scores [rows][1024], w = e2 [1024], bias = codebook [1024][128]
 *                  out = resid - codebook[code] [rows + extra][128]; codes [rows + extra][8] int64: only column q is written.  The code is
 *                  the lowest index of the largest -((|r|^2 - 2 score) + e2) and always lies in 0 .. 1023: a row without any comparable
 *                  distance (all NaN) gets code 0.
 *   TABLES         no launch: reads back the tables built at load time.  out = vc_dft [1280][1312], out2 = vc_win2 [1280] (Vocos weights),
 *                  out3 = en_e2 [8][1024] (EnCodec encoder weights); a NULL table is skipped; VX_ESTATE if an asked one is not loaded.
 * VX_EINVAL, nothing launched and no output touched, for anything outside the above (an unknown op, rows or sizes outside their range,
 * a sequence that leaves its operand, a code outside 0 .. 1023, q outside 0 .. 7, an operand of more than 2^24 elements);
 * VX_ESTATE while a serving session is open. */
#define VX_DEV_SENTINEL_L (-1234567890123456789LL)
#define VX_DEV_WAVE_CODEBOOK_SUM 0
#define VX_DEV_WAVE_IM2COL7 1
#define VX_DEV_WAVE_DWCONV7 2
#define VX_DEV_WAVE_ISTFT_PREP 3
#define VX_DEV_WAVE_OVERLAP_ADD 4
#define VX_DEV_WAVE_IM2COL_SEQ 5
#define VX_DEV_WAVE_LSTM_CELL 6
#define VX_DEV_WAVE_FINAL_CONV 7
#define VX_DEV_WAVE_ENC_FIRST_CONV 8
#define VX_DEV_WAVE_ENC_PAD_ELU 9
#define VX_DEV_WAVE_RVQ_SELECT 10
#define VX_DEV_WAVE_TABLES 11
int vx_dev_wave_op(vx_ctx* ctx, int32_t op, const int32_t* dims, const float* a, const float* b, const float* w, const float* bias,
                   const int32_t* ia, const int32_t* ib, float* out, float* out2, float* out3, int64_t* codes, int32_t* geom);

/* ONE launch of a kernel of the seams between the phases -- the embedding gathers, the NAR arg-max, the prefill -> decode K / V
 * hand-over and the AdaLN GEMV (csrc/rows.hip), the best_of fan-out (csrc/beams.hip), the admission kernels of the continuous
 * schedule and the serving session (csrc/admit.hip, csrc/serve.hip), teacher forcing (csrc/decode.hip) -- through its product
 * launcher on caller operands.  Everything the launch reads or writes is private scratch of the call: the context's arenas, decode
 * state and KV cache are not touched, and the only context state read is what TABLES returns.  Every float output is pre-filled with
 * VX_DEV_SENTINEL_F and every int output with VX_DEV_SENTINEL_I, and holds `extra` (0 .. 64) more rows or words than the launch may
 * write; an IN / OUT operand carries the caller's contents in front of that sentinel tail.  Every index the kernel will form is
 * checked on the host first.  dims is an int32 array whose meaning depends on op; arguments an op does not name may be NULL.  Rows
 * are 1024 floats; "rows" counts are 1 .. 4096 unless stated.
 *
 *   EMBED_ROWS     dims {rows, extra, out_rows, rowsA, rowsB, pe_rows}; fa = tabA [rowsA][1024], fb = tabB [rowsB][1024] or NULL, fc =
 *                  alpha [1], fd = pe [pe_rows][1024]; ia = idA [rows], ib = idB [rows] (-1: no add; NULL with tabB NULL and rowsB 0),
 *                  ic = pos [rows], id = dst [rows] or NULL (the identity; then out_rows >= rows)
 *                  out [out_rows + extra][1024]: out[dst[r]] = (tabA[idA[r]] + tabB[idB[r]]) + (alpha * pe[pos[r]]), every operation
 *                  rounded to fp32 on its own (no fused multiply-add)
 *   NAR_YEMB_INIT  dims {rows, extra, tab_rows}, tab_rows 1 .. 1024; fa = the 8 tables [8][tab_rows][1024] (the entry builds the device
 *                  array of the 8 pointers); ia = codes [rows][8], all 8 inside the tables; ib = nj [rows], 1 .. 8
 *                  out [rows + extra][1024]: out[r] = tab_0[codes[r][0]] + tab_1[codes[r][1]] + ... over j < nj[r], ascending
 *   ADD_PE_SCATTER dims {rows, extra, out_rows, pe_rows}; fa = yemb [rows][1024], fc = alpha, fd = pe, ic = pos, id = dst (required)
 *                  out [out_rows + extra][1024]: out[dst[r]] = yemb[r] + (alpha * pe[pos[r]])
 *   EMBED_ACCUM    dims {n, extra, yrows, tab_rows}; fa = tab [tab_rows][1024]; ia = tok [n]; id = rowidx [n]
 *                  out = yemb [yrows + extra][1024], IN / OUT: yemb[rowidx[i]] += tab[tok[i]]
 *   ARGMAX_ROWS    dims {rows, extra, N, ldx}, 1 <= N <= ldx <= 8192; fa = x [rows][ldx]; iout = idx [rows + extra]: the lowest index
 *                  of the largest of x[r][0 .. N-1] under `>` (so -0.0 and +0.0 tie and NaN is never chosen); a row without any
 *                  value above -inf (all NaN, all -inf) gets 0
 *   KV_SCATTER     dims {M, extra, Tmax, slots}, slots 1 .. 32; fa = qkv [M][3072]; ia = row_b [M] (slot), ib = row_t [M]
 *                  out = kc, out2 = vc [slots][16][Tmax][64] + 64 extra floats: kc[row_b][h][row_t] = qkv[r][1024 + 64 h ..], vc from 2048
 *   GEMV           dims {N, extra, K}, K % 4 == 0; fa = W [N][K], fb = e [K], fc = bias [N] or NULL; out [N + extra] = W e + bias
 *   BEAM_FANOUT    dims {layers, extra, Tmax, slots, npairs, nrows, hrows}; layers 1 .. 64, slots 1 .. 32, npairs, nrows 0 .. 32 (not both
 *                  0); ia = pairs [npairs][3] = {source slot, destination slot, cached rows 0 .. Tmax}; ib = hsrc_row [nrows];
 *                  fa = hsrc [hrows][1024]; out = kc, out2 = vc [layers][slots][16][Tmax][64] + 64 extra floats, IN / OUT (may be NULL
 *                  without pairs); out3 = dh [nrows + extra][1024]: dh[d] = hsrc[hsrc_row[d]]
 *   ADMIT_ROWS     dims {n, extra, gen_stride, hrows}; ia = tab [n][5] (launch_admit_rows, csrc/engine_ctx.h); fa = hsrc [hrows][1024];
 *                  out3 = hres [32 + extra][1024], IN / OUT; iout = the state block
 *   ADMIT_MASK     dims {nrows, extra, gen_stride, phase}, nrows 1 .. 32, phase 0 | 1; ia = admitted [nrows]; iout = the state block
 *   ADMIT_UNIFORMS dims {n, extra, steps, ncols, usteps, seed low word, seed high word}; ncols 1 .. 32, 1 <= steps <= usteps;
 *                  ia = pairs [n][2] = {column d, caller row r}; fa = staged [n][steps] or NULL (the counter-based draws of `seed`);
 *                  out = u [usteps][ncols] + extra floats, IN / OUT
 *   SERVE_UNIFORMS dims {n, extra, gen_stride, ncols, usteps, nstaged}; ia = tab [n][13] (launch_serve_uniforms, csrc/engine_ctx.h:
 *                  draws 0 .. usteps, staged offsets inside `staged`); fa = staged [nstaged] or NULL; out = u as ADMIT_UNIFORMS;
 *                  out2 = sum_logp [32 + extra], IN / OUT; iout = the state block (row_smp, row_flt)
 *   SERVE_CANCEL   dims {nrows, extra, gen_stride, row mask (the 32 bits of the word)}; iout = the state block
 *   FORCE_TOKEN    dims {batch, extra, gen_stride}; ia = tok [batch]; iout = the state block (n_gen >= 0)
 *   TABLES         no launch: out = the positional table [pe_rows][1024], out2 = the AdaLN table [7][2 NL + 1][2048] as the context holds
 *                  them, iout = {pe_rows, NL, 2 NL + 1}; a NULL one is skipped
 * The state block (IN / OUT, int32): every array a state kernel may read or write, at the word offsets VX_DEV_SEAM_ST_* -- 32 words each
 * of cur_tok, cur_pos, ctx_len, n_gen, text_len, active, saved, slot_of (a permutation of 0 .. 31), then slot_meta [32][4], n_active
 * (1 word + 3 of padding), row_smp [32][4], row_flt [32][4], and from VX_DEV_SEAM_ST_GEN gen [32][gen_stride] (gen_stride 1 .. 4096)
 * and the `extra` sentinel words.
 * VX_EINVAL, nothing launched and no output touched: anything outside the above -- an id outside its table, a dst / pos / slot / row
 * index outside its operand, a duplicate in dst, rowidx, (row_b, row_t), the decode rows or columns of an admission table or the
 * destinations of the fan-out pairs (two workgroups would write one row), a fan-out source that is also a destination, an operand of
 * more than 2^24 elements.  VX_ESTATE while a serving session is open or before the weights are finalized. */
#define VX_DEV_SEAM_EMBED_ROWS 0
#define VX_DEV_SEAM_NAR_YEMB_INIT 1
#define VX_DEV_SEAM_ADD_PE_SCATTER 2
#define VX_DEV_SEAM_EMBED_ACCUM 3
#define VX_DEV_SEAM_ARGMAX_ROWS 4
#define VX_DEV_SEAM_KV_SCATTER 5
#define VX_DEV_SEAM_GEMV 6
#define VX_DEV_SEAM_BEAM_FANOUT 7
#define VX_DEV_SEAM_ADMIT_ROWS 8
#define VX_DEV_SEAM_ADMIT_MASK 9
#define VX_DEV_SEAM_ADMIT_UNIFORMS 10
#define VX_DEV_SEAM_SERVE_UNIFORMS 11
#define VX_DEV_SEAM_SERVE_CANCEL 12
#define VX_DEV_SEAM_FORCE_TOKEN 13
#define VX_DEV_SEAM_TABLES 14
#define VX_DEV_SEAM_ST_CUR_TOK 0
#define VX_DEV_SEAM_ST_CUR_POS 32
#define VX_DEV_SEAM_ST_CTX_LEN 64
#define VX_DEV_SEAM_ST_N_GEN 96
#define VX_DEV_SEAM_ST_TEXT_LEN 128
#define VX_DEV_SEAM_ST_ACTIVE 160
#define VX_DEV_SEAM_ST_SAVED 192
#define VX_DEV_SEAM_ST_SLOT_OF 224
#define VX_DEV_SEAM_ST_SLOT_META 256
#define VX_DEV_SEAM_ST_N_ACTIVE 384
#define VX_DEV_SEAM_ST_ROW_SMP 388
#define VX_DEV_SEAM_ST_ROW_FLT 516
#define VX_DEV_SEAM_ST_GEN 644
int vx_dev_seam_op(vx_ctx* ctx, int32_t op, const int32_t* dims, const float* fa, const float* fb, const float* fc, const float* fd,
                   const int32_t* ia, const int32_t* ib, const int32_t* ic, const int32_t* id, float* out, float* out2, float* out3,
                   int32_t* iout);

/* The resampler's tap table (csrc/resample.hip, the kernel behind vx_resample), as the device holds it: geom = {o, n, width, K} of
 * the pair, taps [n][K] = phase kernel p at taps + p K (NULL: the geometry alone, nothing is built).  The table is built and
 * uploaded at the pair's first use and read back FROM THE DEVICE here, so the words a test sees are the words the kernel reads.
 * VX_EINVAL: a rate <= 0, geom NULL, or more than 2^18 taps. */
int vx_dev_resample_taps(vx_ctx* ctx, int32_t orig_rate, int32_t new_rate, float* taps, int32_t* geom);
/* Input samples one launch of vx_resample holds, for later calls on this context: VX_DEV_RESAMPLE_WINDOW_MIN .. VX_RESAMPLE_WINDOW,
 * or 0 for the default (VX_RESAMPLE_WINDOW).  A small window sends short rows through several windows and launches -- what the
 * window tests need; the device buffers keep their size.  While a window below a pair's K is set, vx_resample refuses that pair
 * (VX_EINVAL): a launch must hold one block's taps.  VX_EINVAL, nothing changed, for any other value. */
#define VX_DEV_RESAMPLE_WINDOW_MIN 512
int vx_dev_resample_window(vx_ctx* ctx, int32_t input_samples);

/* The frame table of ONE row as wave_frames_kernel (csrc/finish.hip, the measure pass of vx_finish) writes it: frame f covers samples
 * [f frame, min((f + 1) frame, len)); e[f] = one lane's sum in double of the squares of its samples (non-finite samples as 0) in
 * sample order, p[f] = max |y|, z[f] = its non-finite samples.  e, p, z hold ceil(len / frame) entries each; len = 0 writes nothing.
 * The row goes through the same planner and windows as vx_finish.  VX_EINVAL, nothing written: a NULL pointer, len < 0, frame
 * outside 16 .. 4096. */
int vx_dev_finish_frames(vx_ctx* ctx, const float* wav, int32_t len, int32_t frame, double* e, float* p, int32_t* z);
/* Input samples one launch of vx_finish holds, for later calls on this context: VX_DEV_FINISH_WINDOW_MIN .. VX_FINISH_WINDOW, or 0
 * for the default (VX_FINISH_WINDOW).  A small window sends short rows through several windows and launches of both passes -- what
 * the window tests need; the device buffers keep their size.  A launch always holds at least one frame: a call whose frame exceeds
 * the window runs with a window of one frame.  VX_EINVAL, nothing changed, for any other value. */
#define VX_DEV_FINISH_WINDOW_MIN 512
int vx_dev_finish_window(vx_ctx* ctx, int32_t input_samples);

/* Input samples one launch of vx_stretch holds, for later calls on this context: VX_DEV_STRETCH_WINDOW_MIN .. VX_STRETCH_WINDOW, or 0
 * for the default (VX_STRETCH_WINDOW).  A small window sends short rows through several windows and launches -- what the window tests
 * need; the device buffers keep their size.  One frame can read 2 search + 3 hop samples (its region and the template before it):
 * the minimum holds that at hop 441, search 300; while a window below one frame's span is set, vx_stretch refuses those options
 * (VX_EINVAL).  VX_EINVAL, nothing changed, for any other value. */
#define VX_DEV_STRETCH_WINDOW_MIN 2048
int vx_dev_stretch_window(vx_ctx* ctx, int32_t input_samples);
/* stretch_rows_kernel (csrc/stretch.hip, the kernel behind vx_stretch) on ONE row, through the same planner and windows: out
 * [ceil(len den / num)] and pos [M] as vx_stretch gives them, and cost [M] = the winning D_d of every frame as the kernel computed it,
 * in double (cost[0] = 0: frame 0 is not searched).  At speed 1 the search runs as well (no copy): pos[k] = k hop then holds by the
 * arithmetic, not by a shortcut.  VX_EINVAL, nothing written: a NULL pointer, len < 0, options out of range. */
int vx_dev_stretch_costs(vx_ctx* ctx, const float* wav, int32_t len, const vx_stretch_opts* o, float* out, int32_t* pos, double* cost);

/* Input samples one launch of vx_retime holds, for later calls on this context: VX_DEV_RETIME_WINDOW_MIN .. VX_RETIME_WINDOW, or 0 for
 * the default (VX_RETIME_WINDOW).  A small window puts the segments of one row into different launches -- what the window tests need;
 * the device buffers keep their size.  A walked segment is never cut: while a window below its span (la + 2 search + hop, cut to the
 * row) is set, vx_retime refuses that segment (VX_EINVAL).  VX_EINVAL, nothing changed, for any other value. */
#define VX_DEV_RETIME_WINDOW_MIN 2048
int vx_dev_retime_window(vx_ctx* ctx, int32_t input_samples);

/* The step table of ONE row as loudness_steps_kernel (csrc/loudness.hip, the steps pass of vx_loudness and vx_finish_loud) writes it:
 * z [ceil(n / S)], S = sample_rate / 10, z_j = the K-weighted energy of samples [j S, min((j + 1) S, n)) as include/vallex_hip.h
 * defines it.  The row goes through the same planner and windows as vx_loudness.  VX_EINVAL, nothing written: a NULL pointer, n < 0,
 * sample_rate outside 8000 .. 192000, a window (below) under 3 S. */
int vx_dev_loudness_steps(vx_ctx* ctx, const float* wav, int32_t n, int32_t sample_rate, double* z);
/* Samples one launch of the steps pass holds (warm-ups included), for later calls on this context: VX_DEV_LOUDNESS_WINDOW_MIN ..
 * VX_LOUDNESS_WINDOW, or 0 for the default (VX_LOUDNESS_WINDOW).  A small window sends short rows through several jobs and launches --
 * what the window tests need; the device buffers keep their size.  A launch must hold a warm-up and one step: while a window below
 * 3 S of a call's rate is set, that call is refused (VX_EINVAL), not run with a larger window.  With a window set, vx_finish_loud
 * uploads the kept spans again for the steps pass.  VX_EINVAL, nothing changed, for any other value. */
#define VX_DEV_LOUDNESS_WINDOW_MIN 4096
int vx_dev_loudness_window(vx_ctx* ctx, int32_t samples);

/* The detector readings and the gains of ONE row as limit_rows_kernel (csrc/limit.hip, the kernel behind vx_limit and
 * vx_finish_limited) writes them: P [len] and g [len] as include/vallex_hip.h defines them.  The row goes through the same planner and
 * windows as vx_limit.  VX_EINVAL, nothing written: a NULL pointer, len < 0, anything vx_limit refuses. */
int vx_dev_limit_gain(vx_ctx* ctx, const float* wav, int32_t len, float pre_gain, float ceiling_db, const vx_limit_opts* o, float* P,
                      float* g);
/* Samples one launch of the limiter holds (halos included), for later calls on this context: VX_DEV_LIMIT_WINDOW_MIN ..
 * VX_LIMIT_WINDOW, or 0 for the default (VX_LIMIT_WINDOW).  A small window sends short rows through several parts and launches -- what
 * the window tests need; the device buffers keep their size.  A window that cannot hold a part's two halos of 2 Wn + 7 samples plus
 * one sample is refused by the call (VX_EINVAL), not enlarged.  With a window set, vx_finish_limited brings the limited samples to the
 * host between the limiter and the apply pass.  VX_EINVAL, nothing changed, for any other value. */
#define VX_DEV_LIMIT_WINDOW_MIN 8192
int vx_dev_limit_window(vx_ctx* ctx, int32_t samples);

/* The difference and its normalisation of ONE row as f0_frames_kernel (csrc/f0.hip, the kernel behind vx_f0) computes them: d and dp
 * [M][lag_max + 1] doubles, M = ceil(len / hop), d[k][t] = d(t) and dp[k][t] = d'(t) of frame k as include/vallex_hip.h defines
 * them.  The row goes through the same planner and windows as vx_f0 (fewer frames per launch: the tables take their room).
 * VX_EINVAL, nothing written: a NULL pointer, len < 0, options out of range. */
int vx_dev_f0_table(vx_ctx* ctx, const float* wav, int32_t len, const vx_f0_opts* o, double* d, double* dp);
/* Samples one launch of vx_f0 holds, for later calls on this context: VX_DEV_F0_WINDOW_MIN .. VX_F0_WINDOW, or 0 for the default
 * (VX_F0_WINDOW).  A small window sends short rows through several parts and launches -- what the window tests need; the device
 * buffers keep their size.  One frame reaches window + lag_max samples: the minimum holds that at the largest options (window 2048,
 * lag_max 1024), so no call is refused for its window.  VX_EINVAL, nothing changed, for any other value. */
#define VX_DEV_F0_WINDOW_MIN 3072
int vx_dev_f0_window(vx_ctx* ctx, int32_t samples);

/* The mark costs and the grain table of ONE row as the kernels behind vx_psola (csrc/psola.hip) saw them: cost [N + 1] doubles, the
 * winning cost of every voiced mark below len as psola_marks_kernel wrote it and 0 for the unvoiced marks and the closing one;
 * grains [J][4] int32 = (s_j, a, Wl, Wr) of every grain, read back from the table psola_synth_kernel walked.  *n_marks = N and
 * *n_grains = J are always written on success.  The row goes through the same planner and window as vx_psola.  VX_EINVAL, nothing
 * written: a NULL pointer, len < 0, options or ratios out of range, cost_cap below N + 1 or grain_cap below J
 * (len / 14 + 2 and len / 7 + 2 always suffice). */
int vx_dev_psola_table(vx_ctx* ctx, const float* wav, int32_t len, const int32_t* lag, const int32_t* ratio /* may be NULL */,
                       const vx_psola_opts* o, double* cost, int32_t cost_cap, int32_t* grains, int32_t grain_cap, int32_t* n_marks,
                       int32_t* n_grains);
/* Samples one launch of vx_psola holds, for later calls on this context: VX_DEV_PSOLA_WINDOW_MIN .. VX_PSOLA_WINDOW, or 0 for the
 * default (VX_PSOLA_WINDOW).  A small window sends a ragged batch of short rows through several launches -- what the window tests
 * need; the device buffers keep their size.  A row is never cut, so a row above the window is refused (VX_EINVAL naming lens).
 * VX_EINVAL, nothing changed, for any other value. */
#define VX_DEV_PSOLA_WINDOW_MIN 1024
int vx_dev_psola_window(vx_ctx* ctx, int32_t samples);

/* The FFT network of vx_denoise (csrc/denoise.hip: the device function both of its kernels run) on caller frames: re / im
 * [nframes][512] doubles in natural order, loaded in bit-reversed order as the contract states; out_re / out_im [nframes][512].
 * inverse = 0: the forward network.  inverse = 1: the network with s negated and both components times 1 / 512.  No window, no
 * cleaning of the input words.  VX_EINVAL: a NULL pointer, nframes outside 1 .. VX_DEV_DENOISE_FFT_MAX, inverse not 0 or 1. */
#define VX_DEV_DENOISE_FFT_MAX 1024
int vx_dev_denoise_fft(vx_ctx* ctx, const double* re, const double* im, int32_t nframes, int32_t inverse, double* out_re, double* out_im);
/* What the kernels behind vx_denoise computed of ONE row: P [T][257] and E [T] as denoise_power_kernel wrote them, sel [K] the chosen
 * frames in ascending t as the profile kernel walked them (*n_sel = K; nothing with a noise_psd), gain [T][257] from the device
 * function the synthesis kernel runs, read from the same P and profile.  T = ceil(len / 128) + 3; sel_cap must hold K (T always
 * suffices).  The row goes through the same planner and window as vx_denoise.  VX_EINVAL, nothing written: a NULL pointer other than
 * noise_psd, len < 0 or above VX_DEV_DENOISE_TABLE_MAX, options out of range, sel_cap below K. */
#define VX_DEV_DENOISE_TABLE_MAX (1 << 20)
int vx_dev_denoise_table(vx_ctx* ctx, const float* wav, int32_t len, const vx_denoise_opts* o, const double* noise_psd /* may be NULL */,
                         double* P, double* E, int32_t* sel, int32_t sel_cap, int32_t* n_sel, double* gain);
/* Samples one launch of vx_denoise holds, for later calls on this context: VX_DEV_DENOISE_WINDOW_MIN .. VX_DENOISE_WINDOW, or 0 for
 * the default (VX_DENOISE_WINDOW).  A small window sends a ragged batch of short rows through several launches; the device buffers
 * keep their size.  A row is never cut, so a row above the window is refused (VX_EINVAL naming lens).  VX_EINVAL, nothing changed,
 * for any other value. */
#define VX_DEV_DENOISE_WINDOW_MIN 3072
int vx_dev_denoise_window(vx_ctx* ctx, int32_t samples);
/* q[i] = a[i] / b[i], i in [0, n), by a kernel of csrc/denoise.hip under the flags of its gain: the probe of the contract's claim
 * that double division on the device is correctly rounded.  VX_EINVAL: a NULL pointer, n outside 1 .. 65536. */
int vx_dev_denoise_div(vx_ctx* ctx, const double* a, const double* b, int32_t n, double* q);

/* Staged samples one launch of vx_eq holds (warm-ups included), for later calls on this context: VX_DEV_EQ_WINDOW_MIN .. VX_EQ_WINDOW,
 * or 0 for the default (VX_EQ_WINDOW).  A small window sends short rows through several jobs and launches -- what the window tests
 * need; the device buffers keep their size.  A launch must hold a warm-up and one step: while a window below W + VX_EQ_STEP of a
 * call's filter is set, that call is refused (VX_EINVAL), not run with a larger window.  VX_EINVAL, nothing changed, for any other
 * value. */
#define VX_DEV_EQ_WINDOW_MIN 4096
int vx_dev_eq_window(vx_ctx* ctx, int32_t samples);

#ifdef __cplusplus
}
#endif
#endif /* VALLEX_HIP_DEV_H */
