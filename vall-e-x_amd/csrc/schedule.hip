// The three host schedulers over the engine's phases (engine.hip: prefill, decode step, NAR), and their C ABI entries:
//   vx_infer              micro-batches of <= mbr decode rows, best_of beams included (ar_generate, select_beam)
//   vx_infer_continuous   one decode batch for the whole call; waiting caller rows are admitted into rows that finished (admit.hip)
//   vx_serve_*            a decode batch that outlives any single call; requests with their own best_of, sampling and filters are
//                         admitted as beam groups (serve.hip, serve_sample.hip)
// What they share is here once: the loop plumbing between two host polls, the admission of prefilled rows into a running decode batch
// (admit_common), the gather of a row set into a batch of its own and the delivery of finished rows.  Every admission round and every
// first fill runs behind the f16x2 range guard (engine_ctx.h: guarded).  Host code only: no kernel lives in this file.
#include "engine_ctx.h"

#include <deque>
#include <memory>

namespace vxe {

// ---- loop plumbing of the three schedulers -------------------------------------------------------------------------
// signature of the captured step graph of nrows decode rows ending in dec_sample (the serving session's sampler has its own)
static std::string step_sig(const vx_ctx* c, int nrows, const SampleArgs& sa) {
  char sig[160];
  snprintf(sig, sizeof sig, "b%d ns%d c%d%d%d k%d t%a u%d f%d l%d", nrows, c->nsplit, (int)c->sb_chain, (int)c->sb_qkv, (int)c->split_fused, sa.top_k,
           sa.temperature, sa.uniforms != nullptr, sa.force_eos_at, sa.sum_logp != nullptr);
  return sig;
}
// decode steps between two host polls, and steps per graph launch: GRAPH_STEPS while that never crosses a poll (nsteps is 1 or
// GRAPH_STEPS: two graphs)
static int poll_interval(const vx_sampling& s) { return s.sync_every > 0 ? s.sync_every : 8; }
static int graph_chunk(const vx_ctx* c, int sync_every) { return (c->graph_multi && sync_every % GRAPH_STEPS == 0) ? GRAPH_STEPS : 1; }

// decode steps until `steps` == target, gs per launch where a whole chunk starts aligned and still fits
static int run_steps_to(vx_ctx* c, const SampleArgs* sa, const ServeSampleArgs* rsa, const std::string& sig, long& steps, long target, int gs) {
  while (steps < target) {
    const int n = (steps % gs == 0 && steps + gs <= target) ? gs : 1;
    if (int e = ar_step_run(c, sa, sig, n, rsa)) return e;
    steps += n;
  }
  return VX_OK;
}

// the step to decode up to: the next host poll, or the step by which an occupied decode row has stopped at the latest (its cap: that
// poll is sure to free a row -- without it a row capped between two polls would leave its decode row idle until the next one)
template <typename Occupied>
static long next_target(long steps, int sync_every, const std::vector<int>& done_by, Occupied occupied) {
  long soonest = (steps / sync_every + 1) * sync_every;
  for (size_t d = 0; d < done_by.size(); ++d) if (occupied(d)) soonest = std::min<long>(soonest, done_by[d]);
  return std::max(soonest, steps + 1);
}

// host poll: the active flags (and the frame counts, ng != null) of decode rows 0 .. nd-1.  with_flag: the poll behind the first
// sample of a guarded round (the end of its `once`) -- the range flag of the round's prefill rides on the same sync
static int poll(vx_ctx* c, std::vector<int>& act, std::vector<int>* ng, int nd, bool with_flag = false) {
  D2H(act.data(), c->active, nd * sizeof(int));
  if (ng) D2H(ng->data(), c->n_gen, nd * sizeof(int));
  if (with_flag) return sync_guarded(c);
  SYNC();
  return VX_OK;
}

// ---- AR generation for one micro-batch -----------------------------------------------------------------------
// caller rows r0 .. r0+nb-1, each decoded as `beams` rows (decode row i*beams + j: beam j of row r0 + i); `seed` is the sampler's
// seed for this micro-batch (unused with injected uniforms)
static int ar_generate(vx_ctx* c, const vx_batch* b, const vx_sampling* s, int r0, int nb, std::vector<int>& n_gen,
                std::vector<int>& gen, int beams, unsigned long long seed) {
  const int nb_rows = nb;                            // rows of the caller's batch that this micro-batch prefills
  const long ub = (long)b->batch * beams;            // columns of the caller's uniforms: [steps][batch x best_of]
  nb = nb_rows * beams;                              // decode rows
  SampleArgs sa{};
  std::vector<int> act(nb);
  bool any = true, staged = false;
  // The prefill, then the first token from its logits; the host sync that tells whether anything is still active also brings the
  // range flag of the prefill back.  Raised: the K/V cache, the residual row and the logits are not to be trusted -- guarded() runs
  // both again on the exact-fp32 kernels (the prefill resets the decode state).
  auto once = [&]() -> int {
    if (int e = ar_prefill(c, b, r0, nb_rows, beams)) return e;
    if (!staged) {      // behind the first prefill only: a re-run finds the draws, the seed and the sampler's arguments in place
      staged = true;
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
      sa = make_sample_args(c, s, 1, nullptr);
    }
    HIPCHK(hipMemsetAsync(c->sum_logp, 0, MB * sizeof(float), c->stream));
    LAUNCH(launch_dec_sample(sa, c->stream));
    if (int e = launch_status(c)) return e;
    const int e = poll(c, act, nullptr, nb, true);
    any = std::any_of(act.begin(), act.end(), [](int v) { return v != 0; });
    return e;
  };
  if (int e = guarded(c, prefill_kind(c), once)) return e;
  const std::string sig = step_sig(c, nb, sa);
  const int sync_every = poll_interval(*s), gs = graph_chunk(c, sync_every);
  // with a forced EOS every row is inactive after force_eos_at steps: do not run on to the next host poll
  const long hard_cap = s->force_eos_at >= 0 ? std::min(c->gen_stride + 2, s->force_eos_at) : c->gen_stride + 2;
  long steps = 0;
  while (any && steps < hard_cap) {
    if (int e = run_steps_to(c, &sa, nullptr, sig, steps, std::min(hard_cap, (steps / sync_every + 1) * sync_every), gs)) return e;
    if (steps % sync_every == 0) {
      if (int e = poll(c, act, nullptr, nb)) return e;
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

// ---- delivery: what the schedulers share on the way out -------------------------------------------------------------------------
// the step count by which the sampler has stopped a row at the latest: n_gen = min(16 S, gen_stride, force_eos_at)
static int step_cap(const vx_ctx* c, int S, int force_eos_at) {
  return std::min(force_eos_at >= 0 ? std::min(c->gen_stride, force_eos_at) : c->gen_stride, 16 * S);
}
// a row of T frames that fills the arena although neither EOS, the reference's 16*S cap nor a forced EOS ended it was cut short
static bool cut_by_arena(const vx_ctx* c, int T, int S, int force_eos_at) {
  return T >= c->gen_stride && c->gen_stride < 16 * S && !(force_eos_at >= 0 && force_eos_at <= c->gen_stride);
}
// the NAR stages of a gathered group between two decode steps (codes0 [nb][gen_stride]), timed into st_nar_ms
static int timed_nar(vx_ctx* c, const vx_batch* b, int nb, const std::vector<int>& T, const int* codes0, std::vector<int>& oc, long& sumT) {
  hipEvent_t e1 = c->ev_t[1], e2 = c->ev_t[2];
  HIPCHK(hipEventRecord(e1, c->stream));
  if (int e = nar_generate(c, b, 0, nb, T, codes0, c->gen_stride, oc, sumT)) return e;
  HIPCHK(hipEventRecord(e2, c->stream));
  HIPCHK(hipEventSynchronize(e2));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, e1, e2)); c->st_nar_ms += ms;
  return VX_OK;
}

// ---- admission: prefilled rows into a running decode batch (continuous schedule and serving session) ---------------------------
// rows gathered into a vx_batch of their own (prefill / NAR of a row set that is not a range of one caller batch: caller rows of the
// continuous schedule, requests of a session).  Tight strides: prefill_tables and nar_generate_once read every row by its length.
struct RowView { const int32_t *ids, *lang; int S; const int32_t* pc; int Tp; };      // text ids / language ids [S], prompt codes [Tp][8]
static RowView row_view(const vx_batch* b, int r) {
  return {b->text_ids + (long)r * b->text_stride, b->text_lang + (long)r * b->text_stride, b->text_lens[r],
          b->prompt_codes + (long)r * b->prompt_stride * N_Q, b->prompt_lens[r]};
}
struct Gather {
  std::vector<int32_t> ids, lang, tl, pc, pl;
  vx_batch b{};
  template <typename View>
  Gather(int n, View view) {              // view(i): row i of the gathered batch
    std::vector<RowView> rows(n);
    int ts = 1, ps = 1;
    for (int i = 0; i < n; ++i) { rows[i] = view(i); ts = std::max(ts, rows[i].S); ps = std::max(ps, rows[i].Tp); }
    ids.assign((size_t)n * ts, 0); lang.assign((size_t)n * ts, 0); pc.assign((size_t)n * ps * N_Q, 0); tl.resize(n); pl.resize(n);
    for (int i = 0; i < n; ++i) {
      const RowView& r = rows[i];
      std::copy_n(r.ids, r.S, ids.begin() + (size_t)i * ts);
      std::copy_n(r.lang, r.S, lang.begin() + (size_t)i * ts);
      std::copy_n(r.pc, (size_t)r.Tp * N_Q, pc.begin() + (size_t)i * ps * N_Q);
      tl[i] = r.S; pl[i] = r.Tp;
    }
    b.struct_size = sizeof(vx_batch); b.batch = n;
    b.text_ids = ids.data(); b.text_lang = lang.data(); b.text_stride = ts; b.text_lens = tl.data();
    b.prompt_codes = pc.data(); b.prompt_stride = ps; b.prompt_lens = pl.data();
  }
};

// One admission into the running decode batch (c->cur_batch rows), up to and including the first sample of the admitted rows: the
// prefill of the gathered rows gb, prefill row i into arena slot slot[i]; the fan-out of a request's K / V to its other beams' slots
// (fan [m][3] = {source slot, destination slot, cached rows}, beams.hip; may be empty); the decode state of the n admitted decode
// rows, rows [n][2] = {decode row d, prefill row it continues from} (admit.hip: completed here to the [n][5] table of
// launch_admit_rows); then the first sample, committed for the rows of the mask adm [cur_batch] only.  The rows still decoding keep
// every piece of their state: the prefill scatters K / V into the admitted slots only, its final norm + predict layer run on scratch
// copies (dh2 / xp_att: the step recomputes both before it reads them; the logits of rows that are not admitted are never read).
// The caller has staged the tables of its draws in mb; draws() launches them behind the upload, sample() launches its sampler.
template <typename Draws, typename Sample>
static int admit_common(vx_ctx* c, MetaBuilder& mb, const vx_batch& gb, const std::vector<int>& slot, const std::vector<int>& rows,
                        const std::vector<int>& adm, const std::vector<int>& fan, Draws draws, Sample sample) {
  const int nd = c->cur_batch, n = (int)rows.size() / 2;
  PrefillPlan p;
  if (int e = prefill_tables(c, &gb, 0, gb.batch, p, mb)) return e;
  for (int& rb : p.row_b) rb = slot[rb];
  p.o_rb = mb.add(p.row_b);
  std::vector<int> tab(5 * n), saved(nd, 0);
  for (int j = 0; j < n; ++j) {
    const int i = rows[2 * j + 1];
    tab[5 * j] = rows[2 * j]; tab[5 * j + 1] = gb.prompt_lens[i]; tab[5 * j + 2] = p.seq_len[i]; tab[5 * j + 3] = p.S_[i]; tab[5 * j + 4] = p.hrow(i);
  }
  const long o_tab = mb.add(tab), o_adm = mb.add(adm), o_saved = mb.add(saved), o_fan = fan.empty() ? 0 : mb.add(fan);
  if (int e = upload_meta(c)) return e;
  draws();
  if (int e = prefill_layers(c, p, mb)) return e;
  const float* hsrc = prefill_hsrc(c, p);
  if (!fan.empty())
    launch_beam_fanout(c->kc, c->vc, (long)((size_t)c->mbr * N_HEAD * c->Tmax * D_HEAD), c->NL, c->Tmax, mb.dev(o_fan),
                       (int)fan.size() / 3, hsrc, nullptr, c->dh, 0, c->stream);
  launch_admit_rows(mb.dev(o_tab), n, hsrc, c->dh2, c->cur_tok, c->cur_pos, c->ctx_len, c->n_gen, c->text_len, c->slot_meta,
                    c->slot_of, c->stream);
  launch_dec_reduce_ln_pack(nullptr, 0, D_MODEL, nullptr, c->dh2, nullptr, W(c, "ar_decoder.norm.weight"),
                            W(c, "ar_decoder.norm.bias"), c->xp_att, nd, c->stream);
  launch_skinny_gemm(c->pred_wp, c->xp_att, c->p_logits, PRED_NPAD, D_MODEL, SK_PRED, c->stream);
  int* sv = c->imeta + o_saved;
  launch_admit_mask(0, mb.dev(o_adm), sv, nd, c->active, c->slot_meta, c->slot_of, c->n_active, c->stream);
  sample();
  launch_admit_mask(1, mb.dev(o_adm), sv, nd, c->active, c->slot_meta, c->slot_of, c->n_active, c->stream);
  return launch_status(c);
}

// ---- continuous schedule (vx_infer_continuous) ---------------------------------------------------------------
// One decode batch of nd = min(mbr, batch) rows for the whole call: the first fill is ar_prefill of caller rows 0 .. nd-1 (it sets
// the geometry: slot order, context splits, chain choice -- fixed from then on, so the captured step graph never changes); at every
// host poll (every sync_every steps, and at the step where a row reaches its cap) the rows that stopped are harvested (n_gen + gen row
// to the host) and waiting caller rows, first come first served, are admitted into the freed decode rows: one prefill per admission
// round into the freed rows' KV slots, then the first sample of the admitted rows alone.  Harvested rows go through the NAR stages in
// groups of mbr (the rest once nothing is left to decode), between two decode steps: nar_generate only touches the full-sequence buffers.

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

// admission of caller rows crow[i] into the free decode rows drow[i] of the running decode batch (admit_common)
static int admit_rows(vx_ctx* c, const vx_batch* b, const vx_sampling* s, const SampleArgs& sa, const std::vector<int>& drow,
                      const std::vector<int>& crow, const std::vector<int>& slot_of) {
  const int k = (int)drow.size();
  std::vector<int> slot(k), rows(2 * k), adm(c->cur_batch, 0);
  for (int i = 0; i < k; ++i) {
    slot[i] = slot_of[drow[i]];
    rows[2 * i] = drow[i]; rows[2 * i + 1] = i;
    adm[drow[i]] = 1;
  }
  Gather g(k, [&](int i) { return row_view(b, crow[i]); });
  MetaBuilder mb(c);
  UniformCols uc;
  if (int e = uniform_cols(c, b, s, drow, crow, mb, uc)) return e;
  return admit_common(c, mb, g.b, slot, rows, adm, {}, [&] { uniform_cols_launch(c, s, uc, mb); },
                      [&] { LAUNCH(launch_dec_sample(sa, c->stream)); });
}

static int infer_continuous(vx_ctx* c, const vx_batch* b, const vx_sampling* s, vx_row_done_fn on_row, void* user, int64_t* out_codes,
                     int32_t out_stride, int32_t* out_lens) {
  const int B = b->batch, nd = std::min(c->mbr, B);
  hipEvent_t e0 = c->ev_t[0], e1 = c->ev_t[1];
  HIPCHK(hipEventRecord(e0, c->stream));
  // per decode row: the caller row in it (-1: free) and the step by which it has stopped at the latest (step_cap behind its admission)
  std::vector<int> occ(nd, -1), done_by(nd, 0), act(nd, 0), ng(nd, 0), slot_of(nd);
  std::vector<std::vector<int>> rowgen(B);           // first-codebook ids of every harvested row (D2H target: never reallocated)
  std::vector<int> pend;                             // harvested rows waiting for their NAR stages, in the order they completed
  int next = 0;                                      // first caller row not admitted yet
  long steps = 0;
  SampleArgs sa{};
  // one admission round (first fill or admission) behind the f16x2 range guard: a raised flag re-runs the round, prefill and first
  // sample, on the exact-fp32 kernels; it counts in vx_last_fallbacks and towards sticky mode
  auto round = [&](const std::vector<int>& drow, const std::vector<int>& crow) -> int {
    const bool first = occ[0] < 0 && next == 0;
    auto once = [&]() -> int {
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
      return poll(c, act, &ng, nd, true);
    };
    if (int e = guarded(c, prefill_kind(c), once)) return e;
    for (size_t i = 0; i < drow.size(); ++i) {
      occ[drow[i]] = crow[i];
      done_by[drow[i]] = (int)steps + step_cap(c, b->text_lens[crow[i]], s->force_eos_at);
    }
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
    Gather g(n, [&](int i) { return row_view(b, rows[i]); });
    long sumT = 0, off = 0;
    if (int e = timed_nar(c, &g.b, n, T, codes0.data(), oc, sumT)) return e;
    for (int i = 0; i < n; ++i) {
      const int r = rows[i];
      out_lens[r] = T[i];
      c->st_frames += T[i];
      if (cut_by_arena(c, T[i], b->text_lens[r], s->force_eos_at)) ++c->st_truncated;
      int64_t* o0 = out_codes + (long)r * out_stride * N_Q;
      interleave_codes(o0, &codes0[(size_t)i * c->gen_stride], oc, sumT, off, T[i]);
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
  const std::string sig = step_sig(c, nd, sa);
  const int sync_every = poll_interval(*s), gs = graph_chunk(c, sync_every);
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
    const long target = next_target(steps, sync_every, done_by, [&](size_t d) { return occ[d] >= 0; });
    if (int e = run_steps_to(c, &sa, nullptr, sig, steps, target, gs)) return e;
    if (int e = poll(c, act, &ng, nd)) return e;
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
  RowView view() const { return {ids.data(), lang.data(), S, pc.data(), Tp}; }
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
  if (int e = reset_decode_state(c, mb, nd, o_z, o_1, o_z, o_z, o_1, o_meta, o_slot)) return e;
  HIPCHK(hipMemsetAsync(c->n_active, 0, sizeof(int), c->stream));
  c->cur_batch = nd;
  c->h_L.assign(nd, 0);
  decode_geometry(c, nd, true);
  SYNC();                                      // the staged tables are consumed before the next MetaBuilder reuses imeta
  return VX_OK;
}

// admission of requests rq (their beam rows assigned, rq[i]->rows) into free decode rows (admit_common).  Each request is prefilled
// once, into the arena slot of its first beam row, and fanned out to the other beams' slots; every beam row continues from the
// request's prefill row, with its own draws (keyed on (request seed, beam) or the request's injected column), a zero sum_logp and the
// request's sampling and filter records (launch_serve_uniforms)
static int serve_admit(vx_serve* v, const std::vector<ServeReq*>& rq) {
  vx_ctx* c = v->c;
  const int k = (int)rq.size(), nd = v->nd;
  std::vector<int> slot(k), rows, adm(nd, 0), fan, staged, utab;
  const int cap_steps = c->gen_stride + 1;         // draws a row can ever consume: one per generated frame + the terminating one
  int max_steps = 1;
  std::vector<int> soff(k, -1);                    // injected draws first (their offsets go into the draw table), as float bits in the int tables
  for (int i = 0; i < k; ++i) {
    const ServeReq* r = rq[i];
    const int ctx = r->S + 1 + r->Tp;              // rows the prefill caches
    if (ctx > c->Tmax) FAIL(VX_EINVAL, "request %lld: %d cached rows exceed the arena (%d)", (long long)r->id, ctx, c->Tmax);
    slot[i] = v->slot_of[r->rows[0]];
    for (int j = 0; j < r->N; ++j) {
      const int d = r->rows[j];
      rows.insert(rows.end(), {d, i});
      adm[d] = 1;
      if (j) fan.insert(fan.end(), {slot[i], v->slot_of[d], ctx});
    }
    if (!r->usteps) continue;
    soff[i] = (int)staged.size();
    const int st = std::min(r->usteps, cap_steps);
    for (int j = 0; j < r->N; ++j) {
      const size_t o = staged.size();
      staged.resize(o + st);
      memcpy(&staged[o], &r->u[(size_t)j * r->usteps], st * sizeof(float));
    }
  }
  Gather g(k, [&](int i) { return rq[i]->view(); });
  MetaBuilder mb(c);
  const long o_st = staged.empty() ? 0 : mb.add(staged);
  for (int i = 0; i < k; ++i) {
    const ServeReq* r = rq[i];
    const int st = r->usteps ? std::min(r->usteps, cap_steps) : cap_steps;
    max_steps = std::max(max_steps, st);
    for (int j = 0; j < r->N; ++j) {
      const int rec[] = {r->rows[j], j, r->usteps ? (int)(o_st + soff[i] + (long)j * st) : -1, st, (int)(uint32_t)r->seed,
                         (int)(uint32_t)(r->seed >> 32), r->top_k, __builtin_bit_cast(int, r->temperature), r->force_eos_at,
                         __builtin_bit_cast(int, r->top_p), __builtin_bit_cast(int, r->rep_penalty), r->rep_window, r->min_frames};
      static_assert(sizeof rec / sizeof rec[0] == SERVE_UTAB, "the record launch_serve_uniforms reads (engine_ctx.h)");
      utab.insert(utab.end(), std::begin(rec), std::end(rec));
    }
  }
  const int nbeam = (int)rows.size() / 2;
  if ((long)max_steps * nd > c->uniforms_cap) FAIL(VX_EINVAL, "too many uniforms (%d steps)", max_steps);
  const long o_ut = mb.add(utab);
  return admit_common(c, mb, g.b, slot, rows, adm, fan,
                      [&] {
                        launch_serve_uniforms(mb.dev(o_ut), nbeam, max_steps, reinterpret_cast<const float*>(c->imeta), c->d_uniforms, nd,
                                              c->sum_logp, c->row_smp, c->row_flt, c->stream);
                      },
                      [&] { LAUNCH(launch_serve_sample(v->rsa, c->stream)); });
}

// one admission round behind the f16x2 range guard, as in infer_continuous: a raised flag re-runs the round (prefill, fan-out, first
// sample) on the exact-fp32 kernels; it counts in vx_last_fallbacks and towards sticky mode
static int serve_round(vx_serve* v, const std::vector<ServeReq*>& rq) {
  vx_ctx* c = v->c;
  if (int e = guarded(c, prefill_kind(c), [&]() -> int {
        if (int e2 = serve_admit(v, rq)) return e2;
        return poll(c, v->act, &v->ng, v->nd, true);
      }))
    return e;
  for (ServeReq* r : rq)
    for (int j = 0; j < r->N; ++j) {
      const int d = r->rows[j];
      v->occ[d] = r; v->beam[d] = j; v->done_by[d] = (int)v->steps + step_cap(c, r->S, r->force_eos_at);
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
  Gather g(n, [&](int i) { return rq[i]->view(); });
  long sumT = 0, off = 0;
  if (int e = timed_nar(c, &g.b, n, T, codes0.data(), oc, sumT)) return e;
  std::vector<int64_t> out;
  for (int i = 0; i < n; ++i) {
    c->st_frames += T[i];
    if (cut_by_arena(c, T[i], rq[i]->S, rq[i]->force_eos_at)) ++c->st_truncated;      // the request's own forced EOS
    out.assign((size_t)std::max(1, T[i]) * N_Q, 0);
    interleave_codes(out.data(), &codes0[(size_t)i * c->gen_stride], oc, sumT, off, T[i]);
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
  const int sync_every = poll_interval(v->s), gs = graph_chunk(c, sync_every);
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
    long target = next_target(v->steps, sync_every, v->done_by, [&](size_t d) { return v->occ[d] != nullptr; });
    if (max_steps > 0) target = std::min(target, start + max_steps);
    if (int e = run_steps_to(c, nullptr, &v->rsa, v->sig, v->steps, target, gs)) return e;
    if (int e = poll(c, v->act, &v->ng, nd)) return e;
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
int serve_busy(vx_ctx* c, const char* what) {
  if (!c->serve) return VX_OK;
  FAIL(VX_EINVAL, "%s: a serving session is open on this context (vx_serve_close it first)", what);
}

void serve_free(vx_serve* v) { delete v; }

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
    CHECK_STRUCT(q, vx_request);
    if (smp) {
      const vx_request_sampling& m = smp[i];
      CHECK_STRUCT(m, vx_request_sampling);
      if (!(m.temperature > 0.f) || !std::isfinite(m.temperature))
        FAIL(VX_EINVAL, "request %d: temperature must be > 0 and finite (got %g)", i, (double)m.temperature);
      if (m.force_eos_at < -1) FAIL(VX_EINVAL, "request %d: force_eos_at must be >= -1 (got %d)", i, m.force_eos_at);
      rs[i] = m;
    }
    if (flt) {
      const vx_request_filters& f = flt[i];
      CHECK_STRUCT(f, vx_request_filters);
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
      const int need = step_cap(c, b->text_lens[i], rs[i].force_eos_at) + 1;
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

extern "C" {

int vx_infer(vx_ctx* c, const vx_batch* b, const vx_sampling* s, int64_t* out_codes, int32_t out_stride,
             int32_t* out_lens) {
  if (!c || !s || !out_codes || !out_lens) return VX_EINVAL;
  if (int e = serve_busy(c, "vx_infer")) return e;
  HIPCHK(hipSetDevice(c->dev));
  CHECK_STRUCT(*s, vx_sampling);
  if (int e = check_batch(c, b, c->cfg.max_batch)) return e;
  if (!(s->temperature > 0.f)) FAIL(VX_EINVAL, "temperature must be > 0");
  reset_call_stats(c);
  hipEvent_t e0 = c->ev_t[0], e1 = c->ev_t[1], e2 = c->ev_t[2];      // owned by the context: nothing to leak on an early return
  // best-of-N beams of every row (models/vallex.py:491,525-527): each row is decoded as N beams that sample independently, beams
  // that emit EOS stop; per row, selection on sum(logp) / len^penalty (:583-594), then the NAR stages run on the chosen beams only
  // (:600).  A micro-batch holds R = mbr / N rows = R*N decode rows; row r's result is what a batch-1 call on that row alone
  // returns with the same draws (uniforms column r*N + j = beam j of row r).  N == 1: no selection, no sum_logp round trip, and
  // every micro-batch samples with the caller's seed.
  const int N = std::max(1, s->best_of);
  if (N > c->mbr) FAIL(VX_EINVAL, "best_of %d exceeds the micro-batch (%d)", N, c->mbr);
  const int R = c->mbr / N;
  for (int r0 = 0, k = 0; r0 < b->batch; r0 += R, ++k) {
    const int nb = std::min(R, b->batch - r0);
    std::vector<int> n_gen, gen, oc, picked;
    HIPCHK(hipEventRecord(e0, c->stream));
    if (int e = ar_generate(c, b, s, r0, nb, n_gen, gen, N, N > 1 ? beam_seed(s->seed, k) : s->seed)) return e;
    HIPCHK(hipEventRecord(e1, c->stream));
    if (N > 1) {       // every row reduced to its selected beam: n_gen [nb], gen [nb][gen_stride] from here on
      std::vector<float> slp((size_t)nb * N);
      D2H(slp.data(), c->sum_logp, slp.size() * sizeof(float)); SYNC();
      std::vector<int> T(nb);
      picked.resize((size_t)nb * c->gen_stride);
      for (int i = 0; i < nb; ++i) {
        const int pick = i * N + select_beam(&slp[(size_t)i * N], &n_gen[(size_t)i * N], N, b->prompt_lens[r0 + i], s->length_penalty,
                                             s->return_worst != 0);
        T[i] = n_gen[pick];
        std::copy_n(gen.begin() + (size_t)pick * c->gen_stride, c->gen_stride, picked.begin() + (size_t)i * c->gen_stride);
      }
      n_gen.swap(T); gen.swap(picked);
    }
    for (int i = 0; i < nb; ++i)
      if (n_gen[i] > out_stride) FAIL(VX_EINVAL, "out_stride %d too small for %d frames", out_stride, n_gen[i]);
    long sumT = 0, off = 0;
    if (int e = nar_generate(c, b, r0, nb, n_gen, gen.data(), c->gen_stride, oc, sumT)) return e;
    HIPCHK(hipEventRecord(e2, c->stream));
    HIPCHK(hipEventSynchronize(e2));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1)); c->st_ar_ms += ms;
    HIPCHK(hipEventElapsedTime(&ms, e1, e2)); c->st_nar_ms += ms;
    for (int i = 0; i < nb; ++i) {
      out_lens[r0 + i] = n_gen[i];
      c->st_frames += n_gen[i];
      if (cut_by_arena(c, n_gen[i], b->text_lens[r0 + i], s->force_eos_at)) ++c->st_truncated;
      interleave_codes(out_codes + (long)(r0 + i) * out_stride * N_Q, &gen[(size_t)i * c->gen_stride], oc, sumT, off, n_gen[i]);
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
  CHECK_STRUCT(*s, vx_sampling);
  // any number of rows: the call holds device memory for its min(max_batch, 32) decode rows and one NAR group only
  if (int e = check_batch(c, b, 0x7fffffff)) return e;
  if (!(s->temperature > 0.f)) FAIL(VX_EINVAL, "temperature must be > 0");
  if (s->best_of > 1) FAIL(VX_EINVAL, "vx_infer_continuous does not run best_of > 1 (use vx_infer)");
  reset_call_stats(c);
  return infer_continuous(c, b, s, on_row, user, out_codes, out_stride, out_lens);
}

int vx_serve_open(vx_ctx* c, const vx_sampling* s, vx_serve** out) {
  if (!c || !s || !out) return VX_EINVAL;
  HIPCHK(hipSetDevice(c->dev));
  if (!c->finalized) FAIL(VX_ESTATE, "weights not finalized");
  CHECK_STRUCT(*s, vx_sampling);
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
  reset_call_stats(c);
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

}  // extern "C"
