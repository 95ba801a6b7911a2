// The equaliser with a carried state (vx_eq_carry, vx_eq_carry_plan, include/vallex_hip.h): the cascade of eq.hip without its bounded
// memory.  A row is walked in steps of Sc = VX_EQ_CARRY_STEP samples, three launches per window on the context's stream:
//
//   ends     eq_carry_kernel<NS, false>: ONE lane runs step j from rest over its Sc samples (zeros behind the row's end) and writes
//            the state it ends in, f_j.
//   chain    eq_carry_chain_kernel<NS>: ONE wavefront per job walks z_{j+1} = f_j + M z_j over the job's steps in order and writes
//            every z_j.  M (eq_carry_host.h) is the cascade's own step over Sc zero inputs: the cascade is linear in (state, input).
//   rows     eq_carry_kernel<NS, true>: ONE lane runs step j from z_j over its own samples; each output is rounded once to fp32.  The
//            lane of a row's last step writes the state it holds behind the row's last sample (state_out).
//
// Arithmetic (the contract the tests rest on): per sample eq_host.h's eq_section, in the chain eq_carry_dot's order, both in double
// with contraction off.  An output is a function of its row, the coefficients and the row's state_in: its bits do not depend on the
// batch, the job, the tile, the window or the launch.  No atomics, no inline assembly.
//
// Work decomposition of ends and rows: eq_rows_kernel's (eq.hip) with W = 0 -- grid (tile, job), a tile = 64 consecutive steps, one per
// lane; chunks of 32 samples loaded with coalesced row loads, staged in LDS at a lane stride of 33 floats, the next chunk in flight
// behind the recursion; outputs leave through a third LDS tile as coalesced runs; one record per tile for the counts and the peak.
// One template serves both: what differs (the start state, the outputs, what is written at the end) is compile-time, so neither
// instance carries the other's registers.  A rows lane stops its recursion behind its own samples (only a row's last step is short),
// which is what leaves state_out in its registers; an ends lane runs all Sc samples, as the contract pads the last step.
// The chain is a dependent fp64 chain of 2 D operations per step by construction: lane i < D owns component i with row i of M in
// registers, z_j is broadcast by lane reads, f_j arrives eight steps ahead of its use.
// The step tables (f, z: D doubles per step), the jobs' start states, their end states, the two carry slots and M lie behind the outputs
// in the upper half of rs_out, beside the tile records: at every Sc the header allows they fit, so nothing else is allocated.
#include "wave_stage.h"
#include "eq_carry_host.h"

#include "../../include/vallex_hip_dev.h"

namespace {
// the cascade of this thread's last vx_eq_carry and its M: the D runs over Sc samples are not repeated for the same filter
thread_local struct { double sec[5 * VX_EQ_MAX_SECTIONS], m[vxe::EQC_DMAX * vxe::EQC_DMAX]; int n = 0; } g_eqc_last;
}  // namespace

namespace vxe {

constexpr int EQC_LANES = EQ_TILE;         // steps of a tile: one wavefront
constexpr int EQC_C = 32;                  // samples of a chunk
constexpr int EQC_STRIDE = EQC_C + 1;      // floats between the lanes of a staged chunk
constexpr int EQC_REC = 4;                 // ints of a tile record: {non-finite inputs, non-finite results, bits of the peak, 0}
constexpr int EQC_PF = 8;                  // steps the chain reads f ahead
constexpr int EQC_CONT = 1, EQC_CUT = 2, EQC_LAST = 4;      // flags of a job record
// the tables of a launch, in doubles from rs_out + RS_IN_CAP (the outputs of this stage never reach the upper half)
constexpr long EQC_ST_CAP = RS_IN_CAP / EQC_S + RS_MAX_JOBS;                 // a step per full Sc samples plus a short one per job
constexpr long EQC_REC_CAP = RS_IN_CAP / EQC_S / EQ_TILE + RS_MAX_JOBS;      // a record per full tile plus a cut one per job
constexpr long EQC_F = 0, EQC_Z = EQC_F + EQC_ST_CAP * EQC_DMAX, EQC_Z0 = EQC_Z + EQC_ST_CAP * EQC_DMAX,
               EQC_SOUT = EQC_Z0 + (long)RS_MAX_JOBS * EQC_DMAX, EQC_CARRY = EQC_SOUT + (long)RS_MAX_JOBS * EQC_DMAX, EQC_M = EQC_CARRY + 2 * EQC_DMAX,
               EQC_RECS = EQC_M + EQC_DMAX * EQC_DMAX, EQC_END = EQC_RECS + (EQC_REC_CAP * EQC_REC + 1) / 2;
static_assert(VX_EQ_WINDOW == RS_IN_CAP, "vx_eq_carry runs in the resampler's launch buffers");
static_assert(EQC_END * 2 <= RS_OUT_CAP - RS_IN_CAP, "the step tables and the records fit behind the outputs");
static_assert(VX_DEV_EQ_WINDOW_MIN >= EQC_S, "the smallest window holds a step");
static_assert(EQC_LANES == 64 && EQC_STRIDE % 2 == 1 && EQC_S % EQC_C == 0, "tile shape");

struct EqcCoef { double c[5 * EQ_MAX]; };

// tab [njobs][RS_TAB]: {off, cnt, st_off, rec_off, flags, rslot, wslot}: the job's steps cover in[off .. off + cnt) and write
// out[off .. off + cnt);
// step t of the job -> row st_off + t of the step tables; tile t -> rec[(rec_off + t) EQC_REC ..]; job b -> row b of z0 and sout.
// Every sample read is inside in[off .. off + cnt), every sample written inside out[off .. off + cnt).
template <int NS, bool ROWS>
__global__ __launch_bounds__(EQC_LANES) void eq_carry_kernel(const float* __restrict__ in, const int* __restrict__ tab, float* __restrict__ out,
                                                             int* __restrict__ rec, double* __restrict__ ftab, const double* __restrict__ ztab,
                                                             double* __restrict__ sout, EqcCoef k) {
  constexpr int S = EQC_S, D = 2 * NS;
  __shared__ float xs[2][EQC_LANES * EQC_STRIDE];
  __shared__ float ys[ROWS ? EQC_LANES * EQC_STRIDE : 1];
  const int* tb = tab + blockIdx.y * RS_TAB;
  const long off = tb[0], st0 = tb[2];
  const int cnt = tb[1], nst = (cnt + S - 1) / S, t0 = blockIdx.x * EQC_LANES;
  if (t0 >= nst) return;                                           // block-uniform
  const int tid = threadIdx.x;
  const int own_first = cnt - t0 * S < S ? cnt - t0 * S : S;        // own samples of the tile's first step: the longest stream
  const int nchunk = ROWS ? (own_first + EQC_C - 1) / EQC_C : S / EQC_C;
  const int my = t0 + tid;                                         // this lane's step
  const int own = my < nst ? (cnt - my * S < S ? cnt - my * S : S) : 0;
  // loader: thread tid fills column (tid & 31) of the lanes 2 i + (tid >> 5); stream position q of lane r is job sample (t0 + r) S + q
  const int lcol = tid & (EQC_C - 1), lrow = tid >> 5;
  const long lbase = (long)(t0 + lrow) * S + lcol;
  float reg[EQC_LANES / 2];
  auto fetch = [&](int q0) {
#pragma unroll
    for (int i = 0; i < EQC_LANES / 2; ++i) {
      const long p = lbase + (long)(2 * i) * S + q0;
      reg[i] = p < cnt ? in[off + p] : 0.f;
    }
  };
  auto stage = [&](int b) {
#pragma unroll
    for (int i = 0; i < EQC_LANES / 2; ++i) xs[b][(2 * i + lrow) * EQC_STRIDE + lcol] = reg[i];
  };
  fetch(0);
  stage(0);
  __syncthreads();
  double s1[NS], s2[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    s1[s] = ROWS && my < nst ? ztab[(st0 + my) * D + 2 * s] : 0.0;
    s2[s] = ROWS && my < nst ? ztab[(st0 + my) * D + 2 * s + 1] : 0.0;
  }
  int bad_in = 0, bad_out = 0;
  float peak = 0.f;
  for (int ch = 0; ch < nchunk; ++ch) {
    const int q0 = ch * EQC_C;
    if (ch + 1 < nchunk) fetch(q0 + EQC_C);                        // in flight behind the recursion
    const float* xp = xs[ch & 1] + tid * EQC_STRIDE;
    float* yp = ys + (ROWS ? tid * EQC_STRIDE : 0);
#pragma unroll 4
    for (int j = 0; j < EQC_C; ++j) {
      if (ROWS && q0 + j >= own) continue;                         // behind the lane's own samples the state stands still
      const float xf = xp[j];
      const bool fin = (__float_as_uint(xf) & 0x7f800000u) != 0x7f800000u;
      double u = fin ? (double)xf : 0.0;
#pragma unroll
      for (int s = 0; s < NS; ++s) u = eq_section(k.c + 5 * s, u, s1[s], s2[s]);
      if (ROWS) {
        float y = (float)u;
        const bool ok = (__float_as_uint(y) & 0x7f800000u) != 0x7f800000u;
        y = ok ? y : 0.f;
        bad_in += fin ? 0 : 1;
        bad_out += ok ? 0 : 1;
        peak = fmaxf(peak, fabsf(y));
        yp[j] = y;
      }
    }
    if (ch + 1 < nchunk) stage((ch + 1) & 1);
    __syncthreads();
    if (ROWS) {                                                    // thread tid stores column lcol of the lanes 2 i + lrow
      const int r = q0 + lcol;                                     // sample of the step
#pragma unroll
      for (int i = 0; i < EQC_LANES / 2; ++i) {
        const long o = (long)(t0 + 2 * i + lrow) * S + r;          // sample of the job's steps
        if (o < cnt) out[off + o] = ys[(2 * i + lrow) * EQC_STRIDE + lcol];
      }
      __syncthreads();                                             // ys is written again by the next chunk
    }
  }
  if (!ROWS) {
    if (my < nst) {
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        ftab[(st0 + my) * D + 2 * s] = s1[s];
        ftab[(st0 + my) * D + 2 * s + 1] = s2[s];
      }
    }
    return;
  }
  if ((tb[4] & EQC_LAST) && my == nst - 1) {                       // the state behind the row's last sample
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      sout[(long)blockIdx.y * D + 2 * s] = s1[s];
      sout[(long)blockIdx.y * D + 2 * s + 1] = s2[s];
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    bad_in += __shfl_xor(bad_in, m);
    bad_out += __shfl_xor(bad_out, m);
    peak = fmaxf(peak, __shfl_xor(peak, m));
  }
  if (tid == 0) {
    int* r = rec + ((long)tb[3] + blockIdx.x) * EQC_REC;
    r[0] = bad_in; r[1] = bad_out; r[2] = (int)__float_as_uint(peak); r[3] = 0;
  }
}

// the double of lane `lane` (a constant) to every lane of the wavefront
__device__ inline double eqc_lane(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// f + (m[0] z_0 + m[1] z_1 + ..) in eq_carry_dot's order, z_k from lane k
template <int D>
__device__ inline double eqc_dot(const double (&m)[D], double z, double f) {
  VX_EQ_NO_CONTRACT
  double acc = m[0] * eqc_lane(z, 0);
#pragma unroll
  for (int k = 1; k < D; ++k) acc = acc + m[k] * eqc_lane(z, k);
  return f + acc;
}

// grid (job), one wavefront: z_0 from the job's row of z0 (carry slot `rslot` for a job that continues a cut row), z_j -> row
// st_off + j of ztab for j < the job's steps, the last z of a cut job -> carry slot `wslot`.  The two slots alternate with the launch
// (eq_carry_host.h), so the continuation and the cut that one launch can hold, workgroups in no order, never meet in a slot.  The
// lanes behind D repeat component D - 1 and write nothing.
template <int NS>
__global__ __launch_bounds__(EQC_LANES) void eq_carry_chain_kernel(const int* __restrict__ tab, const double* __restrict__ M, const double* __restrict__ ftab,
                                                                   double* __restrict__ ztab, const double* __restrict__ z0tab, double* carry) {
  constexpr int S = EQC_S, D = 2 * NS;
  const int* tb = tab + blockIdx.x * RS_TAB;
  const int cnt = tb[1], nst = (cnt + S - 1) / S, flags = tb[4];
  const int lane = threadIdx.x, i = lane < D ? lane : D - 1;
  double m[D];
#pragma unroll
  for (int k = 0; k < D; ++k) m[k] = M[i * D + k];
  double z = (flags & EQC_CONT) ? carry[tb[5] * EQC_DMAX + i] : z0tab[(long)blockIdx.x * D + i];
  const double* fp = ftab + (long)tb[2] * D + i;
  double* zp = ztab + (long)tb[2] * D + i;
  double fb[EQC_PF];
#pragma unroll
  for (int u = 0; u < EQC_PF; ++u) fb[u] = u < nst ? fp[(long)u * D] : 0.0;
  for (int j0 = 0; j0 < nst; j0 += EQC_PF) {
    double fc[EQC_PF];
#pragma unroll
    for (int u = 0; u < EQC_PF; ++u) {
      fc[u] = fb[u];
      const int j = j0 + EQC_PF + u;
      fb[u] = j < nst ? fp[(long)j * D] : 0.0;                     // eight steps ahead of their use
    }
#pragma unroll
    for (int u = 0; u < EQC_PF; ++u) {
      if (j0 + u >= nst) break;                                    // wave-uniform
      if (lane < D) zp[(long)(j0 + u) * D] = z;
      z = eqc_dot<D>(m, z, fc[u]);
    }
  }
  if ((flags & EQC_CUT) && lane < D) carry[tb[6] * EQC_DMAX + i] = z;
}

using EqcKernel = void (*)(const float*, const int*, float*, int*, double*, const double*, double*, EqcCoef);
using EqcChain = void (*)(const int*, const double*, const double*, double*, const double*, double*);
static const EqcKernel eqc_ends[EQ_MAX] = {eq_carry_kernel<1, false>, eq_carry_kernel<2, false>, eq_carry_kernel<3, false>, eq_carry_kernel<4, false>,
                                           eq_carry_kernel<5, false>, eq_carry_kernel<6, false>, eq_carry_kernel<7, false>, eq_carry_kernel<8, false>};
static const EqcKernel eqc_rows[EQ_MAX] = {eq_carry_kernel<1, true>, eq_carry_kernel<2, true>, eq_carry_kernel<3, true>, eq_carry_kernel<4, true>,
                                           eq_carry_kernel<5, true>, eq_carry_kernel<6, true>, eq_carry_kernel<7, true>, eq_carry_kernel<8, true>};
static const EqcChain eqc_chain[EQ_MAX] = {eq_carry_chain_kernel<1>, eq_carry_chain_kernel<2>, eq_carry_chain_kernel<3>, eq_carry_chain_kernel<4>,
                                           eq_carry_chain_kernel<5>, eq_carry_chain_kernel<6>, eq_carry_chain_kernel<7>, eq_carry_chain_kernel<8>};

}  // namespace vxe

extern "C" {

int vx_eq_carry_plan(const double* sections, int32_t nsections, double* m, int32_t* step) {
  char why[240];
  int32_t w = 0, s = 0;
  // vx_eq_last_error reads the message eq.hip keeps per thread, and only its two host entries write it: a refusal here is recorded by
  // putting the same question to vx_eq_plan, which fails the same first checks (a NULL argument, eq_check_sections) in its own words
  if (!sections || !m || !step) { vx_eq_plan(nullptr, nsections, &w, &s); return VX_EINVAL; }
  if (vxe::eq_carry_matrix(sections, nsections, vxe::EQC_S, m, why, sizeof why)) { vx_eq_plan(sections, nsections, &w, &s); return VX_EINVAL; }
  *step = vxe::EQC_S;
  return VX_OK;
}

int vx_eq_carry(vx_ctx* c, const float* wav, int64_t wav_stride, const int32_t* lens, int32_t batch, const double* sections, int32_t nsections,
                const double* state_in, float* out, int64_t out_stride, double* state_out, vx_eq_info* info) {
  using namespace vxe;
  if (!c) return VX_EINVAL;
  if (int e = wave_check_rows(c, "vx_eq_carry", wav, wav_stride, lens, batch)) return e;
  if (!sections) FAIL(VX_EINVAL, "vx_eq_carry: sections is NULL");
  if (!out) FAIL(VX_EINVAL, "vx_eq_carry: out is NULL");
  if (!info) FAIL(VX_EINVAL, "vx_eq_carry: info is NULL");
  if (int e = wave_check_out_stride(c, "vx_eq_carry", lens, batch, out_stride, "")) return e;
  char why[240];
  if (eq_check_sections(sections, nsections, why, sizeof why)) FAIL(VX_EINVAL, "vx_eq_carry: %s", why);
  const int D = 2 * nsections, S = EQC_S;
  if (eq_carry_check_state(state_in, batch, D, why, sizeof why)) FAIL(VX_EINVAL, "vx_eq_carry: %s", why);
  if (g_eqc_last.n != nsections || memcmp(g_eqc_last.sec, sections, (size_t)nsections * 5 * sizeof(double))) {
    g_eqc_last.n = 0;
    if (eq_carry_matrix(sections, nsections, S, g_eqc_last.m, why, sizeof why)) FAIL(VX_EINVAL, "vx_eq_carry: %s", why);
    memcpy(g_eqc_last.sec, sections, (size_t)nsections * 5 * sizeof(double));
    g_eqc_last.n = nsections;
  }
  const long win = wave_window(c->eq_window, VX_EQ_WINDOW);
  std::vector<EqCarryJob> jobs;
  if (!eq_carry_plan(lens, batch, S, win, RS_MAX_JOBS, &jobs)) FAIL(VX_EINVAL, "vx_eq_carry: the launch window of %ld samples is below a step of %d", win, S);
  HIPCHK(hipSetDevice(c->dev));
  if (int e = rs_buffers(c)) return e;
  for (int i = 0; i < batch; ++i) {
    info[i] = {0, 0, 0, 0.f};
    for (int d = 0; state_out && d < D; ++d) state_out[(long)i * D + d] = state_in ? state_in[(long)i * D + d] : 0.0;      // a row of length 0
  }
  EqcCoef k;
  memset(&k, 0, sizeof k);
  memcpy(k.c, sections, (size_t)nsections * 5 * sizeof(double));
  double* base = reinterpret_cast<double*>(c->rs_out + RS_IN_CAP);
  int* rec = reinterpret_cast<int*>(base + EQC_RECS);
  std::vector<int> tab, recs;
  std::vector<double> z0, sout;
  return wave_launches(c, jobs, [&](size_t j0, size_t j1) -> int {
    tab.clear();
    z0.assign((j1 - j0) * (size_t)D, 0.0);
    long max_st = 0, nrec = 0, nst = 0;
    int rd = -1, wr = -1;                                           // the carry slots this launch reads and writes
    for (size_t q = j0; q < j1; ++q) {
      const EqCarryJob& j = jobs[q];
      for (long v : {j.off, j.cnt, j.st_off, j.rec_off, (long)(j.cont * EQC_CONT + j.cut * EQC_CUT + j.last * EQC_LAST), (long)j.rslot, (long)j.wslot, 0L}) tab.push_back((int)v);
      if (j.cont) rd = j.rslot;
      if (j.cut) wr = j.wslot;
      max_st = std::max(max_st, eq_nsteps(j.cnt, S));
      nst = j.st_off + eq_nsteps(j.cnt, S);
      nrec = j.rec_off + eq_ntiles(j.cnt, S);
      if (state_in && !j.cont) memcpy(z0.data() + (q - j0) * (size_t)D, state_in + (long)j.row * D, (size_t)D * sizeof(double));
      H2D(c->rs_in + j.off, wav + (long)j.row * wav_stride + j.j0 * S, (size_t)j.cnt * sizeof(float));
    }
    if (rd >= 0 && rd == wr) FAIL(VX_EINVAL, "vx_eq_carry: launch %d reads and writes carry slot %d", jobs[j0].launch, rd);      // the planner rules it out
    if (nst > EQC_ST_CAP || nrec > EQC_REC_CAP)                     // the window rules it out
      FAIL(VX_EINVAL, "vx_eq_carry: %ld steps, %ld tiles in one launch exceed the tables of %ld, %ld", nst, nrec, EQC_ST_CAP, EQC_REC_CAP);
    H2D(c->rs_meta, tab.data(), tab.size() * sizeof(int));
    H2D(base + EQC_Z0, z0.data(), z0.size() * sizeof(double));
    if (j0 == 0) H2D(base + EQC_M, g_eqc_last.m, (size_t)D * D * sizeof(double));
    const dim3 grid((unsigned)((max_st + EQC_LANES - 1) / EQC_LANES), (unsigned)(j1 - j0));
    hipLaunchKernelGGL(eqc_ends[nsections - 1], grid, dim3(EQC_LANES), 0, c->stream, c->rs_in, c->rs_meta, c->rs_out, rec, base + EQC_F, base + EQC_Z,
                       base + EQC_SOUT, k);
    hipLaunchKernelGGL(eqc_chain[nsections - 1], dim3((unsigned)(j1 - j0)), dim3(EQC_LANES), 0, c->stream, c->rs_meta, base + EQC_M, base + EQC_F,
                       base + EQC_Z, base + EQC_Z0, base + EQC_CARRY);
    hipLaunchKernelGGL(eqc_rows[nsections - 1], grid, dim3(EQC_LANES), 0, c->stream, c->rs_in, c->rs_meta, c->rs_out, rec, base + EQC_F, base + EQC_Z,
                       base + EQC_SOUT, k);
    for (size_t q = j0; q < j1; ++q) {
      const EqCarryJob& j = jobs[q];
      D2H(out + (long)j.row * out_stride + j.j0 * S, c->rs_out + j.off, (size_t)j.cnt * sizeof(float));
    }
    recs.resize((size_t)nrec * EQC_REC);
    D2H(recs.data(), rec, recs.size() * sizeof(int));
    sout.resize((j1 - j0) * (size_t)D);
    if (state_out) D2H(sout.data(), base + EQC_SOUT, sout.size() * sizeof(double));
    return VX_OK;
  }, [&](size_t j0, size_t j1) -> int {
    for (size_t q = j0; q < j1; ++q) {
      const EqCarryJob& j = jobs[q];
      vx_eq_info& w = info[j.row];
      for (long t = 0; t < eq_ntiles(j.cnt, S); ++t) {
        const int* r = recs.data() + (size_t)(j.rec_off + t) * EQC_REC;
        float p;
        memcpy(&p, r + 2, sizeof p);
        w.nonfinite += r[0];
        w.nonfinite_out += r[1];
        w.peak = std::max(w.peak, p);
      }
      if (state_out && j.last) memcpy(state_out + (long)j.row * D, sout.data() + (q - j0) * (size_t)D, (size_t)D * sizeof(double));
    }
    return VX_OK;
  });
}

}  // extern "C"
