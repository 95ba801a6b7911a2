// Host side of the carried-state equaliser (eq_carry.hip, vx_eq_carry / vx_eq_carry_plan): the step matrix M of a cascade, the launch
// planner and a sequential reference of the whole contract for one row -- the three passes (ends, chain, rows) in plain C++.
// Plain C++17 without the GPU runtime, so a stand-alone program (tools/eq_carry_host_check.cpp) runs exactly this code on a CPU --
// against the numpy restatement of the contract (tests/_eq_carry_refs.py), through the planner's invariants, under a sanitizer.
// Sections, checks and the per-sample recursion are eq_host.h's; the chain's sum is compiled with contraction off, here and in the
// kernel.
#pragma once

#include "eq_host.h"

namespace vxe {

constexpr int EQC_S = VX_EQ_CARRY_STEP;          // samples of a step
constexpr int EQC_DMAX = 2 * EQ_MAX;             // state doubles of the longest cascade
static_assert(EQC_S >= 32 && EQC_S % 32 == 0, "the kernels walk chunks of 32 samples: Sc is a multiple");

// z_{j+1}[i] of the chain: f + (M[i][0] z[0] + M[i][1] z[1] + ..), summed in this order, every operation rounded on its own
VX_EQ_HD VX_EQ_NO_CONTRACT_FN inline double eq_carry_dot(const double* mrow, const double* z, int D, double f) {
  VX_EQ_NO_CONTRACT
  double acc = mrow[0] * z[0];
  for (int k = 1; k < D; ++k) acc = acc + mrow[k] * z[k];
  return f + acc;
}

// S zero inputs through the cascade from the state z [2 n], in place
VX_EQ_NO_CONTRACT_FN inline void eq_carry_run_zeros(const double* sec, int n, int S, double* z) {
  for (int q = 0; q < S; ++q) {
    double u = 0.0;
    for (int k = 0; k < n; ++k) u = eq_section(sec + 5 * k, u, z[2 * k], z[2 * k + 1]);
  }
}

// M [2 n][2 n] of a cascade at step S.  nullptr; else the message (eq_check_sections' included)
inline const char* eq_carry_matrix(const double* sec, int n, int S, double* m, char* buf, size_t nbuf) {
  if (eq_check_sections(sec, n, buf, nbuf)) return buf;
  const int D = 2 * n;
  for (int k = 0; k < D; ++k) {
    double z[EQC_DMAX] = {0};
    z[k] = 1.0;
    eq_carry_run_zeros(sec, n, S, z);
    for (int i = 0; i < D; ++i) {
      if (!(fabs(z[i]) <= DBL_MAX)) { snprintf(buf, nbuf, "the step matrix M[%d][%d] of this cascade is not finite", i, k); return buf; }
      m[i * D + k] = z[i];
    }
  }
  return nullptr;
}

// nullptr, or the message: an entry of state [batch][D] that is not finite
inline const char* eq_carry_check_state(const double* state, int batch, int D, char* buf, size_t nbuf) {
  for (long i = 0; state && i < (long)batch * D; ++i)
    if (!(fabs(state[i]) <= DBL_MAX)) { snprintf(buf, nbuf, "state_in of row %ld: component %ld is not finite", i / D, i % D); return buf; }
  return nullptr;
}

// The planner.  A job is a run of consecutive steps [j0, j0 + ceil(cnt / S)) of one row.  A launch holds at most `win` samples and
// `max_jobs` jobs; rows are packed greedily in order, a row that does not fit is cut at a step: the later part has `cont` set (its
// z_0 is the chain's last z of the part before, which is then the last job of its launch and has `cut` set).  `last`: the job holds
// the row's last sample.  A row of length 0 has no job.  Only a row's last job has a step that is not full, so a launch has at most
// win / S + max_jobs steps.
// The handed-over z lies in one of TWO carry slots on the device: a cut job writes slot `wslot` = launch & 1, its continuation, the
// first job of the next launch, reads `rslot` = the other one.  One launch can hold both a continuation (its first job) and a cut (its
// last), in workgroups that run in no order: they never touch the same slot.
struct EqCarryJob {
  int launch, row;
  long j0;               // first step of the job in its row
  long cnt;              // the job's samples: row samples [j0 S, j0 S + cnt)
  long off;              // first sample of the job in the launch's input and output buffers
  long st_off;           // first step of the job in the launch's step tables
  long rec_off;          // first tile record of the job in the launch's record table
  int cont, cut, last;
  int rslot, wslot;      // carry slot a `cont` job reads, a `cut` job writes
};

inline bool eq_carry_plan(const int32_t* lens, int batch, int S, long win, long max_jobs, std::vector<EqCarryJob>* jobs) {
  jobs->clear();
  if (S < 1 || win < S || max_jobs < 1) return false;                  // one step fits an empty launch
  int launch = 0;
  long used = 0, sused = 0, rused = 0, njobs = 0;
  for (int i = 0; i < batch; ++i) {
    const long n = lens[i];
    long s = 0;                                                        // a multiple of S
    while (s < n) {
      const long room = win - used, rest = n - s;
      const long take = rest <= room ? rest : room / S * S;
      if (take <= 0 || njobs == max_jobs) {                            // nothing more fits this launch
        ++launch;
        used = sused = rused = njobs = 0;
        continue;
      }
      jobs->push_back({launch, i, s / S, take, used, sused, rused, s > 0, s + take < n, s + take == n, (launch & 1) ^ 1, launch & 1});
      used += take;
      sused += eq_nsteps(take, S);
      rused += eq_ntiles(take, S);
      ++njobs;
      s += take;
    }
  }
  return true;
}

// The whole contract for one row, pass after pass: out [L]; state_in [2 n] or nullptr (rest); state_out [2 n] or nullptr
VX_EQ_NO_CONTRACT_FN inline void eq_carry_reference(const float* x, long L, const double* sec, int n, const double* m, int S, const double* state_in,
                                                    float* out, double* state_out, vx_eq_info* info) {
  const int D = 2 * n;
  const long J = eq_nsteps(L, S);
  info->warm = 0; info->nonfinite = 0; info->nonfinite_out = 0; info->peak = 0.f;
  std::vector<double> z((size_t)(J + 1) * D, 0.0);                     // z_0 .. z_J; f_j is written into the place of z_{j+1} first
  for (int i = 0; state_in && i < D; ++i) z[(size_t)i] = state_in[i];
  for (long j = 0; j < J; ++j) {                                       // ends
    double* f = z.data() + (size_t)(j + 1) * D;
    for (long i = j * S; i < (j + 1) * S; ++i) {
      const float xf = i < L ? x[i] : 0.f;
      double u = xf - xf == 0.f ? (double)xf : 0.0;
      for (int k = 0; k < n; ++k) u = eq_section(sec + 5 * k, u, f[2 * k], f[2 * k + 1]);
    }
  }
  for (long j = 0; j < J; ++j) {                                       // chain
    const double* zj = z.data() + (size_t)j * D;
    double* zn = z.data() + (size_t)(j + 1) * D;
    for (int i = 0; i < D; ++i) zn[i] = eq_carry_dot(m + i * D, zj, D, zn[i]);
  }
  double st[EQC_DMAX] = {0};
  for (int i = 0; i < D; ++i) st[i] = z[(size_t)i];                    // L == 0: state_out = state_in
  for (long j = 0; j < J; ++j) {                                       // rows
    for (int i = 0; i < D; ++i) st[i] = z[(size_t)j * D + i];
    const long end = std::min<long>((j + 1) * S, L);
    for (long i = j * S; i < end; ++i) {
      const float xf = x[i];
      const bool fin = xf - xf == 0.f;
      double u = fin ? (double)xf : 0.0;
      for (int k = 0; k < n; ++k) u = eq_section(sec + 5 * k, u, st[2 * k], st[2 * k + 1]);
      float y = (float)u;
      if (!fin) ++info->nonfinite;
      if (!(y - y == 0.f)) { y = 0.f; ++info->nonfinite_out; }
      out[i] = y;
      info->peak = std::max(info->peak, fabsf(y));
    }
  }
  for (int i = 0; state_out && i < D; ++i) state_out[i] = st[i];
}

}  // namespace vxe
