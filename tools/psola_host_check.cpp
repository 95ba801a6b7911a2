// Stand-alone run of the formant-preserving pitch shift's host code (vall-e-x_amd/csrc/psola_host.h: option checking, period lookup,
// synthesis marks and grain table, gap count, launch planner, the sequential reference of the contract) on a CPU:
//   c++ -std=c++17 -O1 -g -Wall -Wextra -Werror -fsanitize=address,undefined tools/psola_host_check.cpp -o psola_host_check
//   psola_host_check opts HOP PMIN PMAX U RATIO_Q16          "ok", or the refusal (exit code 3)
//   psola_host_check plan HOP PMIN PMAX U WIN MARK_CAP GRAIN_CAP LAG_CAP MAX_JOBS L ...
//                                                one row per line: launch row in_off lag_off m_off g_off;
//                                                exit code 3 and a message when a row does not fit an empty launch
//   psola_host_check ref HOP PMIN PMAX U RATIO_Q16 PER_FRAME IN LAG OUT
//                                                IN: the row as raw fp32; LAG: its lags as raw int32, followed by as many Q16 ratios
//                                                when PER_FRAME is 1; OUT: vx_psola_info, the marks [N + 1] int32, the costs [N + 1]
//                                                doubles, the grains [J][4] int32, the output [L] fp32, all raw
// tests/test_psola_host.py compares all of it with the numpy restatement of the contract (tests/_psola_refs.py).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../vall-e-x_amd/csrc/psola_host.h"

static vx_psola_opts opts_from(char** a, const char* ratio) {     // HOP PMIN PMAX U
  vx_psola_opts o;
  memset(&o, 0, sizeof o);
  o.struct_size = sizeof o;
  o.hop = atoi(a[0]); o.period_min = atoi(a[1]); o.period_max = atoi(a[2]); o.unvoiced_period = atoi(a[3]);
  o.ratio_q16 = atoi(ratio);
  return o;
}

template <class T>
static bool put(FILE* f, const std::vector<T>& v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

template <class T>
static bool get(const char* path, std::vector<T>* v) {
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot read %s\n", path); return false; }
  T buf[1024];
  for (size_t n; (n = fread(buf, sizeof(T), 1024, f)) > 0;) v->insert(v->end(), buf, buf + n);
  fclose(f);
  return true;
}

int main(int argc, char** argv) {
  using namespace vxe;
  const char* cmd = argc > 1 ? argv[1] : "";
  char why[160];
  if (!strcmp(cmd, "opts") && argc == 7) {
    const vx_psola_opts o = opts_from(argv + 2, argv[6]);
    if (ps_check_opts(o, why, sizeof why)) { printf("%s\n", why); return 3; }
    printf("ok\n");
    return 0;
  }
  if (!strcmp(cmd, "plan") && argc >= 11) {
    const vx_psola_opts o = opts_from(argv + 2, "65536");
    if (ps_check_opts(o, why, sizeof why)) { fprintf(stderr, "bad options: %s\n", why); return 2; }
    std::vector<int> lens;
    for (int i = 11; i < argc; ++i) {
      const long L = atol(argv[i]);
      if (L < 0 || L > 0x7fffffffL) { fprintf(stderr, "bad length %s\n", argv[i]); return 2; }
      lens.push_back((int)L);
    }
    std::vector<PsJob> jobs;
    if (!ps_plan(ps_geometry(o), lens.data(), (int)lens.size(), atol(argv[6]), atol(argv[7]), atol(argv[8]), atol(argv[9]), atol(argv[10]),
                 &jobs)) {
      fprintf(stderr, "a row does not fit an empty launch\n");
      return 3;
    }
    for (const PsJob& j : jobs) printf("%d %d %ld %ld %ld %ld\n", j.launch, j.row, j.in_off, j.lag_off, j.m_off, j.g_off);
    return 0;
  }
  if (!strcmp(cmd, "ref") && argc == 11) {
    const vx_psola_opts o = opts_from(argv + 2, argv[6]);
    if (ps_check_opts(o, why, sizeof why)) { fprintf(stderr, "bad options: %s\n", why); return 2; }
    const PsGeom g = ps_geometry(o);
    const bool per_frame = atoi(argv[7]) != 0;
    std::vector<float> x;
    std::vector<int32_t> lr;
    if (!get(argv[8], &x) || !get(argv[9], &lr)) return 2;
    const long L = (long)x.size(), Mf = ps_frames(g, L);
    if ((long)lr.size() != (per_frame ? 2 : 1) * Mf) { fprintf(stderr, "%zu lag words for %ld frames\n", lr.size(), Mf); return 2; }
    for (long k = Mf; k < (long)lr.size(); ++k)
      if (lr[(size_t)k] < PS_RATIO_MIN || lr[(size_t)k] > PS_RATIO_MAX) { fprintf(stderr, "ratio %d out of range\n", lr[(size_t)k]); return 3; }
    lr.push_back(0);                                               // data() of an empty row stays a pointer
    std::vector<int32_t> marks;
    std::vector<double> cost;
    std::vector<PsGrain> grains;
    std::vector<float> out((size_t)L);
    vx_psola_info info;
    psola_reference(g, x.data(), L, lr.data(), per_frame ? lr.data() + Mf : nullptr, &marks, &cost, &grains, out.data(), &info);
    if (info.gaps != ps_gaps(grains, L)) { fprintf(stderr, "gaps: %d by the samples, %d by the intervals\n", info.gaps, ps_gaps(grains, L)); return 4; }
    FILE* fo = fopen(argv[10], "wb");
    if (!fo) { fprintf(stderr, "cannot write %s\n", argv[10]); return 2; }
    const bool ok = fwrite(&info, sizeof info, 1, fo) == 1 && put(fo, marks) && put(fo, cost) && put(fo, grains) && put(fo, out);
    return fclose(fo) == 0 && ok ? 0 : 2;
  }
  fprintf(stderr, "usage: %s opts | plan | ref ... (see the head of tools/psola_host_check.cpp)\n", argv[0]);
  return 2;
}
