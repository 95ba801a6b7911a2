// Stand-alone run of the pitch tracker's host code (vall-e-x_amd/csrc/f0_host.h: option checking, frame geometry, launch planner,
// summary, the sequential reference of the contract) on a CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/f0_host_check.cpp -o f0_host_check
//   f0_host_check opts RATE HOP WINDOW LAG_MIN LAG_MAX THRESHOLD    "ok", or the refusal (exit code 3)
//   f0_host_check geom RATE HOP WINDOW LAG_MIN LAG_MAX L K ...      "M reach" and then s_K for every K given, one per line
//   f0_host_check plan RATE HOP WINDOW LAG_MIN LAG_MAX WIN FRAME_CAP MAX_JOBS L ...
//                                                one job per line: launch row k0 k1 s_lo s_hi in_off f_off;
//                                                exit code 3 and a message when one frame does not fit an empty launch
//   f0_host_check ref RATE HOP WINDOW LAG_MIN LAG_MAX THRESHOLD IN OUT
//                                                IN: the row as raw fp32; OUT: f0 [M] fp32, lag [M] int32, ap [M] fp32, d and d'
//                                                [M][LAG_MAX + 1] doubles, then vx_f0_info, all raw
// tests/test_f0_host.py compares all of it with the numpy restatement of the contract (tests/_f0_refs.py).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../vall-e-x_amd/csrc/f0_host.h"

static vx_f0_opts opts_from(char** a, const char* thr) {     // RATE HOP WINDOW LAG_MIN LAG_MAX
  vx_f0_opts o;
  memset(&o, 0, sizeof o);
  o.struct_size = sizeof o;
  o.sample_rate = atoi(a[0]); o.hop = atoi(a[1]); o.window = atoi(a[2]); o.lag_min = atoi(a[3]); o.lag_max = atoi(a[4]);
  o.threshold = strtof(thr, nullptr);
  return o;
}

template <class T>
static bool put(FILE* f, const std::vector<T>& v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char** argv) {
  using namespace vxe;
  const char* cmd = argc > 1 ? argv[1] : "";
  char why[160];
  if (!strcmp(cmd, "opts") && argc == 8) {
    const vx_f0_opts o = opts_from(argv + 2, argv[7]);
    if (f0_check_opts(o, why, sizeof why)) { printf("%s\n", why); return 3; }
    printf("ok\n");
    return 0;
  }
  if (!strcmp(cmd, "geom") && argc >= 8) {
    const vx_f0_opts o = opts_from(argv + 2, "0.15");
    const long L = atol(argv[7]);
    if (L < 0 || f0_check_opts(o, why, sizeof why)) { fprintf(stderr, "bad options\n"); return 2; }
    const F0Geom g = f0_geometry(o);
    printf("%ld %ld\n", f0_frames(g, L), f0_reach(g));
    for (int i = 8; i < argc; ++i) printf("%ld\n", f0_first(g, atol(argv[i])));
    return 0;
  }
  if (!strcmp(cmd, "plan") && argc >= 10) {
    const vx_f0_opts o = opts_from(argv + 2, "0.15");
    if (f0_check_opts(o, why, sizeof why)) { fprintf(stderr, "bad options: %s\n", why); return 2; }
    std::vector<int> lens;
    for (int i = 10; i < argc; ++i) {
      const long L = atol(argv[i]);
      if (L < 0 || L > 0x7fffffffL) { fprintf(stderr, "bad length %s\n", argv[i]); return 2; }
      lens.push_back((int)L);
    }
    std::vector<F0Job> jobs;
    if (!f0_plan(f0_geometry(o), lens.data(), (int)lens.size(), atol(argv[7]), atol(argv[8]), atol(argv[9]), &jobs)) {
      fprintf(stderr, "no frame fits an empty launch\n");
      return 3;
    }
    for (const F0Job& j : jobs) printf("%d %d %ld %ld %ld %ld %ld %ld\n", j.launch, j.row, j.k0, j.k1, j.s_lo, j.s_hi, j.in_off, j.f_off);
    return 0;
  }
  if (!strcmp(cmd, "ref") && argc == 10) {
    const vx_f0_opts o = opts_from(argv + 2, argv[7]);
    if (f0_check_opts(o, why, sizeof why)) { fprintf(stderr, "bad options: %s\n", why); return 2; }
    const F0Geom g = f0_geometry(o);
    FILE* fi = fopen(argv[8], "rb");
    if (!fi) { fprintf(stderr, "cannot read %s\n", argv[8]); return 2; }
    std::vector<float> x;
    float buf[1024];
    for (size_t n; (n = fread(buf, sizeof(float), 1024, fi)) > 0;) x.insert(x.end(), buf, buf + n);
    fclose(fi);
    const long L = (long)x.size(), M = f0_frames(g, L);
    std::vector<float> f((size_t)M), ap((size_t)M);
    std::vector<int32_t> lag((size_t)M);
    std::vector<double> d((size_t)(M * (g.T + 1))), dp((size_t)(M * (g.T + 1)));
    f0_reference(g, x.data(), L, f.data(), lag.data(), ap.data(), d.data(), dp.data());
    vx_f0_info info;
    f0_summary(f.data(), lag.data(), M, f0_nonfinite(x.data(), L), &info);
    FILE* fo = fopen(argv[9], "wb");
    if (!fo) { fprintf(stderr, "cannot write %s\n", argv[9]); return 2; }
    const bool ok = put(fo, f) && put(fo, lag) && put(fo, ap) && put(fo, d) && put(fo, dp) && fwrite(&info, sizeof info, 1, fo) == 1;
    return fclose(fo) == 0 && ok ? 0 : 2;
  }
  fprintf(stderr, "usage: %s opts | geom | plan | ref ... (see the head of tools/f0_host_check.cpp)\n", argv[0]);
  return 2;
}
