// Stand-alone run of the resampler's host code (vall-e-x_amd/csrc/resample_host.h: geometry, tap builder, window planner) on a CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/resample_host_check.cpp -o resample_host_check
//   resample_host_check taps ORIG NEW            geometry "o n width K" on the first line, then n * K taps, one hex word per line
//   resample_host_check plan ORIG NEW WIN OUT_CAP MAX_JOBS L0 L1 ...
//                                                one job per line: launch row a b s_lo s_hi in_off out_off out_cnt
// tests/test_resample_host.py compares the taps with the torch table word for word and checks the planner's invariants.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../vall-e-x_amd/csrc/resample_host.h"

int main(int argc, char** argv) {
  using namespace vxe;
  if (argc < 4) { fprintf(stderr, "usage: %s taps ORIG NEW | plan ORIG NEW WIN OUT_CAP MAX_JOBS L...\n", argv[0]); return 2; }
  const long orig = atol(argv[2]), neu = atol(argv[3]);
  if (orig <= 0 || neu <= 0) { fprintf(stderr, "rates must be positive\n"); return 2; }
  RsGeom g;
  const bool fits = rs_geometry(orig, neu, &g);
  if (!strcmp(argv[1], "taps")) {
    printf("%ld %ld %ld %ld\n", g.o, g.n, g.width, g.K);
    if (!fits) { fprintf(stderr, "more than %ld taps\n", RS_MAX_TAPS); return 3; }
    std::vector<float> t;
    rs_build_taps(g, t);
    for (float v : t) {
      uint32_t w;
      memcpy(&w, &v, 4);
      printf("%08x\n", w);
    }
    return 0;
  }
  if (!strcmp(argv[1], "plan") && argc >= 7 && fits) {
    std::vector<int> lens;
    for (int i = 7; i < argc; ++i) lens.push_back(atoi(argv[i]));
    std::vector<RsJob> jobs;
    if (!rs_plan(g, lens.data(), (int)lens.size(), atol(argv[4]), atol(argv[5]), atol(argv[6]), &jobs)) { fprintf(stderr, "no block fits an empty launch\n"); return 3; }
    for (const RsJob& j : jobs)
      printf("%d %d %ld %ld %ld %ld %ld %ld %ld\n", j.launch, j.row, j.a, j.b, j.s_lo, j.s_hi, j.in_off, j.out_off, j.out_cnt);
    return 0;
  }
  fprintf(stderr, "bad arguments\n");
  return 2;
}
