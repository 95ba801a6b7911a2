// Stand-alone run of the time-stretch's host code (vall-e-x_amd/csrc/stretch_host.h: option checking, lengths, nominal positions,
// launch planner) on a CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/stretch_host_check.cpp -o stretch_host_check
//   stretch_host_check opts NUM DEN HOP SEARCH   "ok NUM' DEN'" (the speed over its gcd), or the refusal (exit code 3)
//   stretch_host_check geom NUM DEN HOP L K ...  "Lout M" and then n_K for every K given, one per line
//   stretch_host_check plan NUM DEN HOP SEARCH WIN OUT_CAP FRAME_CAP MAX_JOBS L ...
//                                                one job per line: launch row k0 k1 s_lo s_hi in_off out_off out_cnt f_off;
//                                                exit code 3 and a message when one frame does not fit an empty launch
// tests/test_stretch_host.py compares all of it with the numpy restatement of the contract (tests/_stretch_refs.py).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../vall-e-x_amd/csrc/stretch_host.h"

static vx_stretch_opts opts_from(char** a) {     // NUM DEN HOP SEARCH
  vx_stretch_opts o;
  memset(&o, 0, sizeof o);
  o.struct_size = sizeof o;
  o.speed_num = atoi(a[0]); o.speed_den = atoi(a[1]); o.hop = atoi(a[2]); o.search = atoi(a[3]);
  return o;
}

int main(int argc, char** argv) {
  using namespace vxe;
  const char* cmd = argc > 1 ? argv[1] : "";
  char why[160];
  if (!strcmp(cmd, "opts") && argc == 6) {
    const vx_stretch_opts o = opts_from(argv + 2);
    if (st_check_opts(o, why, sizeof why)) { printf("%s\n", why); return 3; }
    long n, d;
    st_reduce_speed(o.speed_num, o.speed_den, &n, &d);
    printf("ok %ld %ld\n", n, d);
    return 0;
  }
  if (!strcmp(cmd, "geom") && argc >= 6) {
    char* a[4] = {argv[2], argv[3], argv[4], (char*)"0"};
    const vx_stretch_opts o = opts_from(a);
    const long L = atol(argv[5]);
    if (L < 0 || st_check_opts(o, why, sizeof why)) { fprintf(stderr, "bad options\n"); return 2; }
    const StGeom g = st_geometry(o);
    printf("%ld %ld\n", st_out_len(g, L), st_frames(g, L));
    for (int i = 6; i < argc; ++i) printf("%ld\n", st_nominal(g, atol(argv[i])));
    return 0;
  }
  if (!strcmp(cmd, "plan") && argc >= 10) {
    const vx_stretch_opts o = opts_from(argv + 2);
    if (st_check_opts(o, why, sizeof why)) { fprintf(stderr, "bad options: %s\n", why); return 2; }
    std::vector<int> lens;
    for (int i = 10; i < argc; ++i) {
      const long L = atol(argv[i]);
      if (L < 0 || L > 0x7fffffffL) { fprintf(stderr, "bad length %s\n", argv[i]); return 2; }
      lens.push_back((int)L);
    }
    std::vector<StJob> jobs;
    if (!st_plan(st_geometry(o), lens.data(), (int)lens.size(), atol(argv[6]), atol(argv[7]), atol(argv[8]), atol(argv[9]), &jobs)) {
      fprintf(stderr, "no frame fits an empty launch\n");
      return 3;
    }
    for (const StJob& j : jobs)
      printf("%d %d %ld %ld %ld %ld %ld %ld %ld %ld\n", j.launch, j.row, j.k0, j.k1, j.s_lo, j.s_hi, j.in_off, j.out_off, j.out_cnt, j.f_off);
    return 0;
  }
  fprintf(stderr, "usage: %s opts | geom | plan ... (see the head of tools/stretch_host_check.cpp)\n", argv[0]);
  return 2;
}
