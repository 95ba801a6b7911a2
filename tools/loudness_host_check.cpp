// Stand-alone run of the loudness host code (vall-e-x_amd/csrc/loudness_host.h: option checking, K-weighting coefficients, step-table
// reduction, gain, launch planner) on a CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/loudness_host_check.cpp -o loudness_host_check
//   loudness_host_check opts RATE TARGET_LUFS CEILING_DB      "ok", or the refusal (exit code 3)
//   loudness_host_check coeffs RATE                           the ten coefficients, one hex word of a double per line
//   loudness_host_check reduce RATE N NONFINITE TARGET_LUFS CEILING_DB MAX_GAIN_DB PEAK(hex float)  < step table
//                                                             the table on standard input, one hex double per line; prints
//                                                             "blocks above_abs gated nonfinite loudness(hex) mean_square(hex)
//                                                             max_momentary(hex) gain(hex)"
//   loudness_host_check plan RATE WIN MAX_JOBS LO:HI ...      one job per line: launch row j0 pre cnt off z_off (exit code 3: the
//                                                             window is below 3 S)
// tests/test_loudness_host.py compares all of it with the numpy restatement of the contract (tests/_loudness_refs.py).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../vall-e-x_amd/csrc/loudness_host.h"

static unsigned long long bits(double v) {
  uint64_t w;
  memcpy(&w, &v, 8);
  return (unsigned long long)w;
}

int main(int argc, char** argv) {
  using namespace vxe;
  const char* cmd = argc > 1 ? argv[1] : "";
  char why[160];
  if (!strcmp(cmd, "opts") && argc == 5) {
    vx_loudness_opts o;
    o.struct_size = sizeof o;
    o.sample_rate = atoi(argv[2]); o.target_lufs = strtof(argv[3], nullptr); o.ceiling_db = strtof(argv[4], nullptr);
    if (ln_check_opts(o, why, sizeof why)) { printf("%s\n", why); return 3; }
    printf("ok\n");
    return 0;
  }
  if (!strcmp(cmd, "coeffs") && argc == 3) {
    if (ln_check_rate(atoi(argv[2]), why, sizeof why)) { printf("%s\n", why); return 3; }
    double c[10];
    ln_coeffs(atoi(argv[2]), c);
    for (double v : c) printf("%016llx\n", bits(v));
    return 0;
  }
  if (!strcmp(cmd, "reduce") && argc == 9) {
    const int rate = atoi(argv[2]);
    const long n = atol(argv[3]);
    if (n < 0 || ln_check_rate(rate, why, sizeof why)) { fprintf(stderr, "bad arguments\n"); return 2; }
    const int S = ln_step(rate);
    std::vector<double> z((size_t)ln_nsteps(n, S));
    for (double& v : z) {
      unsigned long long w;
      if (scanf("%llx", &w) != 1) { fprintf(stderr, "short step table\n"); return 2; }
      const uint64_t w64 = w;
      memcpy(&v, &w64, 8);
    }
    vx_loudness_info li;
    ln_reduce(z.data(), n, S, atoi(argv[4]), &li);
    const uint32_t pw = (uint32_t)strtoul(argv[8], nullptr, 16);
    float peak;
    memcpy(&peak, &pw, 4);
    const float g = ln_gain(li.loudness, strtof(argv[5], nullptr), strtof(argv[6], nullptr), strtof(argv[7], nullptr), peak);
    uint32_t gw;
    memcpy(&gw, &g, 4);
    printf("%d %d %d %d %016llx %016llx %016llx %08x\n", li.blocks, li.above_abs, li.gated, li.nonfinite, bits(li.loudness),
           bits(li.mean_square), bits(li.max_momentary), gw);
    return 0;
  }
  if (!strcmp(cmd, "plan") && argc >= 5) {
    const int rate = atoi(argv[2]);
    if (ln_check_rate(rate, why, sizeof why)) { fprintf(stderr, "%s\n", why); return 2; }
    std::vector<long> lo, hi;
    for (int i = 5; i < argc; ++i) {
      long a = 0, b = 0;
      if (sscanf(argv[i], "%ld:%ld", &a, &b) != 2 || a < 0 || b < a) { fprintf(stderr, "bad span %s\n", argv[i]); return 2; }
      lo.push_back(a); hi.push_back(b);
    }
    std::vector<LnJob> jobs;
    if (!ln_plan(lo.data(), hi.data(), (int)lo.size(), ln_step(rate), atol(argv[3]), atol(argv[4]), &jobs)) {
      fprintf(stderr, "the window is below 3 S\n");
      return 3;
    }
    for (const LnJob& j : jobs) printf("%d %d %ld %ld %ld %ld %ld\n", j.launch, j.row, j.j0, j.pre, j.cnt, j.off, j.z_off);
    return 0;
  }
  fprintf(stderr, "usage: %s opts | coeffs | reduce | plan ... (see the head of tools/loudness_host_check.cpp)\n", argv[0]);
  return 2;
}
