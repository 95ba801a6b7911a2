// Stand-alone run of the limiter's host code (vall-e-x_amd/csrc/limit_host.h: option checking, detector taps, ceiling, gain, launch
// planner, the sequential reference of the contract) on a CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/limit_host_check.cpp -o limit_host_check
//   limit_host_check opts PRE_GAIN CEILING_DB LOOKAHEAD OVERSAMPLE   "ok", or the refusal (exit code 3)
//   limit_host_check taps N                                          "width K", then the n * 15 taps, one hex word of a float per line
//   limit_host_check ref PRE_GAIN(hex float) CEILING_DB WN N L  < samples
//                                                                    the row on standard input, one hex float per line; prints
//                                                                    "ceiling(hex) peak(hex) min_gain(hex) reduced nonfinite", then
//                                                                    one line "out P g" (hex floats) per sample
//   limit_host_check gain LOUDNESS(hex double) TARGET_LUFS MAX_GAIN_DB   the gain of vx_finish_limited, a hex float
//   limit_host_check plan WN WIN MAX_JOBS TILE L ...                 one part per line: launch row s cnt hl hr off out_off rec_off
//                                                                    (exit code 3: the window cannot hold two halos and a sample)
// tests/test_limit_host.py compares all of it with the numpy restatement of the contract (tests/_limit_refs.py).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../vall-e-x_amd/csrc/limit_host.h"

static unsigned fbits(float v) {
  uint32_t w;
  memcpy(&w, &v, 4);
  return (unsigned)w;
}

static float fword(const char* s) {
  const uint32_t w = (uint32_t)strtoul(s, nullptr, 16);
  float v;
  memcpy(&v, &w, 4);
  return v;
}

int main(int argc, char** argv) {
  using namespace vxe;
  const char* cmd = argc > 1 ? argv[1] : "";
  char why[160];
  if (!strcmp(cmd, "opts") && argc == 6) {
    vx_limit_opts o;
    o.struct_size = sizeof o;
    o.lookahead = atoi(argv[4]); o.oversample = atoi(argv[5]);
    if (lm_check_opts(o, strtof(argv[2], nullptr), strtof(argv[3], nullptr), why, sizeof why)) { printf("%s\n", why); return 3; }
    printf("ok\n");
    return 0;
  }
  if (!strcmp(cmd, "taps") && argc == 3) {
    std::vector<float> t;
    if (!lm_taps(atoi(argv[2]), t)) { printf("oversample %d is not one of 1, 2, 4, 8\n", atoi(argv[2])); return 3; }
    printf("%d %d\n", LM_WIDTH, LM_K);
    for (float v : t) printf("%08x\n", fbits(v));
    return 0;
  }
  if (!strcmp(cmd, "ref") && argc == 7) {
    vx_limit_opts o;
    o.struct_size = sizeof o;
    o.lookahead = atoi(argv[4]); o.oversample = atoi(argv[5]);
    const float gs = fword(argv[2]), db = strtof(argv[3], nullptr);
    const long L = atol(argv[6]);
    if (L < 0 || lm_check_opts(o, gs, db, why, sizeof why)) { fprintf(stderr, "bad arguments\n"); return 2; }
    std::vector<float> x((size_t)L), out((size_t)L), P((size_t)L), g((size_t)L), t;
    for (float& v : x) {
      char word[32];
      if (scanf("%31s", word) != 1) { fprintf(stderr, "short row\n"); return 2; }
      v = fword(word);
    }
    lm_taps(o.oversample, t);
    const float c = lm_ceiling(db);
    LmInfo info;
    lm_row_reference(x.data(), L, gs, c, o.lookahead, o.oversample, t.data(), out.data(), P.data(), g.data(), &info);
    printf("%08x %08x %08x %d %d\n", fbits(c), fbits(info.peak), fbits(info.min_gain), info.reduced, info.nonfinite);
    for (long i = 0; i < L; ++i) printf("%08x %08x %08x\n", fbits(out[(size_t)i]), fbits(P[(size_t)i]), fbits(g[(size_t)i]));
    return 0;
  }
  if (!strcmp(cmd, "gain") && argc == 5) {
    const uint64_t w = strtoull(argv[2], nullptr, 16);
    double loud;
    memcpy(&loud, &w, 8);
    printf("%08x\n", fbits(lm_gain(loud, strtof(argv[3], nullptr), strtof(argv[4], nullptr))));
    return 0;
  }
  if (!strcmp(cmd, "plan") && argc >= 6) {
    std::vector<long> len;
    for (int i = 6; i < argc; ++i) {
      const long n = atol(argv[i]);
      if (n < 0) { fprintf(stderr, "bad length %s\n", argv[i]); return 2; }
      len.push_back(n);
    }
    std::vector<LmJob> jobs;
    if (!lm_plan(len.data(), (int)len.size(), atoi(argv[2]), atol(argv[3]), atol(argv[4]), atoi(argv[5]), &jobs)) {
      fprintf(stderr, "the window cannot hold two halos and a sample\n");
      return 3;
    }
    for (const LmJob& j : jobs)
      printf("%d %d %ld %ld %ld %ld %ld %ld %ld\n", j.launch, j.row, j.s, j.cnt, j.hl, j.hr, j.off, j.out_off, j.rec_off);
    return 0;
  }
  fprintf(stderr, "usage: %s opts | taps | ref | gain | plan ... (see the head of tools/limit_host_check.cpp)\n", argv[0]);
  return 2;
}
