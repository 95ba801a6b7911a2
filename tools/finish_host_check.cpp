// Stand-alone run of the output stage's host code (vall-e-x_amd/csrc/finish_host.h: option checking, threshold, frame-table reduction,
// fade tables, launch planner) on a CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/finish_host_check.cpp -o finish_host_check
//   finish_host_check opts FRAME SILENCE_DB TRIM KEEP MODE LEVEL_DB MAX_GAIN_DB FADE_IN FADE_OUT FORMAT
//                                                "ok", or the refusal (exit code 3)
//   finish_host_check thr2 SILENCE_DB            the threshold, one hex word of a double
//   finish_host_check table N                    the N-sample fade table, one hex word per line
//   finish_host_check reduce FRAME SILENCE_DB TRIM KEEP MODE LEVEL_DB MAX_GAIN_DB L  < frame table
//                                                the table on standard input, one frame per line "e(hex double) p(hex float) z";
//                                                prints "begin end active_frames nonfinite peak(hex) gain(hex) mean_square(hex)"
//   finish_host_check plan WIN MAX_JOBS FRAME LO:HI ...
//                                                FRAME 0 = the apply pass; one job per line: launch row s_lo cnt off f_off
// tests/test_finish_host.py compares all of it with the numpy restatement of the contract (tests/_finish_refs.py).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../vall-e-x_amd/csrc/finish_host.h"

static vx_finish_opts opts_from(char** a) {      // FRAME SILENCE_DB TRIM KEEP MODE LEVEL_DB MAX_GAIN_DB
  vx_finish_opts o;
  memset(&o, 0, sizeof o);
  o.struct_size = sizeof o;
  o.frame = atoi(a[0]); o.silence_db = strtof(a[1], nullptr); o.trim = atoi(a[2]); o.keep = atoi(a[3]);
  o.level_mode = atoi(a[4]); o.level_db = strtof(a[5], nullptr); o.max_gain_db = strtof(a[6], nullptr);
  return o;
}

int main(int argc, char** argv) {
  using namespace vxe;
  const char* cmd = argc > 1 ? argv[1] : "";
  if (!strcmp(cmd, "opts") && argc == 12) {
    vx_finish_opts o = opts_from(argv + 2);
    o.fade_in = atoi(argv[9]); o.fade_out = atoi(argv[10]); o.format = atoi(argv[11]);
    char why[160];
    if (fn_check_opts(o, why, sizeof why)) { printf("%s\n", why); return 3; }
    printf("ok\n");
    return 0;
  }
  if (!strcmp(cmd, "thr2") && argc == 3) {
    const double t = fn_thr2(strtof(argv[2], nullptr));
    uint64_t w;
    memcpy(&w, &t, 8);
    printf("%016llx\n", (unsigned long long)w);
    return 0;
  }
  if (!strcmp(cmd, "table") && argc == 3) {
    const int n = atoi(argv[2]);
    if (n < 0 || n > FN_FADE_MAX) { fprintf(stderr, "table length outside 0 .. %d\n", FN_FADE_MAX); return 2; }
    std::vector<float> t;
    fn_fade_table(n, t);
    for (float v : t) {
      uint32_t w;
      memcpy(&w, &v, 4);
      printf("%08x\n", w);
    }
    return 0;
  }
  if (!strcmp(cmd, "reduce") && argc == 10) {
    const vx_finish_opts o = opts_from(argv + 2);
    const long L = atol(argv[9]);
    char why[160];
    if (L < 0 || fn_check_opts(o, why, sizeof why)) { fprintf(stderr, "bad options\n"); return 2; }
    std::vector<FnFrame> t((size_t)fn_nframes(L, o.frame));
    for (FnFrame& f : t) {
      unsigned long long ew;
      unsigned pw;
      if (scanf("%llx %x %d", &ew, &pw, &f.z) != 3) { fprintf(stderr, "short frame table\n"); return 2; }
      const uint64_t e64 = ew;
      const uint32_t p32 = pw;
      memcpy(&f.e, &e64, 8);
      memcpy(&f.p, &p32, 4);
    }
    vx_wave_info w;
    fn_reduce(t.data(), L, o, fn_thr2(o.silence_db), &w);
    uint32_t pk, g;
    uint64_t ms;
    memcpy(&pk, &w.peak, 4); memcpy(&g, &w.gain, 4); memcpy(&ms, &w.mean_square, 8);
    printf("%d %d %d %d %08x %08x %016llx\n", w.begin, w.end, w.active_frames, w.nonfinite, pk, g, (unsigned long long)ms);
    return 0;
  }
  if (!strcmp(cmd, "plan") && argc >= 5) {
    std::vector<long> lo, hi;
    for (int i = 5; i < argc; ++i) {
      long a = 0, b = 0;
      if (sscanf(argv[i], "%ld:%ld", &a, &b) != 2 || a < 0 || b < a) { fprintf(stderr, "bad span %s\n", argv[i]); return 2; }
      lo.push_back(a); hi.push_back(b);
    }
    std::vector<FnJob> jobs;
    if (!fn_plan(lo.data(), hi.data(), (int)lo.size(), atol(argv[2]), atol(argv[3]), atoi(argv[4]), &jobs)) { fprintf(stderr, "no frame fits an empty launch\n"); return 3; }
    for (const FnJob& j : jobs) printf("%d %d %ld %ld %ld %ld\n", j.launch, j.row, j.s_lo, j.cnt, j.off, j.f_off);
    return 0;
  }
  fprintf(stderr, "usage: %s opts | thr2 | table | reduce | plan ... (see the head of tools/finish_host_check.cpp)\n", argv[0]);
  return 2;
}
