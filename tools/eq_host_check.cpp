// Stand-alone run of the equaliser's host code (vall-e-x_amd/csrc/eq_host.h: the cookbook designs, the checks of a cascade, the
// warm-up W, the launch planner, the sequential reference of the contract) on a CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/eq_host_check.cpp -o eq_host_check
//   eq_host_check design KIND RATE F0 Q GAIN_DB    the five coefficients as the hexadecimal words of their doubles, or the refusal
//                                                  (exit code 3)
//   eq_host_check warm SECTIONS                    SECTIONS: raw float64, five per section.  "W S", or the refusal (exit code 3)
//   eq_host_check plan S W WIN OUT_CAP MAX_JOBS L0 L1 ..
//                                                  one job per line: launch row j0 pre cnt off out_off rec_off; exit code 3 when the
//                                                  window does not hold W + S
//   eq_host_check run WAV SECTIONS OUT             WAV: raw float32 samples of one row.  eq_reference at the filter's own W and
//                                                  VX_EQ_STEP: OUT = the row's float32 outputs; prints "W nonfinite nonfinite_out
//                                                  peak" (the peak as the hexadecimal word of its float)
// tests/test_eq_host.py compares all of it with the numpy restatement of the contract (tests/_eq_refs.py).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../vall-e-x_amd/csrc/eq_host.h"

template <typename T>
static bool read_raw(const char* path, std::vector<T>* x) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  T buf[4096];
  size_t n;
  while ((n = fread(buf, sizeof(T), 4096, f)) > 0) x->insert(x->end(), buf, buf + n);
  fclose(f);
  return true;
}

int main(int argc, char** argv) {
  using namespace vxe;
  const char* cmd = argc > 1 ? argv[1] : "";
  char why[240];
  if (!strcmp(cmd, "design") && argc == 7) {
    double c[5];
    if (eq_design(atoi(argv[2]), atoi(argv[3]), atof(argv[4]), atof(argv[5]), atof(argv[6]), c, why, sizeof why)) { printf("%s\n", why); return 3; }
    for (int i = 0; i < 5; ++i) {
      uint64_t w;
      memcpy(&w, c + i, sizeof w);
      printf("%016llx%c", (unsigned long long)w, i == 4 ? '\n' : ' ');
    }
    return 0;
  }
  if (!strcmp(cmd, "warm") && argc == 3) {
    std::vector<double> sec;
    if (!read_raw(argv[2], &sec) || sec.size() % 5) { fprintf(stderr, "no sections in %s\n", argv[2]); return 2; }
    int W = 0;
    if (eq_warm(sec.data(), (int)(sec.size() / 5), &W, why, sizeof why)) { printf("%s\n", why); return 3; }
    printf("%d %d\n", W, EQ_S);
    return 0;
  }
  if (!strcmp(cmd, "plan") && argc >= 7) {
    std::vector<int32_t> lens;
    for (int i = 7; i < argc; ++i) lens.push_back(atoi(argv[i]));
    std::vector<EqJob> jobs;
    if (!eq_plan(lens.data(), (int)lens.size(), atoi(argv[2]), atol(argv[3]), atol(argv[4]), atol(argv[5]), atol(argv[6]), &jobs)) {
      fprintf(stderr, "the window does not hold a warm-up and one step\n");
      return 3;
    }
    for (const EqJob& j : jobs) printf("%d %d %ld %ld %ld %ld %ld %ld\n", j.launch, j.row, j.j0, j.pre, j.cnt, j.off, j.out_off, j.rec_off);
    return 0;
  }
  if (!strcmp(cmd, "run") && argc == 5) {
    std::vector<float> x;
    std::vector<double> sec;
    int W = 0;
    if (!read_raw(argv[2], &x) || !read_raw(argv[3], &sec) || sec.size() % 5 || eq_warm(sec.data(), (int)(sec.size() / 5), &W, why, sizeof why)) {
      fprintf(stderr, "bad file or sections\n");
      return 2;
    }
    std::vector<float> out(x.size());
    vx_eq_info info;
    eq_reference(x.data(), (long)x.size(), sec.data(), (int)(sec.size() / 5), W, EQ_S, out.data(), &info);
    FILE* f = fopen(argv[4], "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", argv[4]); return 2; }
    if (!out.empty()) fwrite(out.data(), sizeof(float), out.size(), f);
    fclose(f);
    uint32_t pk;
    memcpy(&pk, &info.peak, sizeof pk);
    printf("%d %d %d %08x\n", info.warm, info.nonfinite, info.nonfinite_out, pk);
    return 0;
  }
  fprintf(stderr, "usage: %s design | warm | plan | run ... (see the head of tools/eq_host_check.cpp)\n", argv[0]);
  return 2;
}
