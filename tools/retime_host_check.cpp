// Stand-alone run of the time map's host code (vall-e-x_amd/csrc/retime_host.h: option checking, pause reduction, anchor checks,
// frames and nominal positions of a walked segment, launch planner) on a CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/retime_host_check.cpp -o retime_host_check
//   retime_host_check popts FRAME SILENCE_DB MIN_FRAMES KEEP      "ok", or the refusal (exit code 3)
//   retime_host_check pauses WAV FRAME SILENCE_DB MIN_FRAMES KEEP  WAV: raw float32 samples of one row.  The frame table is summed
//                                                  here in sample order in double, then rt_pauses: "begin end" per line
//   retime_host_check opts HOP SEARCH              "ok", or the refusal (exit code 3)
//   retime_host_check anchors HOP L A0 B0 A1 B1 .. "ok Lout frames", or the refusal (exit code 3)
//   retime_host_check plan HOP SEARCH WIN OUT_CAP FRAME_CAP MAX_JOBS TILE ROWS
//                                                  ROWS: a text file, one row per line: L n A0 B0 .. (checked anchors).  One job per
//                                                  line: launch row walk a a1 b lb s_lo s_hi in_off out_off f_off f_row; exit code 3
//                                                  and "row R segment S" when a walked segment does not fit an empty launch
//   retime_host_check walk WAV OUT HOP SEARCH A0 B0 A1 B1 ..
//                                                  a SEQUENTIAL reference of vx_retime on one row, one candidate after the other, on
//                                                  rt_frames / rt_nominal / fn_fade_table: OUT = Lout float32, then the frames' int32
//                                                  positions, then their double costs; prints "Lout frames"
// tests/test_retime_host.py compares all of it with the numpy restatement of the contract (tests/_retime_refs.py).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../vall-e-x_amd/csrc/retime_host.h"

static bool read_floats(const char* path, std::vector<float>* x) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  float buf[4096];
  size_t n;
  while ((n = fread(buf, sizeof(float), 4096, f)) > 0) x->insert(x->end(), buf, buf + n);
  fclose(f);
  return true;
}

static float clean(float v) { return v - v == 0.f ? v : 0.f; }

int main(int argc, char** argv) {
  using namespace vxe;
  const char* cmd = argc > 1 ? argv[1] : "";
  char why[240];
  auto popts = [&](char** a) {
    vx_pause_opts o;
    memset(&o, 0, sizeof o);
    o.struct_size = sizeof o;
    o.frame = atoi(a[0]); o.silence_db = (float)atof(a[1]); o.min_frames = atoi(a[2]); o.keep = atoi(a[3]);
    return o;
  };
  if (!strcmp(cmd, "popts") && argc == 6) {
    if (rt_check_pause_opts(popts(argv + 2), why, sizeof why)) { printf("%s\n", why); return 3; }
    printf("ok\n");
    return 0;
  }
  if (!strcmp(cmd, "pauses") && argc == 7) {
    const vx_pause_opts o = popts(argv + 3);
    std::vector<float> x;
    if (rt_check_pause_opts(o, why, sizeof why) || !read_floats(argv[2], &x)) { fprintf(stderr, "bad options or file\n"); return 2; }
    const long L = (long)x.size(), nf = fn_nframes(L, o.frame);
    std::vector<FnFrame> t((size_t)nf);
    for (long f = 0; f < nf; ++f) {
      double e = 0.0;
      for (long i = f * o.frame; i < std::min<long>(L, (f + 1) * o.frame); ++i) { const double y = clean(x[(size_t)i]); e += y * y; }
      t[(size_t)f] = {e, 0.f, 0};
    }
    std::vector<int> spans;
    rt_pauses(t.data(), L, o, fn_thr2(o.silence_db), &spans);
    for (size_t i = 0; i + 1 < spans.size(); i += 2) printf("%d %d\n", spans[i], spans[i + 1]);
    return 0;
  }
  if (!strcmp(cmd, "opts") && argc == 4) {
    vx_retime_opts o = {sizeof(vx_retime_opts), atoi(argv[2]), atoi(argv[3])};
    if (rt_check_opts(o, why, sizeof why)) { printf("%s\n", why); return 3; }
    printf("ok\n");
    return 0;
  }
  if (!strcmp(cmd, "anchors") && argc >= 4 && (argc - 4) % 2 == 0) {
    std::vector<int> an;
    for (int i = 4; i < argc; ++i) an.push_back(atoi(argv[i]));
    long Lout, frames;
    if (rt_check_anchors(an.data(), (long)an.size() / 2, atol(argv[3]), atoi(argv[2]), &Lout, &frames, why, sizeof why)) { printf("%s\n", why); return 3; }
    printf("ok %ld %ld\n", Lout, frames);
    return 0;
  }
  if (!strcmp(cmd, "plan") && argc == 10) {
    const int H = atoi(argv[2]), D = atoi(argv[3]);
    FILE* f = fopen(argv[9], "r");
    if (!f) { fprintf(stderr, "no file %s\n", argv[9]); return 2; }
    std::vector<std::vector<int>> rows;
    std::vector<int> lens, counts;
    long L, n;
    size_t stride = 2;
    while (fscanf(f, "%ld %ld", &L, &n) == 2) {
      std::vector<int> an((size_t)(2 * n));
      for (int& v : an)
        if (fscanf(f, "%d", &v) != 1) { fclose(f); fprintf(stderr, "short row\n"); return 2; }
      long Lout, frames;
      if (rt_check_anchors(an.data(), n, L, H, &Lout, &frames, why, sizeof why)) { fclose(f); fprintf(stderr, "bad anchors: %s\n", why); return 2; }
      stride = std::max(stride, an.size());
      rows.push_back(an); lens.push_back((int)L); counts.push_back((int)n);
    }
    fclose(f);
    std::vector<int> flat(rows.size() * stride + 1, 0);
    for (size_t r = 0; r < rows.size(); ++r) std::copy(rows[r].begin(), rows[r].end(), flat.begin() + (long)(r * stride));
    std::vector<RtJob> jobs;
    int bad_row;
    long bad_seg;
    if (!rt_plan(flat.data(), (long)stride, counts.data(), lens.data(), (int)rows.size(), H, D, atol(argv[4]), atol(argv[5]), atol(argv[6]),
                 atol(argv[7]), atol(argv[8]), &jobs, &bad_row, &bad_seg)) {
      fprintf(stderr, "row %d segment %ld does not fit an empty launch\n", bad_row, bad_seg);
      return 3;
    }
    for (const RtJob& j : jobs)
      printf("%d %d %d %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld\n", j.launch, j.row, j.walk, j.a, j.a1, j.b, j.lb, j.s_lo, j.s_hi, j.in_off,
             j.out_off, j.f_off, j.f_row);
    return 0;
  }
  if (!strcmp(cmd, "walk") && argc >= 8 && (argc - 6) % 2 == 0) {
    const int H = atoi(argv[4]), D = atoi(argv[5]);
    vx_retime_opts o = {sizeof(vx_retime_opts), H, D};
    std::vector<float> x;
    std::vector<int> an;
    for (int i = 6; i < argc; ++i) an.push_back(atoi(argv[i]));
    long Lout, frames;
    if (rt_check_opts(o, why, sizeof why) || !read_floats(argv[2], &x) ||
        rt_check_anchors(an.data(), (long)an.size() / 2, (long)x.size(), H, &Lout, &frames, why, sizeof why)) {
      fprintf(stderr, "bad options, file or anchors\n");
      return 2;
    }
    const long L = (long)x.size();
    auto y = [&](long s) -> double { return s < 0 || s >= L ? 0.0 : (double)clean(x[(size_t)s]); };
    std::vector<float> w, out((size_t)Lout);
    fn_fade_table(H, w);
    std::vector<int> pos;
    std::vector<double> cost;
    for (size_t i = 0; i + 1 < an.size() / 2; ++i) {
      const long a = an[2 * i], b = an[2 * i + 1], a1 = an[2 * i + 2], b1 = an[2 * i + 3], la = a1 - a, lb = b1 - b;
      if (la == lb) {
        memcpy(out.data() + b, x.data() + a, (size_t)la * sizeof(float));
        continue;
      }
      const long M = rt_frames(lb, H), rem = lb - M * H;
      long p = a;
      for (long j = 0; j < H; ++j) out[(size_t)(b + j)] = (float)y(a + j);
      pos.push_back((int)a); cost.push_back(0.0);
      for (long k = 1; k < M; ++k) {
        const long n = a + rt_nominal(la, lb, H, k);
        const long dlo = k == M - 1 ? 0 : std::max<long>(-D, a - n), dhi = k == M - 1 ? 0 : std::min<long>(D, a1 - H - n);
        double bD = 0.0;
        long bd = 0;
        bool have = false;
        for (long d = dlo; d <= dhi; ++d) {
          double c = 0.0, e = 0.0;
          for (long j = 0; j < H; ++j) {
            const double u = y(n + d + j), t = y(p + H + j);
            const double ut = u * t, uu = u * u;     // exact products, then one addition each
            c += ut; e += uu;
          }
          const double Dd = e - 2.0 * c;
          const long ad = d < 0 ? -d : d, ab = bd < 0 ? -bd : bd;
          if (!have || Dd < bD || (Dd == bD && (ad < ab || (ad == ab && d < bd)))) { bD = Dd; bd = d; have = true; }
        }
        const long pk = n + bd;
        for (long j = 0; j < H; ++j) {
          const double u = y(pk + j) * (double)w[(size_t)j], v = y(p + H + j) * (double)w[(size_t)(H - 1 - j)];
          out[(size_t)(b + k * H + j)] = (float)(u + v);
        }
        pos.push_back((int)pk); cost.push_back(bD);
        p = pk;
      }
      for (long j = 0; j < rem; ++j) out[(size_t)(b + M * H + j)] = (float)y(p + H + j);
    }
    FILE* f = fopen(argv[3], "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
    if (!out.empty()) fwrite(out.data(), sizeof(float), out.size(), f);
    if (!pos.empty()) fwrite(pos.data(), sizeof(int), pos.size(), f);
    if (!cost.empty()) fwrite(cost.data(), sizeof(double), cost.size(), f);
    fclose(f);
    printf("%ld %zu\n", Lout, pos.size());
    return 0;
  }
  fprintf(stderr, "usage: %s popts | pauses | opts | anchors | plan | walk ... (see the head of tools/retime_host_check.cpp)\n", argv[0]);
  return 2;
}
