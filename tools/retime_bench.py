#!/usr/bin/env python
"""Wall time of the time map (vx_pauses and vx_retime, through Engine.pauses / Engine.retime: host staging, upload, one launch whose
jobs -- walked segments and copy tiles -- run side by side, download) with the defaults at 24 kHz (hop 240, search 150):
   1  32 rows x 8 s with six pauses each, shortened to 200 ms (pauses, then pause_map, then retime: each timed)
   2  one 60 s row with 40 pauses, shortened likewise
   3  one 60 s row retimed uniformly at 4/5 through 1 s segments, beside vx_stretch at 4/5 on the same row: the segment-parallel walk
      against the serial one.  The stretch walks the row's frames with one workgroup; the time map walks its 60 segments with 60.
Case 3 is the one with an expectation (the time map should be the faster one); the others are a record.  Both sides of case 3 run in
this process, alternating.  Best of --reps (default 5) after one warm-up call (the first call allocates the buffers and builds the
crossfade table); the host clock stops behind the call's last stream synchronisation.
   python tools/retime_bench.py [--reps 5] [--out profiles/r31_retime.json]
The context is created without weights: the entries need none."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vallex_amd  # noqa: E402,F401
from vallex_amd._capi import Engine  # noqa: E402
from vallex_amd.utils.alignment import pause_map  # noqa: E402

RATE, HOP, SEARCH = 24000, 240, 150


def best(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return min(t), sorted(t)[len(t) // 2], out


def voice(L, rng, f0):
    """a voice-like tone with three partials under a slow random envelope and vibrato, over a -60 dB noise floor"""
    t = np.arange(L) / RATE
    ph = 2 * np.pi * f0 * t + 0.5 * np.sin(2 * np.pi * 5.0 * t)
    env = np.repeat(rng.uniform(0.2, 1.0, -(-L // 2400)), 2400)[:L]
    return (1e-3 * rng.standard_normal(L) + 0.2 * env * (np.sin(ph) + 0.5 * np.sin(2 * ph) + 0.25 * np.sin(3 * ph))).astype(np.float32)


def with_pauses(seconds, n_pauses, pause_s, rng, f0):
    """`seconds` of voice with n_pauses gaps of noise floor of pause_s seconds each, evenly placed"""
    L = seconds * RATE
    x = voice(L, rng, f0)
    P = int(pause_s * RATE)
    for i in range(n_pauses):
        s = (i + 1) * L // (n_pauses + 1) // HOP * HOP
        x[s: s + P] = (1e-3 * rng.standard_normal(P)).astype(np.float32)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    eng = Engine(num_layers=2, max_batch=1, max_text=8, max_prompt=8, max_new=8, with_vocos=False)
    rng = np.random.default_rng(0)
    res = dict(reps=a.reps, hop=HOP, search=SEARCH, cases=[])
    for case, (rows, seconds, n_pauses) in ((1, (32, 8, 6)), (2, (1, 60, 40))):
        xs = [with_pauses(seconds, n_pauses, 0.6, rng, 110.0 + 5.0 * r) for r in range(rows)]
        p_ms, p_med, spans = best(lambda: eng.pauses(xs, RATE, silence_db=-50.0, min_ms=150.0, keep_ms=20.0), a.reps)
        t0 = time.perf_counter()
        maps = [pause_map(len(x), sp, max_len=RATE // 5, hop=HOP) for x, sp in zip(xs, spans)]
        map_ms = (time.perf_counter() - t0) * 1e3
        r_ms, r_med, out = best(lambda: eng.retime(xs, maps, HOP, SEARCH, RATE), a.reps)
        info = eng.last_retime_info
        res["cases"].append(dict(case=case, rows=rows, seconds=seconds, pauses_found=[int(len(s)) for s in spans][:4], in_samples=int(sum(len(x) for x in xs)),
                                 out_samples=int(sum(len(o) for o in out)), walked_segments=int(sum(r["walked"] for r in info)),
                                 frames=int(sum(r["frames"] for r in info)), vx_pauses_wall_ms=p_ms, vx_pauses_median_ms=p_med,
                                 pause_map_host_ms=map_ms, vx_retime_wall_ms=r_ms, vx_retime_median_ms=r_med))
    # case 3: the uniform 4/5 through 1 s segments against the serial walk
    x = voice(60 * RATE, rng, 120.0)
    an = np.array([(i * RATE, i * RATE * 5 // 4) for i in range(61)], np.int32)
    st, rt = [], []
    eng.stretch([x], (4, 5), HOP, SEARCH, RATE)
    eng.retime([x], [an], HOP, SEARCH, RATE)
    for _ in range(a.reps):                                              # alternating, one process
        t0 = time.perf_counter()
        s_out = eng.stretch([x], (4, 5), HOP, SEARCH, RATE)
        st.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        r_out = eng.retime([x], [an], HOP, SEARCH, RATE)
        rt.append((time.perf_counter() - t0) * 1e3)
    frames = eng.last_retime_info[0]["frames"]
    res["cases"].append(dict(case=3, rows=1, seconds=60, segments=60, frames=frames, out_samples=[int(len(s_out[0])), int(len(r_out[0]))],
                             vx_stretch_wall_ms=min(st), vx_stretch_median_ms=sorted(st)[len(st) // 2], vx_retime_wall_ms=min(rt),
                             vx_retime_median_ms=sorted(rt)[len(rt) // 2], stretch_over_retime=min(st) / min(rt),
                             retime_us_per_frame_of_a_segment=min(rt) * 1e3 / (frames / 60)))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
