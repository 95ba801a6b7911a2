#!/usr/bin/env python
"""Time of teacher-forced scoring (vx_score) on the benchmark's workload: 12 layers, 32 rows of bench.make_rows (text ~158 ids,
prompt ~225 frames), 600 given frames per row -- next to the only way the step-level seam offers without it: vx_ar_prefill + 600 x
(vx_ar_logits + vx_ar_step), one row at a time, first codebook only.
   python tools/score_bench.py [--rows 32] [--frames 600] [--reps 3] [--seam-rows 1] [--out profiles/r16_score.json]
The scored codes are what the engine generates for the rows (top_k 10, forced to `frames`); no threshold, the numbers are a record."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import vallex_amd  # noqa: E402,F401
from oracle import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--frames", type=int, default=bench.FRAMES)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seam-rows", type=int, default=1, help="rows timed through the step-level seam (each costs `frames` round trips)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    m = bench.build_model(synth.vallex_state_dict(bench.NUM_LAYERS, 0, eos_gain=0.0), None, 0, a.rows, a.frames)
    eng = m.engine
    rows = bench.make_rows(0, a.rows)
    batch = m.make_batch(rows)
    codes = eng.infer(batch, top_k=10, seed=1, force_eos_at=a.frames, sync_every=16)
    res = dict(rows=a.rows, frames=[int(len(c)) for c in codes], layers=bench.NUM_LAYERS, arith="/".join(eng.arith_mode()),
               text_ids=float(np.mean([len(r["text"]) for r in rows])), prompt_frames=float(np.mean([len(r["prompt"]) for r in rows])))
    for parts, key in ((3, "both"), (1, "ar"), (2, "nar")):
        eng.score(batch, codes, parts)                                   # warm-up (the first call allocates)
        wall, ar_ms, nar_ms = [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out = eng.score(batch, codes, parts)
            wall.append((time.perf_counter() - t0) * 1e3)
            st = eng.last_stats()
            ar_ms.append(st["ar_ms"]); nar_ms.append(st["nar_ms"])
        res["score_" + key] = dict(wall_ms=min(wall), ar_pass_ms=min(ar_ms), nar_pass_ms=min(nar_ms))
    res["mean_logp"] = float(np.mean([o[0][:, 1:].mean() for o in out]))      # of the NAR columns: a sanity figure, not a timing
    # the step-level seam: one row, one host round trip and one 1025-float read-back per frame
    seam = []
    for i in range(min(a.seam_rows, a.rows)):
        b1 = m.make_batch([rows[i]])
        t0 = time.perf_counter()
        eng.ar_prefill(b1)
        for t in range(len(codes[i])):
            eng.ar_logits()
            eng.ar_step(np.array([codes[i][t, 0]], np.int32))
        eng.ar_logits()
        seam.append((time.perf_counter() - t0) * 1e3)
    res["seam_ar_ms_per_row"] = float(np.mean(seam))
    res["seam_ar_ms_all_rows_extrapolated"] = float(np.mean(seam)) * a.rows
    # one generation of the same rows for scale: the AR pass should cost about one prefill of S + 1 + Tp + T rows, the NAR pass what
    # the seven stages of generation cost
    eng.infer(batch, top_k=10, seed=1, force_eos_at=a.frames, sync_every=16)
    st = eng.last_stats()
    res["generation"] = dict(ar_ms=st["ar_ms"], nar_ms=st["nar_ms"])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
