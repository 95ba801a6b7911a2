#!/usr/bin/env python
"""Time of text alignment (vx_align) on the benchmark's workload: 12 layers, 32 rows of bench.make_rows (text ~158 ids, prompt ~225
frames), 600 given frames per row, three ways:
   vx_align with uniform weights (every layer tapped, the pass ends behind the last layer's in_proj),
   vx_align with one weighted layer (--layer, default the middle one: the pass ends there),
   vx_score(parts=VX_SCORE_AR) on the same rows -- the same AR pass without the taps, through the predict layer.
   python tools/align_bench.py [--rows 32] [--frames 600] [--reps 3] [--layer 5] [--out profiles/r19_align.json]
The aligned codes are what the engine generates for the rows (top_k 10, forced to `frames`); no threshold, the numbers are a record."""
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
    ap.add_argument("--layer", type=int, default=bench.NUM_LAYERS // 2 - 1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    m = bench.build_model(synth.vallex_state_dict(bench.NUM_LAYERS, 0, eos_gain=0.0), None, 0, a.rows, a.frames)
    eng = m.engine
    rows = bench.make_rows(0, a.rows)
    batch = m.make_batch(rows)
    codes = eng.infer(batch, top_k=10, seed=1, force_eos_at=a.frames, sync_every=16)
    res = dict(rows=a.rows, frames=[int(len(c)) for c in codes], layers=bench.NUM_LAYERS, arith="/".join(eng.arith_mode()),
               text_ids=float(np.mean([len(r["text"]) for r in rows])), prompt_frames=float(np.mean([len(r["prompt"]) for r in rows])))
    one = np.zeros((bench.NUM_LAYERS, 16), np.float32)
    one[a.layer] = 1.0 / 16
    runs = (("align_uniform", lambda: eng.align(batch, codes)), (f"align_layer{a.layer}", lambda: eng.align(batch, codes, one)),
            ("score_ar", lambda: eng.score(batch, codes, 1)))
    for key, fn in runs:
        fn()                                                             # warm-up (the first call allocates)
        wall, ms = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out = fn()
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(eng.last_stats()["ar_ms"])
        res[key] = dict(wall_ms=min(wall), pass_ms=min(ms))
        if key == "align_uniform":
            res["mean_text_mass"] = float(np.mean([o.sum(1).mean() for o in out]))      # a sanity figure, not a timing
    res["align_uniform_over_score_ar"] = res["align_uniform"]["pass_ms"] / res["score_ar"]["pass_ms"]
    res[f"align_layer{a.layer}_over_score_ar"] = res[f"align_layer{a.layer}"]["pass_ms"] / res["score_ar"]["pass_ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
