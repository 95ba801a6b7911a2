#!/usr/bin/env python
"""Wall time of the speaking rate (vx_stretch, through Engine.stretch: host staging, upload, the one launch that walks every row's
frames in order, download) at speeds 4/5 and 5/4 with the defaults at 24 kHz (hop 240, search 150), beside the numpy restatement of
its contract (tests/_stretch_refs.py) on the same host:
   32 rows x 8 s and 1 row x 60 s: a batch leaving the vocoder, a long reading.
A row is a serial walk over its frames (frame k starts from the position frame k - 1 found), so the 60 s row shows the cost per frame
and the 32-row batch what running rows side by side on different CUs buys.  Best of --reps (default 3) after one warm-up call (the
first call allocates the buffers and builds the crossfade table); the host clock stops behind the call's last stream
synchronisation.  The bytes that cross the host boundary each way are counted from the shapes.  --largest adds 1 row x 8 s at the
largest options (hop 2048, search 1024: the 24-register prefetch and the largest LDS layout of the walk).
   python tools/stretch_bench.py [--reps 3] [--largest] [--out profiles/r23_stretch.json]
The context is created without weights: the entry needs none.  No threshold, the numbers are a record."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vallex_amd  # noqa: E402,F401
from tests import _stretch_refs as R  # noqa: E402
from vallex_amd._capi import Engine  # noqa: E402

RATE, HOP, SEARCH = 24000, 240, 150


def best(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return min(t), out


def speech_like(rows, seconds, rng):
    """a 130 Hz voice-like tone with three partials under a slow random envelope and vibrato, over a -60 dB noise floor"""
    L = seconds * RATE
    t = np.arange(L) / RATE
    x = (1e-3 * rng.standard_normal((rows, L))).astype(np.float32)
    for r in range(rows):
        f0 = 110.0 + 5.0 * r
        ph = 2 * np.pi * f0 * t + 0.5 * np.sin(2 * np.pi * 5.0 * t + r)
        env = np.repeat(rng.uniform(0.2, 1.0, -(-L // 2400)), 2400)[:L]
        x[r] += (0.2 * env * (np.sin(ph) + 0.5 * np.sin(2 * ph) + 0.25 * np.sin(3 * ph))).astype(np.float32)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--largest", action="store_true", help="add 1 row x 8 s at hop 2048, search 1024")
    ap.add_argument("--no-ref", action="store_true", help="skip the numpy restatement (minutes of host time on the large cases)")
    a = ap.parse_args()
    eng = Engine(num_layers=2, max_batch=1, max_text=8, max_prompt=8, max_new=8, with_vocos=False)
    rng = np.random.default_rng(0)
    res = dict(reps=a.reps, hop=HOP, search=SEARCH, cases=[])
    for rows, seconds, hop, search in ((32, 8, HOP, SEARCH), (1, 60, HOP, SEARCH)) + (((1, 8, 2048, 1024),) if a.largest else ()):
        x = speech_like(rows, seconds, rng)
        for num, den in ((4, 5), (5, 4)):
            dev_ms, (dev, pos) = best(lambda: eng.stretch(list(x), (num, den), hop, search, RATE, return_positions=True), a.reps)
            frames = int(sum(len(p) for p in pos))
            case = dict(rows=rows, seconds=seconds, hop=hop, search=search, speed=f"{num}/{den}", in_samples=int(x.size), out_samples=int(sum(len(d) for d in dev)),
                        frames=frames, frames_of_the_longest_row=int(max(len(p) for p in pos)),
                        bytes_to_device=int(x.size) * 4 + rows * 64, bytes_to_host=int(sum(len(d) for d in dev)) * 4 + frames * 4 + rows * 4,
                        vx_stretch_wall_ms=dev_ms, wall_us_per_frame_of_the_longest_row=dev_ms * 1e3 / max(1, max(len(p) for p in pos)))
            if not a.no_ref:
                t0 = time.perf_counter()
                ref = [R.stretch(r, num, den, hop, search) for r in x]          # once: it is slow and it is not what is measured
                case["numpy_restatement_wall_ms"] = (time.perf_counter() - t0) * 1e3
                case["numpy_over_device"] = case["numpy_restatement_wall_ms"] / dev_ms
                case["outputs_equal_the_restatement"] = bool(all(np.array_equal(d.view(np.uint32), w[0].view(np.uint32)) for d, w in zip(dev, ref)))
                case["positions_equal_the_restatement"] = bool(all(np.array_equal(p, w[1]) for p, w in zip(pos, ref)))
            res["cases"].append(case)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
