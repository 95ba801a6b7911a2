#!/usr/bin/env python
"""Wall time of the pitch tracker (vx_f0, through Engine.f0: host staging, one upload, one launch, download of three words per frame,
the host summary) and of the pitch shift (Engine.shift: vx_stretch at q / p, then vx_resample p -> q) at 24 kHz with the defaults
(hop 240, window 600, lags 48 .. 400, threshold 0.15; shift by +3 semitones = 44/37):
   32 rows x 8 s and 1 row x 60 s: a batch leaving the vocoder, a long reading.
The rows are voice-like (three partials under a slow envelope with vibrato over a noise floor).  Recorded beside the times: frames,
voiced frames, the median F0 before and after the shift and how far their ratio is off p / q in cents, the bytes that cross the host
boundary (counted from the shapes).  Best of --reps (default 3) after one warm-up call (the first call allocates the buffers), every
repetition recorded beside it; the host clock stops behind the call's last stream synchronisation.
   python tools/f0_bench.py [--reps 3] [--out profiles/r26_f0.json]
The context is created without weights: the entries need none.  No threshold, the numbers are a record."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vallex_amd  # noqa: E402,F401
from vallex_amd._capi import Engine  # noqa: E402

RATE, PITCH = 24000, 3.0


def best(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return min(t), out, [round(v, 3) for v in t]


def voice_like(rows, seconds, rng):
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
    a = ap.parse_args()
    eng = Engine(num_layers=2, max_batch=1, max_text=8, max_prompt=8, max_new=8, with_vocos=False)
    rng = np.random.default_rng(0)
    r = Engine.pitch_ratio(PITCH)
    res = dict(reps=a.reps, sample_rate=RATE, hop=RATE // 100, window=RATE // 40, lag_min=48, lag_max=400, threshold=0.15,
               pitch_semitones=PITCH, pitch_ratio=[r.numerator, r.denominator], cases=[])
    for rows, seconds in ((32, 8), (1, 60)):
        xs = list(voice_like(rows, seconds, rng))
        f0_ms, (f, voiced, apz, info), f0_all = best(lambda: eng.f0(xs, RATE), a.reps)
        sh_ms, shifted, sh_all = best(lambda: eng.shift(xs, PITCH), a.reps)
        st_ms, stretched, _ = best(lambda: eng.stretch(xs, 1 / r), a.reps)
        info2 = eng.f0(shifted, RATE)[3]
        n = sum(len(x) for x in xs)
        frames = sum(i["frames"] for i in info)
        off = [1200.0 * math.log2(b["f0_median"] / c["f0_median"] / float(r)) for b, c in zip(info2, info) if b["f0_median"] > 0 and c["f0_median"] > 0]
        res["cases"].append(dict(rows=rows, seconds=seconds, samples=n, frames=frames, voiced_frames=sum(i["voiced_frames"] for i in info),
                                 f0_wall_ms=f0_ms, f0_wall_ms_all=f0_all, f0_us_per_frame=round(1e3 * f0_ms / max(frames, 1), 4),
                                 f0_bytes_to_device=n * 4 + rows * 32, f0_bytes_to_host=frames * 12,
                                 shift_wall_ms=sh_ms, shift_wall_ms_all=sh_all, stretch_alone_wall_ms=st_ms,
                                 shifted_lengths_equal=all(len(y) == len(x) for x, y in zip(xs, shifted)),
                                 f0_median_before=[round(i["f0_median"], 3) for i in info][:4],
                                 f0_median_after=[round(i["f0_median"], 3) for i in info2][:4],
                                 worst_cents_off_ratio=round(max(abs(v) for v in off), 4) if off else None))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
