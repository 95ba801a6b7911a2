#!/usr/bin/env python
"""Wall time of levelling to a loudness under a true-peak limiter (vx_finish_limited, through Engine.finish_limited: host staging, one
upload, the frames pass, the loudness steps pass, the limiter, the apply pass over the limited samples on the device, download) against
Engine.finish_loud on the same rows in the same session, at 24 kHz to -16 LUFS, fp32 out, no trim, no fades, oversample 4, look-ahead
120 samples (5 ms):
   32 rows x 8 s and 1 row x 60 s: a batch leaving the vocoder, a long reading.
The rows are voice-like with plosive-like bursts, so that the sample peak, not the target, sets finish_loud's gain -- the case the
limiter is for.  For both calls the bytes that cross the host boundary (counted from the shapes), the loudness reached and the true
peak (Engine.true_peak, 4x) are recorded; Engine.limit alone and Engine.true_peak alone are timed as well.
Best of --reps (default 3) after one warm-up call (the first call allocates the buffers), every repetition recorded beside it; the
host clock stops behind the call's last stream synchronisation.
   python tools/limit_bench.py [--reps 3] [--out profiles/r25_limit.json]
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

RATE, LUFS, LOOKAHEAD, OVERSAMPLE = 24000, -16.0, 120, 4


def best(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return min(t), out, [round(v, 3) for v in t]


def speech_like(rows, seconds, rng):
    """a voice-like tone with three partials under a slow random envelope and vibrato over a -60 dB noise floor, with a 2 ms burst of
    0.6 .. 0.9 every half second: a crest factor of about 20 dB"""
    L = seconds * RATE
    t = np.arange(L) / RATE
    x = (1e-3 * rng.standard_normal((rows, L))).astype(np.float32)
    for r in range(rows):
        f0 = 110.0 + 5.0 * r
        ph = 2 * np.pi * f0 * t + 0.5 * np.sin(2 * np.pi * 5.0 * t + r)
        env = np.repeat(rng.uniform(0.2, 1.0, -(-L // 2400)), 2400)[:L]
        x[r] += (0.2 * env * (np.sin(ph) + 0.5 * np.sin(2 * ph) + 0.25 * np.sin(3 * ph))).astype(np.float32)
        for k in range(6000 + 37 * r, L - 48, 12000):
            x[r, k: k + 48] += (rng.uniform(0.6, 0.9) * np.hanning(48) * np.sin(2 * np.pi * 3100.0 * t[:48])).astype(np.float32)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    eng = Engine(num_layers=2, max_batch=1, max_text=8, max_prompt=8, max_new=8, with_vocos=False)
    rng = np.random.default_rng(0)
    res = dict(reps=a.reps, sample_rate=RATE, lufs=LUFS, lookahead=LOOKAHEAD, oversample=OVERSAMPLE, cases=[])

    def db(v):
        return round(20.0 * math.log10(v), 3) if v > 0 else None

    for rows, seconds in ((32, 8), (1, 60)):
        x = speech_like(rows, seconds, rng)
        xs = list(x)
        lim_ms, (lout, linfos), lim_all = best(lambda: eng.finish_limited(xs, RATE, LUFS, -1.0, LOOKAHEAD, OVERSAMPLE), a.reps)
        minfos = eng.last_limit_info
        loud_ms, (out, infos), loud_all = best(lambda: eng.finish_loud(xs, RATE, LUFS), a.reps)
        only_ms, _, _ = best(lambda: eng.limit(xs, -1.0, 2.0, LOOKAHEAD, OVERSAMPLE), a.reps)
        tp_ms, tp_in, _ = best(lambda: eng.true_peak(xs, OVERSAMPLE), a.reps)
        n = int(x.size)
        steps = rows * -(-x.shape[1] // (RATE // 10))
        frames = n // (RATE // 100)
        tiles = rows * -(-x.shape[1] // 2048)
        up, down = n * 4 + rows * 32, n * 4 + steps * 12 + frames * 16
        case = dict(rows=rows, seconds=seconds, samples=n,
                    finish_limited_wall_ms=lim_ms, finish_loud_wall_ms=loud_ms, limiter_adds_ms=lim_ms - loud_ms, finish_limited_wall_ms_all=lim_all,
                    finish_loud_wall_ms_all=loud_all, limit_only_wall_ms=only_ms,
                    true_peak_only_wall_ms=tp_ms,
                    finish_loud=dict(bytes_to_device=up, bytes_to_host=down,
                                     loudness_after=[round(i["loudness"], 3) for i in eng.loudness(out, RATE)][:4],
                                     true_peak_db_after=[db(i["peak"]) for i in eng.true_peak(out, OVERSAMPLE)][:4],
                                     gains=[round(i["gain"], 4) for i in infos][:4]),
                    finish_limited=dict(bytes_to_device=up + rows * 32, bytes_to_host=down + tiles * 16,
                                        loudness_after=[round(i["loudness"], 3) for i in eng.loudness(lout, RATE)][:4],
                                        true_peak_db_after=[db(i["peak"]) for i in eng.true_peak(lout, OVERSAMPLE)][:4],
                                        gains=[round(i["gain"], 4) for i in linfos][:4], min_gains=[round(i["min_gain"], 4) for i in minfos][:4],
                                        reduced=[i["reduced"] for i in minfos][:4]),
                    true_peak_db_before=[db(i["peak"]) for i in tp_in][:4],
                    worst_true_peak_db_after_limiting=max(db(i["peak"]) for i in eng.true_peak(lout, OVERSAMPLE)),
                    worst_loudness_after_limiting=min(round(i["loudness"], 3) for i in eng.loudness(lout, RATE)))
        res["cases"].append(case)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
