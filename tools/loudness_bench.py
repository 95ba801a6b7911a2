#!/usr/bin/env python
"""Wall time of levelling to a loudness (vx_finish_loud, through Engine.finish_loud: host staging, one upload, the frames pass, the
steps pass that runs the K-weighting recursion of every 100 ms step on a lane of its own, the apply pass, download) at 24 kHz to
-16 LUFS, fp32 out, no trim, no fades:
   32 rows x 8 s and 1 row x 60 s: a batch leaving the vocoder, a long reading.
Beside it, in the same session and on the same rows: Engine.finish in RMS mode (what the loudness pass adds over the unweighted
level), Engine.loudness alone, and the numpy restatement of the contract (tests/_loudness_refs.py) on the library's coefficients.
Best of --reps (default 3) after one warm-up call (the first call allocates the buffers); the host clock stops behind the call's last
stream synchronisation.  The bytes that cross the host boundary each way are counted from the shapes.
   python tools/loudness_bench.py [--reps 3] [--out profiles/r24_loudness.json]
The context is created without weights: the entries need none.  No threshold, the numbers are a record."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vallex_amd  # noqa: E402,F401
from tests import _loudness_refs as R  # noqa: E402
from vallex_amd._capi import LEVEL_RMS, Engine  # noqa: E402

RATE, LUFS = 24000, -16.0


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
    ap.add_argument("--no-ref", action="store_true", help="skip the numpy restatement")
    a = ap.parse_args()
    eng = Engine(num_layers=2, max_batch=1, max_text=8, max_prompt=8, max_new=8, with_vocos=False)
    c = eng.loudness_coeffs(RATE)
    rng = np.random.default_rng(0)
    res = dict(reps=a.reps, sample_rate=RATE, lufs=LUFS, cases=[])
    for rows, seconds in ((32, 8), (1, 60)):
        x = speech_like(rows, seconds, rng)
        loud_ms, (out, infos) = best(lambda: eng.finish_loud(list(x), RATE, LUFS), a.reps)
        linfos = eng.last_loudness_info
        rms_ms, _ = best(lambda: eng.finish(list(x), RATE // 100, level_mode=LEVEL_RMS, level_db=-20.0), a.reps)
        meas_ms, meas = best(lambda: eng.loudness(list(x), RATE), a.reps)
        steps = rows * -(-x.shape[1] // (RATE // 10))
        case = dict(rows=rows, seconds=seconds, samples=int(x.size), steps=steps,
                    bytes_to_device=int(x.size) * 4 + rows * 32, bytes_to_host=int(x.size) * 4 + steps * 12 + (x.size // (RATE // 100)) * 16,
                    finish_loud_wall_ms=loud_ms, finish_rms_wall_ms=rms_ms, loudness_pass_adds_ms=loud_ms - rms_ms, loudness_only_wall_ms=meas_ms,
                    loudness_before=[round(i["loudness"], 3) for i in linfos][:4],
                    loudness_after=[round(i["loudness"], 4) for i in eng.loudness(out, RATE)][:4], gains=[round(i["gain"], 4) for i in infos][:4])
        if not a.no_ref:
            t0 = time.perf_counter()
            ref = [R.measure(r, RATE, c) for r in x]                    # once: it is not what is measured
            case["numpy_restatement_wall_ms"] = (time.perf_counter() - t0) * 1e3
            case["numpy_over_device_measurement"] = case["numpy_restatement_wall_ms"] / meas_ms
            case["mean_squares_equal_the_restatement"] = bool(all(np.float64(m["mean_square"]).view(np.uint64) ==
                                                                  np.float64(w["mean_square"]).view(np.uint64) for m, w in zip(meas, ref)))
        res["cases"].append(case)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
