#!/usr/bin/env python
"""Wall time of the output stage (vx_finish, through Engine.finish: host staging, upload, the measure launch, the host reduction, the
apply launch, download) with trim, RMS level, fades and 16-bit PCM, beside the numpy restatement of its contract
(tests/_finish_refs.py: per-frame cumsum in double, apply, np.rint) on the same host:
   32 rows x 8 s and 1 row x 60 s at 24 kHz (frame 240): a batch leaving the vocoder, a long reading.
Best of --reps (default 3) after one warm-up call (the first call allocates the buffers and builds the fade tables); the host clock
stops behind the call's last stream synchronisation.  The bytes that cross the host boundary each way are counted from the shapes.
   python tools/finish_bench.py [--reps 3] [--out profiles/r22_finish.json]
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
from tests import _finish_refs as R  # noqa: E402
from vallex_amd._capi import Engine  # noqa: E402

RATE, FRAME = 24000, 240
OPTS = dict(silence_db=-40.0, trim=3, keep=2400, level_mode=R.RMS, level_db=-20.0, max_gain_db=20.0, fade_in=240, fade_out=2400, pcm16=True)


def best(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return min(t), out


def speech_like(rows, seconds, rng):
    """noise floor at -80 dB, a 440 Hz tone under a slow random envelope between half a second of lead and of tail"""
    L = seconds * RATE
    x = (1e-4 * rng.standard_normal((rows, L))).astype(np.float32)
    t = np.arange(RATE // 2, L - RATE // 2)
    for r in range(rows):
        env = np.repeat(rng.uniform(0.3, 1.0, -(-len(t) // 2400)), 2400)[: len(t)]
        x[r, t] += (0.25 * env * np.sin(2 * np.pi * 440.0 * t / RATE + r)).astype(np.float32)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    eng = Engine(num_layers=2, max_batch=1, max_text=8, max_prompt=8, max_new=8, with_vocos=False)
    rng = np.random.default_rng(0)
    res = dict(reps=a.reps, frame=FRAME, options=OPTS, cases=[])
    for rows, seconds in ((32, 8), (1, 60)):
        x = speech_like(rows, seconds, rng)
        dev_ms, (dev, infos) = best(lambda: eng.finish(list(x), FRAME, **OPTS), a.reps)
        ref_ms, ref = best(lambda: [R.finish(r, FRAME, **OPTS) for r in x], a.reps)
        same = all(np.array_equal(d, w) for d, (w, _) in zip(dev, ref))
        gain_ulp = max(int(R.ulp_diff([i["gain"]], [w["gain"]])[0]) for i, (_, w) in zip(infos, ref))
        out_samples = int(sum(len(d) for d in dev))
        res["cases"].append(dict(rows=rows, seconds=seconds, in_samples=int(x.size), out_samples=out_samples,
                                 bytes_to_device=int(x.size) * 4 + rows * 32, bytes_to_host=out_samples * 2 + (int(x.size) // FRAME) * 16 + rows * 32,
                                 fp32_bytes_a_host_conversion_would_fetch=int(x.size) * 4,
                                 vx_finish_wall_ms=dev_ms, numpy_restatement_wall_ms=ref_ms, numpy_over_device=ref_ms / dev_ms,
                                 outputs_equal_the_restatement=bool(same), gain_ulp_difference=gain_ulp,
                                 clipped=int(sum(i["clipped"] for i in infos)), active_frames=int(sum(i["active_frames"] for i in infos))))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
