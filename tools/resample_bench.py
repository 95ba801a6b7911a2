#!/usr/bin/env python
"""Wall time of the device resampler (vx_resample, through Engine.resample: host staging, upload, one or more launches, download)
beside the torch-CPU restatement of the enrolment path (utils.prompt_making.resample_sinc_hann, 16 threads) on the same host:
   32 rows x 8 s at 24000 -> 16000 and 24000 -> 44100 (a batch's audio leaving at another rate), one 15 s row at 48000 -> 24000
   (a prompt arriving).  Best of --reps (default 3) after one warm-up call (the first call allocates and builds the tap table).
   python tools/resample_bench.py [--reps 3] [--threads 16] [--out profiles/r20_resample.json]
The context is created without weights: the entry needs none.  No threshold, the numbers are a record."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vallex_amd  # noqa: E402,F401
from vallex_amd._capi import Engine  # noqa: E402
from vallex_amd.utils import prompt_making as PM  # noqa: E402


def best(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return min(t), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    torch.set_num_threads(a.threads)
    eng = Engine(num_layers=2, max_batch=1, max_text=8, max_prompt=8, max_new=8, with_vocos=False)
    rng = np.random.default_rng(0)
    res = dict(reps=a.reps, torch_threads=torch.get_num_threads(), cases=[])
    for rows, seconds, orig, new in ((32, 8, 24000, 16000), (32, 8, 24000, 44100), (1, 15, 48000, 24000)):
        x = (0.1 * rng.standard_normal((rows, seconds * orig))).astype(np.float32)
        dev_ms, dev = best(lambda: eng.resample(list(x), orig, new), a.reps)
        cpu_ms, cpu = best(lambda: PM.resample_sinc_hann(x, orig, new), a.reps)
        err = max(float(np.abs(d - c).max()) for d, c in zip(dev, cpu))
        res["cases"].append(dict(rows=rows, seconds=seconds, orig=orig, new=new, in_samples=int(x.size), out_samples=int(sum(len(d) for d in dev)),
                                 vx_resample_wall_ms=dev_ms, resample_sinc_hann_wall_ms=cpu_ms, cpu_over_device=cpu_ms / dev_ms,
                                 max_abs_difference=err))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
