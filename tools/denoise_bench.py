#!/usr/bin/env python
"""Wall time of the spectral noise suppression at 24 kHz with the defaults (alpha 2, floor -18 dB, frac 0.1, kmin 8): `denoise` (vx_denoise
through Engine.denoise: host staging, upload, the power launch, the download of the energies, the choice of the noise frames on the host,
the profile launch, the synthesis launch, the download) on
   32 rows x 8 s and 1 row x 60 s of the vibrato rows tools/f0_bench.py uses, in white noise of sigma 0.01,
and the same rows under a given profile (no download of the energies, no choice, no profile launch).
Beside the times: the transforms per row -- T = ceil(L / 128) + 3 forward networks in the power pass, and for each of the ceil(L / 128)
hops of the synthesis pass four forward and four inverse ones (the 4x recompute that spares a spectrum buffer) -- at 23 040 double
operations a network (9 stages x 256 butterflies x (4 products + 6 sums)), and the double-precision rate that is of the wall time, a
lower bound of the kernels' own rate: the wall time holds the transfers and the host step, and a kernel-only time is not separable
without an entry of its own.  Recorded too: the RMS of the first row before and after.  Best of --reps (default 3) after one warm-up
call, every repetition recorded beside it; the host clock stops behind the call's last stream synchronisation.
   python tools/denoise_bench.py [--reps 3] [--out profiles/r29_denoise.json]
The context is created without weights: the entries need none.  No threshold, the numbers are a record."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import vallex_amd  # noqa: E402,F401
import numpy as np  # noqa: E402
from f0_bench import RATE, best, voice_like  # noqa: E402
from vallex_amd._capi import Engine  # noqa: E402

NETWORK_FLOP = 9 * 256 * 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    eng = Engine(num_layers=2, max_batch=1, max_text=8, max_prompt=8, max_new=8, with_vocos=False)
    rng = np.random.default_rng(0)
    res = dict(reps=a.reps, sample_rate=RATE, alpha=2.0, floor_db=-18.0, frac=0.1, kmin=8, network_flop=NETWORK_FLOP, cases=[])
    for rows, seconds in ((32, 8), (1, 60)):
        xs = [(x + rng.normal(0.0, 0.01, len(x))).astype(np.float32) for x in voice_like(rows, seconds, rng)]
        ms, (ys, infos), ms_all = best(lambda: eng.denoise(xs), a.reps)
        prof = eng.noise_profile(xs[0])
        gp_ms, _, gp_all = best(lambda: eng.denoise(xs, profile=prof), a.reps)
        hops = [-(-len(x) // 128) for x in xs]
        nets = [(h + 3) + 8 * h for h in hops]
        flop = float(sum(nets)) * NETWORK_FLOP
        res["cases"].append(dict(rows=rows, seconds=seconds, samples=sum(len(x) for x in xs), frames=sum(i["frames"] for i in infos),
                                 noise_frames=[i["k"] for i in infos][:4], wall_ms=ms, wall_ms_all=ms_all,
                                 given_profile_wall_ms=gp_ms, given_profile_wall_ms_all=gp_all,
                                 networks_per_row=nets[0], power_pass_networks_per_row=hops[0] + 3, synthesis_networks_per_row=8 * hops[0],
                                 gflop=round(flop / 1e9, 3), gflops_of_wall=round(flop / 1e6 / ms, 1),
                                 gflops_of_wall_given_profile=round(flop / 1e6 / gp_ms, 1),
                                 bytes_up=4 * sum(len(x) for x in xs), bytes_down=4 * sum(len(x) for x in xs) + 8 * sum(i["frames"] for i in infos),
                                 lengths_equal=all(len(y) == len(x) for x, y in zip(xs, ys)),
                                 rms_in=round(float(np.sqrt(np.mean(xs[0].astype(np.float64) ** 2))), 5),
                                 rms_out=round(float(np.sqrt(np.mean(ys[0].astype(np.float64) ** 2))), 5)))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
