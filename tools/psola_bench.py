#!/usr/bin/env python
"""Wall time of the formant-preserving pitch shift at 24 kHz with the defaults (hop 240, periods 48 .. 400, U 120; +3 semitones = 44/37):
`psola` alone (vx_psola through Engine.psola on lags measured beforehand: host staging, the mark walk, the grain table on the host, the
synthesis, the download) and `shift(formants=True)` (vx_f0, then vx_psola), beside `shift(formants=False)` (vx_stretch, then
vx_resample) on the same rows:
   32 rows x 8 s and 1 row x 60 s of the vibrato rows tools/f0_bench.py uses.
The mark walk is serial per row, as the stretch is.  Its share is read from a second `psola` call on the same rows with every lag
negated (unvoiced: the walk steps by U without a search, and everything else -- transfers, grain table, synthesis -- stays): share =
1 - unvoiced / voiced.  Recorded beside the times: marks, grains and gaps, the median F0 before and after and how far their ratio is
off p / q in cents.  Best of --reps (default 3) after one warm-up call, every repetition recorded beside it; the host clock stops
behind the call's last stream synchronisation.
   python tools/psola_bench.py [--reps 3] [--out profiles/r27_psola.json]
The context is created without weights: the entries need none.  No threshold, the numbers are a record."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import vallex_amd  # noqa: E402,F401
import numpy as np  # noqa: E402
from f0_bench import PITCH, RATE, best, voice_like  # noqa: E402
from vallex_amd._capi import Engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    eng = Engine(num_layers=2, max_batch=1, max_text=8, max_prompt=8, max_new=8, with_vocos=False)
    rng = np.random.default_rng(0)
    r = Engine.pitch_ratio(PITCH)
    o = eng._f0_opts(RATE, None, None, 60.0, 500.0, 0.15)
    res = dict(reps=a.reps, sample_rate=RATE, hop=o.hop, period_min=o.lag_min, period_max=o.lag_max, unvoiced_period=120,
               pitch_semitones=PITCH, pitch_ratio=[r.numerator, r.denominator], cases=[])
    for rows, seconds in ((32, 8), (1, 60)):
        xs = list(voice_like(rows, seconds, rng))
        _, lag, _, info = eng.f0_lags(xs, o)
        ps_ms, (ys, pinfo), ps_all = best(lambda: eng.psola(xs, lag, o.hop, r), a.reps)
        un_ms, _, un_all = best(lambda: eng.psola(xs, [-np.abs(v) for v in lag], o.hop, r), a.reps)
        sf_ms, shifted, sf_all = best(lambda: eng.shift(xs, PITCH, formants=True), a.reps)
        pl_ms, _, pl_all = best(lambda: eng.shift(xs, PITCH), a.reps)
        f0_ms, _, _ = best(lambda: eng.f0_lags(xs, o), a.reps)
        info2 = eng.f0_lags(shifted, o)[3]
        off = [1200.0 * math.log2(b["f0_median"] / c["f0_median"] / float(r)) for b, c in zip(info2, info) if b["f0_median"] > 0 and c["f0_median"] > 0]
        res["cases"].append(dict(rows=rows, seconds=seconds, samples=sum(len(x) for x in xs),
                                 marks=sum(i["marks"] for i in pinfo), voiced_marks=sum(i["voiced_marks"] for i in pinfo),
                                 grains=sum(i["grains"] for i in pinfo), gaps=sum(i["gaps"] for i in pinfo),
                                 psola_wall_ms=ps_ms, psola_wall_ms_all=ps_all, psola_unvoiced_wall_ms=un_ms, psola_unvoiced_wall_ms_all=un_all,
                                 mark_walk_share=round(1.0 - un_ms / ps_ms, 4),
                                 shift_formants_wall_ms=sf_ms, shift_formants_wall_ms_all=sf_all, f0_alone_wall_ms=f0_ms,
                                 shift_plain_wall_ms=pl_ms, shift_plain_wall_ms_all=pl_all,
                                 lengths_equal=all(len(y) == len(x) for x, y in zip(xs, shifted)),
                                 shift_equals_the_steps=all(np.array_equal(p, q) for p, q in zip(ys, shifted)),
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
