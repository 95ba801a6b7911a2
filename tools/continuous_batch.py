#!/usr/bin/env python
"""Continuous batching against the micro-batched schedule: vx_infer (micro-batches of 32 rows, each decoded until its longest row has
stopped) and vx_infer_continuous (one 32-row decode batch, a finished row's decode row refilled with the next waiting row at the next
host poll) on the same rows and the same injected uniforms, 12 synthetic layers.

Workloads:
  ragged128 / ragged256: 128 / 256 rows, prompts shaped like the committed presets (PRESET_SHAPES: prompt frames, at most 8 enrolled
    prompt text ids), total text length S uniform in 12 .. 38 and no forced EOS (eos_gain 0: no row emits EOS), so every row stops at
    the reference's cap of 16 x S frames (192 .. 608): rows of a micro-batch end at different steps;
  equal64: 64 rows with S in 40 .. 60 (caps 640 .. 960) and force_eos_at = 600: every row ends at frame 600, the same step (the
    control: nothing to gain, the admission cost shows).
Both legs of a workload are warmed up (graph capture), then they alternate for --reps rounds.  Prints one JSON object: per workload and
leg the median audio-s/s (frames / 75 per wall second), wall ms, AR steps, frames / (steps x 32), AR / NAR ms, and whether both legs
returned the same ids.
   python tools/continuous_batch.py [--reps 3] [--out profiles/r08_continuous_batch.json]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import vallex_amd  # noqa: E402,F401
from oracle import synth  # noqa: E402
from oracle.make_golden import CODE2LANG, PRESET_SHAPES  # noqa: E402

MBR, FPS = 32, 75.0          # decode rows; EnCodec frames per audio second


def rows_for(n, seed, s_lo=12, s_hi=38):
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        _, tp, sp, code = PRESET_SHAPES[i % len(PRESET_SHAPES)]
        S = int(rng.integers(s_lo, s_hi + 1))
        en = min(sp, 8)
        a, t = synth.synth_prompt(tp, en, seed=seed * 1000 + i)
        rows.append(dict(text=np.concatenate([t[0], synth.synth_text(S - en, seed * 1000 + 500 + i)]), prompt=a[0], enroll=en,
                         prompt_language=CODE2LANG[code], text_language=("en", "zh", "ja")[i % 3]))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("continuous_batch: no GPU (this tool measures the MI355X; it prints no numbers without one)")
    from vallex_amd.models.vallex import VALLE
    m = VALLE(1024, 16, 12, norm_first=True, add_prenet=False, prefix_mode=1, share_embedding=True, nar_scale_factor=1.0,
              prepend_bos=True, num_quantizers=8, engine_max_batch=256, engine_max_text=256, engine_max_prompt=800,
              engine_max_new=616)
    m.to("cuda:0").load_state_dict(synth.vallex_state_dict(12, 0, eos_gain=0.0), strict=True)
    work = {"ragged128": (rows_for(128, 31), None), "ragged256": (rows_for(256, 32), None), "equal64": (rows_for(64, 33, 40, 60), 600)}
    out = dict(tool="tools/continuous_batch.py", device=torch.cuda.get_device_name(0), layers=12, decode_rows=MBR, reps=args.reps,
               sync_every=8, top_k=10, workloads={})
    all_equal = True
    for name, (rows, fe) in work.items():
        us = synth.uniforms(620, len(rows), 2026)
        kw = dict(top_k=10, uniforms=us, force_eos_at=fe, sync_every=8)

        def leg(cont):
            t0 = time.perf_counter()
            o = m.inference_batch(rows, continuous=cont, **kw)
            w = time.perf_counter() - t0
            return w, m.engine.last_stats(), o

        legs = {"micro_batched": False, "continuous": True}
        ref = {k: leg(v)[2] for k, v in legs.items()}              # warm-up: both legs captured
        eq = all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(ref["micro_batched"], ref["continuous"]))
        res = {k: [] for k in legs}
        for _ in range(args.reps):
            for k, v in legs.items():                              # alternating legs
                w, st, o = leg(v)
                eq = eq and all(np.array_equal(a, b) for a, b in zip(o, ref[k]))
                res[k].append((w, st))
        frames = int(sum(len(o) for o in ref["continuous"]))
        lens = [len(o) for o in ref["continuous"]]
        wl = dict(rows=len(rows), force_eos_at=fe, frames=frames, frames_min=int(min(lens)), frames_max=int(max(lens)), ids_equal=bool(eq))
        for k in legs:
            w = statistics.median(x[0] for x in res[k])
            st = res[k][0][1]
            wl[k] = dict(audio_s_per_s=round(frames / FPS / w, 1), wall_ms=round(w * 1e3, 1),
                         wall_ms_all=[round(x[0] * 1e3, 1) for x in res[k]], ar_steps=int(st["ar_steps"]),
                         frames_per_step_row=round(frames / (st["ar_steps"] * MBR), 3),
                         ar_ms=round(statistics.median(x[1]["ar_ms"] for x in res[k]), 1),
                         nar_ms=round(statistics.median(x[1]["nar_ms"] for x in res[k]), 1))
        wl["ratio_audio_s_per_s"] = round(wl["continuous"]["audio_s_per_s"] / wl["micro_batched"]["audio_s_per_s"], 3)
        out["workloads"][name] = wl
        all_equal = all_equal and eq
        print(json.dumps({name: wl}), file=sys.stderr, flush=True)
    out["ids_equal"] = bool(all_equal)
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    if not all_equal:
        sys.exit("continuous_batch: the two schedules returned different ids")


if __name__ == "__main__":
    main()
