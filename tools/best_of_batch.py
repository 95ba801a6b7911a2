#!/usr/bin/env python
"""Batched best_of against one call per request: K = 6 requests shaped like the reference UI's call (launch-ui.py:285-295:
top_k=-100, temperature 1, best_of=5) on 12 synthetic layers, prompts shaped like committed presets, every beam forced to end at
FR frames (fixed work).  Leg (a) runs the K requests as K batch-1 calls (the only option before batched best_of), leg (b) as ONE
call of K rows (K x 5 = 30 decode rows).  Both shapes are warmed up (graph capture), then the legs alternate for --reps rounds.
Prints one JSON object: requests/s, AR ms and NAR ms per leg (median over the rounds; leg (a) summed over its K calls), the
batched / sequential ratio, and whether both legs returned the same ids under the same injected uniforms.
   python tools/best_of_batch.py [--reps 3] [--frames 400] [--out profiles/r07_best_of_batch.json]"""
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

K, N = 6, 5
SHAPES = ["acou_1", "amused", "bronya", "anger", "vctk_1", "neutral"]       # (prompt frames, prompt text ids) of these presets
N_TEXT = [40, 25, 60, 33, 48, 20]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("best_of_batch: no GPU (this tool measures the MI355X; it prints no numbers without one)")
    from vallex_amd.models.vallex import VALLE
    fr = args.frames
    m = VALLE(1024, 16, 12, norm_first=True, add_prenet=False, prefix_mode=1, share_embedding=True, nar_scale_factor=1.0,
              prepend_bos=True, num_quantizers=8, engine_max_batch=32, engine_max_text=256, engine_max_prompt=400,
              engine_max_new=fr + 8)
    m.to("cuda:0").load_state_dict(synth.vallex_state_dict(12, 0, eos_gain=0.0), strict=True)
    shape = {name: (tp, sp, code) for name, tp, sp, code in PRESET_SHAPES}
    rows = []
    for i, name in enumerate(SHAPES):
        tp, sp, code = shape[name]
        a, t = synth.synth_prompt(tp, sp, seed=800 + i)
        rows.append(dict(text=np.concatenate([t[0], synth.synth_text(N_TEXT[i], 900 + i)]), prompt=a[0], enroll=sp,
                         prompt_language=CODE2LANG[code], text_language=("en", "zh", "ja")[i % 3]))
    us = synth.uniforms(fr + 8, K * N, 2026)
    kw = dict(top_k=-100, temperature=1.0, force_eos_at=fr, best_of=N, sync_every=16)

    def sequential():
        t0 = time.perf_counter()
        outs, ar, nar = [], 0.0, 0.0
        for i, r in enumerate(rows):
            outs += m.inference_batch([r], uniforms=us[:, N * i:N * i + N], **kw)
            st = m.engine.last_stats()
            ar += st["ar_ms"]; nar += st["nar_ms"]
        return time.perf_counter() - t0, ar, nar, outs

    def batched():
        t0 = time.perf_counter()
        outs = m.inference_batch(rows, uniforms=us, **kw)
        w = time.perf_counter() - t0
        st = m.engine.last_stats()
        return w, st["ar_ms"], st["nar_ms"], outs

    legs = {"sequential": sequential, "batched": batched}
    ref = {k: f()[3] for k, f in legs.items()}                    # warm-up: both shapes captured
    ids_equal = len(ref["sequential"]) == len(ref["batched"]) == K and all(
        a.shape == b.shape and np.array_equal(a, b) for a, b in zip(ref["sequential"], ref["batched"]))
    res = {k: dict(wall_s=[], ar_ms=[], nar_ms=[]) for k in legs}
    for _ in range(args.reps):
        for k, f in legs.items():                                 # alternating legs
            w, ar, nar, outs = f()
            ids_equal = ids_equal and all(np.array_equal(a, b) for a, b in zip(outs, ref[k]))
            res[k]["wall_s"].append(w); res[k]["ar_ms"].append(ar); res[k]["nar_ms"].append(nar)
    out = dict(tool="tools/best_of_batch.py", device=torch.cuda.get_device_name(0), layers=12, requests=K, best_of=N, frames=fr,
               reps=args.reps, frames_per_request=[int(len(o)) for o in ref["batched"]], ids_equal=bool(ids_equal))
    for k in legs:
        w = statistics.median(res[k]["wall_s"])
        out[k] = dict(requests_per_s=round(K / w, 3), wall_ms=round(w * 1e3, 1), ar_ms=round(statistics.median(res[k]["ar_ms"]), 1),
                      nar_ms=round(statistics.median(res[k]["nar_ms"]), 1), wall_ms_all=[round(x * 1e3, 1) for x in res[k]["wall_s"]])
    out["ratio_requests_per_s"] = round(out["batched"]["requests_per_s"] / out["sequential"]["requests_per_s"], 3)
    out["ratio_ar_ms"] = round(out["sequential"]["ar_ms"] / out["batched"]["ar_ms"], 3)
    out["ratio_nar_ms"] = round(out["sequential"]["nar_ms"] / out["batched"]["nar_ms"], 3)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    if not ids_equal:
        sys.exit("best_of_batch: the batched call returned other ids than the per-request calls")


if __name__ == "__main__":
    main()
