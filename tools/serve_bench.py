#!/usr/bin/env python
"""A serving session against what a server must do without one, on requests that arrive over time.

Setup: 12 synthetic layers (eos_gain 0: no beam emits EOS, every beam of a request runs to the reference's cap of 16 x S frames),
K requests shaped like the reference UI's call (launch-ui.py:285-295: top_k=-100, temperature 1, best_of=5), prompts shaped like the
committed presets (PRESET_SHAPES, at most 8 enrolled prompt text ids), total text length S uniform in --s-lo .. --s-hi (ragged caps),
arrival times from a fixed seed (exponential gaps of mean --gap-ms).  Every request carries its own injected uniforms, so both legs
return the same ids; the tool checks that.
  session  one serving session (Engine.serve): every request is submitted at its arrival, between vx_serve_run calls of --run-steps
           decode steps, and is done when its codes are delivered;
  batched  today's server: whenever requests have arrived, ONE vx_infer best_of call on all of them (6 rows x 5 beams per
           micro-batch); requests arriving during the call wait for the next one.
Both legs are warmed up once (graph capture), then they alternate for --reps rounds.  Prints one JSON object: per leg the median
requests/s (K / (last completion - first arrival)), mean and p95 latency from arrival to codes, AR steps, AR / NAR ms and the
fraction of beam rows live per decode step (5 x frames / (steps x 32): every beam of a request runs to the same cap).
--cancel-frac F adds a third leg, session_cancel: a seeded share F of the requests are cancel candidates, and each candidate that
is still undelivered at the first point between two vx_serve_run calls lying --cancel-after-ms after its arrival is cancelled
(vx_serve_cancel).  Which candidates that catches depends on wall-clock timing, so every repeat records how many it cancelled
("cancelled"), and ids are compared only for requests delivered in both runs.  The JSON then also compares the latency of the
requests that are not candidates with and without the cancellations ("cancel").
--top-p / --repetition-penalty / --repetition-window / --min-frames give every session request those logit filters
(vx_serve_submit_filtered).  With the defaults (1, 1, 0, 0) the session submits exactly as without them.  vx_infer has no filters, so
with any of them set the batched leg still runs unfiltered, for the timing only, and ids are compared between the repeats of the
session legs alone; the JSON records the values under "filters".
   python tools/serve_bench.py [--requests 24] [--gap-ms 60] [--reps 2] [--cancel-frac 0.25] [--out profiles/r09_serve.json]"""
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

N, MBR = 5, 32


def requests_for(k, seed, s_lo, s_hi):
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(k):
        _, tp, sp, code = PRESET_SHAPES[(7 * i) % len(PRESET_SHAPES)]
        S = int(rng.integers(s_lo, s_hi + 1))
        en = min(sp, 8)
        a, t = synth.synth_prompt(tp, en, seed=seed * 1000 + i)
        rows.append(dict(text=np.concatenate([t[0], synth.synth_text(S - en, seed * 1000 + 500 + i)]), prompt=a[0], enroll=en,
                         prompt_language=CODE2LANG[code], text_language=("en", "zh", "ja")[i % 3]))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=24)
    ap.add_argument("--gap-ms", type=float, default=60.0)
    ap.add_argument("--s-lo", type=int, default=10)
    ap.add_argument("--s-hi", type=int, default=24)
    ap.add_argument("--run-steps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--cancel-frac", type=float, default=0.0)
    ap.add_argument("--cancel-after-ms", type=float, default=100.0)
    ap.add_argument("--top-p", type=float, default=1.0)
    ap.add_argument("--repetition-penalty", type=float, default=1.0)
    ap.add_argument("--repetition-window", type=int, default=0)
    ap.add_argument("--min-frames", type=int, default=0)
    args = ap.parse_args()
    flt = {}                                          # only what differs from the neutral values: the default run submits as before
    if args.top_p != 1.0:
        flt["top_p"] = args.top_p
    if args.repetition_penalty != 1.0:
        flt["repetition_penalty"] = args.repetition_penalty
    if args.repetition_window != 0:
        flt["repetition_window"] = args.repetition_window
    if args.min_frames != 0:
        flt["min_frames"] = args.min_frames
    import torch
    if not torch.cuda.is_available():
        sys.exit("serve_bench: no GPU (this tool measures the MI355X; it prints no numbers without one)")
    from vallex_amd.models.vallex import VALLE
    K = args.requests
    cap = 16 * args.s_hi
    m = VALLE(1024, 16, 12, norm_first=True, add_prenet=False, prefix_mode=1, share_embedding=True, nar_scale_factor=1.0,
              prepend_bos=True, num_quantizers=8, engine_max_batch=32, engine_max_text=256, engine_max_prompt=800,
              engine_max_new=cap + 8)
    m.to("cuda:0").load_state_dict(synth.vallex_state_dict(12, 0, eos_gain=0.0), strict=True)
    rows = requests_for(K, 41, args.s_lo, args.s_hi)
    us = [synth.uniforms(cap + 8, N, 5_000 + i) for i in range(K)]
    gaps = np.random.default_rng(2026).exponential(args.gap_ms / 1000.0, size=K)
    arrive = np.concatenate([[0.0], np.cumsum(gaps[1:])])
    eng = m.engine
    n_cancel = int(round(args.cancel_frac * K))
    to_cancel = set(np.random.default_rng(7).choice(K, size=n_cancel, replace=False).tolist()) if n_cancel else set()
    keep = [i for i in range(K) if i not in to_cancel]

    def session(cancel=frozenset()):
        done_t, codes = [None] * K, [None] * K
        st = dict(ar_steps=0, ar_ms=0.0, nar_ms=0.0, frames=0)
        with eng.serve(top_k=-100, temperature=1.0, sync_every=8) as sess:
            rid2i, nxt = {}, 0
            t0 = time.perf_counter()

            def on_done(rid, c):
                i = rid2i[rid]
                done_t[i] = time.perf_counter() - t0
                codes[i] = c

            live, i2rid, cancelled = 0, {}, set()
            while nxt < K or live:
                now = time.perf_counter() - t0
                for i in sorted(cancel - cancelled):
                    if i in i2rid and done_t[i] is None and now - arrive[i] >= args.cancel_after_ms / 1000.0:
                        sess.cancel(i2rid[i])
                        cancelled.add(i)
                if nxt < K and arrive[nxt] > now and not live:
                    time.sleep(arrive[nxt] - now)
                    now = time.perf_counter() - t0
                k0 = nxt
                while nxt < K and arrive[nxt] <= now:
                    nxt += 1
                if nxt > k0:
                    ids = sess.submit(m.make_batch(rows[k0:nxt]), [dict(best_of=N, uniforms=us[i], **flt) for i in range(k0, nxt)])
                    rid2i.update({rid: i for rid, i in zip(ids, range(k0, nxt))})
                    i2rid.update({i: rid for rid, i in zip(ids, range(k0, nxt))})
                live, waiting = sess.run(args.run_steps, on_done)
                live += waiting
                s = eng.last_stats()
                for key in st:
                    st[key] += s[key]
        return done_t, codes, st

    def batched():
        done_t, codes = [None] * K, [None] * K
        st = dict(ar_steps=0, ar_ms=0.0, nar_ms=0.0, frames=0)
        nxt = 0
        t0 = time.perf_counter()
        while nxt < K:
            now = time.perf_counter() - t0
            if arrive[nxt] > now:
                time.sleep(arrive[nxt] - now)
                now = time.perf_counter() - t0
            k0 = nxt
            while nxt < K and arrive[nxt] <= now:
                nxt += 1
            outs = m.inference_batch(rows[k0:nxt], top_k=-100, temperature=1.0, best_of=N, sync_every=8,
                                     uniforms=np.concatenate(us[k0:nxt], axis=1))
            t = time.perf_counter() - t0
            s = eng.last_stats()
            for key in st:
                st[key] += s[key]
            for i, o in zip(range(k0, nxt), outs):
                done_t[i], codes[i] = t, o
        return done_t, codes, st

    legs = {"session": session, "batched": batched}
    if to_cancel:
        legs["session_cancel"] = lambda: session(frozenset(to_cancel))
    ref = {k: f()[1] for k, f in legs.items()}                       # warm-up: graph capture of both legs
    ids_equal = bool(flt) or all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(ref["session"], ref["batched"]))
    if to_cancel:       # the requests that were not cancelled return what they return without the cancellations
        ids_equal = ids_equal and all(np.array_equal(ref["session_cancel"][i], ref["session"][i]) for i in keep)
        ids_equal = ids_equal and all(np.array_equal(a, b) for a, b in zip(ref["session_cancel"], ref["session"]) if a is not None)
    res = {k: dict(req_per_s=[], lat_mean_ms=[], lat_p95_ms=[], ar_steps=[], ar_ms=[], nar_ms=[], live_frac=[], kept_lat_mean_ms=[],
                   kept_lat_p95_ms=[], cancelled=[]) for k in legs}
    for _ in range(args.reps):
        for k, f in legs.items():
            done_t, codes, st = f()
            ids_equal = ids_equal and all(np.array_equal(a, b) for a, b in zip(codes, ref[k]) if a is not None and b is not None)
            got = [i for i in range(K) if done_t[i] is not None]
            lat = (np.array([done_t[i] for i in got]) - arrive[got]) * 1000.0
            kl = (np.array([done_t[i] for i in keep]) - arrive[keep]) * 1000.0
            r = res[k]
            r["req_per_s"].append(len(got) / (max(done_t[i] for i in got) - arrive[0]))
            r["lat_mean_ms"].append(float(lat.mean()))
            r["lat_p95_ms"].append(float(np.percentile(lat, 95)))
            r["kept_lat_mean_ms"].append(float(kl.mean()))
            r["kept_lat_p95_ms"].append(float(np.percentile(kl, 95)))
            r["cancelled"].append(K - len(got))
            r["ar_steps"].append(st["ar_steps"]); r["ar_ms"].append(st["ar_ms"]); r["nar_ms"].append(st["nar_ms"])
            r["live_frac"].append(N * st["frames"] / max(1, st["ar_steps"] * MBR))
    out = dict(tool="tools/serve_bench.py", device=torch.cuda.get_device_name(0), layers=12, requests=K, best_of=N,
               gap_ms=args.gap_ms, arrival_span_s=float(arrive[-1]), text_len=[args.s_lo, args.s_hi], run_steps=args.run_steps,
               reps=args.reps, filters=flt, frames_per_request=[int(len(o)) for o in ref["session"]], ids_equal=bool(ids_equal),
               legs={k: {m_: round(float(statistics.median(v)), 3) for m_, v in r.items()} for k, r in res.items()},
               spread={k: {m_: [round(float(min(v)), 3), round(float(max(v)), 3)] for m_, v in r.items()} for k, r in res.items()})
    s_, b_ = out["legs"]["session"], out["legs"]["batched"]
    out["session_over_batched"] = dict(req_per_s=round(s_["req_per_s"] / b_["req_per_s"], 3),
                                       lat_mean=round(s_["lat_mean_ms"] / b_["lat_mean_ms"], 3))
    if to_cancel:
        c_ = out["legs"]["session_cancel"]
        out["cancel"] = dict(frac=args.cancel_frac, after_ms=args.cancel_after_ms, candidates=sorted(to_cancel),
                             cancelled_per_rep=res["session_cancel"]["cancelled"],
                             kept_lat_mean_ms=[s_["kept_lat_mean_ms"], c_["kept_lat_mean_ms"]],
                             kept_lat_p95_ms=[s_["kept_lat_p95_ms"], c_["kept_lat_p95_ms"]],
                             note="[without cancellation, with cancellation], latency of the requests that are not cancelled")
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
