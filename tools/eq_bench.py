#!/usr/bin/env python
"""Wall time of the equaliser (vx_eq through Engine.eq: the warm-up W of the filter on the host, upload, one launch, download) at
24 kHz, four lines:
   rumble (one section, W 1120) and telephone + presence (six sections)  x  32 rows x 8 s and one 60 s row
Every line is the best of --procs (default 5) FRESH processes; a process makes one warm-up call per line (the first call allocates the
launch buffers and walks the filter's impulse response) and then times --reps calls.  For scale the same process runs vx_loudness on
the same rows: the nearest existing kernel, a fixed two sections with W = 2 S of its own.
   python tools/eq_bench.py [--procs 5] [--out profiles/r33_eq.json]
   python tools/eq_bench.py --steps 128,256,512,1024 --build      build tools/devx_eq<S>/libvallex_hip.so per S (-DVX_EQ_STEP=S on eq.hip)
   python tools/eq_bench.py --steps 128,256,512,1024              the table over S: each library through VX_LIB with VX_DEV=1
VX_EQ_STEP is a constant of the contract; the S with the lowest sum over the four lines is the one the header carries.
The context is created without weights: the entries need none."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RATE = 24000
LINES = [("rumble", 32, 8), ("rumble", 1, 60), ("telephone+presence", 32, 8), ("telephone+presence", 1, 60)]


def voice(L, rng, f0):
    """a voice-like tone with three partials under a slow random envelope, on a DC offset, over a -60 dB noise floor"""
    t = np.arange(L) / RATE
    ph = 2 * np.pi * f0 * t + 0.5 * np.sin(2 * np.pi * 5.0 * t)
    env = np.repeat(rng.uniform(0.2, 1.0, -(-L // 2400)), 2400)[:L]
    return (0.05 + 1e-3 * rng.standard_normal(L) + 0.2 * env * (np.sin(ph) + 0.5 * np.sin(2 * ph) + 0.25 * np.sin(3 * ph))).astype(np.float32)


def child(reps):
    import vallex_amd  # noqa: F401
    from vallex_amd._capi import Engine
    from vallex_amd.utils.generation import Eq
    eng = Engine(num_layers=2, max_batch=1, max_text=8, max_prompt=8, max_new=8, with_vocos=False)
    rng = np.random.default_rng(0)
    rows = {(n, sec): [voice(sec * RATE, rng, 110.0 + 5.0 * r) for r in range(n)] for n, sec in ((32, 8), (1, 60))}
    filt = {"rumble": Eq.rumble().sections(RATE), "telephone+presence": (Eq.telephone() + Eq.presence()).sections(RATE)}

    def best(fn):
        fn()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        return min(t)

    out = dict(step=Engine.eq_plan(filt["rumble"])[1], lines=[], loudness=[])
    for name, n, sec in LINES:
        xs = rows[(n, sec)]
        out["lines"].append(dict(filter=name, rows=n, seconds=sec, warm=Engine.eq_plan(filt[name])[0], wall_ms=best(lambda: eng.eq(xs, filt[name]))))
    for (n, sec), xs in rows.items():
        out["loudness"].append(dict(rows=n, seconds=sec, wall_ms=best(lambda: eng.loudness(xs, RATE))))
    print(json.dumps(out))


def run(lib, procs, reps):
    """the four lines at one library: the best of `procs` fresh processes, every process's figures kept"""
    env = dict(os.environ)
    if lib:
        env.update(VX_DEV="1", VX_LIB=lib)
    runs = []
    for _ in range(procs):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(reps)], env=env, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            raise RuntimeError(f"a child process ended with {r.returncode}; nothing more is started:\n{r.stderr[-2000:]}")
        runs.append(json.loads(r.stdout.strip().split("\n")[-1]))
        print(f"[eq_bench] step {runs[-1]['step']}: process {len(runs)} of {procs}: " + " ".join(f"{ln['wall_ms']:.2f}" for ln in runs[-1]["lines"]) + " ms",
              file=sys.stderr, flush=True)
    res = dict(step=runs[0]["step"], lines=[], loudness=[])
    for i, (name, n, sec) in enumerate(LINES):
        t = [r["lines"][i]["wall_ms"] for r in runs]
        res["lines"].append(dict(filter=name, rows=n, seconds=sec, warm=runs[0]["lines"][i]["warm"], wall_ms=min(t), all_ms=t))
    for i in range(2):
        t = [r["loudness"][i]["wall_ms"] for r in runs]
        res["loudness"].append(dict(rows=runs[0]["loudness"][i]["rows"], seconds=runs[0]["loudness"][i]["seconds"], wall_ms=min(t), all_ms=t))
    res["sum_ms"] = sum(ln["wall_ms"] for ln in res["lines"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", default="")
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        return child(a.reps)
    steps = [int(s) for s in a.steps.split(",") if s]
    if a.build:
        import vallex_amd  # noqa: F401
        from vallex_amd import _build
        for s in steps:
            print(_build.build_library(variant=f"eq{s}:eq.hip:-DVX_EQ_STEP={s}"))
        return
    if steps:
        res = dict(procs=a.procs, reps=a.reps, table=[run(os.path.join(ROOT, "tools", f"devx_eq{s}", "libvallex_hip.so"), a.procs, a.reps) for s in steps])
        for t, s in zip(res["table"], steps):
            assert t["step"] == s, (t["step"], s)
        res["best_step"] = min(res["table"], key=lambda t: t["sum_ms"])["step"]
    else:
        res = dict(procs=a.procs, reps=a.reps, **run("", a.procs, a.reps))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
