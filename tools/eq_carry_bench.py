#!/usr/bin/env python
"""Wall time of the carried-state equaliser (vx_eq_carry through Engine.eq_carry: M on the host, upload, three launches, download) at
24 kHz, four lines:
   hum 50 x 6 Q 35 (six sections) and hum 60 x 4 Q 30 + rumble (five)  x  32 rows x 8 s and one 60 s row
and, in the same process, vx_eq (Engine.eq) on the two filters of these that it accepts: hum 60 x 4 Q 30 + rumble (W = 61 856) and the
rumble filter alone (W = 1 120), carried beside them.
Every line is the best of --procs (default 5) FRESH processes; a process makes one warm-up call per line (the first call allocates the
launch buffers) and then times --reps calls.  The filters run from rest (sections, no priming): what is timed is the stage.
   python tools/eq_carry_bench.py [--procs 5] [--out profiles/r34_eq_carry.json]
   python tools/eq_carry_bench.py --steps 128,256,512,1024 --build     build tools/devx_eqc<S>/libvallex_hip.so per S
                                                                       (-DVX_EQ_CARRY_STEP=S on eq_carry.hip)
   python tools/eq_carry_bench.py --steps 128,256,512,1024             the table over S: each library through VX_LIB with VX_DEV=1
   python tools/eq_carry_bench.py --child --trace                      one 60 s row, a few calls: the process a kernel trace is taken of
VX_EQ_CARRY_STEP is a constant of the contract; the Sc with the lowest sum over the four lines is the one the header carries.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
RATE = 24000
LINES = [("hum50x6", 32, 8), ("hum50x6", 1, 60), ("hum60x4+rumble", 32, 8), ("hum60x4+rumble", 1, 60)]
VERSUS = ["hum60x4+rumble", "rumble"]


def child(reps, trace):
    import vallex_amd  # noqa: F401
    from eq_bench import voice
    from vallex_amd._capi import Engine
    from vallex_amd.utils.generation import Eq
    eng = Engine(num_layers=2, max_batch=1, max_text=8, max_prompt=8, max_new=8, with_vocos=False)
    rng = np.random.default_rng(0)
    hum = lambda L: (0.04 * np.sin(2 * np.pi * 50.0 * np.arange(L) / RATE)).astype(np.float32)
    rows = {(n, sec): [voice(sec * RATE, rng, 110.0 + 5.0 * r) + hum(sec * RATE) for r in range(n)] for n, sec in ((32, 8), (1, 60))}
    filt = {"hum50x6": Eq.hum(50.0, 6, 35.0).sections(RATE), "hum60x4+rumble": (Eq.hum(60.0, 4, 30.0) + Eq.rumble()).sections(RATE),
            "rumble": Eq.rumble().sections(RATE)}
    if trace:
        for _ in range(4):
            eng.eq_carry(rows[(1, 60)], filt["hum50x6"])
        return

    def best(fn):
        fn()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        return min(t)

    out = dict(step=Engine.eq_carry_plan(filt["rumble"])[1], lines=[], versus=[])
    for name, n, sec in LINES:
        xs = rows[(n, sec)]
        out["lines"].append(dict(filter=name, rows=n, seconds=sec, wall_ms=best(lambda: eng.eq_carry(xs, filt[name]))))
    for name in VERSUS:
        for n, sec in ((32, 8), (1, 60)):
            xs = rows[(n, sec)]
            out["versus"].append(dict(filter=name, rows=n, seconds=sec, warm=Engine.eq_plan(filt[name])[0], eq_ms=best(lambda: eng.eq(xs, filt[name])),
                                      eq_carry_ms=best(lambda: eng.eq_carry(xs, filt[name]))))
    print(json.dumps(out))


def run(lib, procs, reps):
    """the lines at one library: the best of `procs` fresh processes, every process's figures kept"""
    env = dict(os.environ)
    if lib:
        env.update(VX_DEV="1", VX_LIB=lib)
    runs = []
    for _ in range(procs):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(reps)], env=env, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            raise RuntimeError(f"a child process ended with {r.returncode}; nothing more is started:\n{r.stderr[-2000:]}")
        runs.append(json.loads(r.stdout.strip().split("\n")[-1]))
        print(f"[eq_carry_bench] step {runs[-1]['step']}: process {len(runs)} of {procs}: " + " ".join(f"{ln['wall_ms']:.2f}" for ln in runs[-1]["lines"]) + " ms",
              file=sys.stderr, flush=True)
    res = dict(step=runs[0]["step"], lines=[], versus=[])
    for i, (name, n, sec) in enumerate(LINES):
        t = [r["lines"][i]["wall_ms"] for r in runs]
        res["lines"].append(dict(filter=name, rows=n, seconds=sec, wall_ms=min(t), all_ms=t))
    for i, v in enumerate(runs[0]["versus"]):
        a, b = [r["versus"][i]["eq_ms"] for r in runs], [r["versus"][i]["eq_carry_ms"] for r in runs]
        res["versus"].append(dict(filter=v["filter"], rows=v["rows"], seconds=v["seconds"], warm=v["warm"], eq_ms=min(a), eq_carry_ms=min(b), eq_all_ms=a,
                                  eq_carry_all_ms=b))
    res["sum_ms"] = sum(ln["wall_ms"] for ln in res["lines"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", default="")
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        return child(a.reps, a.trace)
    steps = [int(s) for s in a.steps.split(",") if s]
    if a.build:
        import vallex_amd  # noqa: F401
        from vallex_amd import _build
        for s in steps:
            print(_build.build_library(variant=f"eqc{s}:eq_carry.hip:-DVX_EQ_CARRY_STEP={s}"))
        return
    if steps:
        res = dict(procs=a.procs, reps=a.reps, table=[run(os.path.join(ROOT, "tools", f"devx_eqc{s}", "libvallex_hip.so"), a.procs, a.reps) for s in steps])
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
