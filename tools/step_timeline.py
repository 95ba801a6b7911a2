#!/usr/bin/env python
"""Kernel-development aid: where does the time of ONE decode layer go -- inside the kernels or between them?
The dev library (python vall-e-x_amd/_build.py --dev) stamps the 100 MHz wall clock in thread 0 of every workgroup of the
decode kernels; this script replays a one-layer step graph (QKV | dec_attn | reduce+LN | linear1 | linear2 | reduce+LN |
predict | sampler) on the state of a real batch-32 run and prints the timeline of the last replay.
   python tools/step_timeline.py            one layer: every replay re-reads the same 45 MB of weights (they stay in the memory-side cache)
   python tools/step_timeline.py --step     the whole 12-layer step: the stamps left are the LAST layer's, whose weights are cold"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import vallex_amd  # noqa: E402,F401
from vallex_amd import _capi  # noqa: E402

_capi.LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dev", "libvallex_hip.so")
from oracle import synth  # noqa: E402
from vallex_amd.models.vallex import VALLE  # noqa: E402

FR = 300
m = VALLE(1024, 16, 12, norm_first=True, add_prenet=False, prefix_mode=1, share_embedding=True, nar_scale_factor=1.0,
          prepend_bos=True, num_quantizers=8, engine_max_batch=32, engine_max_text=256, engine_max_prompt=320,
          engine_max_new=FR + 8)
m.to("cuda:0").load_state_dict(synth.vallex_state_dict(12, 0, eos_gain=0.0), strict=True)
eng = m.engine
batch = m.make_batch(bench.make_rows(0, 32))
eng.infer(batch, top_k=10, seed=1, force_eos_at=FR, sync_every=16)
eng.ar_prefill(batch)                               # live rows again (the run above ended with every row finished)
for _ in range(3):
    eng.ar_step(np.full(32, 5, np.int32))
WHOLE = "--step" in sys.argv
us, _ = eng.bench_kernel(4 if WHOLE else 3, 20, 0)
print(f"{'12-layer step graph (stamps: layer 11)' if WHOLE else 'one-layer step graph'}: {us:.1f} us per replay (20 replays back to back)")
print("switches:", {k: os.environ.get(k, "default") for k in ("VX_L2_KMAP", "VX_L1_INTERLEAVE")})
st = np.zeros(8 * 512 * 8, np.uint64)
eng.lib.vx_dev_stamps(st.ctypes.data_as(C.POINTER(C.c_uint64)))
st = st.reshape(8, 512, 8).astype(np.int64)
names = ["QKV", "linear2", "predict", "linear1", "reduce+LN<16>", "reduce+LN<8>", "dec_attn", "sampler"]
order = [0, 6, 4, 3, 1, 5, 2, 7]                  # launch order inside the step
t0 = min(int(st[k, :, 0][st[k, :, 0] > 0].min()) for k in order if (st[k, :, 0] > 0).any())
print(f"{'kernel':14s} {'WGs':>4s} | first start  last start | stamp offsets from the kernel's first start (avg / max over workgroups), us")
prev_end = None
for k in order:
    live = st[k, :, 0] > 0
    if not live.any():
        continue
    s = st[k][live]
    first = int(s[:, 0].min())
    cols = []
    for j in range(1, 8):
        v = s[:, j][s[:, j] > 0]
        if v.size:
            cols.append(f"s{j}: {(v.mean() - first) / 100:5.2f}/{(v.max() - first) / 100:5.2f}")
    end = max(int(s[:, j].max()) for j in range(8))
    gap = "" if prev_end is None else f"  gap since previous kernel's last stamp: {(first - prev_end) / 100:5.2f}"
    print(f"{names[k]:14s} {int(live.sum()):4d} | {(first - t0) / 100:8.2f}   {(s[:, 0].max() - t0) / 100:8.2f}   | " + "  ".join(cols) + gap)
    prev_end = end

if WHOLE:
    # linear1, lane 0 of every wave (layer 11 of the last replay): is the wave that ends last the one whose loads were issued last,
    # and how much of the tail is the wait at the barrier?  [workgroup][wave][0 start, 1 requests issued, 2 last MFMA, 3 behind the barrier]
    ws = np.zeros(256 * 8 * 4, np.uint64)
    eng.lib.vx_dev_wave_stamps(ws.ctypes.data_as(C.POINTER(C.c_uint64)))
    ws = ws.reshape(256, 8, 4).astype(np.int64)
    ws = ws[(ws > 0).all((1, 2))]
    base = ws[:, :, 0].min(1, keepdims=True)
    rel = (ws - base[:, :, None]) / 100.0
    print(f"linear1 per wave, {len(ws)} workgroups, us from the workgroup's first wave start (mean over workgroups)")
    print("wave   start  issued  last MFMA  behind barrier")
    for w in range(8):
        print(f"{w:4d}  {rel[:, w, 0].mean():6.2f}  {rel[:, w, 1].mean():6.2f}  {rel[:, w, 2].mean():9.2f}  {rel[:, w, 3].mean():14.2f}")
    last_mfma, last_issue = ws[:, :, 2].argmax(1), ws[:, :, 1].argmax(1)
    order_i, order_m = ws[:, :, 1].argsort(1).argsort(1), ws[:, :, 2].argsort(1).argsort(1)
    rho = np.mean([np.corrcoef(a, b)[0, 1] for a, b in zip(order_i, order_m)])
    print(f"the wave with the last MFMA is the wave that issued last in {np.mean(last_mfma == last_issue) * 100:.0f} % of the workgroups;"
          f" it is among waves 4 .. 7 in {np.mean(last_mfma >= 4) * 100:.0f} %; mean rank correlation issue order / MFMA-end order {rho:.2f}")
    spread = (ws[:, :, 2].max(1) - ws[:, :, 2].min(1)) / 100.0
    wait0 = (ws[:, :, 2].max(1) - ws[:, 0, 2]) / 100.0
    sum_t = (st[3][:len(ws), 4].astype(np.int64) - ws[:, 0, 3]) / 100.0 if len(ws) == 256 else np.zeros(1)
    print(f"last MFMA, slowest wave - fastest wave: {spread.mean():.2f} us (max {spread.max():.2f}); wave 0 waits {wait0.mean():.2f} us for the slowest;"
          f" barrier release -> wave 0's store issued (the final sum): {sum_t.mean():.2f} us (max {sum_t.max():.2f})")
