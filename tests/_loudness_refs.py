"""numpy restatement of the loudness contract of include/vallex_hip.h (vx_loudness / vx_finish_loud): K-weighting coefficients, step
energies (vectorised over the steps of a row: every step is its own recursion from rest, so the vector lanes are the device's lanes),
blocks, gates, loudness and gain.  Every float64 operation below is separately rounded, as the contract demands; the only library
calls whose last bit may differ from the C library's are tan / pow / log10, and the tests account for each."""
import math

import numpy as np

RATE_MIN, RATE_MAX = 8000, 192000
ABS_GATE = math.pow(10.0, (-70.0 + 0.691) / 10.0)
FLT_MAX = float(np.finfo(np.float32).max)


def coeffs(rate):
    """{b0, b1, b2, a1, a2} of the shelf, then of the high-pass"""
    fs = float(rate)
    K = math.tan(math.pi * 1681.974450955533 / fs)
    Vh = math.pow(10.0, 3.999843853973347 / 20.0)
    Vb = math.pow(Vh, 0.4996667741545416)
    Q = 0.7071752369554196
    a0 = 1.0 + K / Q + K * K
    c = [(Vh + Vb * (K / Q) + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * (K / Q) + K * K) / a0, 2.0 * (K * K - 1.0) / a0,
         (1.0 - K / Q + K * K) / a0]
    K = math.tan(math.pi * 38.13547087602444 / fs)
    Q = 0.5003270373238773
    a0 = 1.0 + K / Q + K * K
    return np.array(c + [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0], np.float64)


def sanitize(x):
    x = np.asarray(x, np.float32)
    fin = np.isfinite(x)
    return np.where(fin, x, np.float32(0)).astype(np.float64), int((~fin).sum())


def nsteps(n, S):
    return -(-n // S)


def steps(x, rate, c):
    """z [ceil(n / S)]: all steps of the row side by side, each from rest at sample j S - W"""
    S = int(rate) // 10
    W = 2 * S
    y, _ = sanitize(x)
    n = len(y)
    J = nsteps(n, S)
    if J == 0:
        return np.zeros(0, np.float64)
    pad = np.concatenate([np.zeros(W), y, np.zeros(J * S - n)])
    first = np.arange(J) * S                                           # pad index of stream position 0 of step j (row sample j S - W)
    own = np.minimum(S, n - np.arange(J) * S)
    c = [np.float64(v) for v in c]
    s1, s2, t1, t2, z = (np.zeros(J) for _ in range(5))
    for q in range(W + S):
        xq = pad[first + q]
        u = c[0] * xq + s1
        s1 = (c[1] * xq - c[3] * u) + s2
        s2 = c[2] * xq - c[4] * u
        v = c[5] * u + t1
        t1 = (c[6] * u - c[8] * v) + t2
        t2 = c[7] * u - c[9] * v
        if q >= W:
            z = np.where(q - W < own, z + v * v, z)
    return z


def steps_loop(x, rate, c):
    """the same, as a plain sequential loop over Python floats: one step after the other"""
    S = int(rate) // 10
    W = 2 * S
    y = [float(v) for v in sanitize(x)[0]]
    n = len(y)
    c = [float(v) for v in c]
    out = []
    for j in range(nsteps(n, S)):
        s1 = s2 = t1 = t2 = z = 0.0
        for i in range(j * S - W, min((j + 1) * S, n)):
            xq = y[i] if i >= 0 else 0.0
            u = c[0] * xq + s1
            s1 = (c[1] * xq - c[3] * u) + s2
            s2 = c[2] * xq - c[4] * u
            v = c[5] * u + t1
            t1 = (c[6] * u - c[8] * v) + t2
            t2 = c[7] * u - c[9] * v
            if i >= j * S:
                z = z + v * v
        out.append(z)
    return np.array(out, np.float64)


def blocks(z, n, S):
    """m_k of a span of n samples from its step table"""
    z = [float(v) for v in z]
    if n <= 0:
        return []
    if n < 4 * S:
        s = 0.0
        for v in z:
            s = s + v
        return [s / float(n)]
    return [(((z[k] + z[k + 1]) + z[k + 2]) + z[k + 3]) / float(4 * S) for k in range((n - 4 * S) // S + 1)]


def lufs(ms):
    return -0.691 + 10.0 * math.log10(ms) if ms > 0.0 else -math.inf


def reduce(z, n, S, nonfinite=0):
    """vx_loudness_info of a span as a dict"""
    m = blocks(z, n, S)
    above = [v for v in m if v > ABS_GATE]
    gated = []
    if above:
        s = 0.0
        for v in above:
            s = s + v
        rel = 0.1 * (s / float(len(above)))
        gated = [v for v in above if v > rel]
    g = 0.0
    for v in gated:
        g = g + v
    ms = g / float(len(gated)) if gated else 0.0
    return dict(loudness=lufs(ms) if gated else -math.inf, mean_square=ms, max_momentary=lufs(max(m)) if m else -math.inf,
                blocks=len(m), above_abs=len(above), gated=len(gated), nonfinite=int(nonfinite))


def measure(x, rate, c, z=None):
    x = np.asarray(x, np.float32)
    S = int(rate) // 10
    return reduce(steps(x, rate, c) if z is None else z, len(x), S, sanitize(x)[1])


def gate_margin_db(z, n, S):
    """how far, in dB, the nearest block is from either gate (inf without a block above zero): a last bit of log10 / pow cannot flip a
    block whose margin is 0.1 dB"""
    m = [v for v in blocks(z, n, S) if v > 0.0]
    d = [abs(10.0 * math.log10(v / ABS_GATE)) for v in m]
    above = [v for v in m if v > ABS_GATE]
    if above:
        rel = 0.1 * (sum(above) / len(above))
        d += [abs(10.0 * math.log10(v / rel)) for v in above]
    return min(d) if d else math.inf


def gain(loudness, target_lufs, ceiling_db, max_gain_db, peak):
    """double on the host, rounded once to fp32; 1 when nothing passed the gates"""
    if loudness == -math.inf:
        return np.float32(1)
    g = math.pow(10.0, (float(np.float32(target_lufs)) - loudness) / 20.0)
    g = min(g, math.pow(10.0, float(np.float32(max_gain_db)) / 20.0))
    if float(peak) > 0.0:
        g = min(g, math.pow(10.0, float(np.float32(ceiling_db)) / 20.0) / float(np.float32(peak)))
    return np.float32(min(g, FLT_MAX))


def ulp_diff(a, b):
    a, b = np.asarray(a, np.float32).view(np.int32).astype(np.int64), np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(np.where(a < 0, -(a & 0x7fffffff), a) - np.where(b < 0, -(b & 0x7fffffff), b))


# ---- inputs ----------------------------------------------------------------------------------------------------------------------

def tone(n, rate, amp, rng, freq=440.0, noise=1e-4):
    """`amp` of a sine under a slow envelope in [0.7, 1], on a 1e-4-sigma noise floor (-80 dBFS: below the absolute gate)"""
    t = np.arange(n, dtype=np.float64) / rate
    env = 0.85 + 0.15 * np.sin(2 * np.pi * 0.9 * t + rng.uniform(0, 6.28))
    return (amp * env * np.sin(2 * np.pi * freq * t) + noise * rng.standard_normal(n)).astype(np.float32)


def row(n, rate, rng, parts):
    """parts: (fraction of the row, amplitude) in order; amplitude 0 = the noise floor alone"""
    x = np.zeros(n, np.float32)
    a = 0
    for i, (frac, amp) in enumerate(parts):
        b = n if i == len(parts) - 1 else min(n, a + int(round(frac * n)))
        x[a:b] = tone(b - a, rate, amp, rng)
        a = b
    return x


def lengths(rate):
    S = rate // 10
    return {8000: [0, 1, S - 1, S, S + 1, 4 * S - 1, 4 * S, 4 * S + 1, 7 * S + 13, 20 * S + 5], 24000: [4 * S + 1, 6 * S + 7],
            11025: [9 * S + 3]}[rate]


def rows(rate, seed=24):
    """the rows of a rate.  8000: the short ones all tone; 7 S + 13 = a noise-floor lead (blocks the absolute gate removes), then a
    tone; 20 S + 5 = a noise-floor lead, a -51 dBFS tone (passes the absolute gate, removed by the relative one), a -13 dBFS tone."""
    rng = np.random.default_rng(seed)
    S = rate // 10
    out = []
    for n in lengths(rate):
        if n == 20 * S + 5:
            out.append(row(n, rate, rng, [(0.2, 0.0), (0.3, 0.004), (0.5, 0.3)]))
        elif n == 7 * S + 13:
            out.append(row(n, rate, rng, [(0.6, 0.0), (0.4, 0.2)]))
        else:
            out.append(row(n, rate, rng, [(1.0, 0.25)]))
    return out


def quiet_row(n, rate, seed=5):
    """the noise floor alone: blocks, none above the absolute gate"""
    return tone(n, rate, 0.0, np.random.default_rng(seed))
