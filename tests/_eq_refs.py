"""numpy restatement of the equaliser contract of include/vallex_hip.h (vx_eq_design / vx_eq_plan / vx_eq): the cookbook designs, the
warm-up W of a cascade, the bounded recursion (vectorised over the steps of a row: every step is its own recursion from rest, so the
vector lanes are the device's lanes) and the unbounded one it is measured against.  Every float64 operation below is separately
rounded, as the contract demands; the only library calls whose last bit may differ from the C library's are sin / cos / pow / sqrt
of `design`, and the tests use the library's coefficients everywhere else."""
import functools
import math

import numpy as np

KINDS = {"highpass": 0, "lowpass": 1, "bandpass": 2, "notch": 3, "peak": 4, "low_shelf": 5, "high_shelf": 6}
MAX_SECTIONS, WARM_MAX = 8, 65536
BOUND = 2.0 ** -24
IDENTITY = np.array([[1.0, 0.0, 0.0, 0.0, 0.0]])


def design(kind, rate, f0, q=math.sqrt(0.5), gain_db=0.0):
    """b0 b1 b2 a1 a2 over a0, the audio-EQ-cookbook forms in the order of operations of csrc/eq_host.h"""
    w0 = 2.0 * math.pi * f0 / float(rate)
    cw, sw, sh, ch = math.cos(w0), math.sin(w0), math.sin(0.5 * w0), math.cos(0.5 * w0)
    al, omc, opc = sw / (2.0 * q), 2.0 * sh * sh, 2.0 * ch * ch
    if kind in ("highpass", "lowpass", "bandpass", "notch"):
        a0, a1, a2 = 1.0 + al, -2.0 * cw, 1.0 - al
        b0, b1, b2 = {"highpass": (0.5 * opc, -opc, 0.5 * opc), "lowpass": (0.5 * omc, omc, 0.5 * omc), "bandpass": (al, 0.0, -al),
                      "notch": (1.0, -2.0 * cw, 1.0)}[kind]
    else:
        A = math.pow(10.0, gain_db / 40.0)
        if kind == "peak":
            b0, b1, b2 = 1.0 + al * A, -2.0 * cw, 1.0 - al * A
            a0, a1, a2 = 1.0 + al / A, -2.0 * cw, 1.0 - al / A
        else:
            r, p, m = 2.0 * math.sqrt(A) * al, A + 1.0, A - 1.0
            if kind == "low_shelf":
                b0, b1, b2 = A * ((p - m * cw) + r), 2.0 * A * (m - p * cw), A * ((p - m * cw) - r)
                a0, a1, a2 = (p + m * cw) + r, -2.0 * (m + p * cw), (p + m * cw) - r
            else:
                b0, b1, b2 = A * ((p + m * cw) + r), -2.0 * A * (m + p * cw), A * ((p + m * cw) - r)
                a0, a1, a2 = (p - m * cw) + r, 2.0 * (m - p * cw), (p - m * cw) - r
    return np.array([b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0], np.float64)


def check(sections):
    """None, or why the cascade is refused"""
    s = np.asarray(sections, np.float64).reshape(-1, 5)
    if not 1 <= len(s) <= MAX_SECTIONS:
        return f"nsections {len(s)} outside 1 .. {MAX_SECTIONS}"
    for k, c in enumerate(s):
        if not np.isfinite(c).all():
            return f"section {k}: coefficient {int(np.argmin(np.isfinite(c)))} (of b0 b1 b2 a1 a2) is not finite"
        if abs(c[4]) >= 1.0 or abs(c[3]) >= 1.0 + c[4]:
            return f"section {k} is unstable"
    return None


def _section(c, x):
    """one section over a whole sequence of Python floats, from rest: the cascade is feed-forward from section to section, so section
    after section over the sequence is sample after sample through the cascade"""
    b0, b1, b2, a1, a2 = (float(v) for v in c)
    s1 = s2 = 0.0
    out = [0.0] * len(x)
    for i, v in enumerate(x):
        u = b0 * v + s1
        s1 = (b1 * v - a1 * u) + s2
        s2 = b2 * v - a2 * u
        out[i] = u
    return out


@functools.lru_cache(maxsize=None)
def _warm(key, n):
    s = np.frombuffer(key, np.float64).reshape(n, 5)
    h = [1.0] + [0.0] * (2 * WARM_MAX - 1)
    for c in s:
        h = _section(c, h)
    T, best = 0.0, None
    for k in range(2 * WARM_MAX - 1, -1, -1):
        T = abs(h[k]) + T
        if T <= BOUND and k % 32 == 0:                                 # T only grows towards k = 0: the last one kept is the smallest
            best = k
    return best, T


def warm(sections):
    """W of the contract: the smallest multiple of 32 with T(W) <= 2^-24.  ValueError: a cascade `check` refuses, or no W up to
    WARM_MAX"""
    s = np.ascontiguousarray(sections, np.float64).reshape(-1, 5)
    why = check(s)
    if why:
        raise ValueError(why)
    W = _warm(s.tobytes(), len(s))[0]
    if W is None or W > WARM_MAX:
        raise ValueError("the filter's memory is too long")
    return W


def l1(sections):
    """T(0): the sum of |h| over the 2 WARM_MAX samples `warm` walks -- the largest gain of the cascade on a bounded input"""
    s = np.ascontiguousarray(sections, np.float64).reshape(-1, 5)
    return _warm(s.tobytes(), len(s))[1]


def sanitize(x):
    x = np.asarray(x, np.float32)
    fin = np.isfinite(x)
    return np.where(fin, x, np.float32(0)).astype(np.float64), fin


def eq(x, sections, W, S):
    """(out float32 [n], info dict) of one row: all steps side by side, each from rest at sample j S - W"""
    s = np.asarray(sections, np.float64).reshape(-1, 5)
    y, fin = sanitize(x)
    n = len(y)
    J = -(-n // S)
    info = dict(warm=int(W), nonfinite=int((~fin).sum()), nonfinite_out=0, peak=np.float32(0))
    if J == 0:
        return np.zeros(0, np.float32), info
    pad = np.concatenate([np.zeros(W), y, np.zeros(J * S - n)])
    first = np.arange(J) * S                                           # pad index of stream position 0 of step j (row sample j S - W)
    s1, s2 = np.zeros((len(s), J)), np.zeros((len(s), J))
    out = np.zeros(J * S, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for q in range(W + S):
            u = pad[first + q]
            for k, c in enumerate(s):
                v = u
                u = c[0] * v + s1[k]
                s1[k] = (c[1] * v - c[3] * u) + s2[k]
                s2[k] = c[2] * v - c[4] * u
            if q >= W:
                out[first + (q - W)] = u.astype(np.float32)
    out = out[:n]
    bad = ~np.isfinite(out)
    out[bad] = 0
    info["nonfinite_out"] = int(bad.sum())
    info["peak"] = np.abs(out).max() if n else np.float32(0)
    return out, info


def full(x, sections):
    """the unbounded recursion over the whole row from rest at sample 0, float64 and unrounded"""
    u = [float(v) for v in sanitize(x)[0]]
    for c in np.asarray(sections, np.float64).reshape(-1, 5):
        u = _section(c, u)
    return np.array(u, np.float64)


def response(sections, freqs, rate):
    """|H| of the cascade at freqs (Hz), from the coefficients"""
    z = np.exp(-2j * np.pi * np.asarray(freqs, np.float64) / float(rate))
    h = np.ones(len(z), np.complex128)
    for b0, b1, b2, a1, a2 in np.asarray(sections, np.float64).reshape(-1, 5):
        h = h * (b0 + b1 * z + b2 * z * z) / (1.0 + a1 * z + a2 * z * z)
    return np.abs(h)


# ---- filters and inputs ------------------------------------------------------------------------------------------------------------

# (name, rate, specs (kind, f0, q, gain_db)): the six filters the contract's W table was drawn up with
FILTERS = [
    ("rumble", 24000, [("highpass", 80.0, 0.7071, 0.0)]),
    ("highpass 20 Hz at 48 kHz", 48000, [("highpass", 20.0, 0.7071, 0.0)]),
    ("telephone", 24000, [("highpass", 300.0, 0.5412, 0.0), ("highpass", 300.0, 1.3066, 0.0), ("lowpass", 3400.0, 0.5412, 0.0),
                          ("lowpass", 3400.0, 1.3066, 0.0)]),
    ("presence", 24000, [("peak", 3000.0, 1.0, 4.0), ("high_shelf", 8000.0, 0.7071, 3.0)]),
    ("low shelf 100 Hz +6 dB", 24000, [("low_shelf", 100.0, 0.7071, 6.0)]),
    ("peak 1 kHz Q 8 -12 dB", 24000, [("peak", 1000.0, 8.0, -12.0)]),
]
HUM_NOTCH = (24000, ("notch", 50.0, 100.0, 0.0))          # the stated limit: refused


def noise_row(n, seed=33, dc=0.0, amp=0.25):
    """white noise of `amp` sigma on a DC offset"""
    return (dc + amp * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)
