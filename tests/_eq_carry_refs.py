"""numpy restatement of the carried-state equaliser of include/vallex_hip.h (vx_eq_carry_plan / vx_eq_carry): the step matrix M, the
three passes of a row (ends and rows vectorised over the steps, as _eq_refs.eq is: every step is its own recursion, so the vector lanes
are the device's lanes; the chain a Python loop in the contract's order) and the host-side priming of a hum filter.  Every float64
operation below is separately rounded, as the contract demands.  Sections and their checks are _eq_refs'."""
import math

import numpy as np

from tests import _eq_refs as E


def _sec(sections):
    return np.ascontiguousarray(sections, np.float64).reshape(-1, 5)


def _run(s, u, s1, s2):
    """one sample (a vector over the lanes) through the cascade, states in place; the last section's value"""
    for k, c in enumerate(s):
        v = u
        u = c[0] * v + s1[k]
        s1[k] = (c[1] * v - c[3] * u) + s2[k]
        s2[k] = c[2] * v - c[4] * u
    return u


def matrix(sections, Sc):
    """M [D][D]: column k is the state reached from the unit state e_k over Sc zero inputs.  ValueError: a cascade _eq_refs.check
    refuses, or an M that is not finite"""
    s = _sec(sections)
    why = E.check(s)
    if why:
        raise ValueError(why)
    D = 2 * len(s)
    st = np.eye(D)                                                        # lane k starts from e_k
    s1, s2 = st[0::2].copy(), st[1::2].copy()
    for _ in range(Sc):
        _run(s, np.zeros(D), s1, s2)
    m = np.empty((D, D))
    m[0::2], m[1::2] = s1, s2
    if not np.isfinite(m).all():
        raise ValueError("the step matrix is not finite")
    return m


def eq_carry(x, sections, Sc, state_in=None, m=None):
    """(out float32 [n], state_out float64 [D], info dict) of one row"""
    s = _sec(sections)
    D = 2 * len(s)
    m = matrix(s, Sc) if m is None else np.asarray(m, np.float64).reshape(D, D)
    y, fin = E.sanitize(x)
    n = len(y)
    J = -(-n // Sc)
    z0 = np.zeros(D) if state_in is None else np.array(state_in, np.float64).reshape(D)
    info = dict(warm=0, nonfinite=int((~fin).sum()), nonfinite_out=0, peak=np.float32(0))
    if J == 0:
        return np.zeros(0, np.float32), z0, info
    pad = np.concatenate([y, np.zeros(J * Sc - n)]).reshape(J, Sc)
    with np.errstate(over="ignore", invalid="ignore"):
        s1, s2 = np.zeros((len(s), J)), np.zeros((len(s), J))             # ends: every step from rest over Sc samples
        for q in range(Sc):
            _run(s, pad[:, q], s1, s2)
        f = np.empty((J, D))
        f[:, 0::2], f[:, 1::2] = s1.T, s2.T
        z = np.empty((J + 1, D))                                          # chain
        z[0] = z0
        for j in range(J):
            acc = m[:, 0] * z[j, 0]                                       # all components side by side, each its own sum
            for k in range(1, D):
                acc = acc + m[:, k] * z[j, k]
            z[j + 1] = f[j] + acc
        s1, s2 = z[:J, 0::2].T.copy(), z[:J, 1::2].T.copy()               # rows: step j from z_j over its own samples
        out = np.zeros((J, Sc), np.float32)
        last = n - (J - 1) * Sc                                           # samples of the last step
        state = None
        for q in range(Sc):
            out[:, q] = _run(s, pad[:, q], s1, s2).astype(np.float32)
            if q == last - 1:
                state = np.empty(D)
                state[0::2], state[1::2] = s1[:, J - 1], s2[:, J - 1]
    out = out.reshape(-1)[:n].copy()
    bad = ~np.isfinite(out)
    out[bad] = 0
    info["nonfinite_out"] = int(bad.sum())
    info["peak"] = np.abs(out).max()
    return out, state, info


# ---- priming (utils/generation.py: CarriedEq.prime) --------------------------------------------------------------------------------

PRIME_PERIODS, PRIME_CAP_S = 10, 10


def prime_lead(x, sections, rate, prime_hz):
    """the lead of a row, or None when the row starts from rest: the mean of the row's first 10 periods of P = round(rate / prime_hz)
    samples, tiled to the smallest multiple of P that is at least ln(1000) / -ln(r) samples, r = max sqrt(a2) over the sections with
    a2 > 0, and to at most 10 s of samples"""
    s = _sec(sections)
    P = int(round(rate / prime_hz))
    if P < 1 or len(x) < PRIME_PERIODS * P:
        return None
    a2 = [float(c[4]) for c in s if c[4] > 0]
    if not a2:
        return None
    r = max(math.sqrt(v) for v in a2)
    need = math.log(1000.0) / -math.log(r)
    reps = max(1, min(int(math.ceil(need / P)), PRIME_CAP_S * int(rate) // P))
    head = np.where(np.isfinite(x[: PRIME_PERIODS * P]), x[: PRIME_PERIODS * P], np.float32(0)).astype(np.float64)
    period = head.reshape(PRIME_PERIODS, P).mean(axis=0).astype(np.float32)
    return np.tile(period, reps)


def primed(x, sections, Sc, rate, prime_hz):
    """eq_carry of a row from the state its lead (filtered from rest by a call of its own) leaves"""
    lead = prime_lead(x, sections, rate, prime_hz)
    state = None if lead is None else eq_carry(lead, sections, Sc)[1]
    return eq_carry(x, sections, Sc, state)


def hum_specs(f0, harmonics, q, rate):
    """the notches of Eq.hum below the Nyquist of `rate`"""
    return [("notch", f0 * k, q, 0.0) for k in range(1, harmonics + 1) if f0 * k < 0.5 * rate]


def hum_row(n, rate=24000, f0=50.0, harmonics=6, hum_db=-27.0, noise=0.005, dc=0.0, seed=34):
    """(row, its noise alone): mains hum of `harmonics` partials at hum_db dBFS RMS in all over white noise"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / float(rate)
    amp = np.array([1.0 / k for k in range(1, harmonics + 1)])
    hum = sum(a * np.sin(2 * np.pi * f0 * k * t + 0.7 * k) for k, a in zip(range(1, harmonics + 1), amp))
    if n:
        hum = hum * (10.0 ** (hum_db / 20.0) / np.sqrt(np.mean(hum ** 2)))
    nz = noise * rng.standard_normal(n)
    return (dc + hum + nz).astype(np.float32), (dc + nz).astype(np.float32)
