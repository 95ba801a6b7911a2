"""The contract of vx_finish (include/vallex_hip.h) restated in numpy, statement by statement: frames by cumsum, the active rule, the
span, the gain, the smoothstep tables, the apply pass and the S16 rule with np.rint.  Everything the device and the host code are
compared with comes from here; tests/test_finish_refs.py holds this file to a sequential Python loop and to the rule's edge cases."""
import math

import numpy as np

FRAMES = (16, 240, 441)
F32, S16 = 0, 1
NONE, PEAK, RMS = 0, 1, 2
DEFAULTS = dict(silence_db=-40.0, trim=0, keep=0, level_mode=0, level_db=-1.0, max_gain_db=20.0, fade_in=0, fade_out=0, pcm16=False)
SENT_F = np.float32(-1.0e30)
SENT_H = np.int16(-12345)


def sanitize(x):
    """y = isfinite(x) ? x : 0 and the number of non-finite samples"""
    x = np.asarray(x, np.float32)
    fin = np.isfinite(x)
    return np.where(fin, x, np.float32(0)).astype(np.float32), int((~fin).sum())


def nframes(L, F):
    return -(-L // F)


def frames(x, F):
    """the frame table of a row: e (float64: the sequential sum of the exact squares), p (float32 max |y|), z (non-finite count)"""
    x = np.asarray(x, np.float32)
    nf = nframes(len(x), F)
    e, p, z = np.zeros(nf, np.float64), np.zeros(nf, np.float32), np.zeros(nf, np.int32)
    for f in range(nf):
        y, z[f] = sanitize(x[f * F: (f + 1) * F])
        e[f] = np.cumsum(y.astype(np.float64) ** 2)[-1]
        p[f] = np.abs(y).max()
    return e, p, z


def thr2(silence_db):
    return math.pow(10.0, float(np.float32(silence_db)) / 10.0)


def frame_counts(L, F):
    return np.minimum(F, L - F * np.arange(nframes(L, F))).astype(np.int64)


def margin(x, F, silence_db):
    """min over the frames of |log2(e_f / (thr2 n_f))|: how far every frame is from flipping between silent and active"""
    e, _, _ = frames(x, F)
    if not len(e):
        return math.inf
    with np.errstate(divide="ignore"):
        return float(np.abs(np.log2(e / (thr2(silence_db) * frame_counts(len(x), F)))).min())


def span(L, F, active, trim, keep):
    """[begin, end) from the active flags of the frames"""
    idx = np.flatnonzero(active)
    if not len(idx):
        return (0, 0) if trim & 3 else (0, L)
    a, z = int(idx[0]), int(idx[-1])
    begin = max(0, a * F - keep) if trim & 1 else 0
    end = min(L, (z + 1) * F + keep) if trim & 2 else L
    return begin, end


def gain(level_mode, level_db, max_gain_db, peak, mean_square, any_active):
    """double on the host, rounded once to fp32; 1 with no level, no active frame or a zero denominator"""
    if level_mode == NONE or not any_active:
        return np.float32(1)
    den = float(peak) if level_mode == PEAK else math.sqrt(mean_square)
    if den == 0.0:
        return np.float32(1)
    t = math.pow(10.0, float(np.float32(level_db)) / 20.0)
    cap = math.pow(10.0, float(np.float32(max_gain_db)) / 20.0)
    return np.float32(min(t / den, cap, float(np.finfo(np.float32).max)))


def measure(x, F, silence_db=-40.0, trim=0, keep=0, level_mode=0, level_db=-1.0, max_gain_db=20.0, table=None, **_):
    """vx_wave_info of a row as a dict (clipped = 0: nothing was applied); table: frames(x, F) where the caller has it already"""
    x = np.asarray(x, np.float32)
    L = len(x)
    e, p, z = frames(x, F) if table is None else table
    n = frame_counts(L, F)
    active = e > thr2(silence_db) * n.astype(np.float64)
    begin, end = span(L, F, active, trim, keep)
    ms = 0.0
    if active.any():
        es = 0.0
        for v in e[active]:                       # frame order, double
            es += float(v)
        ms = es / float(n[active].sum())
    peak = np.float32(p[begin // F: (end - 1) // F + 1].max()) if end > begin else np.float32(0)
    return dict(begin=begin, end=end, active_frames=int(active.sum()), nonfinite=int(z.sum()), clipped=0, peak=peak,
                gain=gain(level_mode, level_db, max_gain_db, peak, ms, bool(active.any())), mean_square=ms)


def fade_table(n):
    """w(u) = u u (3 - 2u), u = (j + 0.5) / n, in double, rounded once"""
    u = (np.arange(n, dtype=np.float64) + 0.5) / np.float64(max(n, 1))
    return (u * u * (3.0 - 2.0 * u)).astype(np.float32)


def apply(x, begin, end, g, fade_in=0, fade_out=0, pcm16=False):
    """the kept span through gain, fades and format: (out, clipped)"""
    y, _ = sanitize(np.asarray(x, np.float32)[begin:end])
    n = end - begin
    v = (y * np.float32(g)).astype(np.float32)
    i = np.arange(n)
    if fade_in:
        m = i < fade_in
        v[m] = v[m] * fade_table(fade_in)[i[m]]
    if fade_out:
        k = n - 1 - i
        m = k < fade_out
        v[m] = v[m] * fade_table(fade_out)[k[m]]
    if not pcm16:
        return v, int((np.abs(v) > 1).sum())
    r = np.rint(v * np.float32(32768.0))
    c = np.clip(r, -32768.0, 32767.0)
    return c.astype(np.int16), int((c != r).sum())


def finish(x, F, gain_used=None, **kw):
    """(out, info) of one row: measure, then apply with the measured gain -- or with gain_used, the gain a device call reported (pow
    may differ by an ulp between libraries; everything behind the gain is exact)"""
    o = dict(DEFAULTS, **kw)
    info = measure(x, F, **o)
    if gain_used is not None:
        assert ulp_diff([gain_used], [info["gain"]])[0] <= 1, (gain_used, info["gain"])
        info["gain"] = np.float32(gain_used)
    out, info["clipped"] = apply(x, info["begin"], info["end"], info["gain"], o["fade_in"], o["fade_out"], o["pcm16"])
    return out, info


def ulp_diff(a, b):
    a, b = np.asarray(a, np.float32).view(np.int32).astype(np.int64), np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(np.where(a < 0, -(a & 0x7fffffff), a) - np.where(b < 0, -(b & 0x7fffffff), b))


# ---- the inputs of the tests -------------------------------------------------------------------------------------------------
def row(L, F, lead, tail, rng):
    """1e-4-sigma noise; between `lead` and `tail` samples of it, a 440 Hz tone (the rate is 100 F) of amplitude 0.25 times a random
    envelope in [0.6, 1]"""
    x = (1e-4 * rng.standard_normal(L)).astype(np.float32)
    m = L - lead - tail
    if m > 0:
        t = np.arange(lead, L - tail)
        env = rng.uniform(0.6, 1.0, m)
        x[lead: L - tail] += (0.25 * env * np.sin(2 * np.pi * 440.0 * t / (100.0 * F) + 0.3)).astype(np.float32)
    return x


def lengths(F):
    return [0, 1, F - 1, F, F + 1, 3 * F + 7, 4801, 13001]


def rows(F, seed=22):
    """the eight rows of a frame size: the short ones all tone, the three long ones between a lead and a tail of noise"""
    rng = np.random.default_rng(seed)
    edges = {3 * F + 7: (F, F), 4801: (1000, 700), 13001: (2500, 3100)}
    return [row(L, F, *edges.get(L, (0, 0)), rng) for L in lengths(F)]
