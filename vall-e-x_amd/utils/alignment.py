"""Frame-to-text segments from the attention `VALLE.align` returns (numpy only)."""
from __future__ import annotations

import numpy as np

FLOOR = 1e-30      # attention below this counts as this (log of an exact zero)


def monotonic_segments(attn: np.ndarray, enroll: int) -> np.ndarray:
    """The best monotone path of the T frames through the text that was synthesised, columns enroll .. S-1 of attn (T, S).

    The path s_0 .. s_{T-1} starts at column `enroll`, ends at column S - 1 and moves 0 or 1 columns per frame; it maximises
    sum_t log(max(attn[t, s_t], 1e-30)) (Viterbi, float64).  Ties go to the smaller column: walking back from the last frame, a
    frame whose two possible predecessors score the same takes the smaller one.  Returns (S - enroll, 2) int32, the first and the
    last frame of every column.  Raises ValueError when T < S - enroll (no such path).

    This is a rule, not a judgement: it is followed whatever attention it is given.  How well the segments track the speech depends
    on which heads of a trained checkpoint align with it; that is the caller's calibration through `head_weights` of `VALLE.align`."""
    a = np.asarray(attn, np.float64)
    if a.ndim != 2:
        raise ValueError(f"attn is (T, S), got shape {a.shape}")
    T, S = a.shape
    enroll = int(enroll)
    if not 0 <= enroll <= S:
        raise ValueError(f"enroll {enroll} outside 0 .. S = {S}")
    n = S - enroll
    if T < n:
        raise ValueError(f"{T} frames cannot cover {n} text positions")
    if n == 0:
        return np.zeros((0, 2), np.int32)
    lg = np.log(np.maximum(a[:, enroll:], FLOOR))
    score = np.full(n, -np.inf)
    score[0] = lg[0, 0]
    moved = np.zeros((T, n), bool)               # moved[t, j]: the best path into (t, j) comes from column j - 1
    for t in range(1, T):
        stay, move = score, np.concatenate([[-np.inf], score[:-1]])
        moved[t] = move >= stay                  # tie: the smaller predecessor
        moved[t, 0] = False
        score = np.where(moved[t], move, stay) + lg[t]
    path = np.empty(T, np.int64)
    j = n - 1
    for t in range(T - 1, -1, -1):
        path[t] = j
        if moved[t, j]:
            j -= 1
    seg = np.empty((n, 2), np.int32)
    for j in range(n):
        frames = np.flatnonzero(path == j)
        seg[j] = frames[0], frames[-1]
    return seg


def stretched_sample(positions, hop: int, s, out_len=None):
    """Where input sample `s` is heard after `Engine.stretch(..., return_positions=True)`: positions[k] is the input sample output hop k
    starts from, so the answer is k * hop + (s - positions[k]) for the largest k with positions[k] <= s (k = 0 when there is none),
    clamped to the output, [0, out_len - 1] (out_len None: len(positions) * hop, the whole last hop).  `s` may be an array -- the
    frames of `monotonic_segments` times 320, say -- and the result has its shape (int64); a scalar gives an int."""
    p = np.asarray(positions, np.int64).reshape(-1)
    hop = int(hop)
    if hop <= 0:
        raise ValueError(f"hop {hop} below 1")
    sa = np.asarray(s, np.int64)
    if p.size == 0:
        out = np.zeros(sa.shape, np.int64)
    else:
        # positions need not rise; the largest k with positions[k] <= s is the largest k whose SUFFIX minimum is <= s, and those rise
        suffix_min = np.minimum.accumulate(p[::-1])[::-1]
        k = np.maximum(np.searchsorted(suffix_min, sa, side="right") - 1, 0)
        n = p.size * hop if out_len is None else int(out_len)
        out = np.clip(k * hop + (sa - p[k]), 0, max(n - 1, 0))
    return int(out) if np.ndim(s) == 0 else out


def token_pitch(segments, f0, voiced, hop: int, frame: int = 320) -> np.ndarray:
    """The pitch of every text token: `segments` (n, 2) are the first and the last codec frame of each token as `monotonic_segments`
    returns them (a codec frame is `frame` samples: 320 at 24 kHz), f0 / voiced the per-frame output of `Engine.f0` on the SAME
    waveform at hop `hop` (F0 frame k is centred on sample k hop + hop // 2).  Token j covers the samples
    [first_j frame, (last_j + 1) frame); its pitch is the lower median (element (m - 1) // 2 of the m sorted values, as
    vx_f0_info.f0_median) of f0 over the voiced F0 frames whose centre lies in that span.  Returns (n,) float64, NaN for a token
    without a voiced frame.  Host numpy."""
    seg = np.asarray(segments, np.int64).reshape(-1, 2)
    f = np.asarray(f0, np.float64).reshape(-1)
    v = np.asarray(voiced, bool).reshape(-1)
    hop, frame = int(hop), int(frame)
    if hop <= 0 or frame <= 0:
        raise ValueError(f"hop {hop} and frame {frame} must be positive")
    if f.shape != v.shape:
        raise ValueError(f"f0 has {f.size} frames, voiced {v.size}")
    centre = np.arange(f.size, dtype=np.int64) * hop + hop // 2
    out = np.full(len(seg), np.nan, np.float64)
    for j, (a, b) in enumerate(seg):
        vals = np.sort(f[v & (centre >= a * frame) & (centre < (b + 1) * frame)])
        if vals.size:
            out[j] = vals[(vals.size - 1) // 2]
    return out


def range_contour(f0, lag, ratio, scale) -> np.ndarray:
    """The per-frame pitch ratios that scale the intonation of one row around its median: f0 / lag are the per-frame output of
    `Engine.f0_lags` (lag > 0 is voiced), `ratio` the overall pitch ratio, `scale` the factor on the intonation's range (in the log
    domain): voiced frame k gets ratio * (f0_k / median) ** (scale - 1), so that its pitch lands on ratio * median *
    (f0_k / median) ** scale -- scale 0 flattens the contour to the median, 1 leaves it, above 1 widens it.  The median is the lower
    median of f0 over the voiced frames (vx_f0_info.f0_median).  Unvoiced frames get `ratio`.  Returns (M,) int32 in Q16, rounded
    to nearest and clipped to 43691 .. 131072, what `Engine.psola` takes as a row's `contour`.  Host numpy."""
    f = np.asarray(f0, np.float64).reshape(-1)
    v = np.asarray(lag).reshape(-1) > 0
    if f.shape != v.shape:
        raise ValueError(f"f0 has {f.size} frames, lag {v.size}")
    ratio, scale = float(ratio), float(scale)
    if not (np.isfinite(ratio) and ratio > 0 and np.isfinite(scale)):
        raise ValueError(f"ratio {ratio!r} must be positive and scale {scale!r} finite")
    out = np.full(f.size, ratio, np.float64)
    if v.any():
        vals = np.sort(f[v])
        med = vals[(vals.size - 1) // 2]
        out[v] = ratio * (f[v] / med) ** (scale - 1.0)
    return np.clip(np.rint(out * 65536.0), 43691, 131072).astype(np.int32)
