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


# ---- time maps for Engine.retime (vx_retime): anchors (input sample, output sample), integers throughout ---------------------------
def _walkable(la: int, new: int, hop: int) -> int:
    """the output length a segment of la input samples gets when `new` is asked for: la itself (a copy) where it is too short to walk
    (below 2 hop), else `new` clamped to what vx_retime walks: at least 2 hop, and la / new inside 1/4 .. 4"""
    if la < 2 * hop:
        return la
    return min(max(new, 2 * hop, -(-la // 4)), 4 * la)


def _anchors(length: int, spans, new_lens) -> np.ndarray:
    """(0, 0), then the two ends of every span with its new length, then (length, Lout); everything between the spans keeps its
    length.  An anchor that repeats the one before it is dropped."""
    out, shift, prev = [(0, 0)], 0, 0
    for (s, e), n in zip(spans, new_lens):
        s, e, n = int(s), int(e), int(n)
        if not prev <= s < e <= length:
            raise ValueError(f"span ({s}, {e}) is empty, out of order or outside 0 .. {length}")
        for a, b in ((s, s + shift), (e, s + shift + n)):
            if (a, b) != out[-1]:
                out.append((a, b))
        shift += n - (e - s)
        prev = e
    if (length, length + shift) != out[-1]:
        out.append((int(length), int(length) + shift))
    return np.array(out, np.int32).reshape(-1, 2)


def pause_map(length: int, pauses, max_len=None, min_len=None, scale=None, hop: int = 240) -> np.ndarray:
    """Anchors for `Engine.retime` that change the pauses of a row of `length` samples and nothing else: `pauses` (n, 2) are sample
    spans as `Engine.pauses` returns them.  A pause of P samples becomes a walked segment of clamp(round_half_even(P * scale), min_len,
    max_len) samples (scale None: P; a bound of None: none), then clamped to what vx_retime walks at `hop`: at least 2 hop and within
    1/4 .. 4 of P.  A pause below 2 hop stays as it is, and everything between the pauses is copied bit for bit.  Returns (k, 2)
    int32 from (0, 0) to (length, Lout).  Integers and Fractions only: the same anchors on every machine."""
    from fractions import Fraction
    length, hop = int(length), int(hop)
    sp = np.asarray(pauses, np.int64).reshape(-1, 2)
    new = []
    for s, e in sp:
        P = int(e - s)
        n = P if scale is None else int(round(P * Fraction(scale)))          # round(Fraction) rounds half to even
        if min_len is not None:
            n = max(n, int(min_len))
        if max_len is not None:
            n = min(n, int(max_len))
        new.append(_walkable(P, n, hop))
    return _anchors(length, sp, new)


def pace_map(length: int, segments, rates, hop: int = 240) -> np.ndarray:
    """Anchors for `Engine.retime` that speak every token at its own pace: `segments` (n, 2) are the sample spans [first, end) of the
    tokens, in order and not overlapping (the frames of `monotonic_segments` times 320: first * 320, (last + 1) * 320), `rates` (n,)
    the pace of each (a number or Fraction; 2 = twice as fast, half as long).  A token of P samples gets round_half_even(P / rate)
    samples, clamped as `pause_map` clamps; a token below 2 hop, and everything outside the tokens, keeps its length."""
    from fractions import Fraction
    length, hop = int(length), int(hop)
    sp = np.asarray(segments, np.int64).reshape(-1, 2)
    if len(sp) != len(rates):
        raise ValueError(f"{len(sp)} segments and {len(rates)} rates")
    new = []
    for (s, e), r in zip(sp, rates):
        r = Fraction(r)
        if r <= 0:
            raise ValueError(f"rate {r} is not positive")
        P = int(e - s)
        new.append(_walkable(P, int(round(P / r)), hop))
    return _anchors(length, sp, new)


def retimed_sample(anchors, t, inverse: bool = False):
    """Where input sample `t` is heard after `Engine.retime` under `anchors` (k, 2) -- or, with inverse=True, which input sample is
    heard at output sample `t`.  Exact at every anchor and linear in between: b_i + floor((t - a_i) lb / la) inside segment i.
    Inside a copy segment that is exact.  Inside a walked segment of la input and lb output samples the sample truly heard at an
    output time lies within D + 2 H |la / lb - 1| input samples of the line (search D, hop H): a frame is searched within D of its
    nominal position, plays H input samples at the input's own pace while the line moves H la / lb, and the nominal positions aim at
    the end pin, up to 2 H in front of the anchor -- D + 2 H at half or double pace.  Pass positions=True to `Engine.retime` for the
    exact positions.  `t` is clamped to the map's range; it may be an array (int64 out)."""
    an = np.asarray(anchors, np.int64).reshape(-1, 2)
    if len(an) < 1:
        raise ValueError("no anchors")
    src, dst = (an[:, 1], an[:, 0]) if inverse else (an[:, 0], an[:, 1])
    ta = np.clip(np.asarray(t, np.int64), src[0], src[-1])
    if len(an) == 1:
        out = np.full(ta.shape, dst[0], np.int64)
    else:
        i = np.clip(np.searchsorted(src, ta, side="right") - 1, 0, len(an) - 2)
        out = dst[i] + (ta - src[i]) * (dst[i + 1] - dst[i]) // (src[i + 1] - src[i])
    return int(out) if np.ndim(t) == 0 else out
