"""The numpy restatement of vx_denoise's contract (include/vallex_hip.h), shared by the CPU and the GPU tests of the spectral noise
suppression.  Options are a tuple (alpha, floor, frac, kmin), alpha / floor / frac taken as fp32 words and widened, as the options
struct carries them.  The tables (w [512], c [256], s [256]) are an argument: the GPU tests pass the words the library reports
(vx_denoise_tables), the CPU tests `tables()`.  Every floating-point operation is one numpy float64 operation, nothing is contracted;
the butterflies of a stage touch disjoint words, so a stage is one vector operation per product and sum; the energy and the profile
are np.cumsum (sequential, from the first word: 0.0 + x = x for the non-negative powers); the four frames of an output sample are
added in four passes, in ascending t."""
import numpy as np

from tests._psola_refs import vowel

N, H, B = 512, 128, 257
DEFAULTS = (2.0, 10.0 ** (-18.0 / 20.0), 0.1, 8)
LENGTHS = (0, 1, 127, 128, 129, 511, 512, 513, 1300, 3000)
REV = np.array([int(format(i, "09b")[::-1], 2) for i in range(N)])


def tables():
    n, k = np.arange(N, dtype=np.float64), np.arange(N // 2, dtype=np.float64)
    return np.concatenate([np.sqrt(0.5 - 0.5 * np.cos(2 * np.pi * n / N)), np.cos(2 * np.pi * k / N), -np.sin(2 * np.pi * k / N)])


def frames(L):
    return -(-int(L) // H) + 3


def full(L):
    return max(0, int(L) // H - 3)


def clean(x):
    y = np.array(x, np.float32).reshape(-1)
    bad = ~np.isfinite(y)
    y[bad] = 0
    return y, int(bad.sum())


def fft(re, im, tab, inverse=False):
    """the network on frames (..., 512) in natural order -> (re, im); the inverse is NOT scaled"""
    c, s = tab[N: N + N // 2], tab[N + N // 2:]
    if inverse:
        s = -s
    re, im = np.array(re, np.float64)[..., REV], np.array(im, np.float64)[..., REV]
    j = np.arange(N // 2)
    m = 2
    while m <= N:
        h = m // 2
        p = j % h
        i0 = (j // h) * m + p
        i1, q = i0 + h, p * (N // m)
        a, b = c[q] * re[..., i1], s[q] * im[..., i1]
        tr = a - b
        a, b = c[q] * im[..., i1], s[q] * re[..., i1]
        ti = a + b
        ar, ai = re[..., i0], im[..., i0]
        re[..., i0], im[..., i0] = ar + tr, ai + ti
        re[..., i1], im[..., i1] = ar - tr, ai - ti
        m *= 2
    return re, im


def analysis(x, tab):
    """(re, im (T, 512), P (T, 257), E (T,)) of a row"""
    y, _ = clean(x)
    L, T = len(y), frames(len(y))
    pad = np.concatenate([np.zeros(3 * H), y.astype(np.float64), np.zeros((T + 3) * H - 3 * H - L + N)])
    fr = np.stack([pad[t * H: t * H + N] for t in range(T)]) * tab[:N]
    re, im = fft(fr, np.zeros_like(fr), tab)
    a, b = re[:, :B] * re[:, :B], im[:, :B] * im[:, :B]
    P = a + b
    return re, im, P, np.cumsum(P, axis=1)[:, -1]


def words(o):
    """(alpha, floor, frac) as the doubles the library widens from the struct, kmin"""
    return float(np.float32(o[0])), float(np.float32(o[1])), float(np.float32(o[2])), int(o[3])


def k_of(o, F):
    _, _, frac, kmin = words(o)
    return min(max(kmin, int(np.floor(frac * float(F)))), F)


def select(E, L, K):
    """the K full frames smallest in (E[t], t), in ascending t"""
    F = full(L)
    if K <= 0 or F <= 0:
        return np.zeros(0, np.int32)
    order = sorted(range(3, 3 + F), key=lambda t: (E[t], t))[:K]
    return np.array(sorted(order), np.int32)


def gains(P, Nz, o):
    alpha, fl, _, _ = words(o)
    T = len(P)
    t = np.arange(T)
    at = lambda d: P[np.clip(t + d, 0, T - 1)]                      # noqa: E731
    S = ((((at(-2) + at(-1)) + P) + at(1)) + at(2)) / 5.0
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(S > 0.0, 1.0 - (alpha * Nz[None, :]) / S, fl)
    return np.where(g > fl, g, fl)


def denoise(x, o, tab, psd=None):
    """dict(out float32 (L,), P, E, sel int32, psd (257,), gain (T, 257), info)"""
    y, nonf = clean(x)
    L, T, F = len(y), frames(len(y)), full(len(y))
    re, im, P, E = analysis(x, tab)
    if psd is not None:
        K, sel, Nz = 0, np.zeros(0, np.int32), np.array(psd, np.float64)
    else:
        K = k_of(o, F)
        sel = select(E, L, K)
        Nz = np.cumsum(P[sel], axis=0)[-1] / float(K) if K > 0 else np.zeros(B)
    g = gains(P, Nz, o)
    gfull = np.concatenate([g, g[:, B - 2: 0: -1]], axis=1)            # bin k > 256 takes g[N - k]
    yr, _ = fft(re * gfull, im * gfull, tab, inverse=True)
    Y = ((yr * (1.0 / N)) * tab[:N]).reshape(T, 4, H)
    U = T - 3
    acc = 0.0 + Y[0:U, 3]
    acc = acc + Y[1:U + 1, 2]
    acc = acc + Y[2:U + 2, 1]
    acc = acc + Y[3:U + 3, 0]
    out = (0.5 * acc).astype(np.float32).reshape(-1)[:L]
    return dict(out=out, P=P, E=E, sel=sel, psd=Nz, gain=g, info=dict(frames=T, full_frames=F, k=K, nonfinite=nonf))


# ---- rows ---------------------------------------------------------------------------------------------------------------------------

RATE = 24000
VOWELS = ((110.0, 700.0), (220.0, 500.0))
SIGMAS = (0.003, 0.01, 0.03)


def gated_vowel(f0, F1, n=2 * RATE):
    """(row, gate): a 2 s vowel, zero for the first 0.5 s and the last 0.25 s, gated by sin(2 pi 3 t) > -0.3 in between"""
    t = np.arange(n) / RATE
    gate = (t >= 0.5) & (t < n / RATE - 0.25) & (np.sin(2 * np.pi * 3 * t) > -0.3)
    return (vowel(f0, F1, RATE, n) * gate).astype(np.float32), gate


def claim_rows():
    """the six rows of the audible claims: (tag, clean, noisy, gate)"""
    rows = []
    for vi, (f0, F1) in enumerate(VOWELS):
        cl, gate = gated_vowel(f0, F1)
        for si, sigma in enumerate(SIGMAS):
            noise = np.random.default_rng(100 + 10 * vi + si).normal(0.0, sigma, len(cl))
            rows.append((f"{int(f0)}Hz_{sigma}", cl, (cl.astype(np.float64) + noise).astype(np.float32), gate))
    return rows


def far_from(gate, dist=1024):
    """samples more than `dist` from any gated-on sample"""
    on = np.flatnonzero(gate)
    idx = np.arange(len(gate))
    pos = np.searchsorted(on, idx)
    left = np.where(pos > 0, idx - on[np.clip(pos - 1, 0, len(on) - 1)], len(gate))
    right = np.where(pos < len(on), on[np.clip(pos, 0, len(on) - 1)] - idx, len(gate))
    return np.minimum(left, right) > dist


def snr_db(ref, got, mask):
    ref, got = ref.astype(np.float64)[mask], got.astype(np.float64)[mask]
    return 10.0 * np.log10(np.sum(ref * ref) / np.sum((got - ref) ** 2))


def power_db(x, mask):
    v = x.astype(np.float64)[mask]
    return 10.0 * np.log10(np.mean(v * v))


def length_rows(seed=3):
    """a ragged batch: a tone in noise that fades in, so that the quiet frames differ from the loud ones"""
    rng = np.random.default_rng(seed)
    rows = []
    for L in LENGTHS:
        t = np.arange(L)
        rows.append((0.3 * np.sin(2 * np.pi * 0.031 * t) * np.minimum(1.0, t / 1500.0) + rng.normal(0.0, 0.01, L)).astype(np.float32))
    return rows


def odd_row(L=1300, seed=4):
    x = np.random.default_rng(seed).normal(0.0, 0.1, L).astype(np.float32)
    x[[0, 5, 127, 128, 700, L - 1]] = [np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan]
    return x


def same(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    view = {2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    np.testing.assert_array_equal(a.view(view), b.view(view), err_msg=str(what))
