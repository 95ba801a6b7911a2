"""Float64 reference of the serving session's per-request logit filters (serve_sample.hip: repetition penalty, min_frames, top_p on
top of temperature and top_k) and the probe sets the filter tests share.  Builds on tests/_kernel_refs.py; tests/test_filter_refs.py
ties it to the reference's top_k_top_p_filtering on the CPU, tests/test_gpu_kernel_filters.py and tests/test_gpu_serve_filters.py
compare the HIP kernel with it."""
import numpy as np

from tests import _kernel_refs as R

MARGIN_MIN = 2.0 ** -12       # smallest nucleus margin of an input whose kept set the GPU tests compare exactly


def penalised(logits, hist, penalty, window, n_gen):
    """step 1, exact fp32: every token of gen[max(0, n_gen - window) .. n_gen) (window 0: all of gen[0 .. n_gen)), once however often
    it occurs, gets l > 0 ? l / r : l * r -- one correctly rounded fp32 operation.  penalty 1 reads no history."""
    v = np.asarray(logits, np.float32).copy()
    r = np.float32(penalty)
    if r == np.float32(1.0):
        return v
    n_gen = int(n_gen)
    lo = max(0, n_gen - int(window)) if int(window) > 0 else 0
    for t in sorted(set(int(x) for x in np.asarray(hist, np.int64).reshape(-1)[lo:n_gen])):
        if 0 <= t < R.N_LOGITS:
            v[t] = np.float32(v[t] / r) if v[t] > 0 else np.float32(v[t] * r)
    return v


def nucleus_mass(v, kept):
    """(G float64 (1025,), total): G[i] = sum of exp(v_j - max) over kept j with v_j > v_i (the mass strictly above value v_i), in
    float64; entries of tokens outside `kept` are nan"""
    z = np.where(kept, np.asarray(v, np.float64), -np.inf)
    e = np.exp(z - z.max())
    order = np.argsort(-z, kind="stable")
    zs, es = z[order], e[order]
    cum = np.concatenate([[0.0], np.cumsum(es)])            # cum[i] = mass of the i largest
    first = np.searchsorted(-zs, -zs, side="left")          # first sorted position holding the same value: ties share one G
    G = np.full(R.N_LOGITS, np.nan)
    G[order] = cum[first]
    G[~kept] = np.nan
    return G, float(e.sum())


def filtered_sampler_ref(logits, hist, top_k, temperature, top_p, penalty, window, min_frames, n_gen):
    """The filtered sampler on one reduced fp32 logit row.  fp32-exact steps as on the device: the repetition penalty, the
    min_frames mask of EOS, the temperature quotient (sampler_ref) and top_k with ties (sampler_ref).  Then, in float64: the softmax
    numerators, G, the nucleus cut (token i stays iff G(l_i) <= top_p * total; ties with the last kept value stay), the CDF in
    index order and p.  Returns (v fp32 after penalty / mask / temperature, kept bool mask, p float64, cdf float64).  A row left
    without a finite logit returns an empty kept set and p = 1 at EOS (the kernel's non-finite guard samples EOS)."""
    v = penalised(logits, hist, penalty, window, n_gen)
    if int(n_gen) < int(min_frames):
        v[R.EOS] = -np.inf
    if not np.isfinite(v).any():
        p = np.zeros(R.N_LOGITS)
        p[R.EOS] = 1.0
        return v, np.zeros(R.N_LOGITS, bool), p, np.cumsum(p)
    v, kept, p, cdf = R.sampler_ref(v, top_k, temperature)
    tp = np.float64(np.float32(top_p))
    if tp < 1.0:
        G, total = nucleus_mass(v, kept)
        kept = kept & (np.nan_to_num(G, nan=np.inf) <= tp * total)
        z = np.where(kept, v.astype(np.float64), -np.inf)
        e = np.exp(z - z.max())
        p = e / e.sum()
        cdf = np.cumsum(p)
    return v, kept, p, cdf


def nucleus_margin(logits, hist, top_k, temperature, top_p, penalty=1.0, window=0, min_frames=0, n_gen=0):
    """min over the values top_k left (kept or cut by top_p) of |G / total - top_p|: how far the nearest keep / cut decision is from
    flipping, as a share of the probability mass"""
    v, kept, _, _ = filtered_sampler_ref(logits, hist, top_k, temperature, 1.0, penalty, window, min_frames, n_gen)
    G, total = nucleus_mass(v, kept)
    return float(np.nanmin(np.abs(G / total - np.float64(np.float32(top_p)))))


def filter_combos():
    """(row name of sampler_rows(), temperature, top_k, top_p, nucleus size) of every top_p case the GPU tests use.  The sizes are
    pinned here and checked on the CPU (tests/test_filter_refs.py), together with nucleus_margin >= 2^-12 for each."""
    return [("normal_k-100", 1.0, -100, 0.5, 5), ("normal_k-100", 1.0, -100, 0.75, 18), ("normal_k-100", 1.0, -100, 0.85, 31),
            ("normal_k-100", 4.0, -100, 0.25, 55), ("normal_k-100", 4.0, -100, 0.65, 294),
            ("normal_k-100", 100.0, -100, 0.05, 48), ("normal_k-100", 100.0, -100, 0.65, 652), ("normal_k-100", 100.0, -100, 0.9, 916),
            ("normal_k-100", 0.7, -100, 0.9, 15),
            ("normal_k50_T1.0", 1.0, 50, 0.8, 17), ("normal_k50_T1.0", 1.0, 50, 0.9, 28), ("normal_k50_T1.0", 1.0, 50, 0.95, 37)]


def tie_combos():
    """(row name, top_k, top_p, kept tokens) of the tie cases: every token tied with the last kept value stays"""
    return [("all_equal", 10, 0.1, R.N_LOGITS), ("ties_at_kth", 10, 0.95, 12), ("four_finite", 10, 0.5, 2), ("lane_edges", 6, 0.9, None)]


def row_by_name(name):
    return next(r for r in R.sampler_rows() if r["name"] == name)


def penalty_histories():
    """(name, hist tokens, n_gen, window) with gen_stride 64: a repeated token, tokens 0 and 1023, a lane-boundary token (16 | 17 of
    lane 0 | 1), and windows 0, 1, 5 and n_gen"""
    h40 = [(37 * i + 11) % 1024 for i in range(40)]
    h40[3] = h40[20] = h40[39] = 500          # three occurrences: penalised once
    h40[34] = 777                             # position 34 of 40: just outside a window of 5, inside a window of 6
    h40[35:39] = [0, 1023, 16, 17]
    return [("empty", [], 0, 0), ("one", [1023], 1, 0), ("one_w1", [0], 1, 1),
            ("five_all", [17, 17, 0, 1023, 17], 5, 0), ("five_w1", [17, 16, 0, 1023, 500], 5, 1), ("five_w5", [17, 16, 0, 1023, 16], 5, 5),
            ("forty_all", h40, 40, 0), ("forty_w1", h40, 40, 1), ("forty_w5", h40, 40, 5), ("forty_w6", h40, 40, 6),
            ("forty_wn", h40, 40, 40)]
