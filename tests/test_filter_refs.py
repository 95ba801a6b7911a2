"""CPU: the float64 filter reference of tests/_filter_refs.py against the reference's own top_k_top_p_filtering
(models/vallex.py:791-833, rebuilt here from its definition with torch), the penalty formula, and the self-check of every input
the GPU filter tests compare exactly: its nucleus margin is >= 2^-12.

An fp32 sum of at most 1025 non-negative terms plus the error of expf is off by at most about 1025 * 2^-24 = 2^-14 of the total;
2^-12 is four times that, so the exact kept-set comparisons of tests/test_gpu_kernel_filters.py need no allowance."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _filter_refs as FR
from tests import _kernel_refs as R


def reference_filtering(logits, top_k, top_p):
    """top_k_top_p_filtering by its definition: top_k removes `logits < k-th largest`; top_p sorts descending, takes the cumulative
    softmax and removes a token when the cumulative probability of the tokens BEFORE it (itself excluded) exceeds top_p -- the first
    token always stays.  Returns the kept mask."""
    lg = torch.from_numpy(np.asarray(logits, np.float32).copy())[None]
    if top_k > 0:
        kth = torch.topk(lg, min(max(top_k, 1), lg.size(-1)))[0][..., -1, None]
        lg[lg < kth] = -float("inf")
    if top_p < 1.0:
        s, idx = torch.sort(lg, descending=True)
        cum = torch.cumsum(F.softmax(s, dim=-1), dim=-1)
        before = torch.cat([torch.zeros_like(cum[..., :1]), cum[..., :-1]], dim=-1)
        remove = torch.zeros_like(lg, dtype=torch.bool).scatter(1, idx, before > top_p)
        lg[remove] = -float("inf")
    return torch.isfinite(lg)[0].numpy()


@pytest.mark.parametrize("name,T,top_k,top_p,size", FR.filter_combos())
def test_kept_set_equals_the_reference_rule(name, T, top_k, top_p, size):
    row = FR.row_by_name(name)
    v = row["logits"] if T == 1.0 else (row["logits"] / np.float32(T)).astype(np.float32)
    assert len(np.unique(v)) == len(v) or top_k > 0          # tie-free where it matters (the clipped tails are far below the cut)
    _, kept, p, cdf = FR.filtered_sampler_ref(row["logits"], [], top_k, T, top_p, 1.0, 0, 0, 0)
    want = reference_filtering(v, top_k, top_p)
    assert (kept == want).all(), (name, T, top_k, top_p, int(kept.sum()), int(want.sum()))
    assert int(kept.sum()) == size
    assert abs(p.sum() - 1.0) < 1e-12 and (p[~kept] == 0).all() and abs(cdf[-1] - 1.0) < 1e-12


@pytest.mark.parametrize("name,T,top_k,top_p,size", FR.filter_combos())
def test_gpu_inputs_have_a_nucleus_margin(name, T, top_k, top_p, size):
    row = FR.row_by_name(name)
    m = FR.nucleus_margin(row["logits"], [], top_k, T, top_p)
    assert m >= FR.MARGIN_MIN, (name, T, top_k, top_p, m)


def test_unfiltered_row_at_t1_has_thin_margins_at_080_and_095():
    """the two settings the GPU tests must not use: the self-check above would refuse them"""
    row = FR.row_by_name("normal_k-100")
    for tp in (0.8, 0.95):
        assert FR.nucleus_margin(row["logits"], [], -100, 1.0, tp) < FR.MARGIN_MIN


@pytest.mark.parametrize("name,top_k,top_p,size", FR.tie_combos())
def test_tie_rows(name, top_k, top_p, size):
    row = FR.row_by_name(name)
    v, kept, p, _ = FR.filtered_sampler_ref(row["logits"], [], top_k, row["temperature"], top_p, 1.0, 0, 0, 0)
    if size is not None:
        assert int(kept.sum()) == size, (name, int(kept.sum()))
    # every token tied with the smallest kept value is kept, and the kept set is upward closed in value
    lo = v[kept].min()
    _, kk, _, _ = R.sampler_ref(row["logits"], top_k, row["temperature"])
    assert (kept == (kk & (v >= lo))).all()
    assert FR.nucleus_margin(row["logits"], [], top_k, row["temperature"], top_p) >= FR.MARGIN_MIN


def test_penalty_formula():
    lg = np.array([2.5, -1.5, 0.0, 3.0, -4.0] + [0.125] * (R.N_LOGITS - 5), np.float32)
    hist = [0, 1, 0, 0, 4, 2, 3]                       # token 0 three times; token 3 lies outside gen[0 .. n_gen)
    for r in (1.3, 0.8):
        v = FR.penalised(lg, hist, r, 0, 6)
        r32 = np.float32(r)
        assert v[0] == np.float32(np.float32(2.5) / r32)                # once, not per occurrence
        assert v[1] == np.float32(np.float32(-1.5) * r32) and v[4] == np.float32(np.float32(-4.0) * r32)
        assert v[2] == 0.0 and v[3] == np.float32(3.0) and (v[5:] == np.float32(0.125)).all()
        w = FR.penalised(lg, hist, r, 2, 6)                             # window 2: gen[4 .. 6) = {4, 2}
        assert w[0] == np.float32(2.5) and w[1] == np.float32(-1.5) and w[4] == v[4]
    assert (FR.penalised(lg, [9999, -3], 1.0, 0, 2) == lg).all()        # r == 1 reads no history
    assert (FR.penalised(lg, [9999, -3], 1.3, 0, 2) == lg).all()        # out-of-range tokens index nothing


def test_penalty_changes_the_distribution_as_the_formula_says():
    row = FR.row_by_name("normal_k50_T1.0")
    top = int(np.argmax(row["logits"]))
    _, _, p0, _ = FR.filtered_sampler_ref(row["logits"], [], 50, 1.0, 1.0, 1.0, 0, 0, 0)
    _, _, p1, _ = FR.filtered_sampler_ref(row["logits"], [top, top], 50, 1.0, 1.0, 1.3, 0, 0, 2)
    l = np.float64(row["logits"][top])
    want = np.exp(np.float64(np.float32(row["logits"][top] / np.float32(1.3))) - l)      # odds of `top` against the rest
    got = (p1[top] / (1 - p1[top])) / (p0[top] / (1 - p0[top]))
    assert abs(got / want - 1.0) < 1e-9


def test_min_frames_masks_eos_until_reached():
    lg = np.full(R.N_LOGITS, -2.0, np.float32)
    lg[R.EOS] = 9.0
    _, kept, p, _ = FR.filtered_sampler_ref(lg, [], -100, 1.0, 1.0, 1.0, 0, 4, 3)
    assert not kept[R.EOS] and p[R.EOS] == 0.0
    _, kept, p, _ = FR.filtered_sampler_ref(lg, [], -100, 1.0, 1.0, 1.0, 0, 4, 4)
    assert kept[R.EOS] and p[R.EOS] > 0.9
    only = np.full(R.N_LOGITS, -np.inf, np.float32)
    only[R.EOS] = 1.0
    _, kept, p, _ = FR.filtered_sampler_ref(only, [], -100, 1.0, 1.0, 1.0, 0, 4, 0)
    assert not kept.any() and p[R.EOS] == 1.0                           # nothing finite left: the guard's EOS
