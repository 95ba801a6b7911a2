"""CPU: the references of the alignment tests agree with each other, and utils.alignment.monotonic_segments is the exhaustive
search over all monotone paths."""
import numpy as np
import pytest

from oracle import synth
from oracle.vallex_oracle import VallexOracle
from tests import _align_refs as A
from tests._score_refs import oracle64
from vallex_amd.utils.alignment import monotonic_segments


def test_the_two_kernel_references_agree_on_tiny_operands():
    rng = np.random.default_rng(3)
    seqs = [(1, 0, 1), (3, 2, 5), (7, 0, 2)]
    tab, M, rows = A.make_tab(seqs, q_first=[None, 6, None])
    qkv = rng.normal(0.0, 1.0, (M, 3072)).astype(np.float32)
    for w in (np.full(16, 1 / 16), np.eye(16)[5], rng.uniform(0, 1, 16) * (rng.random(16) < 0.5)):
        r64, r32 = A.align_rows_ref(qkv, tab, w), A.align_rows_fp32_yardstick(qkv, tab, w)
        assert sum(len(r) for r in r64) == rows
        for (S, Tp, T), a, b, t in zip(seqs, r64, r32, tab):
            assert a.shape == b.shape == (t[4], S)
            assert np.abs(a - b).max() <= 1e-6 * max(1.0, float(np.sum(w)))
            assert (a >= 0).all() and (a.sum(1) <= np.sum(w) * (1 + 1e-12)).all()
    # q = 0: every visible key has the same probability, 1 / (r + 1)
    zq = qkv.copy()
    zq[:, :1024] = 0
    for ref in (A.align_rows_ref, A.align_rows_fp32_yardstick):
        for res, t in zip(ref(zq, tab, np.full(16, 0.125)), tab):
            want = 2.0 / (t[3] + np.arange(t[4]) + 1)
            np.testing.assert_allclose(res, np.repeat(want[:, None], t[2], 1), rtol=1e-6)
    # a zero-weight head is left out, not multiplied: NaN there changes nothing
    w = np.eye(16)[4]
    bad = qkv.copy()
    bad[:, 64 * 9: 64 * 10] = np.nan
    for a, b in zip(A.align_rows_ref(qkv, tab, w), A.align_rows_ref(bad, tab, w)):
        np.testing.assert_array_equal(a, b)


@pytest.fixture(scope="module")
def pass_refs():
    nl = 2
    sd = synth.vallex_state_dict(nl, 3, 1.0)
    a, t = synth.synth_prompt(9, 3, seed=21)
    row = dict(text=np.concatenate([t[0], synth.synth_text(5, 21)]), prompt=a[0], enroll=3, prompt_language="en", text_language="en")
    codes0 = np.random.default_rng(21).integers(0, 1024, 11)
    return nl, sd, row, codes0


def test_pass_reference_rows_are_non_negative_and_bounded_by_the_weights(pass_refs):
    nl, sd, row, codes0 = pass_refs
    o64 = oracle64(sd, nl)
    S = len(row["text"])
    uni = A.align_ref64(o64, row, codes0)
    assert uni.shape == (len(codes0), S) and uni.dtype == np.float64
    assert (uni >= 0).all() and (uni.sum(1) <= 1 + 1e-12).all()
    hw = np.random.default_rng(5).uniform(0, 1, (nl, 16))
    got = A.align_ref64(o64, row, codes0, hw)
    assert (got >= 0).all() and (got.sum(1) <= hw.sum() * (1 + 1e-12)).all()
    # layers add: both = layer 0 + layer 1
    h0, h1 = hw.copy(), hw.copy()
    h0[1] = 0
    h1[0] = 0
    np.testing.assert_allclose(A.align_ref64(o64, row, codes0, h0) + A.align_ref64(o64, row, codes0, h1), got, rtol=0, atol=1e-14)
    # the fp32 oracle (the pass's yardstick) is the same function
    y = A.align_ref(VallexOracle(sd, nl), row, codes0, hw)
    assert y.dtype == np.float32 and np.abs(y - got).max() <= 1e-5 * hw.sum()


@pytest.mark.parametrize("n", [1, 2, 3, 4])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 6, 7])
def test_monotonic_segments_is_the_exhaustive_search(T, n):
    rng = np.random.default_rng(100 * T + n)
    for enroll in (0, 2):
        attn = rng.uniform(0.01, 1.0, (T, enroll + n))                 # tie-free with probability 1
        if T < n:
            with pytest.raises(ValueError):
                monotonic_segments(attn, enroll)
            continue
        seg = monotonic_segments(attn, enroll)
        assert seg.shape == (n, 2) and seg.dtype == np.int32
        path = A.path_of_segments(seg, T)
        score, want = A.best_monotone_path(attn, enroll)
        np.testing.assert_array_equal(path, want)
        assert path[0] == 0 and path[-1] == n - 1 and ((np.diff(path) == 0) | (np.diff(path) == 1)).all()
        got = float(np.log(attn[np.arange(T), enroll + path]).sum())
        assert abs(got - score) <= 1e-12 * max(1.0, abs(score))


def test_monotonic_segments_diagonal_ties_zeros_and_errors():
    eye = np.eye(5) * 0.9 + 0.01
    np.testing.assert_array_equal(monotonic_segments(eye, 0), np.stack([np.arange(5), np.arange(5)], 1))
    # enroll columns are ignored, whatever they hold
    wide = np.concatenate([np.full((5, 2), 7.0), eye], 1)
    np.testing.assert_array_equal(monotonic_segments(wide, 2), monotonic_segments(eye, 0))
    # every path ties: the smaller column as long as possible
    flat = np.full((6, 3), 0.25)
    np.testing.assert_array_equal(A.path_of_segments(monotonic_segments(flat, 0), 6), [0, 0, 0, 0, 1, 2])
    sc, want = A.best_monotone_path(flat, 0)
    np.testing.assert_array_equal(want, [0, 0, 0, 0, 1, 2])
    # one tie in the middle: frame 2 may sit on column 0 or 1 at the same score
    tie = np.array([[0.9, 0.1], [0.9, 0.1], [0.5, 0.5], [0.1, 0.9]])
    np.testing.assert_array_equal(A.path_of_segments(monotonic_segments(tie, 0), 4), [0, 0, 0, 1])
    # exact zeros count as 1e-30, not as -inf
    z = np.zeros((3, 2))
    assert monotonic_segments(z, 0).shape == (2, 2)
    assert monotonic_segments(np.ones((4, 3)), 3).shape == (0, 2)
    with pytest.raises(ValueError):
        monotonic_segments(np.ones((2, 5)), 1)
    with pytest.raises(ValueError):
        monotonic_segments(np.ones(4), 0)
