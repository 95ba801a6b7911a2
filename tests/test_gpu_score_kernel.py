"""GPU: score_rows_kernel (csrc/score.hip), one launch at a time through vx_dev_score_rows, against float64 on chosen rows.

rank is a count of exact fp32 comparisons, so it must EQUAL the float64 count on the same fp32 values; logp is held to
tests/_score_refs.lse_bound (derived there from the roundings of the kernel's arithmetic, not from its output).  Pad columns
(ncols .. ld-1) hold +1e30: a kernel that reads them loses every assertion at once."""
import numpy as np
import pytest

from tests._score_refs import lse_bound, score_ref
from tests._util import get_model

pytestmark = pytest.mark.gpu

ROWS = [1, 3, 4, 5, 257]                       # one wave, a partial block, a full block, two blocks, 65 blocks with a 1-row tail
SHAPES = [(1024, 1024), (1025, 1028), (1025, 1032)]
SENT_F, SENT_I = np.float32(-1.0e30), -123456789
EXTRA = 3


@pytest.fixture(scope="module")
def eng():
    return get_model(2, 1, 0.0, max_new=160, max_prompt=96, max_text=32, max_batch=32).engine


def _last_col_row(ncols):
    """the i with 7 i = ncols - 1 (mod ncols): the peak row that puts its peak into the last column"""
    return next(i for i in range(ncols) if (7 * i) % ncols == ncols - 1)


def _sets(rows, ncols):
    """name -> (logits (rows, ncols) float32, targets (rows,), exact rank or None)"""
    rng = np.random.default_rng(1000 * ncols + rows)
    out = {}
    # peak rows: 30.0 at column 7 i mod ncols; rows 0 .. 255 reach every lane (column / 4 mod 64) and every element of a 16-byte
    # group, and one row is the one whose peak is column ncols - 1
    ii = np.arange(rows)
    ii[-1 if rows > 1 else 0] = _last_col_row(ncols)
    peak = (7 * ii) % ncols
    l = np.zeros((rows, ncols), np.float32)
    l[np.arange(rows), peak] = 30.0
    out["peak"] = (l, peak, np.zeros(rows, np.int64))
    out["peak_neighbour"] = (l, (peak + 1) % ncols, np.ones(rows, np.int64))
    ramp = np.broadcast_to(np.arange(ncols, dtype=np.float32) / 64, (rows, ncols)).copy()
    tg = np.array([0, 1, 63, 64, 1023, ncols - 1])[np.arange(rows) % 6]
    out["ramp"] = (ramp, tg, ncols - 1 - tg)
    out["ramp_1e4"] = (ramp + np.float32(1e4), tg[::-1].copy(), ncols - 1 - tg[::-1])
    assert len(np.unique(out["ramp_1e4"][0][0])) == ncols          # still ncols distinct fp32 values
    out["equal"] = (np.full((rows, ncols), 3.25, np.float32), rng.integers(0, ncols, rows), np.zeros(rows, np.int64))
    spread = np.stack([rng.permutation(np.linspace(-200, 200, ncols)) for _ in range(rows)]).astype(np.float32)
    out["spread200"] = (spread, rng.integers(0, ncols, rows), None)
    for s in (1, 25, 100):
        out[f"normal_x{s}"] = ((rng.standard_normal((rows, ncols)) * s).astype(np.float32), rng.integers(0, ncols, rows), None)
    return out


def _padded(l, ld):
    x = np.full((l.shape[0], ld), 1e30, np.float32)
    x[:, : l.shape[1]] = l
    return x


@pytest.mark.parametrize("ncols,ld", SHAPES)
@pytest.mark.parametrize("rows", ROWS)
def test_rank_exact_and_logp_within_bound(eng, rows, ncols, ld):
    for name, (l, tg, want_rank) in _sets(rows, ncols).items():
        logp, rank = eng.dev_score_rows(_padded(l, ld), tg, ncols, extra_rows=EXTRA)
        ref_lp, ref_rk, _ = score_ref(l, tg)
        if want_rank is not None:
            np.testing.assert_array_equal(ref_rk, want_rank, err_msg=name)
        np.testing.assert_array_equal(rank[:rows], ref_rk, err_msg=f"{name}: rank")
        err = np.abs(logp[:rows].astype(np.float64) - ref_lp)
        bound = lse_bound(l, tg)
        worst = int(np.argmax(err - bound))
        assert (err <= bound).all(), (name, worst, err[worst], bound[worst])
        if name == "equal":
            assert np.abs(logp[:rows] + np.log(float(ncols))).max() <= 4e-5
        # rows behind `rows` are not written
        assert (logp[rows:] == SENT_F).all() and (rank[rows:] == SENT_I).all(), name


def test_refused_arguments_leave_the_outputs_untouched(eng):
    from vallex_amd import VallexHipError
    from vallex_amd._capi import VX_EINVAL
    ok = np.zeros((4, 1028), np.float32)
    tg = np.zeros(4, np.int32)

    def refused(x, t, ncols, n_out=None):
        lp = np.full(len(x) + 2 if n_out is None else n_out, 7.5, np.float32)
        rk = np.full(len(lp), 77, np.int32)
        with pytest.raises(VallexHipError) as e:
            eng.dev_score_rows(x, t, ncols, logp=lp, rank=rk)
        assert e.value.code == VX_EINVAL, e.value
        assert (lp == 7.5).all() and (rk == 77).all()

    refused(np.zeros((0, 1028), np.float32), np.zeros(0, np.int32), 1025)              # rows below 1
    refused(np.zeros((4097, 1024), np.float32), np.zeros(4097, np.int32), 1024)        # rows above 4096
    refused(ok, tg, 1000)                                                              # ncols neither 1024 nor 1025
    refused(ok, tg, 1026)
    refused(np.zeros((4, 1024), np.float32), tg, 1025)                                 # ld below ncols
    refused(np.zeros((4, 1030), np.float32), tg, 1025)                                 # ld % 4
    refused(np.zeros((4, 8196), np.float32), tg, 1025)                                 # ld above 8192
    refused(ok, np.array([0, 0, -1, 0], np.int32), 1025)                               # a target below 0
    refused(ok, np.array([0, 1025, 0, 0], np.int32), 1025)                             # a target at ncols
    refused(ok, np.array([0, 1024, 0, 0], np.int32), 1024)
    refused(ok, tg, 1025, n_out=3)                                                     # rows_out below rows
    refused(ok, tg, 1025, n_out=4 + 65)                                                # rows_out above rows + 64
    logp, rank = eng.dev_score_rows(ok, np.array([0, 1024, 5, 1027 - 3], np.int32), 1025, extra_rows=64)      # the limits themselves
    assert np.abs(logp[:4] + np.log(1025.0)).max() <= 4e-5 and (rank[:4] == 0).all() and (rank[4:] == SENT_I).all()
