"""CPU: the float64 references of tests/_kernel_refs.py agree with the oracle, so a wrong reference fails here and not on the GPU.
  * sampler: tokens and log p of VallexOracle.sample on every probe of the chosen logit rows, and the kept sets the rows pin;
  * attention: VallexOracle._mha's softmax(Q K^T / 8) V (identity out_proj) with the prefix-LM mask and without a mask."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.vallex_oracle import VallexOracle
from tests import _kernel_refs as R

ROWS = R.sampler_rows()


@pytest.mark.parametrize("row", ROWS, ids=[r["name"] for r in ROWS])
def test_sampler_reference_matches_oracle(row):
    v, kept, p, cdf = R.sampler_ref(row["logits"], row["top_k"], row["temperature"])
    if row["kept"] is not None:
        assert int(kept.sum()) == row["kept"]
    assert abs(p.sum() - 1.0) < 1e-12 and not p[~kept].any()
    probes = R.token_probes(p, cdf)
    assert probes
    lg = torch.from_numpy(row["logits"])
    first, last = np.flatnonzero(kept)[[0, -1]]
    for tok, u in probes + [(int(first), np.float32(0.0))] + ([(int(last), np.float32(1.0 - 2.0 ** -24))] if p[last] >= R.P_MIN else []):
        assert R.sample_token(p, cdf, u) == tok
        otok, ologp = VallexOracle.sample(lg, row["top_k"], row["temperature"], float(u))
        if tok == first and u == 0.0 and p[first] < R.P_MIN:
            continue                              # fp32 underflow may move the end (T = 0.05)
        assert otok == tok, (row["name"], tok, float(u), otok)
        assert abs(ologp - np.log(p[tok])) < 2e-5, (row["name"], tok, ologp, np.log(p[tok]))


def test_pinned_kept_sets():
    by = {r["name"]: r for r in ROWS}
    _, kept, _, _ = R.sampler_ref(by["four_finite"]["logits"], 10, 1.0)
    assert list(np.flatnonzero(kept)) == [0, 17, 1019, 1024]
    _, kept, _, _ = R.sampler_ref(by["lane_edges"]["logits"], 6, 1.0)
    assert list(np.flatnonzero(kept)) == [0, 16, 17, 1019, 1020, 1024]
    _, kept, _, _ = R.sampler_ref(by["two_maxima_k1"]["logits"], 1, 1.0)
    assert list(np.flatnonzero(kept)) == [5, 1024]
    # the unfiltered rows have enough wide CDF intervals to probe
    for name in ("normal_k-100", "normal_k1025", "normal_k1024"):
        _, _, p, cdf = R.sampler_ref(by[name]["logits"], by[name]["top_k"], 1.0)
        assert len(R.token_probes(p, cdf)) >= 64


@pytest.mark.parametrize("splitk", [2, 4])
def test_split_partials_sum_back_exactly(splitk):
    rng = np.random.default_rng(3)
    for row in ROWS:
        parts = R.split_partials(row["logits"], splitk, rng)
        assert parts.shape == (splitk, R.N_LOGITS) and parts.dtype == np.float32
        np.testing.assert_array_equal(R.reduce_partials(parts), row["logits"])
        fin = np.isfinite(row["logits"])
        assert np.count_nonzero(parts[1:, fin]) > 0.9 * (splitk - 1) * fin.sum()        # real addends, not zeros


@pytest.mark.parametrize("masked", [False, True])
def test_attention_reference_matches_oracle_mha(masked):
    g = torch.Generator().manual_seed(11)
    d = 1024
    w = {"a.in_proj_weight": (torch.randn(3 * d, d, generator=g) * 0.06).numpy(), "a.in_proj_bias": (torch.randn(3 * d, generator=g) * 0.1).numpy(),
         "a.out_proj.weight": torch.eye(d).numpy(), "a.out_proj.bias": torch.zeros(d).numpy()}
    orc = VallexOracle(w, 1)
    lens, pre = (5, 33, 70), (2, 33, 40)
    want, qkvs = [], []
    for n, s in zip(lens, pre):
        x = torch.randn(n, d, generator=g)
        mask = None
        if masked:
            mask = torch.zeros(n, n, dtype=torch.bool)                            # models/vallex.py:535-549
            mask[:s, s:] = True
            mask[s:, s:] = torch.triu(torch.ones(n - s, n - s, dtype=torch.bool), diagonal=1)
        y, _ = orc._mha(x, "a", mask)
        want.append(y.numpy())
        qkvs.append(F.linear(x, orc.w["a.in_proj_weight"], orc.w["a.in_proj_bias"]).numpy())
    want, qkv = np.concatenate(want), np.concatenate(qkvs)
    got = R.attention_ref(qkv, lens, pre if masked else None)
    assert np.abs(got - want).max() < 2e-5, np.abs(got - want).max()
    # the fp32 yardstick is the same arithmetic as the oracle's
    yard = R.attention_fp32_yardstick(qkv, lens, pre if masked else None)
    assert np.abs(yard - want).max() < 2e-6
    if masked:                                        # and the mask matters: the unmasked result is far away
        assert np.abs(R.attention_ref(qkv, lens, None) - want).max() > 1e-2


def test_layer_norm_reference():
    rng = np.random.default_rng(2)
    x, g, b = rng.normal(0, 2, (7, 1024)), rng.normal(1, 0.2, 1024), rng.normal(0, 0.2, 1024)
    want = F.layer_norm(torch.from_numpy(x), (1024,), torch.from_numpy(g), torch.from_numpy(b), 1e-5).numpy()
    assert np.abs(R.layer_norm_ref(x, g, b) - want).max() < 1e-12
