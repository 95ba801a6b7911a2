"""CPU: the float64 references of tests/_kernel_refs.py agree with the oracle, so a wrong reference fails here and not on the GPU.
  * sampler: tokens and log p of VallexOracle.sample on every probe of the chosen logit rows, and the kept sets the rows pin;
  * attention: VallexOracle._mha's softmax(Q K^T / 8) V (identity out_proj) with the prefix-LM mask and without a mask;
  * the decode attention block: VallexOracle._mha(..., past=...) on one new token, from x (the small-batch chain's view) and from
    in_proj slabs (the dec_attn chains' view), and the launch plans of tests/test_gpu_kernel_dec_attn.py cover what they claim."""
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


def _dec_weights(g, d=1024):
    return dict(in_w=(torch.randn(3 * d, d, generator=g) * 0.03).numpy(), in_b=(torch.randn(3 * d, generator=g) * 0.1).numpy(),
                out_w=(torch.randn(d, d, generator=g) * 0.03).numpy(), out_b=(torch.randn(d, generator=g) * 0.1).numpy(),
                n1_w=(1.0 + 0.1 * torch.randn(d, generator=g)).numpy(), n1_b=(0.1 * torch.randn(d, generator=g)).numpy(),
                l2_b=(0.1 * torch.randn(d, generator=g)).numpy())


@pytest.mark.parametrize("kind,chain,skp,balanced", [("model", "sb_qkv", 0, False), ("uniform", "sb_qkv", 8, False),
                                                      ("sharp", "unfused", 0, False), ("new_heavy", "fused", 0, True)])
def test_dec_attn_reference_matches_oracle_mha(kind, chain, skp, balanced):
    g = torch.Generator().manual_seed(23)
    w = _dec_weights(g)
    orc = VallexOracle({"a.in_proj_weight": w["in_w"], "a.in_proj_bias": w["in_b"], "a.out_proj.weight": w["out_w"],
                        "a.out_proj.bias": w["out_b"]}, 1)
    ctx = [1, 2, 18, 130]
    case = R.dec_case(kind, ctx, w, chain, seed=5, skp=skp, balanced=balanced, tmax=160)
    nsplit = 3
    ref = R.dec_attn_block_ref(case, w, nsplit)
    yard = R.dec_attn_block_fp32(case, w, nsplit)
    # small-batch chain: the oracle gets x and runs in_proj itself.  dec_attn chains: the slabs ARE in_proj's result, so the oracle
    # gets a zero in_proj weight with the reference's q | k | v as bias and computes softmax(q K^T / 8) V and out_proj on it.
    for r, c in enumerate(ctx):
        past = (torch.from_numpy(case["k_rows"][r]).transpose(0, 1), torch.from_numpy(case["v_rows"][r]).transpose(0, 1))
        if chain == "sb_qkv":
            xi = torch.from_numpy(case["x_in"])
            x = xi[r:r + 1] if not skp else F.layer_norm(xi[:8, r].sum(0) + xi[8, r] + torch.from_numpy(w["l2_b"]), (1024,),
                                                         torch.from_numpy(w["n1_w"]), torch.from_numpy(w["n1_b"]), 1e-5)[None]
            y, (k, v) = orc._mha(x, "a", None, past)
        else:
            o2 = VallexOracle({"a.in_proj_weight": np.zeros((3072, 1024), np.float32), "a.in_proj_bias": ref["qkv"][r].astype(np.float32),
                               "a.out_proj.weight": w["out_w"], "a.out_proj.bias": w["out_b"]}, 1)
            y, (k, v) = o2._mha(torch.zeros(1, 1024), "a", None, past)
        want = y.numpy()[0].astype(np.float64)
        got = ref["proj"][r] + w["out_b"]
        scale = np.abs(want).max()
        assert np.abs(got - want).max() < 2e-5 * max(scale, 1.0), (r, c, np.abs(got - want).max(), scale)
        assert k.shape[-2] == c and np.abs(k[:, -1].numpy().reshape(-1) - ref["qkv"][r, 1024:2048]).max() < 1e-4
        assert np.abs(v[:, -1].numpy().reshape(-1) - ref["qkv"][r, 2048:]).max() < 1e-4 * max(1.0, np.abs(ref["qkv"][r, 2048:]).max())
        if chain != "sb_qkv":
            np.testing.assert_allclose(ref["h"][r], case["resid"][r] + got, rtol=0, atol=1e-12)
    # the fp32 yardstick is the same computation: close to float64, and not equal to it
    key = "proj" if chain == "sb_qkv" else "h"
    err = np.abs(yard[key] - ref[key]).max()
    assert 0 < err < 1e-3 * max(1.0, np.abs(ref[key]).max()), err
    # (m, l) of the splits put the softmax back together: sum_s l_s e^(m_s - M) = the full denominator
    M = ref["m"].max(-1, keepdims=True)
    tot = (ref["l"] * np.exp(ref["m"] - M)).sum(-1)
    for r, c in enumerate(ctx):
        n_terms = c - (1 if chain == "sb_qkv" else 0)
        if n_terms == 0:
            assert (ref["m"][r] == -1e30).all() and (ref["l"][r] == 0).all()
        else:
            assert (tot[r] >= 1.0 - 1e-12).all() and (tot[r] <= n_terms + 1e-9).all()
    assert np.abs(yard["m"] - ref["m"])[ref["l"] > 0].max() < 1e-3 * max(1.0, np.abs(ref["m"][ref["l"] > 0]).max())


def test_dec_attn_operand_sets_are_what_they_claim():
    g = torch.Generator().manual_seed(29)
    w = _dec_weights(g)
    for chain in ("sb_qkv", "unfused"):
        share = {}
        for kind in R.DEC_KINDS:
            case = R.dec_case(kind, [300, 130], w, chain, seed=9, tmax=320)
            ref = R.dec_attn_block_ref(case, w, 1)
            q = ref["qkv"][:, :1024].reshape(2, 16, 64)
            kn = ref["qkv"][:, 1024:2048].reshape(2, 16, 64)
            spread, new = [], []
            for r in range(2):
                sc = np.einsum("hd,thd->ht", q[r], case["k_rows"][r].astype(np.float64)) / 8.0
                sn = (q[r] * kn[r]).sum(-1) / 8.0
                spread.append((sc.max(-1) - sc.min(-1)).mean())
                mx = np.maximum(sc.max(-1), sn)
                new.append((np.exp(sn - mx) / (np.exp(sc - mx[:, None]).sum(-1) + np.exp(sn - mx))).mean())
            share[kind] = (np.mean(spread), np.mean(new))
        assert share["sharp"][0] > 200, share
        assert share["new_heavy"][1] > 0.99 and share["new_light"][1] < 1e-4, share
        assert 1e-4 < share["uniform"][1] < 0.5 and 1e-4 < share["model"][1] < 0.5, share


def test_dec_attn_launch_plans_cover_the_edges():
    chains = set()
    for n in R.DEC_ROWS:
        chain, ns = R.dec_geometry(n)
        chains.add((chain, ns))
        plans = R.dec_launch_contexts(n)
        seen = [c for p in plans for c in p]
        assert all(len(p) == n for p in plans) and set(seen) == set(R.DEC_CTX), n
        assert max(seen) <= R.DEC_TMAX and len(plans) <= 12
        empty = exact = past1 = False
        for c in seen:
            b = R.dec_split_bounds(c - 1, ns)
            assert b[0][0] == 0 and max(t1 for _, t1 in b) == c - 1 and all(b[i][1] == b[i + 1][0] or b[i + 1][0] == b[i + 1][1] for i in range(ns - 1))
            filled = [t1 - t0 for t0, t1 in b if t1 > t0]
            empty |= len(filled) < ns
            exact |= bool(filled) and filled[-1] % 16 == 0
            past1 |= bool(filled) and filled[-1] % 16 == 1
        assert (empty or ns == 1) and exact and past1, (n, ns, empty, exact, past1)
        if n >= 8:                      # two rows per workgroup: launch slots y and y + ceil(n / 2)
            gy = (n + 1) // 2
            pairs = [(p[y], p[y + gy]) for p in plans for y in range(n - gy)]
            assert any(a >= 127 and b <= 33 for a, b in pairs) and any(a <= 33 and b >= 127 for a, b in pairs), n
            assert n % 2 or any(a == b for a, b in pairs), n
            order = R.balance_order(plans[0])
            assert sorted(order) == list(range(n)) and list(order) != list(range(n))
    # one row count per chain x split count of the engine's table
    assert chains == {("sb_qkv", 16), ("sb_qkv", 8), ("sb_qkv", 4), ("unfused", 3), ("unfused", 2), ("split_fused", 4), ("split_fused", 3),
                      ("split_fused", 2), ("fused", 1)}
