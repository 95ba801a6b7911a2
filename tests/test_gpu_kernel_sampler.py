"""GPU: dec_sample_kernel (decode.hip) and serve_sample_kernel (serve_sample.hip) on chosen logit rows, against the float64
reference of tests/_kernel_refs.py (vx_dev_sample, include/vallex_hip_dev.h).  Every probe runs on both kernels and with the
predict layer's split-K factors 1, 2 and 4 (random fp32 addends whose fp32 sum is the logit row); every logit row is placed in
decode rows 0, 1, 31 and 13.

Exact-token probes: for every token with float64 p >= 2^-12, u = fp32(midpoint of its CDF interval) must return that token.
Any fp32 summation order of the 1088 terms is off by at most 1088 * 2^-24 of the total; with the error of exp (2^-22) and the
rounding of u * total (2^-24) that is below 2^-13, half the narrowest probed interval.  Random draws may differ from the float64
token only when u lies within 2^-13 of a CDF boundary.

Measured on an MI355X (printed by the tests; docs/log_r11.md): 9288 midpoint probes returned their token, no random draw differed
from the float64 token, max |sum_logp increment - float64 log p| = 1.27e-6 (bound 1e-4), fused norm1 6.92e-7 against
torch-CPU fp32's 6.92e-7 (ratio 1.00, bound 4)."""
import numpy as np
import pytest

from oracle import synth
from tests import _kernel_refs as R
from tests._util import get_model

pytestmark = pytest.mark.gpu

SENT_I = -123456789
SENT_F = np.float32(-1.0e30)
ORDER = [0, 1, 31, 13] + [r for r in range(32) if r not in (0, 1, 31, 13)]      # decode rows in the order a launch fills them
BASE = dict(active=1, n_gen=3, cur_pos=40, ctx_len=77, text_len=4, gen_stride=16, force_eos_at=-1, sum_logp=0.25)
EDGE = 2.0 ** -13


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run_cases(eng, cases):
    """cases that share their launch constants -> one output record per case.  Case j of a launch goes to decode row ORDER[j], so
    even a handful of cases lands on rows 0, 1, 31 and 13; the other rows of a launch are inactive fillers, returned under
    'fillers'.  Adds 'n_active_want' (active cases minus stopped cases of the case's launch)."""
    cases = list(cases)
    while len(cases) < 4:
        cases = cases + cases[: 4 - len(cases)]
    flat, where, fill = [], [], []
    for l0 in range(0, len(cases), 32):
        chunk = cases[l0:l0 + 32]
        launch = [dict(chunk[0], active=0, u=0.5) for _ in range(32)]
        for j, cs in enumerate(chunk):
            launch[ORDER[j]] = cs
            where.append(len(flat) + ORDER[j])
        fill += [len(flat) + r for r in range(32) if r not in ORDER[: len(chunk)]]
        flat += launch
    out = eng.dev_sample(flat)
    want_na = np.zeros(len(flat), np.int32)
    for l0 in range(0, len(flat), 32):
        sl = slice(l0, l0 + 32)
        stopped = sum(c["active"] for c in flat[sl]) - int(out["active"][sl].sum())
        assert stopped >= 0
        want_na[sl] = sum(c["active"] for c in flat[sl]) - stopped        # one decrement per stopped row, none for the others
    res = {k: v[where] for k, v in out.items()}
    res["n_active_want"] = want_na[where]
    res["fillers"] = {k: v[fill] for k, v in out.items()}
    res["filler_cases"] = [flat[i] for i in fill]
    res["cases"] = cases
    return res


@pytest.fixture(scope="module")
def eng():
    return get_model(2, 1, 0.0, max_new=160, max_prompt=96, max_text=32, max_batch=32).engine


@pytest.fixture(scope="module")
def weights():
    from vallex_amd.models.vallex import sine_pe_table
    sd = synth.vallex_state_dict(2, 1, 0.0)
    return dict(emb=sd["ar_audio_embedding.word_embeddings.weight"], alpha=np.float32(sd["ar_audio_position.alpha"][0]),
                pe=sine_pe_table(4000), g=sd["ar_decoder.layers.0.norm1.weight"], b=sd["ar_decoder.layers.0.norm1.bias"])


@pytest.fixture(scope="module")
def probes(eng):
    """every probe of every logit row on both kernels and the three split-K factors, run once and shared by the tests below:
    list of dicts(row, kernel, splitk, ref = (v, kept, p, cdf), kind [n] in {'tok', 'first', 'last', 'rand'}, want [n], u [n], out)"""
    rng = np.random.default_rng(99)
    runs = []
    for row in R.sampler_rows():
        ref = R.sampler_ref(row["logits"], row["top_k"], row["temperature"])
        v, kept, p, cdf = ref
        first, last = (int(i) for i in np.flatnonzero(p > 0)[[0, -1]])
        pr = [("tok", t, u) for t, u in R.token_probes(p, cdf)]
        pr += [("first", first, np.float32(0.0)), ("last", last, np.float32(1.0 - 2.0 ** -24))]
        if row["filtered"]:
            pr += [("rand", R.sample_token(p, cdf, u), u) for u in rng.random(512, dtype=np.float32)]
        for splitk in (1, 2, 4):
            part = R.split_partials(row["logits"], splitk, rng)
            for kernel in (0, 1):
                cases = [dict(BASE, kernel=kernel, splitk=splitk, top_k=row["top_k"], temperature=row["temperature"], u=float(u),
                              partial=part, cur_pos=40 + (j % 5)) for j, (_, _, u) in enumerate(pr)]
                runs.append(dict(row=row, kernel=kernel, splitk=splitk, ref=ref, kind=[k for k, _, _ in pr],
                                 want=np.array([t for _, t, _ in pr]), u=np.array([u for _, _, u in pr], np.float32),
                                 out=run_cases(eng, cases)))
    return runs


def _token(out):
    """the sampled token: cur_tok of a surviving row, EOS for a row the pick stopped (nothing else stops a probe row)"""
    return np.where(out["active"] == 1, out["cur_tok"], R.EOS)


def test_probe_sets_are_complete(probes):
    for r in probes:
        row, kinds = r["row"], np.array(r["kind"])
        ntok = int((kinds == "tok").sum())
        if row["kept"] is not None and not row["name"].startswith("normal"):
            assert ntok == row["kept"], (row["name"], ntok)             # tie and lane-edge rows: no kept token is left out
        if not row["filtered"] and row["kept"] is None:
            assert ntok >= 64, (row["name"], ntok)


def test_reduced_logits_are_the_fp32_sum_bit_for_bit(probes):
    for r in probes:
        lg = r["out"]["logits"]
        if r["kernel"] == 0:
            assert (_bits(lg) == _bits(r["row"]["logits"])[None]).all(), (r["row"]["name"], r["splitk"])
            fl = r["out"]["fillers"]["logits"]                          # inactive rows are still reduced and exported (vx_ar_logits)
            assert (_bits(fl) == _bits(r["row"]["logits"])[None]).all()
        else:
            assert (lg == SENT_F).all()                                 # the session's sampler has no logits export


def test_midpoint_probes_return_their_token(probes):
    n = 0
    for r in probes:
        kinds, tok = np.array(r["kind"]), _token(r["out"])
        m = kinds == "tok"
        bad = np.flatnonzero(m & (tok != r["want"]))
        assert not len(bad), (r["row"]["name"], r["kernel"], r["splitk"], [(int(r["want"][i]), int(tok[i]), float(r["u"][i])) for i in bad[:5]])
        n += int(m.sum())
        p = r["ref"][2]
        for kind in ("first", "last"):                                  # u = 0 / u = 1 - 2^-24: the ends of the kept set
            i = r["kind"].index(kind)
            if p[r["want"][i]] >= R.P_MIN:                              # (T = 0.05: fp32 underflow legitimately moves the ends)
                assert tok[i] == r["want"][i], (r["row"]["name"], kind, r["kernel"], r["splitk"], int(tok[i]))
            assert r["ref"][1][tok[i]], (r["row"]["name"], kind, int(tok[i]))
    print(f"\n[sampler] {n} midpoint probes returned their token")


def test_random_draws_follow_the_float64_cdf(probes):
    worst = 0.0
    for r in probes:
        kinds, tok = np.array(r["kind"]), _token(r["out"])
        m = np.flatnonzero(kinds == "rand")
        if not len(m):
            continue
        v, kept, p, cdf = r["ref"]
        assert kept[tok[m]].all(), (r["row"]["name"], "a token outside the kept set")
        diff = m[tok[m] != r["want"][m]]
        edges = cdf[np.flatnonzero(kept)]
        for i in diff:
            assert np.abs(edges - float(r["u"][i])).min() <= EDGE, (r["row"]["name"], r["kernel"], r["splitk"], float(r["u"][i]),
                                                                    int(tok[i]), int(r["want"][i]))
        near = np.array([np.abs(edges - float(u)).min() <= EDGE for u in r["u"][m]])
        assert near.mean() <= 0.05, (r["row"]["name"], near.mean())     # expected share <= 50 * 2^-12 = 1.2 %
        worst = max(worst, len(diff) / len(m))
    print(f"\n[sampler] largest share of random draws that differ from the float64 token (all next to a CDF boundary): {worst:.4f}")


def test_sum_logp_increment(probes):
    worst = 0.0
    for r in probes:
        tok, p = _token(r["out"]), r["ref"][2]
        inc = r["out"]["sum_logp"].astype(np.float64) - np.float64(np.float32(BASE["sum_logp"]))
        err = np.abs(inc - np.log(p[tok]))
        assert err.max() < 1e-4, (r["row"]["name"], r["kernel"], r["splitk"], float(err.max()))
        worst = max(worst, float(err.max()))
    print(f"\n[sampler] max |sum_logp increment - float64 log p[token]| = {worst:.3e} (bound 1e-4)")


def test_surviving_rows_commit_their_token(probes):
    for r in probes:
        o, cs = r["out"], r["out"]["cases"]
        alive = o["active"] == 1
        tok = _token(o)
        ngen = np.array([c["n_gen"] for c in cs])
        pos = np.array([c["cur_pos"] for c in cs])
        ctx = np.array([c["ctx_len"] for c in cs])
        assert (tok[alive] != R.EOS).all()
        assert (o["gen"][alive] == tok[alive]).all() and (o["n_gen"][alive] == ngen[alive] + 1).all()
        assert (o["cur_pos"][alive] == pos[alive] + 1).all() and (o["ctx_len"][alive] == ctx[alive] + 1).all()
        assert (o["slot_meta"][alive, 1] == ctx[alive] + 1).all() and (o["slot_meta"][alive, 2] == 1).all()
        # an EOS pick: the row stops and leaves everything but the active flags where it was
        dead = ~alive
        assert (o["gen"][dead] == SENT_I).all() and (o["cur_tok"][dead] == SENT_I).all() and (o["n_gen"][dead] == ngen[dead]).all()
        assert (o["cur_pos"][dead] == pos[dead]).all() and (o["ctx_len"][dead] == ctx[dead]).all()
        assert (o["slot_meta"][dead, 1] == ctx[dead]).all() and (o["slot_meta"][dead, 2] == 0).all()
        assert (o["emb_h"][dead] == SENT_F).all() and (o["emb_xp"][dead] == SENT_F).all()
        assert (o["slot_meta"][:, 3] == SENT_I).all() and (o["n_active"] == o["n_active_want"]).all()
        # inactive rows of the same launches are untouched
        f = o["fillers"]
        assert (f["active"] == 0).all() and (f["cur_tok"] == SENT_I).all() and (f["gen"] == SENT_I).all()
        assert (f["n_gen"] == BASE["n_gen"]).all() and (f["ctx_len"] == BASE["ctx_len"]).all() and (f["sum_logp"] == np.float32(0.25)).all()
        assert (f["slot_meta"][:, 1] == BASE["ctx_len"]).all() and (f["slot_meta"][:, 2] == 0).all()
        assert (f["emb_h"] == SENT_F).all() and (f["emb_xp"] == SENT_F).all()


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("splitk", [1, 2, 4])
def test_stop_rule(eng, kernel, splitk):
    """EOS pick, force_eos_at reached, 1 + n_gen > 16 text_len and n_gen >= gen_stride each stop the row; one step before each of
    them the row survives"""
    row = next(r for r in R.sampler_rows() if r["name"] == "lane_edges")          # kept {0, 16, 17, 1019, 1020, 1024}
    v, kept, p, cdf = R.sampler_ref(row["logits"], row["top_k"], row["temperature"])
    part = R.split_partials(row["logits"], splitk, np.random.default_rng(4))
    u_of = {t: float(u) for t, u in R.token_probes(p, cdf)}
    base = dict(BASE, kernel=kernel, splitk=splitk, top_k=row["top_k"], temperature=1.0, partial=part)
    groups = [   # (launch constants and row state, stops?, token)
        (dict(base, u=u_of[1024]), True, 1024),
        (dict(base, u=u_of[1019]), False, 1019),
        (dict(base, u=u_of[17], force_eos_at=3, n_gen=3), True, 1024),
        (dict(base, u=u_of[17], force_eos_at=4, n_gen=3), False, 17),
        (dict(base, u=u_of[16], force_eos_at=0, n_gen=3), True, 1024),
        (dict(base, u=u_of[16], text_len=1, n_gen=16, gen_stride=32), True, 16),
        (dict(base, u=u_of[16], text_len=1, n_gen=15, gen_stride=32), False, 16),
        (dict(base, u=u_of[0], text_len=0, n_gen=0), True, 0),
        (dict(base, u=u_of[1020], n_gen=16, gen_stride=16), True, 1020),
        (dict(base, u=u_of[1020], n_gen=15, gen_stride=16), False, 1020),
        (dict(base, u=u_of[1020], active=0), None, None),
    ]
    for cs, stops, tok in groups:
        o = run_cases(eng, [cs])
        if stops is None:                                                # an inactive row is untouched
            assert (o["active"] == 0).all() and (o["n_gen"] == cs["n_gen"]).all() and (o["cur_tok"] == SENT_I).all()
            assert (o["gen"] == SENT_I).all() and (o["sum_logp"] == np.float32(0.25)).all() and (o["n_active"] == 0).all()
            assert (o["slot_meta"][:, :3] == [[r, cs["ctx_len"], 0] for r in ORDER[:4]]).all() and (o["emb_h"] == SENT_F).all()
            continue
        assert (o["active"] == (0 if stops else 1)).all(), cs
        assert (o["slot_meta"][:, 2] == (0 if stops else 1)).all() and (o["n_active"] == (0 if stops else 4)).all(), cs
        assert (o["slot_meta"][:, 0] == ORDER[:4]).all() and (o["slot"] == [(7 * r + 3) % 32 for r in ORDER[:4]]).all()
        if stops:
            assert (o["gen"] == SENT_I).all() and (o["cur_tok"] == SENT_I).all() and (o["n_gen"] == cs["n_gen"]).all(), cs
            assert (o["cur_pos"] == cs["cur_pos"]).all() and (o["ctx_len"] == cs["ctx_len"]).all() and (o["slot_meta"][:, 1] == cs["ctx_len"]).all()
            assert (o["emb_h"] == SENT_F).all() and (o["emb_xp"] == SENT_F).all()
        else:
            assert (o["gen"] == tok).all() and (o["cur_tok"] == tok).all() and (o["n_gen"] == cs["n_gen"] + 1).all(), cs
            assert (o["cur_pos"] == cs["cur_pos"] + 1).all() and (o["ctx_len"] == cs["ctx_len"] + 1).all()
            assert (o["slot_meta"][:, 1] == cs["ctx_len"] + 1).all()
        # sum_logp is accumulated before the stop test, with the sampled (not the forced) token
        assert np.abs(o["sum_logp"].astype(np.float64) - 0.25 - np.log(p[tok if not (stops and cs["force_eos_at"] >= 0) else
                                                                         R.sample_token(p, cdf, cs["u"])])).max() < 1e-4


def test_fused_next_step_embedding(probes, weights):
    import torch
    import torch.nn.functional as F
    k_err = y_err = 0.0
    rows = 0
    for r in probes:
        o = r["out"]
        alive = np.flatnonzero(o["active"] == 1)
        if not len(alive):
            continue
        tok = o["cur_tok"][alive]
        pos = np.array([o["cases"][i]["cur_pos"] for i in alive])
        # the multiply and the add are rounded separately (no fma)
        h = (weights["emb"][tok] + (weights["alpha"] * weights["pe"][pos + 1]).astype(np.float32)).astype(np.float32)
        assert (_bits(o["emb_h"][alive]) == _bits(h)).all(), (r["row"]["name"], r["kernel"], r["splitk"])
        want = R.layer_norm_ref(h, weights["g"], weights["b"])
        yard = F.layer_norm(torch.from_numpy(h), (1024,), torch.from_numpy(weights["g"]), torch.from_numpy(weights["b"]), 1e-5).numpy()
        k_err = max(k_err, float(np.abs(o["emb_xp"][alive] - want).max()))
        y_err = max(y_err, float(np.abs(yard - want).max()))
        rows += len(alive)
    print(f"\n[sampler] fused norm1 on {rows} rows: max |kernel - float64| = {k_err:.3e}, torch-CPU fp32 F.layer_norm = {y_err:.3e} "
          f"(ratio {k_err / y_err:.2f}, bound 4)")
    assert rows > 1000 and k_err <= 4.0 * y_err


def test_dec_and_serve_agree_bit_for_bit(probes):
    by = {(r["row"]["name"], r["splitk"], r["kernel"]): r["out"] for r in probes}
    n = 0
    for (name, splitk, kernel), a in by.items():
        if kernel:
            continue
        b = by[(name, splitk, 1)]
        for key in ("active", "n_gen", "cur_tok", "cur_pos", "ctx_len", "slot_meta", "gen", "n_active", "slot"):
            np.testing.assert_array_equal(a[key], b[key], err_msg=f"{name} splitk {splitk}: {key}")
            np.testing.assert_array_equal(a["fillers"][key], b["fillers"][key], err_msg=f"{name} splitk {splitk}: filler {key}")
        for key in ("sum_logp", "emb_h", "emb_xp"):
            assert (_bits(a[key]) == _bits(b[key])).all(), (name, splitk, key)
        n += len(a["active"])
    print(f"\n[sampler] dec_sample and serve_sample identical on {n} cases")
