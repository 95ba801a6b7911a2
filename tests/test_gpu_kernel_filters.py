"""GPU: serve_sample_kernel's per-row filter record (top_p, repetition penalty, min_frames) through vx_dev_sample_filtered, against
the float64 reference of tests/_filter_refs.py.  Every probe runs with the predict layer's split-K factors 1, 2 and 4, and the
cases of a launch fill decode rows 0, 1, 31 and 13 first.

Exact-token probes as in tests/test_gpu_kernel_sampler.py: u = fp32(midpoint of the CDF interval) of every kept token with float64
p >= 2^-12 must return that token; u = 0 and u = 1 - 2^-24 must return the first and the last kept token by index, which pins both
ends of the nucleus.  tests/test_filter_refs.py checks on the CPU that every top_p input used here keeps every keep / cut decision
at least 2^-12 of the mass away from flipping (four times the fp32 summation error), so the comparisons carry no allowance.
The bound on the sum_logp increment is the project's bound for this kernel, 1e-4.

The tests print their probe counts and the largest sum_logp error; docs/log_r12.md says what has been measured so far."""
import numpy as np
import pytest

from tests import _filter_refs as FR
from tests import _kernel_refs as R
from tests._util import get_model

pytestmark = pytest.mark.gpu

SENT_I = -123456789
SENT_F = np.float32(-1.0e30)
ORDER = [0, 1, 31, 13] + [r for r in range(32) if r not in (0, 1, 31, 13)]
BASE = dict(kernel=1, active=1, n_gen=3, cur_pos=40, ctx_len=77, text_len=4, gen_stride=64, force_eos_at=-1, sum_logp=0.25)
SLP0 = np.float64(np.float32(0.25))
U_LAST = np.float32(1.0 - 2.0 ** -24)
STATE = ("active", "n_gen", "cur_tok", "cur_pos", "ctx_len", "slot_meta", "gen", "slot")
FLOATS = ("sum_logp", "emb_h", "emb_xp")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run_placed(eng, launches, filtered=True):
    """launches: lists of (decode row, case); the other rows of a launch are inactive fillers.  Returns one output record per placed
    case, in order, and the fillers' under 'fillers'."""
    flat, where, fill = [], [], []
    for placed in launches:
        first = placed[0][1]
        launch = [dict(first, active=0, u=0.5) for _ in range(32)]
        for row, cs in placed:
            launch[row] = cs
            where.append(len(flat) + row)
        used = {row for row, _ in placed}
        fill += [len(flat) + r for r in range(32) if r not in used]
        flat += launch
    out = (eng.dev_sample_filtered if filtered else eng.dev_sample)(flat)
    res = {k: v[where] for k, v in out.items()}
    res["fillers"] = {k: v[fill] for k, v in out.items()}
    res["cases"] = [flat[i] for i in where]
    return res


def run_cases(eng, cases, filtered=True):
    """cases that share splitk and gen_stride; case j of a launch goes to decode row ORDER[j]"""
    cases = list(cases)
    while len(cases) < 4:
        cases = cases + cases[: 4 - len(cases)]
    return run_placed(eng, [[(ORDER[j], cs) for j, cs in enumerate(cases[l0:l0 + 32])] for l0 in range(0, len(cases), 32)], filtered)


def _token(out):
    return np.where(out["active"] == 1, out["cur_tok"], R.EOS)


def probes_of(p, cdf):
    """(kind, token, u): the midpoint of every token with p >= 2^-12, then the two ends of the kept set"""
    first, last = (int(i) for i in np.flatnonzero(p > 0)[[0, -1]])
    return [("tok", t, u) for t, u in R.token_probes(p, cdf)] + [("first", first, np.float32(0.0)), ("last", last, U_LAST)]


def check_probes(tag, out, pr, p):
    """every probe returned its token; returns the largest |sum_logp increment - float64 log p|"""
    tok = _token(out)[: len(pr)]
    want = np.array([t for _, t, _ in pr])
    bad = np.flatnonzero(tok != want)
    assert not len(bad), (tag, [(pr[i][0], int(want[i]), int(tok[i]), float(pr[i][2])) for i in bad[:5]])
    err = np.abs(out["sum_logp"][: len(pr)].astype(np.float64) - SLP0 - np.log(p[tok]))
    assert err.max() < 1e-4, (tag, float(err.max()))
    return float(err.max())


@pytest.fixture(scope="module")
def eng():
    return get_model(2, 1, 0.0, max_new=160, max_prompt=96, max_text=32, max_batch=32).engine


@pytest.fixture(scope="module")
def parts():
    """exact split-K addends of every logit row the tests use, computed once: parts[(row name, splitk)]"""
    rng = np.random.default_rng(1212)
    rows = {r["name"]: r["logits"] for r in R.sampler_rows()}
    rows.update(penalty_rows())
    rows["only_eos"] = only_eos_row()
    return {(name, sk): R.split_partials(lg, sk, rng) for name, lg in rows.items() for sk in (1, 2, 4)}, rows


def penalty_rows():
    """two rows whose history tokens (0, 16, 17, 500, 777, 1023) are all likely: 'pen' with those logits positive (l / r), 'pen_neg'
    the same row moved below zero (l * r)"""
    rng = np.random.default_rng(77)
    lg = rng.normal(0.0, 1.5, R.N_LOGITS).astype(np.float32)
    lg[[0, 16, 17, 500, 777, 1023]] = [4.0, 3.5, 4.25, 5.0, 4.5, 3.75]
    lg[R.EOS] = -1.0
    return {"pen": lg, "pen_neg": (lg - np.float32(9.0)).astype(np.float32)}


def only_eos_row():
    lg = np.full(R.N_LOGITS, -np.inf, np.float32)
    lg[R.EOS] = 1.0
    return lg


# ---- 1. neutral records ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splitk", [1, 2, 4])
def test_neutral_record_is_todays_sampler_bit_for_bit(eng, parts, splitk):
    """vx_dev_sample_filtered with (top_p 1, penalty 1, window 0, min_frames 0) and a history that must not be read (out-of-range
    tokens included) against vx_dev_sample kernel 1 on the round-11 rows, the tie rows included: tokens, every state word, sum_logp,
    emb_h and emb_xp, and the inactive rows of the launches"""
    parts, _ = parts
    cases = []
    for row in R.sampler_rows():
        v, kept, p, cdf = R.sampler_ref(row["logits"], row["top_k"], row["temperature"])
        pr = probes_of(p, cdf)
        pr = pr[:: max(1, len(pr) // 6)] + pr[-2:]
        for j, (_, _, u) in enumerate(pr):
            cases.append(dict(BASE, splitk=splitk, top_k=row["top_k"], temperature=row["temperature"], u=float(u),
                              partial=parts[(row["name"], splitk)], cur_pos=40 + j % 5))
    a = run_cases(eng, cases, filtered=False)
    b = run_cases(eng, [dict(c, top_p=1.0, repetition_penalty=1.0, repetition_window=0, min_frames=0,
                             hist=[int(np.argmax(c["partial"].sum(0))), 2_000_000, -7]) for c in cases])
    for key in STATE + ("n_active",):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
        np.testing.assert_array_equal(a["fillers"][key], b["fillers"][key], err_msg="filler " + key)
    for key in FLOATS:
        assert (_bits(a[key]) == _bits(b[key])).all(), key
        assert (_bits(a["fillers"][key]) == _bits(b["fillers"][key])).all(), key
    assert (b["active"] == 1).sum() > len(cases) // 2
    print(f"\n[filters] neutral record identical to vx_dev_sample on {len(cases)} cases (split-K {splitk})")


# ---- 2. top_p -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splitk", [1, 2, 4])
def test_top_p_keeps_the_float64_nucleus(eng, parts, splitk):
    parts, rows = parts
    worst, n = 0.0, 0
    runs = []
    cases = []
    for name, T, top_k, top_p, size in FR.filter_combos():
        _, kept, p, cdf = FR.filtered_sampler_ref(rows[name], [], top_k, T, top_p, 1.0, 0, 0, 0)
        assert int(kept.sum()) == size
        pr = probes_of(p, cdf)
        runs.append((name, T, top_k, top_p, pr, p, len(cases)))
        cases += [dict(BASE, splitk=splitk, top_k=top_k, temperature=T, top_p=top_p, u=float(u), partial=parts[(name, splitk)],
                       cur_pos=40 + j % 5) for j, (_, _, u) in enumerate(pr)]
    out = run_cases(eng, cases)
    for name, T, top_k, top_p, pr, p, o in runs:
        sub = {k: out[k][o:o + len(pr)] for k in ("active", "cur_tok", "sum_logp")}
        worst = max(worst, check_probes((name, T, top_k, top_p, splitk), sub, pr, p))
        n += len(pr)
    print(f"\n[filters] top_p: {n} probes returned their token (split-K {splitk}), max |sum_logp increment - float64 log p| = {worst:.3e} "
          "(bound 1e-4)")


# ---- 3. ties --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splitk", [1, 2, 4])
def test_ties_at_the_cut_are_kept(eng, parts, splitk):
    parts, rows = parts
    want_kept = {"all_equal": R.N_LOGITS, "ties_at_kth": 12, "four_finite": 2, "lane_edges": 5}
    for name, top_k, top_p, _ in FR.tie_combos():
        row = FR.row_by_name(name)
        _, kept, p, cdf = FR.filtered_sampler_ref(rows[name], [], top_k, row["temperature"], top_p, 1.0, 0, 0, 0)
        assert int(kept.sum()) == want_kept[name], (name, int(kept.sum()))
        pr = probes_of(p, cdf)
        if name == "all_equal":                        # p = 1 / 1025 each: above 2^-12, all 1025 are probed; the last is EOS
            assert len(pr) == R.N_LOGITS + 2 and pr[-1][1] == R.EOS and pr[-2][1] == 0
        if name == "lane_edges":                       # the lane boundaries 16 | 17 and the last lane's 1024 stay, 1020 is cut
            assert sorted(np.flatnonzero(kept)) == [0, 16, 17, 1019, 1024]
        out = run_cases(eng, [dict(BASE, splitk=splitk, top_k=top_k, temperature=row["temperature"], top_p=top_p, u=float(u),
                                   partial=parts[(name, splitk)]) for _, _, u in pr])
        check_probes((name, splitk), out, pr, p)


# ---- 4. repetition penalty ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splitk", [1, 2, 4])
def test_repetition_penalty_follows_the_reference(eng, parts, splitk):
    parts, rows = parts
    worst, n = 0.0, 0
    cases, runs = [], []
    for name in ("pen", "pen_neg"):
        for r in (1.3, 0.8):
            for hname, hist, n_gen, window in FR.penalty_histories():
                _, _, p, cdf = FR.filtered_sampler_ref(rows[name], hist, 20, 1.0, 1.0, r, window, 0, n_gen)
                pr = probes_of(p, cdf)
                runs.append(((name, r, hname), pr, p, len(cases)))
                cases += [dict(BASE, splitk=splitk, top_k=20, temperature=1.0, repetition_penalty=r, repetition_window=window,
                               n_gen=n_gen, hist=hist, u=float(u), partial=parts[(name, splitk)]) for _, _, u in pr]
    out = run_cases(eng, cases)
    for tag, pr, p, o in runs:
        sub = {k: out[k][o:o + len(pr)] for k in ("active", "cur_tok", "sum_logp")}
        worst = max(worst, check_probes(tag + (splitk,), sub, pr, p))
        n += len(pr)
    # the surviving rows wrote their token behind the history and left the history alone (gen[n_gen] is reported)
    alive = out["active"] == 1
    assert (out["gen"][alive] == out["cur_tok"][alive]).all()
    print(f"\n[filters] penalty: {n} probes returned their token (split-K {splitk}), max |sum_logp increment - float64 log p| = {worst:.3e}")


def test_penalty_probes_tell_the_window_and_the_repeat_apart():
    """the inputs above are sensitive to what they are meant to catch (CPU-only reasoning on the reference, run with the GPU file so
    it sits next to the cases): token 777 lies just outside a window of 5 and inside a window of 6; token 500 occurs three times"""
    rows = penalty_rows()
    hist = dict((h[0], h) for h in FR.penalty_histories())
    for name in ("pen", "pen_neg"):
        lg = rows[name]
        p5 = FR.filtered_sampler_ref(lg, hist["forty_w5"][1], 20, 1.0, 1.0, 1.3, 5, 0, 40)[2]
        p6 = FR.filtered_sampler_ref(lg, hist["forty_w6"][1], 20, 1.0, 1.0, 1.3, 6, 0, 40)[2]
        assert abs(np.log(p5[777]) - np.log(p6[777])) > 1e-2
        v = FR.penalised(lg, hist["forty_all"][1], 1.3, 0, 40)
        thrice = np.float32(np.float32(v[500] / np.float32(1.3)) / np.float32(1.3)) if lg[500] > 0 else np.float32(np.float32(
            v[500] * np.float32(1.3)) * np.float32(1.3))
        assert abs(float(thrice) - float(v[500])) > 1e-2                # per-occurrence would move log p by far more than 1e-4


# ---- 5. min_frames --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splitk", [1, 2, 4])
def test_min_frames(eng, parts, splitk):
    parts, rows = parts
    row = FR.row_by_name("lane_edges")                 # top_k 6 keeps {0, 16, 17, 1019, 1020, 1024}; EOS (3.9) is the largest logit
    assert int(np.argmax(row["logits"])) == R.EOS
    base = dict(BASE, splitk=splitk, top_k=6, temperature=1.0, partial=parts[("lane_edges", splitk)])
    # n_gen < m: no draw returns EOS, the row stays active and follows the masked distribution
    _, kept, p, cdf = FR.filtered_sampler_ref(row["logits"], [], 6, 1.0, 1.0, 1.0, 0, 4, 3)
    # EOS is masked before top_k, so the sixth place goes to the next largest logit
    assert not kept[R.EOS] and int(kept.sum()) == 6 and kept[[0, 16, 17, 1019, 1020]].all()
    pr = probes_of(p, cdf) + [("rand", R.sample_token(p, cdf, u), u) for u in np.linspace(0.01, 0.99, 23, dtype=np.float32)]
    out = run_cases(eng, [dict(base, min_frames=4, n_gen=3, hist=[1, 2, 3], u=float(u)) for _, _, u in pr])
    assert (out["active"] == 1).all() and (out["cur_tok"] != R.EOS).all() and (out["n_gen"] == 4).all()
    check_probes(("min_frames below", splitk), {k: out[k][: len(pr) - 23] for k in ("active", "cur_tok", "sum_logp")}, pr[:-23], p)
    assert kept[out["cur_tok"]].all()
    # n_gen == m: EOS is back
    _, kept, p, cdf = FR.filtered_sampler_ref(row["logits"], [], 6, 1.0, 1.0, 1.0, 0, 4, 4)
    assert kept[R.EOS]
    pr = probes_of(p, cdf)
    out = run_cases(eng, [dict(base, min_frames=4, n_gen=4, hist=[1, 2, 3, 4], u=float(u)) for _, _, u in pr])
    check_probes(("min_frames reached", splitk), out, pr, p)
    eos = np.array([t for _, t, _ in pr]) == R.EOS
    assert eos.any() and (out["active"][: len(pr)] == np.where(eos, 0, 1)).all()
    # force_eos_at <= n_gen still forces EOS, whatever min_frames says
    out = run_cases(eng, [dict(base, min_frames=10, n_gen=3, hist=[1, 2, 3], force_eos_at=f, u=0.3) for f in (0, 2, 3)])
    assert (out["active"] == 0).all() and (out["gen"] == SENT_I).all() and (out["n_gen"] == 3).all()
    out = run_cases(eng, [dict(base, min_frames=10, n_gen=3, hist=[1, 2, 3], force_eos_at=4, u=0.3)])
    assert (out["active"] == 1).all() and (out["cur_tok"] != R.EOS).all()
    # the 16 x text length stop still fires (1 + n_gen > 16 text_len), with a non-EOS token
    out = run_cases(eng, [dict(base, min_frames=100, text_len=1, n_gen=16, hist=list(range(16)), u=0.3)])
    assert (out["active"] == 0).all() and (out["n_gen"] == 16).all() and (out["gen"] == SENT_I).all()
    out = run_cases(eng, [dict(base, min_frames=100, text_len=1, n_gen=15, hist=list(range(15)), u=0.3)])
    assert (out["active"] == 1).all() and (out["n_gen"] == 16).all()
    # only EOS finite and n_gen < m: nothing finite is left, the guard samples EOS, the row stops and writes nothing else
    out = run_cases(eng, [dict(base, partial=parts[("only_eos", splitk)], top_k=tk, min_frames=4, n_gen=3, hist=[1, 2, 3], u=u)
                          for tk in (6, -100) for u in (0.0, 0.5, float(U_LAST))])
    assert (out["active"] == 0).all() and (out["n_gen"] == 3).all() and (out["gen"] == SENT_I).all() and (out["cur_tok"] == SENT_I).all()
    assert (out["cur_pos"] == 40).all() and (out["ctx_len"] == 77).all() and (out["slot_meta"][:, 1] == 77).all()
    assert (out["slot_meta"][:, 2] == 0).all() and (out["slot_meta"][:, 3] == SENT_I).all() and (out["n_active"] == 0).all()
    assert (out["emb_h"] == SENT_F).all() and (out["emb_xp"] == SENT_F).all()
    f = out["fillers"]
    assert (f["active"] == 0).all() and (f["cur_tok"] == SENT_I).all() and (f["gen"] == SENT_I).all() and (f["emb_h"] == SENT_F).all()
    assert (f["sum_logp"] == np.float32(0.25)).all() and (f["slot_meta"][:, 3] == SENT_I).all()


# ---- 6. mixed rows --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splitk", [1, 2, 4])
def test_mixed_launch_equals_single_rows(eng, parts, splitk):
    """one launch whose 32 rows mix top_p, penalty, min_frames, ties and neutral records: every row equals what it returns alone in
    the same decode row of its own launch, bit for bit"""
    parts, rows = parts
    h40 = dict((h[0], h) for h in FR.penalty_histories())["forty_w5"][1]
    kinds = [dict(top_k=-100, temperature=1.0, top_p=0.85, _row="normal_k-100"),
             dict(top_k=50, temperature=1.0, top_p=0.9, _row="normal_k50_T1.0"),
             dict(top_k=-100, temperature=4.0, top_p=0.65, _row="normal_k-100"),
             dict(top_k=20, temperature=1.0, repetition_penalty=1.3, repetition_window=5, n_gen=40, hist=h40, _row="pen"),
             dict(top_k=20, temperature=1.0, repetition_penalty=0.8, n_gen=40, hist=h40, top_p=0.9, _row="pen_neg"),
             dict(top_k=6, temperature=1.0, min_frames=4, n_gen=3, hist=[1, 2, 3], _row="lane_edges"),
             dict(top_k=10, temperature=1.0, top_p=0.1, _row="all_equal"),
             dict(top_k=10, temperature=1.0, _row="ties_at_kth"),
             dict(top_k=-100, temperature=0.7, _row="normal_k-100"),
             dict(top_k=6, temperature=1.0, min_frames=9, n_gen=3, hist=[5, 5, 5], force_eos_at=3, _row="lane_edges"),
             dict(top_k=-100, temperature=1.0, min_frames=4, n_gen=3, hist=[1, 2, 3], _row="only_eos")]
    us = np.random.default_rng(splitk).random(32, dtype=np.float32)
    placed = []
    for r in range(32):
        k = dict(kinds[r % len(kinds)])
        name = k.pop("_row")
        placed.append((r, dict(BASE, **dict(dict(hist=[7, 8, 9]), **k), splitk=splitk, u=float(us[r]), partial=parts[(name, splitk)],
                               cur_pos=40 + r % 5)))
    mixed = run_placed(eng, [placed])
    single = run_placed(eng, [[pc] for pc in placed])
    for key in STATE:
        np.testing.assert_array_equal(mixed[key], single[key], err_msg=key)
    for key in FLOATS:
        same = _bits(mixed[key]) == _bits(single[key])
        nan = np.isnan(mixed[key]) & np.isnan(single[key])               # the only_eos rows: sum_logp of a non-finite row
        assert (same | nan).all(), key
    stopped = int((mixed["active"] == 0).sum())
    assert 0 < stopped < 32 and (mixed["n_active"] == 32 - stopped).all()
