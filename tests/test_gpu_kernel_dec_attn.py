"""GPU: the attention block of one decode step (csrc/decode.hip: dec_attn_qkv_kernel, dec_attn_kernel in its unfused / split-fused /
fused variants, dec_attn_combine_kernel, dec_reduce_ln_split_kernel and the out_proj launches between them) on caller-chosen operands
against float64, through vx_dev_dec_attn (include/vallex_hip_dev.h), which runs the launch sequence of the engine's step with the
geometry the engine's own rule picks for the row count.

Row counts 1, 2, 3, 4, 5, 7, 8, 9, 11, 16, 17, 32: one per chain x split count, odd and even pair counts.  Contexts (with the new
token) 1, 2, 16, 17, 18, 33, 127, 128, 129, 130, 257, 300 mixed over the rows of the launches (tests/_kernel_refs.py
dec_launch_contexts; tests/test_kernel_refs.py checks on the CPU that every split count meets empty splits, a last split filled to a
16-row boundary and one row past it, and that the row pairs hold long + short, short + long and equal contexts).  The arena rows at
and behind ctx - 1 hold finite values of order 1e4 of both signs: a slot reused by a shorter request.

Tolerance: the yardstick is the error of a torch-CPU fp32 computation of the same block (F.layer_norm / F.linear / F.softmax and
matmuls) against float64 on the same fp32 operands; per row count and operand set, over the rows of all its launches, a chain's rms
error and its max error may each be at most 4 x the yardstick's.  The same rule holds (m, l) of the context splits against the
float64 split maximum and sum, and the small-batch chain's appended k_new / v_new (a VALU dot product).  The dec_attn chains append
the fp32 slab sum ((p0 + p1) + p2) + p3 + bias: bit for bit.  The measured ratios are printed ([dec_attn] lines); docs/log_r13.md records them."""
import numpy as np
import pytest

from oracle import synth
from tests import _kernel_refs as R
from tests._util import get_model

pytestmark = pytest.mark.gpu

SENT_F = np.float32(-1.0e30)
FACTOR = 4.0
TMAX = R.DEC_TMAX
_REF = {}


@pytest.fixture(scope="module")
def model():
    return get_model(2, 1, 0.0, max_new=160, max_prompt=96, max_text=32, max_batch=32)


@pytest.fixture(scope="module")
def eng(model):
    return model.engine


@pytest.fixture(scope="module")
def W():
    return R.dec_layer0_weights(synth.vallex_state_dict(2, 1, 0.0))


def launches(nrows, kind, W, stale=True, flip_layout=False):
    """[(case, float64 reference, fp32 yardstick)] of a row count and operand set, computed once.  Launch j of a dec_attn chain feeds
    the balanced slab layout (the product's default) for even j and four slabs for odd j; the small-batch chain reads the packed x
    (layer 0) for even j and eight linear2 slabs + residual for odd j.  flip_layout: the other layout, slabs with the same sums."""
    key = (nrows, kind, stale, flip_layout)
    if key not in _REF:
        chain, nsplit = R.dec_geometry(nrows)
        out = []
        for j, ctx in enumerate(R.dec_launch_contexts(nrows)):
            case = R.dec_case(kind, ctx, W, chain, seed=1000 * nrows + j, skp=8 * (j % 2), balanced=(j % 2 == 0) != flip_layout, stale=stale)
            if flip_layout:
                _, ref, yard = launches(nrows, kind, W, stale)[j]             # the same float64 sums: the same reference
            else:
                ref, yard = R.dec_attn_block_ref(case, W, nsplit), R.dec_attn_block_fp32(case, W, nsplit)
            out.append((case, ref, yard))
        if len(_REF) >= 8:
            _REF.pop(next(iter(_REF)))
        _REF[key] = out
    return _REF[key]


def run(eng, case, **kw):
    args = {k: v for k, v in case.items() if k not in ("kind", "chain")}
    args.update(kw)
    res = eng.dev_dec_attn(**args)
    chain, nsplit = R.dec_geometry(len(case["ctx_len"]))
    got = "sb_qkv" if res["sb_qkv"] else "split_fused" if res["split_fused"] else "fused" if res["nsplit"] == 1 else "unfused"
    assert (got, res["nsplit"]) == (chain, nsplit), ("the engine's rule picked another chain", got, res["nsplit"], chain, nsplit)
    return res


def result(case, res, ref, yard):
    """(kernel result, float64, yardstick) of the out_proj output: the small-batch chain hands out its four split-K slabs (summed here,
    exactly, in float64; no bias), the others h = resid + out_b + W_o attn"""
    if case["chain"] == "sb_qkv":
        return res["out"].astype(np.float64).sum(0), ref["proj"], yard["proj"]
    assert (res["out"][1:] == SENT_F).all()
    return res["out"][0].astype(np.float64), ref["h"], yard["h"]


def check_arena(case, res, W, ref, live):
    """every word of every arena stream is unchanged, except row ctx - 1 of the live rows: the appended k_new / v_new.  Returns the
    appended rows (n, 2, 16, 64)."""
    n = len(case["ctx_len"])
    new = np.zeros((n, 2, 16, 64), np.float32)
    for name, i in (("k", 0), ("v", 1)):
        after, before = res[name].copy(), res[name + "0"]
        for r in range(n):
            if live[r]:
                p = int(case["ctx_len"][r]) - 1
                new[r, i] = after[r, :, p]
                after[r, :, p] = before[r, :, p]
        diff = np.argwhere(after.view(np.uint32) != before.view(np.uint32))
        assert not len(diff), (name, "arena word changed at (row, head, t, d)", diff[:4].tolist(), len(diff))
    if case["chain"] != "sb_qkv":
        ek, ev = R.dec_append_expected(case, W)
        for r in range(n):
            if live[r]:
                np.testing.assert_array_equal(new[r, 0].view(np.uint32), ek[r].view(np.uint32), err_msg=f"appended K of row {r}")
                np.testing.assert_array_equal(new[r, 1].view(np.uint32), ev[r].view(np.uint32), err_msg=f"appended V of row {r}")
    return new


class Errors:
    """kernel and yardstick errors of one quantity over the case set; ratios of the rms and of the max"""

    def __init__(self):
        self.k, self.y = [], []

    def add(self, got, want, yard):
        got, want, yard = (np.asarray(a, np.float64).reshape(-1) for a in (got, want, yard))
        assert np.isfinite(got).all() and not (got == float(SENT_F)).any()
        self.k.append(got - want)
        self.y.append(yard - want)

    def ratios(self, tag):
        k, y = np.concatenate(self.k), np.concatenate(self.y)
        k_rms, y_rms, k_max, y_max = np.sqrt(np.mean(k ** 2)), np.sqrt(np.mean(y ** 2)), np.abs(k).max(), np.abs(y).max()
        assert y_rms > 0 and y_max > 0, tag
        print(f"[dec_attn] {tag}: rms {k_rms:.3e} = {k_rms / y_rms:.2f} x yardstick ({y_rms:.3e}), max {k_max:.3e} = {k_max / y_max:.2f} x "
              f"yardstick ({y_max:.3e}), {len(k)} values")
        return float(k_rms / y_rms), float(k_max / y_max)


def check_part_ml(case, res, ref, yard, live, em, el):
    """empty splits hold exactly (-1e30, 0); the others go into the error pools; what the chain does not write keeps the sentinel"""
    nsplit = res["nsplit"]
    pm = res["part_ml"]
    if case["chain"] == "fused":
        assert (pm == SENT_F).all(), "the one-split chain writes no (m, l)"
        return
    assert (pm[:, :, nsplit:] == SENT_F).all(), "(m, l) behind the last context split"
    for r in range(len(case["ctx_len"])):
        if not live[r]:
            continue
        empty = ref["l"][r] == 0
        assert (pm[r, :, :nsplit, 0][empty] == np.float32(-1.0e30)).all() and (pm[r, :, :nsplit, 1][empty] == 0).all(), (r, "empty split")
        em.add(pm[r, :, :nsplit, 0][~empty], ref["m"][r][~empty], yard["m"][r][~empty])
        el.add(pm[r, :, :nsplit, 1][~empty], ref["l"][r][~empty], yard["l"][r][~empty])


def run_set(eng, W, nrows, kind, stale=True, flip_layout=False, **kw):
    """all launches of (nrows, kind): arena / append / part_ml checks per launch, (errors of the result, of m, of l, of the sb chain's
    appended k | v) pooled over the launches, and the raw results"""
    eo, em, el, ea = Errors(), Errors(), Errors(), Errors()
    results = []
    for case, ref, yard in launches(nrows, kind, W, stale, flip_layout):
        res = run(eng, case, **kw)
        live = np.ones(nrows, bool)
        new = check_arena(case, res, W, ref, live)
        eo.add(*result(case, res, ref, yard))
        check_part_ml(case, res, ref, yard, live, em, el)
        if case["chain"] == "sb_qkv":
            ea.add(new.reshape(nrows, 2048), ref["qkv"][:, 1024:], yard["qkv"][:, 1024:])
        if case["chain"] == "unfused":
            # the combined attention output in front of out_proj, by the same rule
            ea.add(res["xp_att"], ref["attn"], yard["attn"])
        else:
            assert (res["xp_att"] == SENT_F).all(), "only the unfused chain stores the attention output"
        results.append(res)
    return eo, em, el, ea, results


def assert_bound(tag, pools):
    bad = []
    for name, e in pools:
        if e.k:
            r_rms, r_max = e.ratios(f"{tag} / {name}")
            if r_rms > FACTOR or r_max > FACTOR:
                bad.append((name, round(r_rms, 2), round(r_max, 2)))
    assert not bad, f"{tag}: error above {FACTOR} x the fp32 yardstick (quantity, rms ratio, max ratio): {bad}"


@pytest.mark.parametrize("kind", R.DEC_KINDS)
@pytest.mark.parametrize("nrows", R.DEC_ROWS)
def test_block_against_float64(eng, W, nrows, kind):
    chain, nsplit = R.dec_geometry(nrows)
    print(f"\n[dec_attn] {nrows} rows ({chain}, {nsplit} splits) / {kind}")
    eo, em, el, ea, _ = run_set(eng, W, nrows, kind)
    assert_bound(f"{nrows} rows {chain} / {kind}", [("out_proj result", eo), ("split m", em), ("split l", el),
                                                    ("appended k|v" if chain == "sb_qkv" else "attention output", ea)])


@pytest.mark.parametrize("nrows", [1, 5, 9, 17])
def test_zero_rows_behind_the_context(eng, W, nrows):
    """the state a fresh arena has: zeros at and behind ctx - 1 (one chain each)"""
    chain, _ = R.dec_geometry(nrows)
    eo, em, el, ea, _ = run_set(eng, W, nrows, "uniform", stale=False)
    assert_bound(f"{nrows} rows {chain} / uniform, zero fill", [("out_proj result", eo), ("split m", em), ("split l", el), ("k|v / attention", ea)])


@pytest.mark.parametrize("nrows", [5, 7, 8, 9, 11, 16, 17, 32])
def test_slot_order_does_not_matter(eng, W, nrows):
    """The arena and the slot records are indexed by launch slot, slabs and outputs by batch row.  From decode.hip: a row's arithmetic
    never depends on its slot or on its workgroup partner -- the unfused kernel runs one row per workgroup; the fused kernels run rows
    y and y + ceil(n / 2) in waves 0-7 and 8-15 of one workgroup, both halves execute the same instruction sequence on their own
    registers and their own sh_o / sh_ot rows, the early first tile of the one-split kernel holds the same values as the late one, and
    a missing or finished partner only skips stores.  So EVERY row's result, (m, l) and appended K / V must be bit-identical under any
    slot order, on every chain; the bound against float64 is checked again per order."""
    chain, _ = R.dec_geometry(nrows)
    base = run_set(eng, W, nrows, "model")
    orders = {"balanced": [R.balance_order(c["ctx_len"]) for c, _, _ in launches(nrows, "model", W)],
              "reversed": [np.arange(nrows - 1, -1, -1, dtype=np.int32)] * 12}
    for name, per_launch in orders.items():
        pools = [Errors() for _ in range(4)]
        for j, (case, ref, yard) in enumerate(launches(nrows, "model", W)):
            order = per_launch[j]
            assert sorted(order) == list(range(nrows))
            res = run(eng, case, slot_order=order)
            check_arena(case, res, W, ref, np.ones(nrows, bool))
            pools[0].add(*result(case, res, ref, yard))
            for k in ("out", "part_ml", "xp_att", "k", "v"):
                np.testing.assert_array_equal(res[k].view(np.uint32), base[4][j][k].view(np.uint32), err_msg=f"{name} order, launch {j}: {k}")
        assert_bound(f"{nrows} rows {chain} / model / {name} order", [("out_proj result", pools[0])])


FINISHED = {3: [1], 5: [2], 9: [0, 6, 2, 7], 16: [0, 9, 2, 10], 17: [0, 10, 2, 11]}


@pytest.mark.parametrize("nrows", list(FINISHED))
def test_finished_rows(eng, W, nrows):
    """a finished row (active 0) in the first half of a pair, one in the second half, a pair with both halves finished (9 rows: pairs
    (0, 5), (1, 6), (2, 7); 16: (0, 8), (1, 9), (2, 10); 17: (0, 9), (1, 10), (2, 11)), and one at <= 4 rows and on the unfused chain.
    Its whole arena stream is unchanged bit for bit, and what a chain writes per live row keeps the sentinel: (m, l) on the small-batch
    and the unfused chain, the unfused chain's attention output.  The split-fused kernel stores (m, l) of a finished half under
    `valid`, not `live`, when the other half is live: the new token alone (l = 1, every other split empty), asserted here so that a
    finished half can never come to read a stale context; a pair of two finished halves returns before any store.  (The reduce kernels and the small-batch out_proj compute every row of the launch.)  The live rows are bit-identical to the launch in which every row is live."""
    chain, nsplit = R.dec_geometry(nrows)
    case, ref, yard = launches(nrows, "model", W)[0]
    full = run(eng, case)
    active = np.ones(nrows, np.int32)
    active[FINISHED[nrows]] = 0
    res = run(eng, case, active=active)
    live = active.astype(bool)
    check_arena(case, res, W, ref, live)
    for r in FINISHED[nrows]:
        if chain in ("sb_qkv", "unfused"):
            assert (res["part_ml"][r] == SENT_F).all(), (r, "(m, l) of a finished row")
        if chain == "split_fused":
            gy = (nrows + 1) // 2
            mate = r + gy if r < gy else r - gy                     # the other half of the workgroup (identity order)
            if mate >= nrows or not live[mate]:                     # both halves finished: the workgroup returns before any store
                assert (res["part_ml"][r] == SENT_F).all(), (r, "(m, l) of a finished pair")
                continue
            # a finished half beside a live one streams nothing (ctx = 1 whatever its record says): its splits are empty and the last
            # one holds the new token alone, l = 1 exactly and m = q . k_new / 8 of the row's own slabs
            pm = res["part_ml"][r, :, :nsplit]
            assert (pm[:, :-1, 0] == np.float32(-1.0e30)).all() and (pm[:, :-1, 1] == 0).all(), (r, "a finished half streamed rows")
            assert (pm[:, -1, 1] == 1.0).all(), (r, "l of a finished half", pm[:, -1, 1])
            q, kn = ref["qkv"][r, :1024].reshape(16, 64), ref["qkv"][r, 1024:2048].reshape(16, 64)
            want = (q * kn).sum(-1) / 8.0                 # (64 fp32 products of size <= ~10 each: rounding far below 1e-4)
            assert np.abs(pm[:, -1, 0] - want).max() <= 1e-4 * max(1.0, np.abs(want).max()), (r, "m of a finished half")
        if chain == "unfused":
            assert (res["xp_att"][r] == SENT_F).all(), (r, "attention output of a finished row")
    out = res["out"] if chain == "sb_qkv" else res["out"][:1]
    for k, a, b in (("out", out[:, live], (full["out"] if chain == "sb_qkv" else full["out"][:1])[:, live]),
                    ("part_ml", res["part_ml"][live], full["part_ml"][live]), ("xp_att", res["xp_att"][live], full["xp_att"][live]),
                    ("k", res["k"][live], full["k"][live]), ("v", res["v"][live], full["v"][live])):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=f"{k} of the live rows")
    eo = Errors()
    g, w_, y = result(case, res, ref, yard)
    eo.add(g[live], w_[live], y[live])
    assert_bound(f"{nrows} rows {chain} / model / rows {FINISHED[nrows]} finished", [("out_proj result", eo)])


@pytest.mark.parametrize("nrows", [5, 7, 8, 9, 11, 16, 17, 32])
def test_slab_layouts_agree(eng, W, nrows):
    """every launch of the row count in both layouts -- four slabs of q | k | v and the balanced layout (eight of q, four of k and v)
    -- with the same float64 sums: each layout meets the bound against the same float64 result, pooled over its launches; k and v
    have the same four slabs in both layouts, so the appended rows are bit-identical"""
    chain, _ = R.dec_geometry(nrows)
    a = run_set(eng, W, nrows, "model")
    b = run_set(eng, W, nrows, "model", flip_layout=True)
    pools = {"balanced slabs": Errors(), "four slabs": Errors()}
    plan_a, plan_b = launches(nrows, "model", W), launches(nrows, "model", W, flip_layout=True)
    for j, ((ca, ref, yard), (cb, _, _)) in enumerate(zip(plan_a, plan_b)):
        assert {ca["qkv"].shape[0], cb["qkv"].shape[0]} == {4, 8}
        np.testing.assert_array_equal(ca["qkv"].astype(np.float64).sum(0)[:, :1024], cb["qkv"].astype(np.float64).sum(0)[:, :1024])
        np.testing.assert_array_equal(ca["qkv"][:4, :, 1024:], cb["qkv"][:4, :, 1024:])
        for case, res in ((ca, a[4][j]), (cb, b[4][j])):
            pools["balanced slabs" if case["qkv"].shape[0] == 8 else "four slabs"].add(*result(case, res, ref, yard))
        for k in ("k", "v"):
            np.testing.assert_array_equal(a[4][j][k].view(np.uint32), b[4][j][k].view(np.uint32), err_msg=f"launch {j}: appended {k}")
    assert_bound(f"{nrows} rows {chain} / model / layouts", list(pools.items()))


def test_entry_refusals_and_context_state(model, eng, W):
    from vallex_amd import VallexHipError
    from vallex_amd._capi import VX_EINVAL, VX_ESTATE
    a, t = synth.synth_prompt(40, 8, seed=4)
    row = dict(text=np.concatenate([t[0], synth.synth_text(12, 4)]), prompt=a[0], enroll=8, prompt_language="en", text_language="en")
    eng.ar_prefill(model.make_batch([row]))
    before = eng.ar_logits()[0].copy()
    case5 = launches(5, "uniform", W)[0][0]
    case3 = launches(3, "uniform", W)[0][0]

    def refused(code, case, **kw):
        with pytest.raises(VallexHipError) as e:
            run(eng, case, **kw)
        assert e.value.code == code, (e.value, kw)

    refused(VX_EINVAL, case5, slot_order=np.array([0, 1, 1, 3, 4], np.int32))            # no permutation
    refused(VX_EINVAL, case5, slot_order=np.array([0, 1, 2, 3, 5], np.int32))            # out of range
    refused(VX_EINVAL, case3, slot_order=np.array([1, 0, 2], np.int32))                  # <= 4 rows: the identity only
    refused(VX_EINVAL, case5, tmax=int(case5["ctx_len"].max()) - 1, k_fill=0.0, v_fill=0.0)      # a context beyond Tmax
    refused(VX_EINVAL, R.dec_case("uniform", [1, 2, 16], W, "sb_qkv", seed=1, stale=False, tmax=R.DEC_TILE - 1))      # Tmax below one tile
    refused(VX_EINVAL, R.dec_case("uniform", [1], W, "sb_qkv", seed=1, stale=False, tmax=4097))                      # ... above the entry's 4096
    none = [np.zeros((0, 16, 64), np.float32)] * 5
    refused(VX_EINVAL, dict(case5, ctx_len=np.array([1, 1, 0, 1, 1], np.int32), k_rows=none, v_rows=none, k_fill=0.0, v_fill=0.0))
    # the entry works on private scratch: the decode state of the context is as the prefill left it
    run(eng, case5)
    np.testing.assert_array_equal(eng.ar_logits()[0], before)
    with eng.serve():
        refused(VX_ESTATE, case5)
    eng.ar_prefill(model.make_batch([row]))
    np.testing.assert_array_equal(eng.ar_logits()[0], before)
