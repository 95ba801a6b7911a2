"""GPU: the attention block of one decode step on the chains the kernel-selection switches select, against float64 -- the launch
sequences the default rule never reaches (tests/test_gpu_kernel_dec_attn.py holds the default ones): the unfused kernel with 8, 10 and
16 context splits + combine, the unfused one-split chain at 17 .. 32 rows (also what a context with Tmax < 128 decodes on), the
split-fused kernel at 5 .. 7 and 17 .. 32 rows, the fused one-split kernel at 5 .. 16 rows, the small-batch chain with other split
counts, and the small-batch chain WITHOUT the fused QKV (unfused dec_attn, the combine in the prologue of out_proj).

One test per line of the switch table (tests/_kernel_refs.py DEC_SWITCH_LINES; tests/test_kernel_refs.py pins (chain, splits) per row
count by hand and checks that the launch plans meet empty splits, a last split filled to a 16-row boundary and one row past it).  Each
test creates its own 2-layer context under the switch (tests/_util.py switched_model: never cached, dropped at teardown), which
asserts what vx_dev_switches reports; then the geometry vx_dev_dec_attn reports against the restated rule; then the launches:
stale arena rows of order 1e4 behind every context, the balanced and the four-slab layout on alternating launches (the small-batch
chain without QKV reads four slabs only; sb_qkv: packed x and eight linear2 slabs + residual alternate), one finished row per launch
from 3 rows up, and above 4 rows a permuted slot order (the engine's balanced order on even launches, the reversed one on odd ones).

Tolerance and bit-for-bit checks are those of tests/test_gpu_kernel_dec_attn.py, unchanged: rms and max error of the out_proj result,
of (m, l) and of the stored attention output at most 4 x the torch-CPU fp32 yardstick's against float64; empty splits (-1e30, 0);
sentinels behind the last split and in every output the chain does not write; appended K / V = the fp32 slab sum + bias; every other
arena word unchanged.  The measured ratios are printed ([dec_attn] lines); docs/log_r28.md records them."""
import numpy as np
import pytest

from oracle import synth
from tests import _kernel_refs as R
from tests import test_gpu_kernel_dec_attn as T
from tests._util import drop_switched, switched_model

pytestmark = pytest.mark.gpu

SENT_F = T.SENT_F
_REF = {}


@pytest.fixture(scope="module")
def W():
    return R.dec_layer0_weights(synth.vallex_state_dict(2, 1, 0.0))


@pytest.fixture
def context(monkeypatch):
    """engine of a fresh context under a line's switches, with the geometry of tests/test_gpu_kernel_dec_attn.py"""
    def make(line):
        spec = R.DEC_SWITCH_LINES[line]
        return switched_model(monkeypatch, spec["env"], spec["fields"], 2, 1, 0.0, max_new=160, max_prompt=96, max_text=32, max_batch=32).engine
    yield make
    drop_switched()


def launches(nrows, kind, W, chain, nsplit):
    """[(case, float64 reference, fp32 yardstick, active, slot order)] of a row count, operand set and geometry, computed once"""
    key = (nrows, kind, chain, nsplit)
    if key not in _REF:
        out = []
        for j, (ctx, fin) in enumerate(R.dec_switch_launches(nrows)):
            case = R.dec_case(kind, ctx, W, chain, seed=7000 + 100 * nrows + j, skp=8 * (j % 2) if chain == "sb_qkv" else 0,
                              balanced=j % 2 == 0 and chain not in ("sb", "sb_qkv"), stale=True)
            active = np.ones(nrows, np.int32)
            if fin is not None:
                active[fin] = 0
            order = np.arange(nrows, dtype=np.int32) if nrows <= 4 else R.balance_order(ctx) if j % 2 == 0 else np.arange(nrows - 1, -1, -1, dtype=np.int32)
            out.append((case, R.dec_attn_block_ref(case, W, nsplit), R.dec_attn_block_fp32(case, W, nsplit), active, order))
        if len(_REF) >= 4:
            _REF.pop(next(iter(_REF)))
        _REF[key] = out
    return _REF[key]


def chain_of(res, fuse_out):
    return ("sb_qkv" if res["sb_qkv"] else "sb" if res["sb_chain"] else "split_fused" if res["split_fused"]
            else "fused" if fuse_out and res["nsplit"] == 1 else "unfused")


def run_rows(eng, W, line, nrows, kind):
    """all launches of (line, row count, operand set): geometry, arena, append, (m, l) and sentinel checks per launch; the pooled errors"""
    fuse_out = R.DEC_SWITCH_LINES[line]["fields"].get("fuse_out", 1)
    chain, nsplit = R.dec_switch_geometry(line, nrows)
    eo, em, el, ea = T.Errors(), T.Errors(), T.Errors(), T.Errors()
    plan = launches(nrows, kind, W, chain, nsplit)
    assert nrows <= 4 or any(list(o) != list(range(nrows)) for *_, o in plan)
    for case, ref, yard, active, order in plan:
        args = {k: v for k, v in case.items() if k not in ("kind", "chain")}
        res = eng.dev_dec_attn(active=active, slot_order=order, **args)
        # above 4 rows the rule does not look at the slot order; up to 4 the order is the identity
        assert (chain_of(res, fuse_out), res["nsplit"]) == (chain, nsplit), ("the engine's rule picked another chain", line, nrows, res["nsplit"])
        live = active.astype(bool)
        new = T.check_arena(case, res, W, ref, live)
        if chain in ("sb", "sb_qkv"):                 # four split-K slabs of out_proj, summed exactly in float64; no bias
            got, want, y = res["out"].astype(np.float64).sum(0), ref["proj"], yard["proj"]
        else:
            assert (res["out"][1:] == SENT_F).all()
            got, want, y = res["out"][0].astype(np.float64), ref["h"], yard["h"]
        eo.add(got[live], want[live], y[live])
        if chain == "fused" or (chain == "unfused" and nsplit == 1):
            assert (res["part_ml"] == SENT_F).all(), "a chain with one split writes no (m, l)"
        else:
            T.check_part_ml(case, res, ref, yard, live, em, el)
        if chain == "sb_qkv":
            ea.add(new.reshape(nrows, 2048)[live], ref["qkv"][live, 1024:], yard["qkv"][live, 1024:])
        if chain == "unfused":                        # the (combined) attention output in front of out_proj
            ea.add(res["xp_att"][live], ref["attn"][live], yard["attn"][live])
        else:
            assert (res["xp_att"] == SENT_F).all(), "only the unfused chain stores the attention output"
        for r in np.flatnonzero(~live):
            # a finished row: its arena stream is unchanged (check_arena); the kernels that run one row per workgroup store nothing for it
            if chain in ("sb", "sb_qkv", "unfused"):
                assert (res["part_ml"][r] == SENT_F).all(), (r, "(m, l) of a finished row")
                assert (res["xp_att"][r] == SENT_F).all(), (r, "attention output of a finished row")
    return chain, nsplit, [("out_proj result", eo), ("split m", em), ("split l", el), ("appended k|v" if chain == "sb_qkv" else "attention output", ea)]


TWO = pytest.mark.parametrize("kind", ("model", "sharp"))
ALL = pytest.mark.parametrize("kind", R.DEC_KINDS)


def run_line(context, W, line, kind):
    eng = context(line)                               # asserts vx_dev_switches
    spec = R.DEC_SWITCH_LINES[line]
    for n in spec.get("geometry_only", ()):           # a row count the switch must leave alone
        chain, nsplit = R.dec_switch_geometry(line, n)
        case = R.dec_case("uniform", R.dec_launch_contexts(n)[0], W, chain, seed=1, stale=False)
        res = eng.dev_dec_attn(**{k: v for k, v in case.items() if k not in ("kind", "chain")})
        assert (chain_of(res, spec["fields"].get("fuse_out", 1)), res["nsplit"]) == (chain, nsplit) == R.dec_geometry(n), (line, n)
    for nrows in spec["rows"]:
        chain, nsplit, pools = run_rows(eng, W, line, nrows, kind)
        print(f"\n[dec_attn] {line}: {nrows} rows ({chain}, {nsplit} splits) / {kind}")
        T.assert_bound(f"{line} {nrows} rows {chain} {nsplit} / {kind}", pools)


@ALL
def test_sb_qkv_0(context, W, kind):
    """VX_SB_QKV=0, 1 .. 4 rows: the small-batch chain without the fused QKV, 16 | 16 | 8 | 8 splits -- no other test reaches it: all
    five operand sets"""
    run_line(context, W, "sb_qkv_0", kind)


@TWO
def test_sb_qkv_2(context, W, kind):
    """VX_SB_QKV=2: 2 rows on the sb_qkv chain (8 splits), 3 rows on the small-batch chain without QKV (8)"""
    run_line(context, W, "sb_qkv_2", kind)


@TWO
def test_sb_qkv_nsplit_4(context, W, kind):
    run_line(context, W, "sb_qkv_nsplit_4", kind)


@TWO
def test_sb_qkv_nsplit_8(context, W, kind):
    run_line(context, W, "sb_qkv_nsplit_8", kind)


@TWO
def test_sb_qkv_nsplit_16(context, W, kind):
    run_line(context, W, "sb_qkv_nsplit_16", kind)


@TWO
def test_sb_qkv_nsplit_5(context, W, kind):
    """a split count dec_attn_qkv_kernel is not instantiated for: the rule falls back to the small-batch chain without QKV, 16 splits"""
    run_line(context, W, "sb_qkv_nsplit_5", kind)


@ALL
def test_sb_fuse_0(context, W, kind):
    """VX_SB_FUSE=0, 1 .. 4 rows: the general unfused chain with 16 | 16 | 10 | 8 splits + combine -- no other test reaches these split
    counts: all five operand sets"""
    run_line(context, W, "sb_fuse_0", kind)


@TWO
def test_fuse_out_0(context, W, kind):
    """VX_FUSE_OUT=0: 8, 9, 16 rows unfused + combine with 2 splits; 17, 32 rows unfused with one split, no combine launch -- the chain
    a context with Tmax < 128 decodes 17 .. 32 rows on"""
    run_line(context, W, "fuse_out_0", kind)


@TWO
def test_fuse_split_0(context, W, kind):
    """VX_FUSE_SPLIT=0: 8, 11 rows unfused + combine with 2 splits; 17 rows stay on the fused chain"""
    run_line(context, W, "fuse_split_0", kind)


@TWO
def test_att_nsplit_1(context, W, kind):
    """VX_ATT_NSPLIT=1: the fused one-split kernel at 5 and 8 rows: the early first-tile request with 3 and 4 row pairs"""
    run_line(context, W, "att_nsplit_1", kind)


@TWO
def test_att_nsplit_2(context, W, kind):
    run_line(context, W, "att_nsplit_2", kind)


@TWO
def test_att_nsplit_4(context, W, kind):
    run_line(context, W, "att_nsplit_4", kind)


@TWO
def test_att_nsplit_8(context, W, kind):
    run_line(context, W, "att_nsplit_8", kind)


@TWO
def test_att_nsplit_16(context, W, kind):
    run_line(context, W, "att_nsplit_16", kind)


@TWO
def test_att_nsplit_3_fuse_split_0(context, W, kind):
    run_line(context, W, "att_nsplit_3_fuse_split_0", kind)


def test_switches_entry_refusals(context):
    from vallex_amd import Engine, VallexHipError
    from vallex_amd._capi import DEV_SWITCHES, VX_EINVAL, VX_ESTATE
    eng = context("sb_qkv_0")
    with pytest.raises(VallexHipError) as e:
        eng.dev_switches(n=len(DEV_SWITCHES) - 1)
    assert e.value.code == VX_EINVAL
    fresh = Engine(num_layers=2, max_batch=1, max_text=8, max_prompt=8, max_new=8, with_vocos=False)          # created, never finalized
    try:
        with pytest.raises(VallexHipError) as e:
            fresh.dev_switches()
        assert e.value.code == VX_ESTATE
    finally:
        fresh.close()


def test_small_batch_chain_without_qkv_refuses_the_balanced_layout(context, W):
    from vallex_amd import VallexHipError
    from vallex_amd._capi import VX_EINVAL
    eng = context("sb_qkv_0")
    case = R.dec_case("uniform", [18, 2, 130], W, "sb", seed=3, balanced=True, stale=False)
    with pytest.raises(VallexHipError) as e:
        eng.dev_dec_attn(**{k: v for k, v in case.items() if k not in ("kind", "chain")})
    assert e.value.code == VX_EINVAL and "four in_proj slabs" in str(e.value)
