"""GPU: the GEMM / FFN / LayerNorm half of one decode step (csrc/decode.hip: skinny_gemm_kernel in its four roles, skinny_qkv_bal_kernel,
skinny16_relu_pack_kernel, dec_reduce_ln_pack_kernel<0 | 4 | 8 | 16>, the small-batch consumers skinny_gemm_sb_kernel<0, 8> and
skinny16_sb_kernel<4>, dec_embed_ln_pack_kernel, and the load-time images of pack_weight_kernel / pack_weight16_kernel), one launch at a
time through vx_dev_dec_op (include/vallex_hip_dev.h) on the context's own weight images.

Exact probes, bit for bit: one-hot rows 2^e e_k read every word of every packed weight back through the kernel that consumes it (the
owning K slice holds W[n][k] 2^e, every other slab the kernel writes holds 0, what it does not write keeps the sentinel); the ordered
fp32 slab sum of the reduce kernels; the two roundings of the embedding and its identity with the sampler's fused embedding; the
small-batch consumers against the stand-alone kernels they claim to repeat operation for operation.

Float64 comparisons: per op, row count and operand set, over the rows of all launches, the rms and the max error against float64 may
each be at most 4 x those of the torch-CPU fp32 formulation (F.linear, F.layer_norm) on the same fp32 operands -- the rule of
tests/test_gpu_kernel_dec_attn.py.  tests/test_kernel_refs.py ties the references to the oracle and asserts that no yardstick pool is
zero.  The measured ratios are printed ([dec_ffn] lines); docs/log_r14.md records them."""
import numpy as np
import pytest

from oracle import synth
from tests import _kernel_refs as R
from tests._util import get_model

pytestmark = pytest.mark.gpu

SENT_F = np.float32(-1.0e30)
FACTOR = 4.0
NL = 2


@pytest.fixture(scope="module")
def model():
    return get_model(2, 1, 0.0, max_new=160, max_prompt=96, max_text=32, max_batch=32)


@pytest.fixture(scope="module")
def eng(model):
    return model.engine


@pytest.fixture(scope="module")
def W():
    return R.ffn_weights(synth.vallex_state_dict(2, 1, 0.0), NL)


@pytest.fixture(scope="module")
def pe():
    from vallex_amd.models.vallex import sine_pe_table
    return sine_pe_table(4000)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b, what):
    d = np.argwhere(bits(a) != bits(b))
    assert not len(d), (what, "first differing word at", d[0].tolist(), "of", len(d), np.asarray(a)[tuple(d[0])], np.asarray(b)[tuple(d[0])])


def same_values(a, b, what):
    """equal as numbers (a zero of either sign is a zero); the sentinel compares as itself"""
    d = np.argwhere(~(np.asarray(a) == np.asarray(b)))
    assert not len(d), (what, "first differing word at", d[0].tolist(), "of", len(d), np.asarray(a)[tuple(d[0])], np.asarray(b)[tuple(d[0])])


class Errors:
    """kernel and yardstick errors of one quantity over the launches of a set; ratios of the rms and of the max"""

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
        print(f"[dec_ffn] {tag}: rms {k_rms:.3e} = {k_rms / y_rms:.2f} x yardstick ({y_rms:.3e}), max {k_max:.3e} = {k_max / y_max:.2f} x "
              f"yardstick ({y_max:.3e}), {len(k)} values")
        return float(k_rms / y_rms), float(k_max / y_max)


def assert_bound(tag, pools):
    bad = []
    for name, e in pools:
        r_rms, r_max = e.ratios(f"{tag} / {name}")
        if r_rms > FACTOR or r_max > FACTOR:
            bad.append((name, round(r_rms, 2), round(r_max, 2)))
    assert not bad, f"{tag}: error above {FACTOR} x the fp32 yardstick (quantity, rms ratio, max ratio): {bad}"


def slab_sum(op, out, n):
    """the exact (float64) sum of the fp32 slabs a GEMM launch left, rows < n; the balanced layout: q from eight slabs, k | v from four"""
    o = out.astype(np.float64)
    if op == "qkv_bal":
        assert (out[4:, :, 1024:] == SENT_F).all(), "the k, v columns of slabs 4 .. 7 are not written"
        return np.concatenate([o[:, :n, :1024].sum(0), o[:4, :n, 1024:].sum(0)], -1)
    return o[:, :n].sum(0)


def check_reduce_exact(launch, res, sk):
    """h of a reduce launch = resid + ((((p0 + p1) + ...) + p_last) + bias) in fp32, in that order; the residual buffer"""
    a = launch["args"]
    n = a["nrows"]
    if sk == 0:
        assert (res["h"] == SENT_F).all(), "reduce_ln without slabs stores no h"
        same_bits(res["resid"], a["resid"], "the residual rows of reduce_ln without slabs")
        return
    want = R.reduce_h_exact(a["slabs"][:, :n], launch["bias"], a["resid"])
    same_bits(res["h"], want, f"{a['op']}: h = the ordered fp32 slab sum")
    if a["op"] == "reduce_ln":
        same_bits(res["resid"], want, "reduce_ln works in place")
    else:
        same_bits(res["resid"], a["resid"], f"{a['op']}: the residual buffer (the other half of the dh / dh2 pair)")


def run_case(eng, W, op, nrows, kind):
    """all launches of (op, rows, set): the exact side checks per launch and the error pools of its quantities"""
    name, _, arg = op.partition(":")
    pools = {}
    for j, launch in enumerate(R.ffn_case(op, nrows, kind, W)):
        a = launch["args"]
        res = eng.dev_dec_op(**a)
        n = nrows
        if name in ("gemm", "qkv_bal", "sb_ln_gemm"):
            N = 1025 if arg == "predict" else res["out"].shape[-1]
            got = {"sum": slab_sum(name, res["out"], n)[:, :N]}
            if arg == "predict":
                assert (res["out"][:, :n, 1025:] == 0).all(), "predict's padding columns"
        elif name in ("linear1", "sb_linear1"):
            got = {"act": res["out"][:n]}
        else:
            got = {"xp": res["xp"][:n]}
            assert (res["xp"][n:] == SENT_F).all(), "image rows behind the last row"
            if kind == "const" and j == 0:              # (v - mean) is exactly 0: the result is the norm's bias whatever rstd is
                same_bits(res["xp"][:n], np.repeat(np.asarray(launch["norm"][1], np.float32)[None], n, 0), "LayerNorm of a constant row")
        if name in ("reduce_ln", "sb_ln_gemm", "sb_linear1"):
            check_reduce_exact(launch, res, int(arg) if name == "reduce_ln" else 8 if name == "sb_ln_gemm" else 4)
        if name == "sb_ln_gemm":
            assert (res["out"][:, n:] == 0).all(), "rows behind the batch are zero columns of the MFMA"
        if name == "sb_linear1":
            same_bits(res["out"][n:16], np.repeat(np.maximum(W[a["layer"]]["l1_b"], np.float32(0))[None], 16 - n, 0), "rows behind the batch: relu(0 + b1)")
            assert (res["out"][16:] == SENT_F).all(), "the second 16-row column block does not exist at these batch sizes"
        for q, g in got.items():
            pools.setdefault(q, Errors()).add(g, launch["ref"][q], launch["yard"][q])
            if kind == "cancel" and name != "linear1":
                cols = R.cancel_columns(arg or "in_proj")
                pools.setdefault(q + ", cancelling columns", Errors()).add(g[:, cols], launch["ref"][q][:, cols], launch["yard"][q][:, cols])
    return pools


# ---- float64 comparisons ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nrows", R.FFN_ROWS)
@pytest.mark.parametrize("op", R.FFN_OPS)
def test_op_against_float64(eng, W, op, nrows):
    print()
    for kind in R.ffn_sets(op):
        assert_bound(f"{op} / {nrows} rows / {kind}", list(run_case(eng, W, op, nrows, kind).items()))


@pytest.mark.parametrize("nrows", R.FFN_SB_ROWS)
@pytest.mark.parametrize("op", R.FFN_SB_OPS)
def test_small_batch_op_against_float64(eng, W, op, nrows):
    print()
    for kind in R.ffn_sets(op):
        assert_bound(f"{op} / {nrows} rows / {kind}", list(run_case(eng, W, op, nrows, kind).items()))


@pytest.mark.parametrize("nrows", R.FFN_SB_ROWS + R.FFN_ROWS)
def test_chain_against_float64(eng, W, nrows):
    """norm2 -> linear1 -> linear2 -> reduce -> predict of the last layer, every stage fed the previous stage's GPU output: the general
    kernels from 5 rows, the small-batch consumers (with linear2's stand-alone GEMM between them) up to 4.  The logits (slab sum)
    against the float64 chain from the first input."""
    slabs, resid = R.ln_operands("normal", 4, W[1]["out_b"], nrows, 500 + nrows)[0]
    ref, yard = R.ffn_chain_ref(slabs[:, :nrows], resid, W, 1)
    if nrows <= 4:
        a = eng.dev_dec_op("sb_linear1", nrows, layer=1, slabs=slabs, resid=resid)
        l2 = eng.dev_dec_op("gemm", nrows, layer=1, weight="linear2", x=a["out"])["out"]
        out = eng.dev_dec_op("sb_ln_gemm", nrows, layer=1, weight="predict", slabs=l2, resid=a["h"])["out"]
    else:
        a = eng.dev_dec_op("reduce_ln", nrows, layer=1, sk=4, slabs=slabs, resid=resid)
        act = eng.dev_dec_op("linear1", nrows, layer=1, x=a["xp"])["out"]
        l2 = eng.dev_dec_op("gemm", nrows, layer=1, weight="linear2", x=act)["out"]
        b = eng.dev_dec_op("reduce_ln", nrows, layer=1, sk=8, slabs=l2, resid=a["h"])
        out = eng.dev_dec_op("gemm", nrows, layer=1, weight="predict", x=b["xp"])["out"]
    e = Errors()
    e.add(slab_sum("gemm", out, nrows)[:, :1025], ref, yard)
    print()
    assert_bound(f"chain / {nrows} rows", [("logits", e)])


# ---- identity probes --------------------------------------------------------------------------------------------------------------
PROBED = [("gemm", "in_proj"), ("qkv_bal", "in_proj"), ("gemm", "out_proj"), ("linear1", "linear1"), ("gemm", "linear2"), ("gemm", "predict")]


@pytest.mark.parametrize("op,wname", PROBED, ids=[f"{o}-{w}" for o, w in PROBED])
def test_identity_probes_read_every_weight_word(eng, W, op, wname):
    """K / 32 launches of 32 one-hot rows walk every k of the weight (layer 0): every word W[n][k] comes back, scaled by the row's
    power of two, from the slab that owns k, and every other slab the kernel writes holds 0 in that row -- the products are exact and
    every other addend is a zero, so there is no tolerance.  Then one launch at 5 rows whose image rows 5 .. 31 hold the sentinel."""
    wt = R.ffn_weight(W, wname, 0)
    N, K = wt.shape
    args = dict(op=op, layer=0)
    if op == "gemm":
        args["weight"] = wname
    npad, sk = (R.FFN_GEMMS[wname][1], R.FFN_GEMMS[wname][3]) if op == "gemm" else (3072, 8)
    plan = R.probe_plan(K)
    words = 0
    for nrows, launches in ((32, plan), (5, plan[1:2])):
        for ks in launches:
            out = eng.dev_dec_op(nrows=nrows, x=R.probe_image(ks, K, nrows), **args)["out"]
            if op == "linear1":
                exp = R.probe_expected_linear1(wt, W[0]["l1_b"], ks)
            else:
                exp = R.probe_expected(wt, ks, npad, sk, balanced=op == "qkv_bal")
            same_values(out[..., :nrows, :], exp[..., :nrows, :], f"{op} {wname}, {nrows} rows, k = {ks[:3].tolist()} ...")
            words += nrows * N
    assert words == N * K + 5 * N


# ---- the slab sums, the embedding, the small-batch consumers ---------------------------------------------------------------------
@pytest.mark.parametrize("sk", [0, 4, 8, 16])
def test_reduce_slab_sum_order(eng, W, sk):
    """slabs whose fp32 sum depends on the order (+-1e4 pairs that cancel to order 1): h = resid + ((((p0 + p1) + ...) + p_last) + bias)
    bit for bit at every row count and on both layers; no slabs: nothing is stored where h would go"""
    for nrows in R.FFN_ROWS:
        for layer in (0, 1):
            bias, norm = R.ffn_reduce_params(W, layer, sk)
            slabs, resid = R.ln_operands("slabs1e4" if sk else "normal", sk, bias, nrows, 40 + nrows)[0]
            res = eng.dev_dec_op("reduce_ln", nrows, layer=layer, sk=sk, slabs=slabs if sk else None, resid=resid)
            check_reduce_exact(dict(args=dict(op="reduce_ln", nrows=nrows, slabs=slabs, resid=resid), bias=bias), res, sk)
            if sk:                          # and the order matters on these operands: the bias in front of the slabs gives other bits
                other = R.reduce_h_exact(np.concatenate([np.repeat(np.asarray(bias, np.float32)[None, None], nrows, 1), slabs[:, :nrows]]), None, resid)
                assert (bits(other) != bits(res["h"])).any()


EMB_TOK = (0, 1, 1023, 1024)
EMB_POS = (0, 1, 3999)


def test_embedding_two_roundings_and_the_sampler(eng, W, pe):
    """h = fp32(emb + fp32(alpha pe)) bit for bit (a contraction into one fma differs on these rows: tests/test_kernel_refs.py), norm1
    of layer 0 against float64, and for the same (tok, pos) h and the x image are bit-identical to what the decode samplers' fused
    embedding leaves (the token forced with top_k = 1; the sampler embeds at cur_pos + 1 and never embeds EOS = 1024)"""
    import torch
    import torch.nn.functional as F
    tok = np.repeat(EMB_TOK, len(EMB_POS)).astype(np.int32)
    pos = np.tile(EMB_POS, len(EMB_TOK)).astype(np.int32)
    n = len(tok)
    res = eng.dev_dec_op("embed", n, tok=tok, pos=pos)
    want = R.embed_exact(W["emb"], W["alpha"], pe, tok, pos)
    same_bits(res["h"], want, "h of embed")
    assert (res["xp"][n:] == SENT_F).all()
    g, b = W[0]["n1"]
    e = Errors()
    e.add(res["xp"][:n], R.layer_norm_ref(want, g, b), F.layer_norm(torch.from_numpy(want), (1024,), torch.from_numpy(g), torch.from_numpy(b), 1e-5).numpy())
    print()
    assert_bound("embed / norm1", [("xp", e)])
    # one row alone gives the same bits as the row inside a launch
    one = eng.dev_dec_op("embed", 1, tok=tok[5:6], pos=pos[5:6])
    same_bits(one["h"][0], res["h"][5], "one row")
    same_bits(one["xp"][0], res["xp"][5], "one row, image")
    sel = [i for i in range(n) if tok[i] != 1024 and pos[i] >= 1]
    assert len(sel) == 6
    for kernel in (0, 1):
        cases = []
        for i in sel:
            lg = np.full((1, 1025), -10.0, np.float32)
            lg[0, tok[i]] = 10.0
            cases.append(dict(kernel=kernel, splitk=1, top_k=1, temperature=1.0, u=0.5, active=1, n_gen=3, cur_pos=int(pos[i]) - 1, ctx_len=77,
                              text_len=4, gen_stride=16, force_eos_at=-1, partial=lg))
        o = eng.dev_sample(cases)
        assert (o["cur_tok"] == tok[sel]).all() and (o["cur_pos"] == pos[sel]).all()
        same_bits(o["emb_h"], res["h"][sel], f"sampler kernel {kernel}: emb_h")
        same_bits(o["emb_xp"], res["xp"][sel], f"sampler kernel {kernel}: emb_xp")


@pytest.mark.parametrize("nrows", R.FFN_SB_ROWS)
def test_small_batch_ops_repeat_the_stand_alone_kernels(eng, W, nrows):
    """decode.hip: 'the arithmetic of a row is the code of the stand-alone kernels, operation for operation'.  sb_ln_gemm (in_proj of
    layer 1, predict) is bit-identical in rows < nrows to reduce_ln 8 followed by the general GEMM on the same operands, sb_linear1
    (both layers) to reduce_ln 4 followed by linear1; rows behind the batch: zero columns of the MFMA."""
    for kind in ("normal", "slabs1e4", "mean1e3"):
        for weight, layer, rl in (("in_proj", 1, 0), ("predict", 1, 1)):
            bias, _ = R.ffn_reduce_params(W, rl, 8)
            slabs, resid = R.ln_operands(kind, 8, bias, nrows, 900 + nrows)[0]
            a = eng.dev_dec_op("sb_ln_gemm", nrows, layer=layer, weight=weight, slabs=slabs, resid=resid)
            b1 = eng.dev_dec_op("reduce_ln", nrows, layer=rl, sk=8, slabs=slabs, resid=resid)
            b2 = eng.dev_dec_op("gemm", nrows, layer=layer, weight=weight, x=b1["xp"])
            same_bits(a["h"], b1["h"], f"sb_ln_gemm {weight} / {kind}: h")
            same_bits(a["out"][:, :nrows], b2["out"][:, :nrows], f"sb_ln_gemm {weight} / {kind}: slabs")
            assert (a["out"][:, nrows:] == 0).all()
            same_bits(a["resid"], resid, "resid")
        for layer in (0, 1):
            slabs, resid = R.ln_operands(kind, 4, W[layer]["out_b"], nrows, 950 + nrows)[0]
            a = eng.dev_dec_op("sb_linear1", nrows, layer=layer, slabs=slabs, resid=resid)
            b1 = eng.dev_dec_op("reduce_ln", nrows, layer=layer, sk=4, slabs=slabs, resid=resid)
            b2 = eng.dev_dec_op("linear1", nrows, layer=layer, x=b1["xp"])
            same_bits(a["h"], b1["h"], f"sb_linear1 layer {layer} / {kind}: h")
            same_bits(a["out"][:nrows], b2["out"][:nrows], f"sb_linear1 layer {layer} / {kind}: the activation image")
            # behind the batch the x columns are zero: relu(0 + b1) in rows nrows .. 15 (linear2 never reads them into a live row);
            # the second 16-row block is not computed at all
            same_bits(a["out"][nrows:16], np.repeat(np.maximum(W[layer]["l1_b"], np.float32(0))[None], 16 - nrows, 0), "rows behind the batch")
            assert (a["out"][16:] == SENT_F).all()
            same_bits(a["resid"], resid, "resid")


def test_write_through_flag_does_not_change_a_bit(eng, W):
    """launch_skinny_gemm stores write-through from 5 rows up and plainly up to 4: the same operands give the same slabs"""
    for weight in ("in_proj", "out_proj", "linear2", "predict"):
        x = R.gemm_operands("model", R.ffn_weight(W, weight, 1), weight, 32, 77)
        a = eng.dev_dec_op("gemm", 4, layer=1, weight=weight, x=x)["out"]
        b = eng.dev_dec_op("gemm", 5, layer=1, weight=weight, x=x)["out"]
        same_bits(a, b, weight)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_entry_refusals_and_context_state(model, eng, W):
    from vallex_amd import VallexHipError
    from vallex_amd._capi import VX_EINVAL, VX_ESTATE
    a, t = synth.synth_prompt(40, 8, seed=4)
    row = dict(text=np.concatenate([t[0], synth.synth_text(12, 4)]), prompt=a[0], enroll=8, prompt_language="en", text_language="en")
    eng.ar_prefill(model.make_batch([row]))
    before = eng.ar_logits()[0].copy()
    x = np.zeros((32, 1024), np.float32)
    s8, s4, r4 = np.zeros((8, 32, 1024), np.float32), np.zeros((4, 32, 1024), np.float32), np.zeros((4, 1024), np.float32)

    def refused(code, *args, **kw):
        with pytest.raises(VallexHipError) as e:
            eng.dev_dec_op(*args, **kw)
        assert e.value.code == code, (e.value, args, kw)

    refused(VX_EINVAL, 7, 4, x=x)                                                          # an unknown op
    refused(VX_EINVAL, -1, 4, x=x)
    refused(VX_EINVAL, "gemm", 4, weight=4, x=x)                                           # an unknown weight
    refused(VX_EINVAL, "reduce_ln", 4, sk=2, slabs=np.zeros((2, 32, 1024), np.float32), resid=r4)          # a slab count not compiled in
    refused(VX_EINVAL, "linear1", 4, sk=1, x=x)                                            # a variant of an op that has none
    refused(VX_EINVAL, "gemm", 0, weight="in_proj", x=x)                                   # nrows outside 1 .. 32
    refused(VX_EINVAL, "gemm", 33, weight="in_proj", x=x)
    refused(VX_EINVAL, "sb_linear1", 5, slabs=s4, resid=np.zeros((5, 1024), np.float32))   # a small-batch op above SB_ROWS rows
    refused(VX_EINVAL, "sb_ln_gemm", 5, layer=1, weight="predict", slabs=s8, resid=np.zeros((5, 1024), np.float32))
    refused(VX_EINVAL, "gemm", 4, layer=2, weight="in_proj", x=x)                          # a layer the context does not have
    refused(VX_EINVAL, "gemm", 4, layer=-1, weight="in_proj", x=x)
    refused(VX_EINVAL, "sb_ln_gemm", 4, layer=0, weight="in_proj", slabs=s8, resid=r4)     # no linear2 in front of layer 0's in_proj
    refused(VX_EINVAL, "sb_ln_gemm", 4, layer=0, weight="predict", slabs=s8, resid=r4)     # predict follows the last layer
    refused(VX_EINVAL, "sb_ln_gemm", 4, layer=1, weight="out_proj", slabs=s8, resid=r4)
    refused(VX_EINVAL, "gemm", 4, weight="in_proj")                                        # a missing operand
    for tok, pos in ((1026, 0), (-1, 0), (0, 4000), (0, -1)):                              # outside the embedding / positional table
        refused(VX_EINVAL, "embed", 2, tok=np.array([0, tok], np.int32), pos=np.array([0, pos], np.int32))
    eng.dev_dec_op("embed", 2, tok=np.array([0, 1025], np.int32), pos=np.array([0, 3999], np.int32))           # the last rows of both tables
    # the entry works on private scratch: the decode state of the context is as the prefill left it
    eng.dev_dec_op("gemm", 32, layer=1, weight="linear2", x=np.ones((32, 4096), np.float32))
    np.testing.assert_array_equal(eng.ar_logits()[0], before)
    with eng.serve():
        refused(VX_ESTATE, "gemm", 4, weight="in_proj", x=x)
        refused(VX_ESTATE, "embed", 1, tok=np.zeros(1, np.int32), pos=np.zeros(1, np.int32))
    eng.ar_prefill(model.make_batch([row]))
    np.testing.assert_array_equal(eng.ar_logits()[0], before)
