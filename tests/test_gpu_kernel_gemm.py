"""GPU: the full-sequence GEMM kernels (csrc/gemm_f16x2.hip: split2h_kernel, absmax_kernel, the five instantiations behind
launch_gemm_f16x2 and their epilogues; csrc/gemm_f32.hip: the register-staged and the three LDS-DMA kernels; the two bf16x3 kernels)
and layernorm_kernel<1024, 4> / <384, 2> (csrc/rows.hip), one launch at a time through vx_dev_gemm / vx_dev_layernorm
(include/vallex_hip_dev.h) on caller-chosen operands.

Exact probes, bit for bit: the planes split2h_kernel, layernorm_kernel and the out_planes epilogue write against h2_split_ref; one-hot
rows 2^e e_k that read every word of a weight's planes (caller weights and the context's own load-time planes) and of the activation
planes back through each kernel's LDS staging and MFMA operand mapping; all f16x2 kernel codes against each other; sentinels behind the
last row; the range flag at the edge of the fp16 range.

Float64 comparisons: per pool (operand set and K, over all compared rows of its launches) the rms and the max error may each be at most
4 x those of the torch-CPU fp32 formulation (F.linear, F.layer_norm) against the same float64 -- the rule of the two decode files; the
pools that measured above it for the summation order alone are held to the bound K 2^-24 sum |a_k w_k| instead (CHAIN_POOLS).  The
f16x2 kernels are compared twice: against the float64 model of the split product on the reconstructed operands (yardstick: F.linear on
head + tail) and against the float64 truth on the original operands.  tests/test_kernel_refs.py ties the references to the oracle and
asserts that no yardstick pool is zero.  Measured ratios are printed ([gemm] lines); docs/log_r15.md records them."""
import numpy as np
import pytest

from oracle import synth
from tests import _kernel_refs as R
from tests._util import get_model

pytestmark = pytest.mark.gpu

SENT_F = np.float32(-1.0e30)
SENT_H = R.H2_SENT
FACTOR = 4.0
F16_CODES = ("f16x2", "f16x2_256x128", "f16x2_256x256_w8", "f16x2_256x256_w4", "f16x2_128x128", "f16x2_128x128_s2")
F32_CODES = ("f32", "f32_reg", "f32_dma256x128", "f32_dma128x128", "f32_dma256x256")
WMAX = (None, 1e-3, 0.05, 3.0)


@pytest.fixture(scope="module")
def model():
    return get_model(2, 1, 0.0, max_new=160, max_prompt=96, max_text=32, max_batch=32)


@pytest.fixture(scope="module")
def eng(model):
    return model.engine


@pytest.fixture(scope="module")
def sd():
    return synth.vallex_state_dict(2, 1, 0.0)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same_bits(a, b, what):
    assert np.shape(a) == np.shape(b), (what, np.shape(a), np.shape(b))
    d = np.argwhere(bits(a) != bits(b))
    assert not len(d), (what, "first differing word at", d[0].tolist(), "of", len(d), np.asarray(a)[tuple(d[0])], np.asarray(b)[tuple(d[0])])


def planes_of(x, shift, rows256):
    """(2, rows256, K) uint16: h2_split_ref of x in the rows it has, the sentinel behind them"""
    h, t = R.h2_split_ref(x, shift)
    out = np.full((2, rows256, x.shape[1]), SENT_H, np.uint16)
    out[0, :len(x)], out[1, :len(x)] = h.view(np.uint16), t.view(np.uint16)
    return out


# The pools held to the summation bound instead of the yardstick factor: exactly those that measured above 4 on an MI355X with the
# factor 4 everywhere (docs/log_r15.md has the figures), keyed (family, reference, set, K).  Every kernel here adds the products of an
# output element into ONE fp32 accumulator in k order, so its rounding error grows like sqrt(K) while the yardstick's blocked summation
# barely grows; the exact-fp32 MFMA kernel, a pure fma chain, is the worst.  Every exact probe of this file -- one product per element,
# every word of both operands' planes, all kernel codes bit for bit -- holds on the same launch paths, and a k-ordered fp32 chain in
# numpy shows the same ratios on the CPU (tests/test_kernel_refs.py): it is the summation order.  These pools are bound element by
# element by K 2^-24 sum_k |a_k w_k| (K additions, each off by at most 2^-24 of a partial sum); every other pool keeps the factor 4.
CHAIN_POOLS = frozenset(
    [("f16x2", ref, kind, 4096) for ref in ("model", "truth") for kind in ("normal", "model", "wide")] +
    [("f32", "truth", kind, 4096) for kind in ("normal", "model", "wide", "cancel")] + [("f32", "truth", "normal", 1024)] +
    [("bf16x3", "truth", "normal", 4096)])


def chain_pool(family, ref, kind, K):
    return (family, ref, kind, K) in CHAIN_POOLS


class Errors:
    """kernel and yardstick errors of one pool; ratios of the rms and of the max.  chain: the pool is held to `bound` per element"""

    def __init__(self, chain=False):
        self.k, self.y, self.b, self.chain = [], [], [], chain

    def add(self, got, want, yard, bound=None):
        got, want, yard = (np.asarray(a, np.float64).reshape(-1) for a in (got, want, yard))
        assert np.isfinite(got).all() and not (got == float(SENT_F)).any()
        self.k.append(got - want)
        self.y.append(yard - want)
        if self.chain:
            self.b.append(np.asarray(bound, np.float64).reshape(-1))

    def ratios(self, tag):
        k, y = np.concatenate(self.k), np.concatenate(self.y)
        k_rms, y_rms, k_max, y_max = np.sqrt(np.mean(k ** 2)), np.sqrt(np.mean(y ** 2)), np.abs(k).max(), np.abs(y).max()
        assert y_rms > 0 and y_max > 0, tag
        print(f"[gemm] {tag}: rms {k_rms:.3e} = {k_rms / y_rms:.2f} x yardstick ({y_rms:.3e}), max {k_max:.3e} = {k_max / y_max:.2f} x "
              f"yardstick ({y_max:.3e}), {len(k)} values")
        return float(k_rms / y_rms), float(k_max / y_max)


def assert_bound(tag, pools):
    bad = []
    for name in sorted(pools, key=str):
        e = pools[name]
        r_rms, r_max = e.ratios(f"{tag} / {name}")
        if e.chain:
            frac = float((np.abs(np.concatenate(e.k)) / np.concatenate(e.b)).max())
            print(f"[gemm] {tag} / {name}: held to K 2^-24 sum |a_k w_k|: the largest error is {frac:.4f} of it")
            if not frac <= 1.0:
                bad.append((name, "summation bound", round(frac, 4)))
        elif r_rms > FACTOR or r_max > FACTOR:
            bad.append((name, round(r_rms, 2), round(r_max, 2)))
    assert not bad, f"{tag}: error above {FACTOR} x the fp32 yardstick (pool, rms ratio, max ratio): {bad}"


def run(eng, kernel, a, w, m=None, **kw):
    """one launch; the checks every launch gets: the range flag is 0, nothing is written behind row M"""
    res = eng.dev_gemm(kernel, a, w, m=m, **kw)
    assert res["flag"] == 0, (kernel, "range flag")
    M = m if m is not None else len(kw["gather"]) if kw.get("gather") is not None else len(a)
    if res["c"] is not None:
        assert (res["c"][M:] == SENT_F).all() and len(res["c"]) > M, "rows behind M keep the sentinel"
        assert not (res["c"][:M] == SENT_F).any()
    for key in ("planes", "a_planes"):
        if res[key] is not None:
            assert (res[key][:, M:] == SENT_H).all(), f"{key}: pad rows of the last tile keep the sentinel"
    return res


# ---- exact probes: planes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K", [(1, 32), (255, 64), (257, 1024), (600, 64)])
def test_split2h_planes_equal_the_reference_word_for_word(eng, M, K):
    a, w = R.gemm_set("wide", M, 128, K, 11)
    perm = np.random.default_rng(1).permutation(M + 9)[:M].astype(np.int32)
    big = np.full((M + 9, K + 32), 7.0, np.float32)              # lda > K, and more rows than M: the gather picks
    big[perm, :K] = a
    for gather, src in ((None, a), (perm, big)):
        res = run(eng, "f16x2", src, w, m=M, k=K, gather=gather, a_planes=True)
        same_bits(res["a_planes"], planes_of(a, R.H2_ACT_SHIFT, res["a_planes"].shape[1]), f"A planes, gather {gather is not None}")
        assert res["shift"] == R.h2_weight_shift_ref(np.abs(w).max())


LN_PLANE_ROWS = (1, 4, 5, 255, 256, 257, 600)


@pytest.mark.parametrize("rows", LN_PLANE_ROWS)
def test_layernorm_planes_equal_the_split_of_its_own_rows(eng, rows):
    rng = np.random.default_rng(rows)
    x = R.ln_set("normal", rows, 1024, rows)
    g, b, aw, ab = (rng.normal(1.0, 0.3, 1024).astype(np.float32), rng.normal(0.0, 0.3, 1024).astype(np.float32),
                    rng.normal(1.0, 0.3, 1024).astype(np.float32), rng.normal(0.0, 0.3, 1024).astype(np.float32))
    both = eng.dev_layernorm(x, 1024, g, b, aw, ab, want_y=True, want_planes=True)
    only = eng.dev_layernorm(x, 1024, g, b, aw, ab, want_y=False, want_planes=True)
    plain = eng.dev_layernorm(x, 1024, g, b, aw, ab, want_y=True, want_planes=False)
    assert both["flag"] == only["flag"] == plain["flag"] == 0
    assert (both["y"][rows:] == SENT_F).all() and not (both["y"][:rows] == SENT_F).any()
    same_bits(both["y"], plain["y"], "y with and without planes")
    same_bits(both["planes"], planes_of(both["y"][:rows], R.H2_ACT_SHIFT, both["planes"].shape[1]), "planes = h2_split of the fp32 rows")
    same_bits(only["planes"], both["planes"], "planes without y")


@pytest.mark.parametrize("kernel", ["f16x2_256x256_w8", "f16x2_256x256_w4", "f16x2_128x128", "f16x2_128x128_s2", "f16x2_256x128"])
@pytest.mark.parametrize("M", [300, 513])
def test_out_planes_equal_the_split_of_the_rows_the_same_launch_writes(eng, kernel, M):
    a, w = R.gemm_set("model", M, 512, 64, 21)
    bias = np.random.default_rng(3).normal(0.0, 1.0, 512).astype(np.float32)
    rows = run(eng, kernel, a, w, bias=bias, act=1)
    pl = run(eng, kernel, a, w, bias=bias, act=1, out_planes=True)
    assert (rows["c"][:M] == 0).any() and (rows["c"][:M] > 0).any()
    same_bits(pl["planes"], planes_of(rows["c"][:M], R.H2_ACT_SHIFT, pl["planes"].shape[1]), "out_planes = h2_split of the fp32 rows")


# ---- exact probes: identity -----------------------------------------------------------------------------------------------------------
def one_hot_rows(K):
    a = np.zeros((K, K), np.float32)
    e = (np.arange(K) % 5 - 2).astype(np.float64)
    a[np.arange(K), np.arange(K)] = 2.0 ** e
    return a, 2.0 ** e


def exact32(v):
    """v as fp32, asserted exact.  The accumulators start at +0 and (+0) + (-0) = +0, so a product that is a zero of either sign leaves +0"""
    assert (v.astype(np.float32).astype(np.float64) == v).all()
    return (v + 0.0).astype(np.float32)


def weight_probe_expected(w, shift, scale):
    """C[m][n] = (head + tail)(W[n][m]) 2^-shift 2^e(m): a single product per element, exact in fp32"""
    return exact32(R.h2_value(w, shift).T * scale[:, None])


@pytest.mark.parametrize("kernel", F16_CODES)
@pytest.mark.parametrize("K,N,wmax", [(64, 128, 1e-3), (64, 384, 3.0), (1024, 256, 0.05), (1024, 512, None), (1024, 384, 1e-3)])
def test_one_hot_rows_read_every_word_of_a_weights_planes(eng, kernel, K, N, wmax):
    _, w = R.gemm_set("wide" if wmax is None else "normal", 1, N, K, 5, wmax)
    a, scale = one_hot_rows(K)
    res = run(eng, kernel, a, w)
    assert res["shift"] == R.h2_weight_shift_ref(np.abs(w).max())
    same_bits(res["c"][:K], weight_probe_expected(w, res["shift"], scale), f"{kernel}: W planes through the kernel")


CTX_WEIGHTS = {"in_proj": "self_attn.in_proj_weight", "out_proj": "self_attn.out_proj.weight", "linear1": "linear1.weight", "linear2": "linear2.weight"}


@pytest.mark.parametrize("stack,layer", [("ar", 1), ("nar", 0)])
@pytest.mark.parametrize("name", list(CTX_WEIGHTS))
def test_one_hot_rows_read_the_contexts_own_weight_planes(eng, sd, stack, layer, name):
    """what the loader wrote (absmax -> shift -> split2h at load) is what the product's own choice of kernel reads"""
    w = sd[f"{stack}_decoder.layers.{layer}.{CTX_WEIGHTS[name]}"]
    N, K = w.shape
    a, scale = one_hot_rows(K)
    shift = R.h2_weight_shift_ref(np.abs(w).max())
    for kernel in ("f16x2", "f16x2_128x128") if name == "out_proj" else ("f16x2",):
        res = run(eng, kernel, a, None, w_src=f"{stack}.{name}", w_layer=layer, n=N)
        assert res["shift"] == shift, "the shift the loader recorded"
        same_bits(res["c"][:K], weight_probe_expected(w, shift, scale), f"{stack}.{layer}.{name}")


@pytest.mark.parametrize("kernel", F16_CODES)
@pytest.mark.parametrize("M,K", [(1, 64), (255, 256), (257, 256), (300, 1024), (513, 256)])
def test_scaled_identity_weights_read_every_word_of_the_activation_planes(eng, kernel, M, K):
    a, _ = R.gemm_set("wide", M, 4, K, 13)
    w, scale = one_hot_rows(K)
    res = run(eng, kernel, a, w)
    assert res["shift"] == 12                                   # max |w| = 4: heads exact, tails 0
    same_bits(res["c"][:M], exact32(R.h2_value(a, R.H2_ACT_SHIFT) * scale[None, :]), f"{kernel}: A planes through the kernel")


@pytest.mark.parametrize("kernel", F32_CODES + ("bf16x3", "bf16x3_dma"))
def test_identity_probes_of_the_fp32_and_bf16x3_kernels(eng, kernel):
    """every product of these kernels is exact too (bf16x3: three planes hold all 24 bits): C = W^T 2^e, C = A 2^e"""
    for K, N in ((64, 128), (1024, 384)):
        _, w = R.gemm_set("wide", 1, N, K, 6)
        a, scale = one_hot_rows(K)
        res = run(eng, kernel, a, w)
        same_bits(res["c"][:K], exact32(w.astype(np.float64).T * scale[:, None]), f"{kernel}: W")
    for M, K in ((1, 64), (257, 256), (1100, 64)):
        a, _ = R.gemm_set("wide", M, 4, K, 14)
        w, scale = one_hot_rows(K)
        res = run(eng, kernel, a, w)
        same_bits(res["c"][:M], exact32(a.astype(np.float64) * scale[None, :]), f"{kernel}: A")


# ---- float64: f16x2 ---------------------------------------------------------------------------------------------------------------------
#          M     N     K    what the shape is there for
F16_SHAPES = ((1, 128, 32),        # one row, one K tile: the four-wave kernel steps aside
              (77, 128, 64),
              (255, 256, 1024),
              (256, 384, 64),      # N no multiple of 256: the last W tile is half pad
              (257, 1024, 1024),
              (300, 1024, 4096),
              (513, 3072, 1024),   # three row tiles of 256, five of 128: middle tiles
              (1100, 4096, 64))    # the cost model's 128 x 128 tiles on two LDS stages (more than 256 tiles)


def f16_case(eng, kind, M, N, K, wmax, seed, pools, codes=F16_CODES, **epi):
    """one operand set through every kernel code: code 0 of `codes` against float64, the others against it bit for bit"""
    a, w = R.gemm_set(kind, M, N, K, seed, wmax)
    first = None
    for kernel in codes:
        res = run(eng, kernel, a, w, **epi.get("launch", {}))
        c = res["c"][:M]
        if first is None:
            first, shift = c, res["shift"]
            assert shift == R.h2_weight_shift_ref(np.abs(w).max())
        else:
            same_bits(c, first, f"{kernel} against {codes[0]} ({M} x {N} x {K}, {kind})")
    ref = epi.get("ref", {})
    am, wm = R.h2_value(a, R.H2_ACT_SHIFT).astype(np.float32), R.h2_value(w, shift).astype(np.float32)
    model = R.gemm_ref(a, w, pre=R.h2_gemm_model(a, w, shift), **ref)
    truth = R.gemm_ref(a, w, **ref)
    bound = R.chain_bound(a, w)
    pools.setdefault(("model", kind, K), Errors(chain_pool("f16x2", "model", kind, K))).add(first, model, R.gemm_fp32(am, wm, **ref), bound)
    pools.setdefault(("truth", kind, K), Errors(chain_pool("f16x2", "truth", kind, K))).add(first, truth, R.gemm_fp32(a, w, **ref), bound)
    if kind == "cancel" and not ref:                        # the columns that cancel, on their own
        cols = R.gemm_cancel_rows(N, K)
        pools.setdefault(("model", "cancelling columns", K), Errors()).add(first[:, cols], model[:, cols], R.gemm_fp32(am, wm)[:, cols])
        pools.setdefault(("truth", "cancelling columns", K), Errors()).add(first[:, cols], truth[:, cols], R.gemm_fp32(a, w)[:, cols])
    return first, truth


@pytest.mark.parametrize("kind", R.GEMM_SETS)
def test_f16x2_gemm_against_float64(eng, kind):
    pools = {}
    for i, (M, N, K) in enumerate(F16_SHAPES):
        f16_case(eng, kind, M, N, K, None if kind == "wide" else WMAX[i % 4], 100 + i, pools)
    assert_bound(f"f16x2 {kind}", pools)


@pytest.mark.parametrize("M,N,K,pick", [(3841, 4096, 64, "w4_256x256"), (3841, 4096, 32, "w8_256x256")])
def test_f16x2_cost_model_shapes_with_middle_tiles(eng, M, N, K, pick):
    """the two shapes at which the product's own choice is a 256 x 256 tile: sixteen row tiles, every row compared"""
    assert R.f16x2_choice(M, N, K) == pick
    pools = {}
    f16_case(eng, "normal", M, N, K, 0.05, 7, pools, codes=("f16x2", "f16x2_128x128"))
    assert_bound(f"f16x2 {pick}", pools)


def epilogues(M, N, seed):
    """name -> (launch arguments, reference arguments) of the epilogue cases at a ragged M"""
    rng = np.random.default_rng(seed)
    bias = rng.normal(0.0, 1.0, N).astype(np.float32)
    resid = rng.normal(0.0, 3.0, (M, N)).astype(np.float32)
    wide = np.full((M, N + 64), 5.0, np.float32)
    wide[:, :N] = resid
    long = rng.normal(0.0, 3.0, (M + 77, N)).astype(np.float32)
    rmap = ((np.arange(M) * 7919 + 13) % (M + 77)).astype(np.int32)
    return {"bias": (dict(bias=bias), dict(bias=bias)),
            "relu": (dict(bias=bias, act=1), dict(bias=bias, act=1)),
            "resid": (dict(bias=bias, resid=wide), dict(bias=bias, resid=resid)),
            "inplace": (dict(bias=bias, resid=resid, inplace=True), dict(bias=bias, resid=resid)),
            "resid_rows": (dict(bias=bias, resid=long, resid_rows=rmap), dict(bias=bias, resid=long[rmap]))}


@pytest.mark.parametrize("epi", ["bias", "relu", "resid", "inplace", "resid_rows", "gather"])
def test_f16x2_epilogues_against_the_float64_contract(eng, epi):
    M, N, K = 300, 512, 1024
    pools = {}
    if epi == "gather":
        a, w = R.gemm_set("normal", M + 50, N, K, 31, 0.05)
        g = np.random.default_rng(2).permutation(M + 50)[:M].astype(np.int32)
        first = None
        for kernel in F16_CODES:
            c = run(eng, kernel, a, w, gather=g)["c"][:M]
            first = c if first is None else first
            same_bits(c, first, kernel)
        pools["truth"] = Errors()
        pools["truth"].add(first, R.gemm_ref(a[g], w), R.gemm_fp32(a[g], w))
    else:
        launch, ref = epilogues(M, N, 17)[epi]
        got, truth = f16_case(eng, "normal", M, N, K, 0.05, 31, pools, launch=launch, ref=ref)
        if epi == "relu":
            k = pools[("truth", "normal", K)]
            bound = FACTOR * np.abs(k.y[0]).max()
            pre = R.gemm_ref(*R.gemm_set("normal", M, N, K, 31, 0.05), bias=ref["bias"])
            neg = pre < -bound
            assert neg.any() and (bits(got)[neg] == 0).all(), "ReLU'd zeros are exactly +0"
    assert_bound(f"f16x2 epilogue {epi}", pools)


# ---- float64: the fp32 and bf16x3 kernels -------------------------------------------------------------------------------------------------
F32_SHAPES = ((1, 128, 32), (77, 1100, 64), (255, 256, 1024), (257, 384, 1024), (300, 1024, 4096), (513, 1100, 1024), (2100, 256, 64))


@pytest.mark.parametrize("kind", R.GEMM_SETS)
def test_fp32_gemm_kernels_against_float64(eng, kind):
    """the four fp32 kernels agree bit for bit (the same MFMA sequence per element); the product's choice against float64"""
    pools = {}
    for i, (M, N, K) in enumerate(F32_SHAPES):
        a, w = R.gemm_set(kind, M, N, K, 200 + i, None if kind == "wide" else WMAX[i % 4])
        first = None
        for kernel in F32_CODES:
            c = run(eng, kernel, a, w)["c"][:M]
            first = c if first is None else first
            same_bits(c, first, f"{kernel} ({M} x {N} x {K})")
        chain = chain_pool("f32", "truth", kind, K)
        pools.setdefault((kind, K), Errors(chain)).add(first, R.gemm_ref(a, w), R.gemm_fp32(a, w), R.chain_bound(a, w) if chain else None)
    assert_bound(f"f32 {kind}", pools)


@pytest.mark.parametrize("epi", ["bias", "relu", "resid", "inplace", "resid_rows", "gather_lda", "colscale_gelu", "colscale_elu"])
def test_fp32_gemm_epilogues_against_the_float64_contract(eng, epi):
    M, N, K = 300, 1100, 64
    rng = np.random.default_rng(23)
    a, w = R.gemm_set("normal", M + 50, N, K, 41, 3.0)
    if epi == "gather_lda":
        big = np.full((M + 50, K + 32), 9.0, np.float32)
        big[:, :K] = a
        g = rng.permutation(M + 50)[:M].astype(np.int32)
        launch, ref, rows, src = dict(gather=g, k=K), {}, a[g], big
    elif epi.startswith("colscale"):
        act = 2 if epi.endswith("gelu") else 3
        e = dict(bias=rng.normal(0, 1, N).astype(np.float32), colscale=rng.normal(0, 2, N).astype(np.float32), act=act,
                 resid=rng.normal(0, 3, (M, N)).astype(np.float32))
        launch, ref, rows, src = e, e, a[:M], a[:M]
    else:
        (launch, ref), rows, src = epilogues(M, N, 19)[epi], a[:M], a[:M]
    first = None
    for kernel in F32_CODES:
        c = run(eng, kernel, src, w, m=M, **launch)["c"][:M]
        first = c if first is None else first
        same_bits(c, first, kernel)
    pools = {"truth": Errors()}
    pools["truth"].add(first, R.gemm_ref(rows, w, **ref), R.gemm_fp32(rows, w, **ref))
    if epi == "relu":
        neg = R.gemm_ref(rows, w, bias=ref["bias"]) < -FACTOR * np.abs(pools["truth"].y[0]).max()
        assert neg.any() and (bits(first)[neg] == 0).all(), "ReLU'd zeros are exactly +0"
    assert_bound(f"f32 epilogue {epi}", pools)


@pytest.mark.parametrize("kernel", ["bf16x3", "bf16x3_dma"])
def test_bf16x3_gemm_kernels_against_float64(eng, kernel):
    pools = {}
    for i, (M, N, K) in enumerate(((1, 128, 32), (255, 384, 1024), (300, 1024, 4096), (1100, 256, 1024))):
        for kind in ("normal", "wide"):
            a, w = R.gemm_set(kind, M, N, K, 300 + i, None if kind == "wide" else WMAX[i % 4])
            c = run(eng, kernel, a, w)["c"][:M]
            chain = chain_pool("bf16x3", "truth", kind, K)
            pools.setdefault((kind, K), Errors(chain)).add(c, R.gemm_ref(a, w), R.gemm_fp32(a, w), R.chain_bound(a, w) if chain else None)
    assert_bound(kernel, pools)


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------------------
LN_ROWS = (1, 3, 4, 5, 257)
LN_MODES = ("plain", "affine", "ada", "affine_ada")


def ln_params(mode, C, seed):
    rng = np.random.default_rng(seed)
    g, b, aw, ab = (rng.normal(1.0, 0.3, C).astype(np.float32), rng.normal(0.0, 0.3, C).astype(np.float32),
                    rng.normal(1.0, 0.3, C).astype(np.float32), rng.normal(0.0, 0.3, C).astype(np.float32))
    return {"plain": (None, None, None, None), "affine": (g, b, None, None), "ada": (None, None, aw, ab), "affine_ada": (g, b, aw, ab)}[mode]


@pytest.mark.parametrize("C", [1024, 384])
@pytest.mark.parametrize("kind", R.LN_SETS)
def test_layernorm_against_float64(eng, C, kind):
    pools = {}
    for mode in LN_MODES:
        p = ln_params(mode, C, 5)
        for rows in LN_ROWS:
            x = R.ln_set(kind, rows, C, 50 + rows)
            res = eng.dev_layernorm(x, C, *p)
            assert res["flag"] == 0 and (res["y"][rows:] == SENT_F).all()
            y = res["y"][:rows]
            if rows == 5:                                   # the engine normalises out of the QKV buffer: ldx 3072
                big = np.full((rows, 3072), 1.0e6, np.float32)
                big[:, :C] = x
                same_bits(eng.dev_layernorm(big, C, *p)["y"][:rows], y, "ldx 3072")
            lo = 0
            if kind == "const":                             # row 0 is exactly constant: (x - mean) = 0, the result is the bias path
                g, b, aw, ab = p
                base = np.zeros(C, np.float32) if b is None else b
                if aw is None:
                    same_bits(y[0], base, f"{mode}: a constant row")
                else:
                    one = (aw.astype(np.float64) * base + ab).astype(np.float32)                       # contracted into one fma
                    two = ((aw * base).astype(np.float32) + ab).astype(np.float32)                     # or two roundings
                    assert ((y[0] == one) | (y[0] == two)).all(), f"{mode}: a constant row"
                lo = 1                                       # (the yardstick is exact on that row: it stays out of the ratio)
            if rows > lo:
                pools.setdefault(mode, Errors()).add(y[lo:], R.ln_ref(x[lo:], *p), R.ln_fp32(x[lo:], *p))
    assert_bound(f"layernorm<{C}> {kind}", pools)


# ---- the range flag -----------------------------------------------------------------------------------------------------------------------
BELOW = np.nextafter(np.float32(2047.0), np.float32(0.0))          # 32 x this is the largest X below 65504
EDGE = ((BELOW, 0), (-BELOW, 0), (np.float32(2047.0), 1), (np.float32(-2047.0), 1), (np.float32(np.inf), 1), (np.float32(-np.inf), 1),
        (np.float32(np.nan), 1))


def test_range_flag_of_split2h(eng):
    _, w = R.gemm_set("normal", 1, 128, 64, 1)
    for v, want in EDGE:
        a = np.zeros((3, 64), np.float32)
        a[2, 37] = v
        assert R.h2_range_bad(a, R.H2_ACT_SHIFT) == bool(want)
        assert eng.dev_gemm("f16x2", a, w)["flag"] == want, v
    # a weight whose given shift pushes it out of range raises it as well (the loader passes the same flag)
    assert eng.dev_gemm("f16x2", np.zeros((3, 64), np.float32), w, w_shift=24)["flag"] == int(R.h2_range_bad(w, 24)) == 1


def test_range_flag_of_the_layernorm_planes(eng):
    x = R.ln_set("normal", 5, 1024, 3)
    for v, want in EDGE:
        ab = np.zeros(1024, np.float32)
        ab[7] = v
        res = eng.dev_layernorm(x, 1024, None, None, np.zeros(1024, np.float32), ab, want_planes=True)       # y = 0 . LN(x) + ab
        if np.isfinite(v):
            assert (res["y"][:5, 7] == v).all()
        assert res["flag"] == want, v
        assert eng.dev_layernorm(x, 1024, None, None, np.zeros(1024, np.float32), ab)["flag"] == 0, "no planes, no range to leave"


@pytest.mark.parametrize("kernel", ["f16x2_256x256_w8", "f16x2_256x256_w4", "f16x2_128x128"])
def test_range_flag_of_the_out_planes_epilogue(eng, kernel):
    """a linear1 result at or above 2047 behind the ReLU raises the flag.  As the code behaves: the ReLU runs in front of the split, so a
    negative value of any magnitude -- and a NaN, which fmaxf(NaN, 0) turns into 0 -- leaves as a zero and does NOT raise it"""
    a = np.zeros((3, 64), np.float32)
    _, w = R.gemm_set("normal", 1, 256, 64, 1)
    for v, want in EDGE + ((np.float32(-3.0e4), 0), (np.float32(3.0e4), 1)):
        bias = np.zeros(256, np.float32)
        bias[200] = v
        res = eng.dev_gemm(kernel, a, w, bias=bias, act=1, out_planes=True)
        want = want if v > 0 else 0                         # negative, -inf and NaN: swallowed by the ReLU
        assert res["flag"] == want, (kernel, v)
        if want == 0:                                       # what left: the split of v behind the ReLU, i.e. of 0 unless v > 0
            out = np.float32(v) if v > 0 else np.float32(0.0)
            same_bits(res["planes"][:, :3, 200], planes_of(np.full((3, 1), out, np.float32), R.H2_ACT_SHIFT, 3)[:, :, 0], "the planes at the edge")


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_entry_refusals(eng):
    from vallex_amd import VallexHipError
    from vallex_amd._capi import VX_EINVAL, VX_ESTATE
    a, w = R.gemm_set("normal", 8, 128, 64, 1)

    def refused(code, fn, *args, **kw):
        with pytest.raises(VallexHipError) as e:
            fn(*args, **kw)
        assert e.value.code == code, (e.value, args, kw)

    G, L = eng.dev_gemm, eng.dev_layernorm
    refused(VX_EINVAL, G, 5, a, w)                                                  # an unknown kernel code
    refused(VX_EINVAL, G, "f16x2", np.zeros((8, 48), np.float32), np.zeros((128, 48), np.float32))      # K % 32
    refused(VX_EINVAL, G, "f32", a, np.zeros((130, 64), np.float32))                # N % 4
    refused(VX_EINVAL, G, "f32", np.zeros((4097, 32), np.float32), np.zeros((128, 32), np.float32))     # M above the cap
    refused(VX_EINVAL, G, "f32", np.zeros((8, 4128), np.float32), np.zeros((128, 4128), np.float32))    # K above the cap
    refused(VX_EINVAL, G, "f32", a, w, m=9)                                         # more rows than A has
    refused(VX_EINVAL, G, "f32", a, w, gather=np.array([0, 8], np.int32))           # a gather outside A
    refused(VX_EINVAL, G, "f32", a, w, resid=np.zeros((7, 128), np.float32))        # a residual shorter than M
    refused(VX_EINVAL, G, "f32", a, w, resid=np.zeros((8, 128), np.float32), resid_rows=np.array([0] * 7 + [8], np.int32))
    refused(VX_EINVAL, G, "f32", a, w, resid_rows=np.zeros(8, np.int32))            # a row map without a residual
    refused(VX_EINVAL, G, "f32", a, w, resid=np.zeros((8, 132), np.float32), inplace=True)
    refused(VX_EINVAL, G, "f16x2", a, w, colscale=np.ones(128, np.float32))         # colscale / GELU: the fp32 kernels'
    refused(VX_EINVAL, G, "f16x2", a, w, act=2)
    refused(VX_EINVAL, G, "f32", a, w, act=4)
    refused(VX_EINVAL, G, "bf16x3", a, w, bias=np.ones(128, np.float32))            # bf16x3: plain epilogue only
    refused(VX_EINVAL, G, "f32", a, w, out_planes=True)
    refused(VX_EINVAL, G, "f16x2", a, w, out_planes=True)                           # N % 256
    refused(VX_EINVAL, G, "f32", a, w, a_planes=True)
    refused(VX_EINVAL, G, "f16x2", a, w, w_shift=25)
    refused(VX_EINVAL, G, "f16x2", a, w, extra_rows=65)
    refused(VX_EINVAL, G, "f16x2", a, None, w_src="ar.in_proj", w_layer=0, n=3072)  # K is not the weight's
    refused(VX_EINVAL, G, "f16x2", np.zeros((8, 1024), np.float32), None, w_src="ar.in_proj", w_layer=2, n=3072)
    refused(VX_EINVAL, G, "f32", np.zeros((8, 1024), np.float32), None, w_src="ar.in_proj", w_layer=0, n=3072)
    x = np.zeros((4, 1024), np.float32)
    refused(VX_EINVAL, L, x, 512)
    refused(VX_EINVAL, L, np.zeros((4, 386), np.float32), 384)                      # ldx % 4
    refused(VX_EINVAL, L, x, 1024, np.ones(1024, np.float32), None)                 # g without b
    refused(VX_EINVAL, L, x, 1024, want_y=False)                                    # nothing to write
    refused(VX_EINVAL, L, np.zeros((4, 384), np.float32), 384, want_planes=True)
    refused(VX_EINVAL, L, np.zeros((4097, 384), np.float32), 384)
    with eng.serve():
        refused(VX_ESTATE, G, "f32", a, w)
        refused(VX_ESTATE, L, x, 1024)
    assert eng.dev_gemm("f32", a, w)["flag"] == 0
