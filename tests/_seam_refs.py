"""Plain numpy restatements of the kernels of the seams between the phases -- embed_rows, nar_yemb_init, add_pe_scatter, embed_accum,
argmax_rows, kv_scatter, gemv (csrc/rows.hip), beam_fanout (csrc/beams.hip), admit_rows, admit_mask, admit_uniforms (csrc/admit.hip),
serve_uniforms, serve_cancel (csrc/serve.hip), dec_force_token (csrc/decode.hip) -- the shared inputs of their GPU tests
(tests/test_gpu_kernel_seam.py) and THE assertion helper.  tests/test_seam_refs.py pins the restatements to what the project already
trusts and shows on the CPU that the helper rejects wrong kernels on these very inputs.

Every reference returns what a correct kernel LEAVES IN THE BUFFERS of vx_dev_seam_op: the sentinel wherever nothing may be written,
`extra` rows or words behind every output included.  The embedding kernels are single fp32 operations in the reference's order, the
draws Python integers, the state kernels dictionaries of arrays: all of that is bit-identical.  gemv alone has a bound (gemv_ref).

`mutant=` selects a WRONG kernel (what a plausible defect would leave in the same buffers); the CPU tests feed those to `check`.
"""
import numpy as np

import vallex_amd  # noqa: F401  (registers the package under an importable name)
from tests._wave_refs import SENT_F, bits, gamma
from tests._wave_refs import check as check_bound
from vallex_amd._capi import DEV_SEAM_STATE, DEV_SENTINEL_I

f32, f64, i32 = np.float32, np.float64, np.int32
SENT_I = DEV_SENTINEL_I
EXTRA = 3
D = 1024
ALPHA = 0.8731                      # not a power of two: alpha * pe rounds, so a fused multiply-add shows (tests/test_seam_refs.py)
STATE_KEYS = ("cur_tok", "cur_pos", "ctx_len", "n_gen", "text_len", "active", "saved", "slot_of", "slot_meta", "n_active", "row_smp",
              "row_flt", "gen")
STATE_WORDS = dict(cur_tok=32, cur_pos=32, ctx_len=32, n_gen=32, text_len=32, active=32, saved=32, slot_of=32, slot_meta=128, n_active=4,
                   row_smp=128, row_flt=128)


def check(got, want, name):
    """THE assertion of the seam tests: `got` holds exactly the words of `want` -- float32 compared bit by bit (a -0.0 is not a +0.0, a
    sentinel is a sentinel), integers by value -- in every element, the sentinel tails and the words nobody may write included.  Tuples
    and dictionaries are compared member by member."""
    if isinstance(want, dict):
        assert set(got) == set(want), (name, sorted(got), sorted(want))
        for k in want:
            check(got[k], want[k], f"{name} {k}")
        return
    if isinstance(want, (tuple, list)):
        assert len(got) == len(want), (name, len(got), len(want))
        for i, (g, w) in enumerate(zip(got, want)):
            check(g, w, f"{name} [{i}]")
        return
    if want is None:                                                       # an output the launch does not have
        assert got is None, name
        return
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, want.dtype, got.shape, want.shape)
    assert got.dtype in (f32, i32), (name, got.dtype)
    bad = bits(got) != bits(want) if got.dtype == f32 else got != want
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{name}: element {i} is {got[i]!r}, must be exactly {want[i]!r} ({int(bad.sum())} such elements)")


def rejects(got, want, name="mutant"):
    try:
        check(got, want, name)
    except AssertionError:
        return True
    return False


def _ints(shape, base=0):
    """base + the flat index: every element names its own place (exact in fp32: below 2^24)"""
    n = int(np.prod(shape))
    assert base + n <= 2 ** 24
    return (base + np.arange(n)).reshape(shape).astype(f32)


def _sent(shape):
    return np.full(shape, SENT_F, f32)


# ---------------------------------------------------------------------------------------------------------------------------------
# the embedding kernels: single fp32 operations in the reference's order
# ---------------------------------------------------------------------------------------------------------------------------------
def fma32(a, p, v):
    """float32(a * p + v) with ONE rounding: the product of two float32 is exact in float64 (48 bits), the sum is formed in float64"""
    return (np.asarray(a, f64) * np.asarray(p, f64) + np.asarray(v, f64)).astype(f32)


def mul_add(a, p, v, mutant=None):
    """v + (a * p): the product rounded to fp32, then the sum (modules/embedding.py:93-97 in torch)"""
    a = f32(a)
    if mutant == "fma":
        return fma32(a, p, v)
    return (v + (a * p).astype(f32)).astype(f32)


def embed_rows_ref(tabA, idA, tabB, idB, alpha, pe, pos, dst, out_rows, extra=0, mutant=None):
    out = _sent((out_rows + extra, D))
    a = f32(alpha)
    for r in range(len(idA)):
        v = tabA[idA[r]].copy()
        ap = (a * pe[pos[r]]).astype(f32)
        lang = None
        if tabB is not None and (idB[r] >= 0 or mutant == "idb_row0"):
            lang = tabB[max(int(idB[r]), 0)]
        if mutant == "reassoc" and lang is not None:
            v = (v + (lang + ap).astype(f32)).astype(f32)
        else:
            if lang is not None:
                v = (v + lang).astype(f32)
            v = mul_add(a, pe[pos[r]], v, mutant)
        out[r if dst is None else dst[r]] = v
    return out


def embed_rows_cases():
    rng = np.random.default_rng(2101)
    rows = 9
    tabA, tabB, pe = (rng.standard_normal((n, D)).astype(f32) for n in (6, 3, 12))
    idA = np.array([4, 0, 5, 4, 4, 2, 0, 5, 1], i32)                       # ids that repeat
    idB = np.array([2, -1, 0, 1, -1, 2, 2, -1, 0], i32)
    pos = np.array([0, 11, 5, 5, 1, 10, 0, 11, 7], i32)                    # 0 and pe_rows - 1
    dst = np.array([7, 0, 11, 3, 9, 1, 10, 4, 6], i32)                     # rows 2, 5, 8 of out stay unwritten
    base = dict(tabA=tabA, idA=idA, alpha=ALPHA, pe=pe, pos=pos, extra=EXTRA)
    return [dict(name="lang+dst", kw=dict(base, tabB=tabB, idB=idB, dst=dst, out_rows=12)),
            dict(name="dst", kw=dict(base, tabB=None, idB=None, dst=dst, out_rows=12)),
            dict(name="lang", kw=dict(base, tabB=tabB, idB=idB, dst=None, out_rows=11)),
            dict(name="plain", kw=dict(base, tabB=None, idB=None, dst=None, out_rows=9))]


def nar_yemb_init_ref(tabs, codes, nj, extra=0, mutant=None):
    out = _sent((len(codes) + extra, D))
    for r in range(len(codes)):
        v = tabs[0][codes[r][0]].copy()
        for j in range(1, min(int(nj[r]) + (mutant == "one_more"), 8)):
            v = (v + tabs[j][codes[r][j]]).astype(f32)
        out[r] = v
    return out


def nar_yemb_init_cases():
    rng = np.random.default_rng(2102)
    tabs = rng.standard_normal((8, 3, D)).astype(f32)
    tabs[:, 2] = 1e30                                                      # the row a column >= nj points at: one add too many is seen
    nj = np.array([1, 2, 7, 8, 3, 8], i32)
    codes = rng.integers(0, 2, (len(nj), 8)).astype(i32)
    for r, n in enumerate(nj):
        codes[r, n:] = 2
    return [dict(name="nj 1 2 7 8", kw=dict(tabs=tabs, codes=codes, nj=nj, extra=EXTRA))]


def add_pe_scatter_ref(yemb, alpha, pe, pos, dst, out_rows, extra=0, mutant=None):
    out = _sent((out_rows + extra, D))
    for r in range(len(yemb)):
        out[dst[r]] = mul_add(alpha, pe[pos[r]], yemb[r], mutant)
    return out


def add_pe_scatter_cases():
    rng = np.random.default_rng(2103)
    yemb, pe = rng.standard_normal((9, D)).astype(f32), rng.standard_normal((12, D)).astype(f32)
    pos = np.array([0, 11, 5, 5, 1, 10, 0, 11, 7], i32)
    dst = np.array([7, 0, 11, 3, 9, 1, 10, 4, 6], i32)
    return [dict(name="scatter", kw=dict(yemb=yemb, alpha=ALPHA, pe=pe, pos=pos, dst=dst, out_rows=12, extra=EXTRA))]


def embed_accum_ref(yemb, tab, tok, rowidx, extra=0, mutant=None):
    out = np.concatenate([yemb, _sent((extra, D))])
    for i in range(len(tok)):
        out[rowidx[i]] = (out[rowidx[i]] + tab[tok[i]]).astype(f32)
    return out


def embed_accum_cases():
    rng = np.random.default_rng(2104)
    yemb, tab = rng.standard_normal((10, D)).astype(f32), rng.standard_normal((5, D)).astype(f32)
    return [dict(name="subset", kw=dict(yemb=yemb, tab=tab, tok=np.array([3, 0, 3, 4, 1], i32), rowidx=np.array([8, 2, 5, 9, 3], i32),
                                        extra=EXTRA))]


# ---------------------------------------------------------------------------------------------------------------------------------
# argmax_rows
# ---------------------------------------------------------------------------------------------------------------------------------
def argmax_row(x, mutant=None):
    """The kernel's rule: candidates are the values above -inf under `>` (NaN is never one); the lowest index of the largest wins, -0.0
    and +0.0 being equal; no candidate: 0."""
    x = np.asarray(x, f32)
    with np.errstate(invalid="ignore"):
        cand = np.flatnonzero(x > -np.inf)
    if len(cand) == 0:
        return 0
    if mutant == "negzero":                                                # -0.0 < +0.0: order by (value, sign bit cleared first)
        key = x[cand].astype(f64) - np.where(np.signbit(x[cand]) & (x[cand] == 0), 1e-300, 0.0)
        return int(cand[np.flatnonzero(key == key.max())[0]])
    top = cand[x[cand] == x[cand].max()]
    if mutant == "last":
        return int(top[-1])
    if mutant == "lane_first":                                             # lanes merged by lane number, not by index
        return int(min(top, key=lambda c: (c % 64, c)))
    return int(top[0])


def argmax_rows_ref(x, N, extra=0, mutant=None):
    return np.array([argmax_row(r[:N], mutant) for r in x] + [SENT_I] * extra, i32)


ARGMAX_ROWS = ("max@0", "max@63", "max@64", "max@1023", "max@N-1", "tie 5 69", "tie 69 70", "tie 64 3", "-0 then +0", "+0 then -0",
               "all -inf", "+inf twice", "all NaN", "NaN and finite", "NaN at 0, tie 64 3")


def argmax_cases():
    """one launch per (N, rows): rows 1, 4, 5 (the 4-rows-per-block tail) draw from the 15 special rows of argmax_special"""
    out = []
    for N in (1024, 1025):
        special = argmax_special(N)
        for rows, first in ((1, 0), (4, 1), (5, 5), (5, 10)):
            out.append(dict(name=f"N {N} rows {rows} from {first}", kw=dict(x=special[first:first + rows].copy(), N=N, extra=EXTRA)))
    return out


def argmax_special(N, pad=7):
    rng = np.random.default_rng(2105 + N)
    x = rng.standard_normal((len(ARGMAX_ROWS), N + pad)).astype(f32)
    x[:, N:] = 1e30                                                        # pad columns N .. ldx - 1: must influence nothing
    for r, c in enumerate((0, 63, 64, 1023, N - 1)):
        x[r, c] = 9.0
    x[5, [5, 69]] = 9.0                                                    # the same lane
    x[6, [69, 70]] = 9.0                                                   # neighbouring lanes
    x[7, [64, 3]] = 9.0                                                    # the higher index in the lower lane
    x[8, :N] = -1.0 - np.abs(x[8, :N])
    x[8, 70], x[8, 200] = -0.0, 0.0
    x[9, :N] = -1.0 - np.abs(x[9, :N])
    x[9, 70], x[9, 200] = 0.0, -0.0
    x[10, :N] = -np.inf
    x[11, [130, 66]] = np.inf
    x[12, :N] = np.nan
    x[13, 0:N:3] = np.nan
    x[13, 100] = 9.0
    x[14, 0] = np.nan
    x[14, [64, 3]] = 9.0
    return x


# ---------------------------------------------------------------------------------------------------------------------------------
# kv_scatter, beam_fanout: data movement
# ---------------------------------------------------------------------------------------------------------------------------------
def kv_scatter_ref(qkv, row_b, row_t, Tmax, slots, extra=0, mutant=None):
    kc, vc = _sent(slots * 16 * Tmax * 64 + extra * 64), _sent(slots * 16 * Tmax * 64 + extra * 64)
    k3 = 0 if mutant == "q_for_k" else 1
    for r in range(len(qkv)):
        for h in range(16):
            at = (((row_b[r] * Tmax + row_t[r]) * 16 + h) if mutant == "swap_ht" else ((row_b[r] * 16 + h) * Tmax + row_t[r])) * 64
            kc[at:at + 64] = qkv[r, k3 * D + 64 * h:k3 * D + 64 * h + 64]
            vc[at:at + 64] = qkv[r, 2 * D + 64 * h:2 * D + 64 * h + 64]
    return kc, vc


def kv_scatter_cases():
    qkv = _ints((7, 3 * D))
    qkv[:, :D] = np.nan                                                    # the q third must appear nowhere
    return [dict(name="M 7", kw=dict(qkv=qkv, row_b=np.array([1, 1, 0, 2, 1, 2, 0], i32), row_t=np.array([39, 3, 0, 39, 0, 17, 39], i32),
                                     Tmax=40, slots=3, extra=EXTRA))]


def beam_fanout_ref(kc, vc, pairs, hsrc, hsrc_row, layers, Tmax, slots, extra=0, mutant=None):
    """kc, vc [layers][slots][16][Tmax][64] or None (no pairs); returns (kc, vc, dh) as the buffers come back"""
    outs = []
    for cache in (kc, vc):
        if cache is None:
            outs.append(None)
            continue
        src = cache.reshape(layers, slots, 16, Tmax * 64)
        o = src.copy()
        for s, d, n in pairs:
            n = max(0, min(Tmax, n + (mutant == "len+1") - (mutant == "len-1")))
            o[:, d, :, :n * 64] = src[:, s, :, :n * 64]
        outs.append(np.concatenate([o.reshape(-1), _sent(extra * 64)]))
    dh = None
    if hsrc_row is not None and len(hsrc_row):
        dh = _sent((len(hsrc_row) + extra, D))
        for d, r in enumerate(hsrc_row):
            dh[d] = dh[(d // 3) * 3].copy() if mutant == "dh_from_dh" and d % 3 else hsrc[r]
    return outs[0], outs[1], dh


FANOUT_GEOM = dict(layers=2, Tmax=136, slots=5)


def beam_fanout_cases():
    """lengths 1, 15, 16, 47, 48, 63, 64, 65, 129: len x 16 float4 straddles 256 (one pass of the tail loop), 768 (the guard of the
    unrolled loop) and 1024 (its step)"""
    n = 2 * 5 * 16 * 136 * 64
    kc, vc = _ints((n,)), _ints((n,), 2 ** 23)                             # K and V, and every (layer, slot, head, row), name themselves
    hsrc = _ints((4, D), 2 ** 22)
    hrow = np.array([2, 2, 0, 3, 1, 0, 3], i32)                            # two rows from one source; d = 0, 2 are source slots
    g = dict(FANOUT_GEOM, extra=EXTRA)
    mk = lambda name, pairs, rows=hrow, k=kc, v=vc: dict(name=name, kw=dict(g, kc=k, vc=v, pairs=np.array(pairs, i32).reshape(-1, 3), hsrc=hsrc,
                                                                               hsrc_row=rows))
    return [mk("len 1 15 16 47", [(0, 1, 1), (0, 2, 15), (0, 3, 16), (0, 4, 47)]),
            mk("len 48 63 64 65", [(2, 0, 48), (2, 1, 63), (2, 3, 64), (2, 4, 65)]),
            mk("len 129 0", [(1, 0, 129), (3, 4, 0)], rows=np.zeros(0, i32)),
            mk("residual rows only", [], k=None, v=None)]


# ---------------------------------------------------------------------------------------------------------------------------------
# the decode state and its kernels
# ---------------------------------------------------------------------------------------------------------------------------------
def make_state(seed, gen_stride=6):
    """every array a state kernel may read or write, each word recognisable; slot_of a non-identity permutation"""
    rng = np.random.default_rng(seed)
    st = {k: (1000 * (i + 1) + np.arange(n)).astype(i32) for i, (k, n) in enumerate(STATE_WORDS.items())}
    st["active"] = rng.integers(0, 2, 32).astype(i32)
    st["active"][[3, 30]] = 1
    st["active"][[4, 31]] = 0
    st["saved"] = rng.integers(0, 2, 32).astype(i32)
    st["slot_of"] = ((7 * np.arange(32) + 3) % 32).astype(i32)             # the engine's balanced order has this shape
    st["n_gen"] = rng.integers(0, gen_stride, 32).astype(i32)
    st["gen"] = (20000 + np.arange(32 * gen_stride)).astype(i32).reshape(32, gen_stride)
    return st


def pack_state(st, extra=0):
    gs = st["gen"].shape[1]
    blk = np.full(DEV_SEAM_STATE["gen"] + 32 * gs + extra, SENT_I, i32)
    for k, n in STATE_WORDS.items():
        blk[DEV_SEAM_STATE[k]:DEV_SEAM_STATE[k] + n] = st[k]
    blk[DEV_SEAM_STATE["gen"]:DEV_SEAM_STATE["gen"] + 32 * gs] = st["gen"].reshape(-1)
    return blk


def unpack_state(blk, gen_stride, extra=0):
    st = {k: blk[DEV_SEAM_STATE[k]:DEV_SEAM_STATE[k] + n].copy() for k, n in STATE_WORDS.items()}
    g0 = DEV_SEAM_STATE["gen"]
    st["gen"] = blk[g0:g0 + 32 * gen_stride].reshape(32, gen_stride).copy()
    st["tail"] = blk[g0 + 32 * gen_stride:].copy()                          # the sentinel words behind the block
    assert len(st["tail"]) == extra
    return st


def _copy_state(st, extra):
    out = {k: v.copy() for k, v in st.items()}
    out["tail"] = np.full(extra, SENT_I, i32)
    return out


def admit_rows_ref(tab, hsrc, hres, state, extra=0, mutant=None):
    st, h = _copy_state(state, extra), np.concatenate([hres, _sent((extra, D))])
    for d, tp, ctx, s_len, row in tab:
        h[d] = hsrc[row]
        st["cur_pos"][d], st["ctx_len"][d], st["n_gen"][d], st["cur_tok"][d], st["text_len"][d] = tp, ctx, 0, 0, s_len
        st["slot_meta"][4 * (d if mutant == "meta_of_row" else st["slot_of"][d]) + 1] = ctx
    return h, st


def admit_mask_ref(phase, admitted, state, extra=0, mutant=None):
    st = _copy_state(state, extra)
    n = 0
    for d in range(len(admitted)):
        if phase == 0:
            st["saved"][d] = 0 if admitted[d] else st["active"][d]
            st["active"][d] = admitted[d]
        else:
            v = int((st["active"][d] if mutant == "forget_saved" else (st["active"][d] | st["saved"][d])) != 0)
            st["active"][d] = v
            st["slot_meta"][4 * st["slot_of"][d] + 2] = v
            n += v
    if phase == 1:
        st["n_active"][0] = n
    return st


def serve_cancel_ref(mask, nrows, state, extra=0, mutant=None):
    st = _copy_state(state, extra)
    n = 0
    for d in range(nrows):
        v = 0 if (mask >> d) & 1 else int(st["active"][d] != 0)
        st["active"][d] = v
        st["slot_meta"][4 * st["slot_of"][d] + 2] = v
        n += v
    if mutant != "no_recount":
        st["n_active"][0] = n
    return st


def force_token_ref(tok, state, extra=0, mutant=None):
    st = _copy_state(state, extra)
    gs = st["gen"].shape[1]
    for b in range(len(tok)):
        n = st["n_gen"][b]
        if not st["active"][b] or n >= gs:
            continue
        st["gen"][b, n] = tok[b]
        st["n_gen"][b] = n + 1
        st["cur_tok"][b] = tok[b]
        st["cur_pos"][b] += 1
        st["ctx_len"][b] += 1
        st["slot_meta"][4 * st["slot_of"][b] + 1] = st["ctx_len"][b]
    return st


M64 = (1 << 64) - 1


def mix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def draw(seed, key, t, shift=40):
    """include/vallex_hip.h: u = (splitmix64(splitmix64(splitmix64(seed) + key) + t) >> 40) x 2^-24, in Python integers; the 24-bit
    integer and the product with 2^-24 are exact in float32"""
    return f32(mix64((mix64((mix64(seed) + key) & M64) + t) & M64) >> shift) * f32(1.0 / 16777216.0)


SEEDS = (0, 1, 2 ** 32, 2 ** 63 + 12345, 0x80000000, 0xFFFFFFFF00000001)      # 32-bit halves with the sign bit set among them
STEPS = (1, 255, 256, 257)


def admit_uniforms_ref(pairs, staged, steps, ncols, seed, u, extra=0, mutant=None):
    out = np.concatenate([u.reshape(-1), _sent(extra)])
    for i, (d, r) in enumerate(pairs):
        for t in range(steps):
            key = d if mutant == "key_is_row" else r
            out[t * ncols + d] = staged[i, t] if staged is not None else draw(seed, int(key), t, 39 if mutant == "shift39" else 40)
    return out


def uniforms_buffer(usteps, ncols):
    return _ints((usteps, ncols), 2 ** 20)                                  # the caller's contents: no draw (< 1) looks like them


def admit_uniforms_cases():
    out = []
    for k, (seed, steps) in enumerate(zip(SEEDS[:4], STEPS)):
        ncols = (32, 32, 5, 1)[k]
        pairs = np.array([[[31, 0], [0, 31], [7, 40]], [[2, 31], [30, 0]], [[4, 7], [1, 31], [0, 0]], [[0, 1000]]][k], i32)
        out.append(dict(name=f"seed {seed:#x} steps {steps}", kw=dict(pairs=pairs, staged=None, steps=steps, ncols=ncols, seed=seed,
                                                                    u=uniforms_buffer(steps + 2, ncols), extra=EXTRA)))
    staged = _ints((2, 9), 2 ** 21)
    out.append(dict(name="staged", kw=dict(pairs=np.array([[3, 1], [0, 0]], i32), staged=staged, steps=9, ncols=4, seed=5, u=uniforms_buffer(9, 4),
                                           extra=EXTRA)))
    return out


def _fbits(v):
    return int(np.array(v, f32).view(i32))


def serve_tab_entry(d, j, off, steps, seed, top_k=-100, temperature=1.0, force_eos_at=-1, top_p=1.0, penalty=1.0, window=0, min_frames=0):
    lo, hi = seed & 0xFFFFFFFF, seed >> 32
    s32 = lambda w: w - (1 << 32) if w >= 1 << 31 else w
    return [d, j, off, steps, s32(lo), s32(hi), top_k, _fbits(temperature), force_eos_at, _fbits(top_p), _fbits(penalty), window, min_frames]


def serve_uniforms_ref(tab, staged, ncols, u, sum_logp, state, extra=0, mutant=None):
    st = _copy_state(state, extra)
    out, sl = np.concatenate([u.reshape(-1), _sent(extra)]), np.concatenate([sum_logp, _sent(extra)])
    for e in tab:
        d, j, off, steps = (int(v) for v in e[:4])
        seed = (int(e[4]) & 0xFFFFFFFF) | ((int(e[5]) & 0xFFFFFFFF) << 32)
        sl[d] = 0.0
        st["row_smp"][4 * d:4 * d + 4] = [e[6], e[7], e[8], 0]
        st["row_flt"][4 * d:4 * d + 4] = e[9:13]
        for t in range(steps):
            out[t * ncols + d] = staged[off + t] if off >= 0 else draw(seed, d if mutant == "key_is_row" else j, t, 39 if mutant == "shift39" else 40)
    return out, sl, st


def serve_uniforms_cases():
    staged = _ints((40,), 2 ** 21)
    e = serve_tab_entry
    tabs = [
        # different steps in one launch (the grid is sized by the longest), every seed, keys 0 and 31, decode rows 0 and 31
        ("steps 257 1 255 256", 32, 260, [e(31, 0, -1, 257, SEEDS[3], 10, 0.7, 50, 0.9, 1.3, 16, 4), e(0, 31, -1, 1, SEEDS[2]),
                                          e(5, 1, -1, 255, SEEDS[1], -100, 1.0, -1), e(17, 3, -1, 256, SEEDS[0], 1, 2.5, 0, 0.5, 2.0, 0, 9)]),
        # no draw at all, staged draws from an offset, and a sign-bit seed word
        ("steps 0, staged", 6, 12, [e(4, 2, -1, 0, 77, 3, 0.5, 7, 0.25, 1.5, 3, 2), e(1, 0, 7, 12, 0), e(3, 1, 28, 12, 0), e(0, 31, -1, 12, SEEDS[4]),
                                    e(5, 0, -1, 3, SEEDS[5])]),
    ]
    out = []
    for name, ncols, usteps, tab in tabs:
        out.append(dict(name=name, kw=dict(tab=np.array(tab, i32), staged=staged, ncols=ncols, u=uniforms_buffer(usteps, ncols),
                                           sum_logp=(np.arange(32) + 0.5).astype(f32), state=make_state(2110), extra=EXTRA)))
    return out


def admit_rows_cases():
    out = []
    hsrc = _ints((6, D))
    for n in (1, 5, 32):
        rng = np.random.default_rng(2120 + n)
        rows = rng.permutation(32)[:n]
        tab = np.array([[d, 10 + i, 40 + 3 * i, 7 + i, rng.integers(0, 6)] for i, d in enumerate(rows)], i32)
        out.append(dict(name=f"n {n}", kw=dict(tab=tab, hsrc=hsrc, hres=_ints((32, D), 2 ** 20), state=make_state(2121 + n), extra=EXTRA)))
    return out


def admit_mask_cases():
    """phase 0 then phase 1 on the state phase 0 left (the GPU test chains the launches the same way); rows 3 and 30 were active before
    and are admitted: their predecessor's flag must not come back through `saved`"""
    out = []
    for nrows in (1, 5, 32):
        st = make_state(2130 + nrows)
        st["active"][0] = 1
        admitted = np.zeros(nrows, i32)
        admitted[[d for d in (0, 3, 4, 30) if d < nrows]] = 1
        out.append(dict(name=f"nrows {nrows}", kw=dict(admitted=admitted, state=st, extra=EXTRA)))
    return out


def admit_mask_sampled(st, admitted):
    """what the first sample of the admitted rows may do between the phases: admitted row 3 -- whose predecessor was still active when it
    was admitted -- finishes at once, and phase 1 must not revive it"""
    st = {k: v.copy() for k, v in st.items() if k != "tail"}
    if len(admitted) > 3 and admitted[3]:
        st["active"][3] = 0
    return st


def serve_cancel_cases():
    out = []
    for nrows, masks in ((1, (0, 1)), (5, (0, 1 << 3, 0b10110)), (32, (0, 1 << 3, 1 << 31, 0xFFFFFFFF))):
        for mask in masks:
            st = make_state(2140 + nrows)
            st["active"][2] = 7                                             # a flag that is not 0 | 1 comes back as 1
            out.append(dict(name=f"nrows {nrows} mask {mask:#x}", kw=dict(mask=mask, nrows=nrows, state=st, extra=EXTRA)))
    return out


def force_token_cases():
    out = []
    for batch in (1, 5, 32):
        st = make_state(2150 + batch)
        st["active"][0], st["n_gen"][0] = 1, 2
        if batch > 4:
            st["active"][3], st["n_gen"][3] = 1, st["gen"].shape[1]         # a full row: nothing written, nothing advanced
            st["active"][4] = 0                                             # an inactive row
        out.append(dict(name=f"batch {batch}", kw=dict(tok=(500 + np.arange(batch)).astype(i32), state=st, extra=EXTRA)))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# gemv: float64 with a derived bound
# ---------------------------------------------------------------------------------------------------------------------------------
def gemv_roundings(K):
    """The most fp32 roundings any product of a row passes through in gemv_kernel, with or without contraction of its multiply-adds: its
    own product (1), the three adds of its group of four (3), one add into the lane's sum per 256-column step (ceil(K / 256)), the six
    adds of the wave reduction (6), the bias (1)."""
    return 1 + 3 + -(-K // 256) + 6 + 1


def gemv_ref(W, e, bias, extra=0):
    """(ref, bound) in the shape of tests/_wave_refs.check: NaN = the sentinel; bound = gamma_n (sum |w| |x| + |b|)"""
    W64, e64 = W.astype(f64), e.astype(f64)
    ref = W64 @ e64 + (0 if bias is None else bias.astype(f64))
    mag = np.abs(W64) @ np.abs(e64) + (0 if bias is None else np.abs(bias.astype(f64)))
    bound = gamma(gemv_roundings(W.shape[1])) * mag
    return np.concatenate([ref, np.full(extra, np.nan)]), np.concatenate([bound, np.zeros(extra)])


GEMV_SHAPES = ((2048, 1024), (5, 1024), (4, 4), (7, 260))


def gemv_cases():
    out = []
    for N, K in GEMV_SHAPES:
        rng = np.random.default_rng(2160 + N + K)
        W, e, b = rng.standard_normal((N, K)).astype(f32), rng.standard_normal(K).astype(f32), rng.standard_normal(N).astype(f32)
        out += [dict(name=f"{N}x{K} bias", kw=dict(W=W, e=e, bias=b, extra=EXTRA)), dict(name=f"{N}x{K}", kw=dict(W=W, e=e, bias=None, extra=EXTRA))]
    return out


def ada_table_ref(sd, NL):
    """(ref, bound) [7][2 NL + 1][2048] of the AdaLN table the loader builds: W e + b of every (stage, norm) in float64"""
    names = [f"nar_decoder.layers.{n // 2}.norm{1 + n % 2}.project_layer." for n in range(2 * NL)] + ["nar_decoder.norm.project_layer."]
    ref, bound = np.empty((7, len(names), 2048)), np.empty((7, len(names), 2048))
    for st in range(7):
        e = np.asarray(sd[f"nar_stage_embeddings.{st}.word_embeddings.weight"], f32).reshape(-1)[:D]
        for n, p in enumerate(names):
            ref[st, n], bound[st, n] = gemv_ref(np.asarray(sd[p + "weight"], f32), e, np.asarray(sd[p + "bias"], f32))
    return ref, bound
