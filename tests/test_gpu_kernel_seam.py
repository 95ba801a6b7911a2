"""GPU: the kernels of the seams between the phases -- embed_rows, nar_yemb_init, add_pe_scatter, embed_accum, argmax_rows, kv_scatter,
gemv (csrc/rows.hip), beam_fanout (csrc/beams.hip), admit_rows, admit_mask, admit_uniforms (csrc/admit.hip), serve_uniforms,
serve_cancel (csrc/serve.hip), dec_force_token (csrc/decode.hip) -- one launch at a time through vx_dev_seam_op, against the
restatements of tests/_seam_refs.py (pinned to the oracle and shown to bite on the CPU by tests/test_seam_refs.py), and the tables
built at load time (the positional table, the AdaLN table).

Everything but gemv is bit-identical, the `extra` rows or words behind every output and every word nobody may write included.

Worst observed err / bound on MI355X (printed by the tests; 1.0 is the limit; bound = gamma_n (sum |w||x| + |b|), n = 12 + ceil(K / 256)):
  gemv 2048x1024 0.020, 5x1024 0.008, 4x4 0.065, 7x260 0.015 (with bias; without: 0.018, 0.004, 0.051, 0.012)
  AdaLN table (35 slots x 2048): 0.027; the nearest OTHER slot misses its bound by a factor of 1.9e5
"""
import numpy as np
import pytest

from oracle import synth
from tests import _seam_refs as R
from tests._util import get_model

pytestmark = pytest.mark.gpu
f32, f64, i32 = np.float32, np.float64, np.int32
EXTRA = R.EXTRA
MODEL = dict(num_layers=2, seed=0, eos_gain=2.5)


@pytest.fixture(scope="module")
def eng():
    return get_model(MODEL["num_layers"], MODEL["seed"], MODEL["eos_gain"], vocos=True, max_new=64, max_prompt=96, max_text=32, max_batch=4).engine


def _state_io(kw):
    gs = kw["state"]["gen"].shape[1]
    return gs, R.pack_state(kw["state"], kw["extra"])


def launch(eng, op, kw):
    """one vx_dev_seam_op launch of `op` on the keyword arguments of its reference; returns the buffers as they come back, in the shape
    the reference returns them"""
    ex = kw.get("extra", 0)
    if op == "embed_rows":
        out = np.empty((kw["out_rows"] + ex, 1024), f32)
        eng.dev_seam_op(op, [len(kw["idA"]), ex, kw["out_rows"], len(kw["tabA"]), 0 if kw["tabB"] is None else len(kw["tabB"]), len(kw["pe"])],
                        fa=kw["tabA"], fb=kw["tabB"], fc=[kw["alpha"]], fd=kw["pe"], ia=kw["idA"], ib=kw["idB"], ic=kw["pos"], id=kw["dst"], out=out)
        return out
    if op == "nar_yemb_init":
        out = np.empty((len(kw["codes"]) + ex, 1024), f32)
        eng.dev_seam_op(op, [len(kw["codes"]), ex, kw["tabs"].shape[1]], fa=kw["tabs"], ia=kw["codes"], ib=kw["nj"], out=out)
        return out
    if op == "add_pe_scatter":
        out = np.empty((kw["out_rows"] + ex, 1024), f32)
        eng.dev_seam_op(op, [len(kw["yemb"]), ex, kw["out_rows"], len(kw["pe"])], fa=kw["yemb"], fc=[kw["alpha"]], fd=kw["pe"], ic=kw["pos"],
                        id=kw["dst"], out=out)
        return out
    if op == "embed_accum":
        out = np.concatenate([kw["yemb"], np.zeros((ex, 1024), f32)])
        eng.dev_seam_op(op, [len(kw["tok"]), ex, len(kw["yemb"]), len(kw["tab"])], fa=kw["tab"], ia=kw["tok"], id=kw["rowidx"], out=out)
        return out
    if op == "argmax_rows":
        idx = np.zeros(len(kw["x"]) + ex, i32)
        eng.dev_seam_op(op, [len(kw["x"]), ex, kw["N"], kw["x"].shape[1]], fa=kw["x"], iout=idx)
        return idx
    if op == "kv_scatter":
        n = (kw["slots"] * 16 * kw["Tmax"] + ex) * 64
        kc, vc = np.zeros(n, f32), np.zeros(n, f32)
        eng.dev_seam_op(op, [len(kw["qkv"]), ex, kw["Tmax"], kw["slots"]], fa=kw["qkv"], ia=kw["row_b"], ib=kw["row_t"], out=kc, out2=vc)
        return kc, vc
    if op == "gemv":
        out = np.zeros(len(kw["W"]) + ex, f32)
        eng.dev_seam_op(op, [kw["W"].shape[0], ex, kw["W"].shape[1]], fa=kw["W"], fb=kw["e"], fc=kw["bias"], out=out)
        return out
    if op == "beam_fanout":
        tail = np.zeros(ex * 64, f32)
        kc, vc = (None if c is None else np.concatenate([c.reshape(-1), tail]) for c in (kw["kc"], kw["vc"]))
        nrows = len(kw["hsrc_row"])
        dh = np.zeros((nrows + ex, 1024), f32) if nrows else None
        eng.dev_seam_op(op, [kw["layers"], ex, kw["Tmax"], kw["slots"], len(kw["pairs"]), nrows, len(kw["hsrc"])], fa=kw["hsrc"],
                        ia=kw["pairs"] if len(kw["pairs"]) else None, ib=kw["hsrc_row"] if nrows else None, out=kc, out2=vc, out3=dh)
        return kc, vc, dh
    if op == "admit_uniforms":
        u = np.concatenate([kw["u"].reshape(-1), np.zeros(ex, f32)])
        seed = kw["seed"]
        eng.dev_seam_op(op, [len(kw["pairs"]), ex, kw["steps"], kw["ncols"], len(kw["u"])] + [int(np.array(w, np.uint32).view(i32)) for w in (seed & 0xFFFFFFFF, seed >> 32)],
                        fa=kw["staged"], ia=kw["pairs"], out=u)
        return u
    gs, blk = _state_io(kw)
    back = lambda: R.unpack_state(blk, gs, ex)
    if op == "serve_uniforms":
        u, sl = np.concatenate([kw["u"].reshape(-1), np.zeros(ex, f32)]), np.concatenate([kw["sum_logp"], np.zeros(ex, f32)])
        eng.dev_seam_op(op, [len(kw["tab"]), ex, gs, kw["ncols"], len(kw["u"]), len(kw["staged"])], fa=kw["staged"], ia=kw["tab"], out=u, out2=sl, iout=blk)
        return u, sl, back()
    if op == "admit_rows":
        h = np.concatenate([kw["hres"], np.zeros((ex, 1024), f32)])
        eng.dev_seam_op(op, [len(kw["tab"]), ex, gs, len(kw["hsrc"])], fa=kw["hsrc"], ia=kw["tab"], out3=h, iout=blk)
        return h, back()
    if op == "admit_mask":
        eng.dev_seam_op(op, [len(kw["admitted"]), ex, gs, kw["phase"]], ia=kw["admitted"], iout=blk)
    elif op == "serve_cancel":
        eng.dev_seam_op(op, [kw["nrows"], ex, gs, int(np.array(kw["mask"], np.uint32).view(i32))], iout=blk)
    elif op == "force_token":
        eng.dev_seam_op(op, [len(kw["tok"]), ex, gs], ia=kw["tok"], iout=blk)
    else:
        raise KeyError(op)
    return back()


REFS = dict(embed_rows=R.embed_rows_ref, nar_yemb_init=R.nar_yemb_init_ref, add_pe_scatter=R.add_pe_scatter_ref, embed_accum=R.embed_accum_ref,
            argmax_rows=R.argmax_rows_ref, kv_scatter=R.kv_scatter_ref, beam_fanout=R.beam_fanout_ref, admit_uniforms=R.admit_uniforms_ref,
            serve_uniforms=R.serve_uniforms_ref, admit_rows=R.admit_rows_ref, admit_mask=R.admit_mask_ref, serve_cancel=R.serve_cancel_ref,
            force_token=R.force_token_ref)


def run_cases(eng, op, cases):
    for c in cases:
        R.check(launch(eng, op, c["kw"]), REFS[op](**c["kw"]), f"{op} {c['name']}")
    print(f"{op}: {len(cases)} launches, exact")


def test_embed_rows_keeps_the_two_roundings_and_its_own_rows(eng):
    run_cases(eng, "embed_rows", R.embed_rows_cases())


def test_nar_yemb_init_adds_exactly_nj_tables(eng):
    run_cases(eng, "nar_yemb_init", R.nar_yemb_init_cases())


def test_add_pe_scatter_keeps_the_two_roundings(eng):
    run_cases(eng, "add_pe_scatter", R.add_pe_scatter_cases())


def test_embed_accum_touches_the_named_rows_only(eng):
    run_cases(eng, "embed_accum", R.embed_accum_cases())


def test_argmax_rows_ties_signed_zeros_and_rows_without_a_candidate(eng):
    """The kernel's rule, pinned: the lowest index of the largest value under `>`; -0.0 and +0.0 tie (the first wins); a row of -inf or
    of NaN gets 0.  NaN next to numbers: torch.argmax returns the first NaN, the kernel SKIPS NaN and returns the first largest number
    (tests/test_seam_refs.py shows both) -- such a pass raised the range flag and is re-run in fp32, its ids only index tables."""
    run_cases(eng, "argmax_rows", R.argmax_cases())
    for c in R.argmax_cases():
        idx = launch(eng, "argmax_rows", c["kw"])[:len(c["kw"]["x"])]
        assert (0 <= idx).all() and (idx < c["kw"]["N"]).all()


def test_kv_scatter_moves_k_and_v_to_their_head_major_rows(eng):
    run_cases(eng, "kv_scatter", R.kv_scatter_cases())


def test_beam_fanout_copies_len_rows_and_every_residual_row(eng):
    run_cases(eng, "beam_fanout", R.beam_fanout_cases())


def test_admit_and_serve_uniforms_are_the_counter_formula(eng):
    run_cases(eng, "admit_uniforms", R.admit_uniforms_cases())
    run_cases(eng, "serve_uniforms", R.serve_uniforms_cases())


def test_admit_rows_writes_the_admitted_rows_state_only(eng):
    run_cases(eng, "admit_rows", R.admit_rows_cases())


def test_admit_mask_saves_and_restores_around_the_first_sample(eng):
    for c in R.admit_mask_cases():
        kw = dict(c["kw"], phase=0)
        st0 = launch(eng, "admit_mask", kw)
        R.check(st0, R.admit_mask_ref(**kw), f"admit_mask phase 0 {c['name']}")
        kw = dict(c["kw"], phase=1, state=R.admit_mask_sampled(st0, c["kw"]["admitted"]))
        R.check(launch(eng, "admit_mask", kw), R.admit_mask_ref(**kw), f"admit_mask phase 1 {c['name']}")


def test_serve_cancel_clears_the_named_rows_and_recounts(eng):
    run_cases(eng, "serve_cancel", R.serve_cancel_cases())


def test_force_token_commits_like_the_sampler(eng):
    run_cases(eng, "force_token", R.force_token_cases())


def test_gemv_against_float64(eng):
    for c in R.gemv_cases():
        ref, bound = R.gemv_ref(**c["kw"])
        print(f"gemv {c['name']}: worst err / bound = {R.check_bound(launch(eng, 'gemv', c['kw']), ref, bound, 'gemv ' + c['name']):.3f}")


def test_tables_built_at_load_time(eng):
    from vallex_amd.models.vallex import sine_pe_table
    geom = np.zeros(3, i32)
    eng.dev_seam_op("tables", [], iout=geom)
    pe_rows, NL, nnorm = (int(v) for v in geom)
    assert NL == MODEL["num_layers"] and nnorm == 2 * NL + 1 and pe_rows >= 1
    pe, ada = np.empty((pe_rows, 1024), f32), np.empty((7, nnorm, 2048), f32)
    eng.dev_seam_op("tables", [], out=pe, out2=ada)
    R.check(pe, sine_pe_table(pe_rows), "positional table")
    ref, bound = R.ada_table_ref(synth.vallex_state_dict(MODEL["num_layers"], MODEL["seed"], MODEL["eos_gain"]), NL)
    print(f"tables: ada worst err / bound = {R.check_bound(ada, ref, bound, 'AdaLN table'):.3f}")
    # a permuted (stage, norm) index cannot pass: no slot lies within the bound of any OTHER slot's float64 value
    got, ref, bound = (a.reshape(7 * nnorm, 2048) for a in (ada.astype(f64), ref, bound))
    nearest = np.inf
    for s in range(len(got)):
        over = (np.abs(got[s][None] - ref) / bound).max(1)                 # worst element against every slot's reference
        assert over[s] <= 1.0
        nearest = min(nearest, np.delete(over, s).min())
    print(f"tables: ada, the nearest other slot misses its bound by a factor of {nearest:.3g}")
    assert nearest > 1.0


# ---- refused arguments ---------------------------------------------------------------------------------------------------------
def _refused(eng, op, dims, code=None, **args):
    from vallex_amd import VallexHipError
    from vallex_amd._capi import VX_EINVAL
    outs = [v for k, v in args.items() if k in ("out", "out2", "out3", "iout") and v is not None]
    before = [o.copy() for o in outs]
    with pytest.raises(VallexHipError) as e:
        eng.dev_seam_op(op, dims, **args)
    assert e.value.code == (VX_EINVAL if code is None else code), e.value
    assert all((R.bits(a) == R.bits(b)).all() if a.dtype == f32 else (a == b).all() for a, b in zip(outs, before)), op


def test_refused_indices_leave_the_outputs_untouched_rows(eng):
    out = np.full((16, 1024), 75, f32)
    kw = R.embed_rows_cases()[0]["kw"]
    dims = [9, EXTRA, 12, 6, 3, 12]
    base = dict(fa=kw["tabA"], fb=kw["tabB"], fc=[kw["alpha"]], fd=kw["pe"], ia=kw["idA"], ib=kw["idB"], ic=kw["pos"], id=kw["dst"], out=out)
    bump = lambda v, i, x: np.concatenate([v[:i], [x], v[i + 1:]]).astype(i32)
    for bad in (dict(ia=bump(kw["idA"], 2, 6)), dict(ia=bump(kw["idA"], 2, -1)), dict(ib=bump(kw["idB"], 0, 3)), dict(ib=bump(kw["idB"], 0, -2)),
                dict(ic=bump(kw["pos"], 8, 12)), dict(id=bump(kw["dst"], 1, 12)), dict(id=bump(kw["dst"], 1, 7)), dict(ib=None), dict(fb=None)):
        _refused(eng, "embed_rows", dims, **dict(base, **bad))
    _refused(eng, "embed_rows", [9, 65, 12, 6, 3, 12], **base)
    _refused(eng, "embed_rows", [9, EXTRA, 8, 6, 3, 12], **dict(base, id=None))                       # no dst: out must hold the rows
    kw = R.nar_yemb_init_cases()[0]["kw"]
    base = dict(fa=kw["tabs"], ia=kw["codes"], ib=kw["nj"], out=out)
    codes = kw["codes"].copy()
    codes[0, 7] = 3                                                                                 # a column >= nj is checked, too
    for bad in (dict(ia=codes), dict(ib=bump(kw["nj"], 1, 0)), dict(ib=bump(kw["nj"], 1, 9))):
        _refused(eng, "nar_yemb_init", [6, EXTRA, 3], **dict(base, **bad))
    kw = R.add_pe_scatter_cases()[0]["kw"]
    base = dict(fa=kw["yemb"], fc=[kw["alpha"]], fd=kw["pe"], ic=kw["pos"], id=kw["dst"], out=out)
    for bad in (dict(ic=bump(kw["pos"], 0, 12)), dict(id=bump(kw["dst"], 0, -1)), dict(id=bump(kw["dst"], 0, 0)), dict(id=None)):
        _refused(eng, "add_pe_scatter", [9, EXTRA, 12, 12], **dict(base, **bad))
    kw = R.embed_accum_cases()[0]["kw"]
    base = dict(fa=kw["tab"], ia=kw["tok"], id=kw["rowidx"], out=out)
    for bad in (dict(id=bump(kw["rowidx"], 4, 8)), dict(id=bump(kw["rowidx"], 4, 10)), dict(ia=bump(kw["tok"], 0, 5))):      # a duplicate first
        _refused(eng, "embed_accum", [5, EXTRA, 10, 5], **dict(base, **bad))
    idx = np.full(8, 75, i32)
    x = np.zeros((4, 1032), f32)
    for dims in ([4, EXTRA, 1025, 1024], [4, EXTRA, 0, 1032], [0, EXTRA, 1024, 1032], [4, EXTRA, 1024, 8193]):
        _refused(eng, "argmax_rows", dims, fa=x, iout=idx)
    kw = R.kv_scatter_cases()[0]["kw"]
    kc, vc = np.full((3 * 16 * 40 + EXTRA) * 64, 75, f32), np.full((3 * 16 * 40 + EXTRA) * 64, 75, f32)
    base = dict(fa=kw["qkv"], ia=kw["row_b"], ib=kw["row_t"], out=kc, out2=vc)
    for bad in (dict(ia=bump(kw["row_b"], 0, 3)), dict(ib=bump(kw["row_t"], 0, 40)), dict(ib=bump(kw["row_t"], 1, -1)), dict(ib=bump(kw["row_t"], 1, 0))):
        _refused(eng, "kv_scatter", [7, EXTRA, 40, 3], **dict(base, **bad))                           # the last: rows 1 and 4 share (1, 0)
    for dims in ([4, EXTRA, 6], [0, EXTRA, 4], [4, EXTRA, 0]):
        _refused(eng, "gemv", dims, fa=np.ones((4, 8), f32), fb=np.ones(8, f32), out=out[0])
    for op in (15, -1):
        _refused(eng, op, [1, 0], fa=out, out=out)


def test_refused_indices_leave_the_outputs_untouched_fanout_and_state(eng):
    kw = R.beam_fanout_cases()[0]["kw"]
    g = [kw["layers"], EXTRA, kw["Tmax"], kw["slots"]]
    kc, vc, dh = kw["kc"].copy(), kw["vc"].copy(), np.full((7 + EXTRA, 1024), 75, f32)
    kc, vc = np.concatenate([kc, np.zeros(EXTRA * 64, f32)]), np.concatenate([vc, np.zeros(EXTRA * 64, f32)])
    base = dict(fa=kw["hsrc"], ib=kw["hsrc_row"], out=kc, out2=vc, out3=dh)
    for pairs in ([(0, 1, 5), (1, 2, 5)],                                                           # a chained pair
                  [(0, 1, 5), (2, 1, 5)], [(0, 5, 5)], [(-1, 1, 5)], [(0, 1, 137)], [(0, 1, -1)], [(2, 2, 5)]):
        _refused(eng, "beam_fanout", g + [len(pairs), 7, 4], ia=np.array(pairs, i32), **base)
    _refused(eng, "beam_fanout", g + [0, 7, 4], **dict(base, ib=np.array([0, 1, 2, 3, 4, 0, 0], i32)))   # an hsrc row outside hsrc
    _refused(eng, "beam_fanout", g + [0, 0, 4], **base)
    c = R.admit_rows_cases()[1]["kw"]
    gs, blk = _state_io(c)
    h = np.full((32 + EXTRA, 1024), 75, f32)
    tab = c["tab"].copy()
    for i, j, v in ((0, 0, 32), (0, 0, -1), (1, 0, int(tab[0, 0])), (2, 4, 6)):                      # row outside, a row twice, hsrc row outside
        t = tab.copy()
        t[i, j] = v
        _refused(eng, "admit_rows", [5, EXTRA, gs, 6], fa=c["hsrc"], ia=t, out3=h, iout=blk)
    bad_slot = blk.copy()
    bad_slot[R.DEV_SEAM_STATE["slot_of"] + 5] = bad_slot[R.DEV_SEAM_STATE["slot_of"] + 6]              # slot_of is no permutation
    _refused(eng, "admit_rows", [5, EXTRA, gs, 6], fa=c["hsrc"], ia=tab, out3=h, iout=bad_slot)
    _refused(eng, "serve_cancel", [33, EXTRA, gs, 1], iout=blk)
    _refused(eng, "serve_cancel", [0, EXTRA, gs, 1], iout=blk)
    _refused(eng, "admit_mask", [5, EXTRA, gs, 2], ia=np.ones(5, i32), iout=blk)
    _refused(eng, "force_token", [33, EXTRA, gs], ia=np.ones(33, i32), iout=blk)
    _refused(eng, "force_token", [5, EXTRA, 0], ia=np.ones(5, i32), iout=blk)
    u = R.uniforms_buffer(10, 4).reshape(-1)
    for dims, pairs in (([2, 0, 9, 4, 10, 1, 0], [[4, 0], [0, 1]]), ([2, 0, 9, 4, 10, 1, 0], [[3, 0], [3, 1]]), ([2, 0, 11, 4, 10, 1, 0], [[3, 0], [0, 1]]),
                        ([2, 0, 9, 33, 10, 1, 0], [[3, 0], [0, 1]]), ([2, 0, 9, 4, 10, 1, 0], [[3, -1], [0, 1]])):
        _refused(eng, "admit_uniforms", dims, ia=np.array(pairs, i32), out=u)
    s = R.serve_uniforms_cases()[1]["kw"]
    gs, blk = _state_io(s)
    su, sl = np.concatenate([s["u"].reshape(-1), np.zeros(EXTRA, f32)]), np.concatenate([s["sum_logp"], np.zeros(EXTRA, f32)])
    for i, j, v in ((0, 0, 6), (0, 0, 1), (0, 3, 13), (1, 2, 29), (1, 2, -2), (0, 1, -1)):           # row outside / twice, draws, staged range, beam
        t = s["tab"].copy()
        t[i, j] = v
        _refused(eng, "serve_uniforms", [5, EXTRA, gs, 6, 12, 40], fa=s["staged"], ia=t, out=su, out2=sl, iout=blk)


def test_entry_is_refused_inside_a_serving_session_and_leaves_the_product_alone(eng):
    from vallex_amd._capi import VX_ESTATE
    codes = np.random.default_rng(3).integers(0, 1024, (5, 8))
    before = eng.vocos_decode([codes])[0].copy()
    kw = R.gemv_cases()[2]["kw"]
    with eng.serve():
        out, geom = np.full(4 + EXTRA, 75, f32), np.full(3, 75, i32)
        _refused(eng, "gemv", [4, EXTRA, 4], code=VX_ESTATE, fa=kw["W"], fb=kw["e"], fc=kw["bias"], out=out)
        _refused(eng, "tables", [], code=VX_ESTATE, iout=geom)
    launch(eng, "gemv", kw)
    np.testing.assert_array_equal(eng.vocos_decode([codes])[0], before)


# ---- the product path with position scales that are no powers of two ---------------------------------------------------------------
ALPHAS = {"ar_text_position.alpha": 0.8731, "ar_audio_position.alpha": 1.2345, "nar_text_position.alpha": 2.5, "nar_audio_position.alpha": 0.6107}
_PRODUCT = {}


def _product_case():
    """weights of get_model(2, ...) with the four position scales overwritten, one short row, and the oracle's greedy ids for it"""
    if not _PRODUCT:
        from oracle.vallex_oracle import VallexOracle
        sd = dict(synth.vallex_state_dict(2, 7))
        for k, v in ALPHAS.items():
            assert k in sd and np.frexp(f32(v))[0] != 0.5
            sd[k] = np.array([v], f32)
        a, t = synth.synth_prompt(16, 5, seed=9)
        text = np.concatenate([t[0], synth.synth_text(7, 9)])
        ref = VallexOracle(sd, 2).inference(text[None], np.array([len(text)]), a, 5, top_k=1, prompt_language="zh", text_language="en", force_eos_at=10)
        _PRODUCT.update(sd=sd, a=a, text=text, ref=ref)
    return _PRODUCT


@pytest.mark.parametrize("arith", ["default", "f32"])
def test_product_ids_equal_the_oracle_with_alphas_that_round(arith):
    """every committed synthetic checkpoint has NAR position scales of 1.0 (and the goldens were generated with them): a contracted
    multiply-add in embed_rows / add_pe_scatter would change no id there.  Here all four scales round, end to end."""
    from vallex_amd.models.vallex import VALLE
    p = _product_case()
    m = VALLE(1024, 16, 2, norm_first=True, add_prenet=False, prefix_mode=1, share_embedding=True, nar_scale_factor=1.0, prepend_bos=True,
              num_quantizers=8, engine_max_new=32, engine_max_prompt=32, engine_max_text=32, engine_max_batch=2, engine_arith=arith)
    m.to("cuda:0").load_state_dict(p["sd"], strict=True)
    out = m.inference(p["text"][None], np.array([len(p["text"])]), p["a"], 5, top_k=1, prompt_language="zh", text_language="en", force_eos_at=10).numpy()
    assert out.shape == p["ref"].shape and out.shape[1] == 10 and (out == p["ref"]).all(), np.argwhere(out != p["ref"])[:4]
