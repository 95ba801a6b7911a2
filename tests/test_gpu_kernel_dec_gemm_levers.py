"""The request-order and block-mapping switches of the decode step's weight-streaming GEMMs (csrc/decode.hip, round 35):
  VX_L2_KMAP        linear2 of the 5 .. 32-row chain cuts its block id with the K slice fastest (one K slice per XCD),
  VX_L1_INTERLEAVE  linear1 requests w[u], x0[u], x1[u] per k-block instead of all of x and then the weights.
Both decide where a workgroup runs or in which order it asks for its operands, never what it computes.

GPU: every launch of the GEMM half of the step through vx_dev_dec_op, on a context with the defaults and on one with both switches
off, must leave the same words: the whole slab image (the packed image, unpacked, for linear1), rows behind the batch included --
these kernels compute all 32 MFMA columns whatever the row count, so the rows behind the batch are written (from the sentinel rows
of the input image) and compared like the others; the one region a kernel of this file leaves alone, the k / v columns of slabs
4 .. 7 of the balanced in_proj, must keep the entry's sentinel under both settings.  CPU: a model of the block-id cut, a bijection on every grid the kernel runs."""
import numpy as np
import pytest

from oracle import synth
from tests import _kernel_refs as R
from tests import _util
from tests._util import get_model

SENT_F = np.float32(-1.0e30)
GEOM = dict(max_new=160, max_prompt=96, max_text=32, max_batch=32)      # the 2-layer context of tests/test_gpu_kernel_dec_ffn.py
OPS = ("gemm:linear2", "gemm:in_proj", "gemm:out_proj", "gemm:predict", "linear1", "qkv_bal")
ROWS = (5, 17, 32)
SETS = ("normal", "cancel")


# ---- the block-id cut (CPU) ---------------------------------------------------------------------------------------------------------
def kmap(block_id, splitk):
    """skinny_gemm_kernel with kslog = log2(splitk): linear block id (column tile fastest in the grid) -> (column tile, K slice)"""
    kslog = splitk.bit_length() - 1
    assert 1 << kslog == splitk
    return block_id >> kslog, block_id & (splitk - 1)


@pytest.mark.parametrize("tiles,splitk", [(32, 8), (32, 4), (96, 4), (33, 4)])
def test_block_id_cut_is_a_bijection(tiles, splitk):
    ids = [x + tiles * y for y in range(splitk) for x in range(tiles)]          # blockIdx.x + gridDim.x * blockIdx.y
    assert sorted(ids) == list(range(tiles * splitk))
    cut = [kmap(i, splitk) for i in ids]
    assert sorted(cut) == [(t, k) for t in range(tiles) for k in range(splitk)], "every (column tile, K slice) exactly once"
    # the point of it: workgroups are dealt to the 8 XCDs by id % 8, and an XCD sees 8 / splitk ... 1 K slices instead of all
    for xcd in range(8):
        slices = {k for i, (t, k) in zip(ids, cut) if i % 8 == xcd}
        assert slices == ({xcd} if splitk == 8 else {xcd % splitk}), (xcd, slices)
    # the plain mapping, for contrast: every XCD holds every slice of the (32, 8) grid
    if (tiles, splitk) == (32, 8):
        assert all({i // tiles for i in ids if i % 8 == xcd} == set(range(8)) for xcd in range(8))


# ---- old against new (GPU) ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def W():
    return R.ffn_weights(synth.vallex_state_dict(2, 1, 0.0), 2)


@pytest.fixture(scope="module")
def engines():
    """(defaults, both switches off).  The default context is finalized before the environment is touched; the switched one is made
    by tests/_util.switched_model, which clears every VX_ switch of the caller's shell first."""
    new = get_model(2, 1, 0.0, **GEOM).engine
    levers = new.dev_gemm_levers()
    mp = pytest.MonkeyPatch()
    try:
        old = _util.switched_model(mp, {"VX_L2_KMAP": "0", "VX_L1_INTERLEAVE": "0"}, {}, 2, 1, 0.0, **GEOM).engine
        assert old.dev_gemm_levers() == {"l2_kmap": 0, "l1_interleave": 0}, "the context did not read the switches"
    finally:
        mp.undo()
    yield new, old, levers
    _util.drop_switched()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.gpu
def test_defaults_are_the_new_behaviour(engines):
    import os
    want = {f: int(os.environ.get(v, "1")[:1] != "0") for f, v in (("l2_kmap", "VX_L2_KMAP"), ("l1_interleave", "VX_L1_INTERLEAVE"))}
    assert engines[2] == want          # {1, 1} unless the caller's shell sets a lever


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
def test_old_and_new_leave_the_same_words(engines, W, op):
    new, old, _ = engines
    name = op.partition(":")[0]
    for nrows in ROWS:
        for kind in SETS:
            for launch in R.ffn_case(op, nrows, kind, W):
                a, b = new.dev_dec_op(**launch["args"])["out"], old.dev_dec_op(**launch["args"])["out"]
                assert a.shape == b.shape
                d = np.argwhere(bits(a) != bits(b))
                assert not len(d), (op, nrows, kind, "first differing word at", d[0].tolist(), "of", len(d))
                for o in (a, b):
                    if name == "qkv_bal":
                        assert (o[4:, :, 1024:] == SENT_F).all(), "the k, v columns of slabs 4 .. 7 are not written"
                        assert (o[:4] != SENT_F).all() and (o[4:, :, :1024] != SENT_F).all()
                    else:
                        assert (o[..., :nrows, :] != SENT_F).all(), "a word of the batch rows was not written"
