"""CPU (cross-compiles, no GPU): what the request orders of round 35 must look like in the generated gfx950 code (csrc/decode.hip).
Whichever order a decode GEMM asks for its operands in, a whole round of them is out before the first MFMA -- a load sunk to its use
is one more memory round trip on the step's latency chain --, the weight stream is non-temporal, and nothing spills."""
import re

from tests.test_isa import asm, kernel_body, metadata  # noqa: F401  (asm is the module's fixture)

# kernel symbol prefix, metadata name, loads of a round (x + weights [+ bias]), non-temporal loads among them
# (skinny_gemm_kernel: two rounds -- the second, requested under `i + 8 < kb_per_wave`, also stands in front of the first round's MFMAs)
ROUNDS = ((r"_ZN2vx18skinny_gemm_kernelE", "skinny_gemm_kernel", 32, 16),
          (r"_ZN2vx25skinny16_relu_pack_kernelE", "skinny16_relu_pack_kernel", 25, 8),
          (r"_ZN2vx32skinny16_relu_pack_xfirst_kernelE", "skinny16_relu_pack_xfirst_kernel", 25, 8),
          (r"_ZN2vx21skinny_qkv_bal_kernelE", "skinny_qkv_bal_kernel", 16, 8))


def _head(lines, sym):
    body = kernel_body(lines, sym)
    first_mfma = next(i for i, ln in enumerate(body) if ln.startswith("v_mfma"))
    return body, [ln for ln in body[:first_mfma] if ln.startswith("global_load_dwordx4")], first_mfma


def test_a_whole_round_is_requested_before_the_first_mfma(asm):
    lines = asm("decode.hip")
    for sym, name, n_loads, n_nt in ROUNDS:
        body, loads, first_mfma = _head(lines, sym)
        assert len(loads) == n_loads, (name, len(loads))
        assert sum(" nt" in ln for ln in loads) == n_nt, (name, "the weight stream must be non-temporal")
        assert not [ln for ln in body[:first_mfma] if ln.startswith("s_waitcnt") and "vmcnt(0)" in ln], (name, "a full wait in front of the first MFMA")
        assert metadata(lines, name, "private_segment_fixed_size") == 0, name


def test_linear1_interleaves_weights_and_activations(asm):
    """per k-block w[u], x0[u], x1[u] (the bias in front): the weight stream starts with the first request, and the first MFMA waits
    for little more than the bias and its own w[0], x0[0] (22 of the 25 loads still in flight with the compiler this was written on;
    at least 20 is what the property needs: a wait that drains the queue would be vmcnt(0))"""
    lines = asm("decode.hip")
    body, loads, first_mfma = _head(lines, r"_ZN2vx25skinny16_relu_pack_kernelE")
    kinds = "".join("w" if " nt" in ln else "x" for ln in loads)
    assert kinds == "x" + "wxx" * 8, kinds
    waits = [ln for ln in body[:first_mfma] if ln.startswith("s_waitcnt") and "vmcnt" in ln]
    assert waits and int(re.search(r"vmcnt\((\d+)\)", waits[-1]).group(1)) >= 20, waits
    # the order of rounds 2 .. 34 under the old switch: all of x, then the weights
    _, old, _ = _head(lines, r"_ZN2vx32skinny16_relu_pack_xfirst_kernelE")
    assert "".join("w" if " nt" in ln else "x" for ln in old) == "x" * 17 + "w" * 8
