"""CPU: the conditions the GPU channel tests (tests/test_gpu_circuit_channels.py) rest on, from the case
table and the oracle alone: the table covers what it claims, the float32 oracle's own error leaves the
1e-5 floor as the operative fp32-class bound (ten times inside the 1e-4 gate), ``resolve_dtype`` knows
the channel count, the facade sizes its variables from k, and the oracle's images are independent."""
import numpy as np
import pytest

import circuit_channel_cases as C
import circuit_shape_cases as S
import hgru_variant_cases as HV
from helpers import FP32_REL_TOL, pkg


def test_case_table_is_well_formed_and_covers_its_claims():
    assert len({C.case_id(c) for c in C.CASES}) == len(C.CASES)
    for c in C.CASES:
        assert c.dtype in ("fp32_split", "fp32") and c.ssf in (3, 5, 15), c
        assert 4 <= c.k <= 256 and c.n >= 1 and c.h >= 1 and c.w >= 1, c
        assert c.variant in HV.VARIANTS, c
        assert (c.k == 64) == c.nhwc_loop, c        # 64 channels reach the loop by the flag only
    ks = {c.k for c in C.CASES}
    assert any(k % 4 for k in ks) and any(k < 16 for k in ks) and any(k > 64 for k in ks)
    assert min(ks) == 4 and max(ks) == 128
    assert any(c.h < c.ssf and c.w < c.ssf for c in C.CASES)           # a map smaller than its filter
    assert any(c.w % 32 and c.h % 16 for c in C.CASES)
    assert {c.dtype for c in C.CASES} == {"fp32_split", "fp32"}
    assert {c.ssf for c in C.CASES if c.dtype == "fp32_split"} == {3, 5, 15}
    assert any(c.k % 4 for c in C.CASES if c.dtype == "fp32")
    flags = [C.derived_flags(c.variant) for c in C.CASES]
    for f in flags[0]:                                                 # every derived flag on and off
        assert {d[f] for d in flags} == {False, True}, f
    assert {C.aux_of(c.variant)['integration_type'] for c in C.CASES} >= {"alternate", "mely"}
    assert {C.aux_of(c.variant)['recurrent_nl'] for c in C.CASES} >= {"tanh", "relu"}
    # the 64-channel case is one the 64-channel tilings reject
    c64 = [c for c in C.CASES if c.nhwc_loop]
    assert c64 and not any(S.map_ok(d, c64[0].h, c64[0].w) for d in ("fp32", "fp32_split", "fp32_fft"))
    assert C.REUSE_SEQUENCE[0] == C.REUSE_SEQUENCE[-1] and len(set(C.REUSE_SEQUENCE)) == 3
    assert {r[-1] for r in C.REJECTED} == {C.MP_ERR_WEIGHT, C.MP_ERR_UNSUPPORTED}


@pytest.mark.parametrize("c", C.CASES, ids=C.case_id)
def test_float32_oracle_is_ten_times_inside_the_gate(c):
    """the condition that makes max(10 * e32, 1e-5) a bound the 1e-4 gate does not already imply"""
    O, I, so, si = C.oracle(*C.shape_of(c), c.variant)
    assert O.dtype == np.float64 and O.shape == (c.n, c.h, c.w, c.k)
    for a in (O, I, *so, *si):
        assert np.isfinite(a).all() and np.abs(a).max() > 1e-2
    e = C.e32(*C.shape_of(c), c.variant)
    print(C.case_id(c), "e32 O", ["%.2e" % v for v in e["O"]], "I", ["%.2e" % v for v in e["I"]])
    for v in e["O"] + e["I"]:
        assert 10 * v <= FP32_REL_TOL, (c, v)
        assert S.fp32_class_bound(v) <= FP32_REL_TOL / 10


def test_variant_moves_the_oracle():
    """a case cannot pass with its variant's flag ignored"""
    for c in C.CASES:
        if c.variant != "pose":
            a = C.oracle(*C.shape_of(c), c.variant)[0]
            b = C.oracle(*C.shape_of(c), "pose")[0]
            assert np.abs(a - b).max() >= 1e-2 * np.abs(a).max(), c


def test_resolve_dtype_knows_the_channel_count():
    L = pkg()._lib
    for h, w in [(64, 64), (7, 9), (32, 32), (20, 28)]:
        for k in (4, 25, 128):
            assert L.resolve_dtype('auto', h, w, k) == 'fp32_split'
            assert L.resolve_dtype('fp32', h, w, k) == 'fp32'
            assert L.resolve_dtype('fp32_split', h, w, k=k) == 'fp32_split'
            for name in ('fp32_fft', 'bf16'):
                with pytest.raises(ValueError, match=str(k)):
                    L.resolve_dtype(name, h, w, k)
        assert L.resolve_dtype('auto', h, w, 64, nhwc_loop=True) == 'fp32_split'
        with pytest.raises(ValueError, match="64"):
            L.resolve_dtype('fp32_fft', h, w, 64, True)
        assert L.resolve_dtype('auto', h, w, 64) == L.resolve_dtype('auto', h, w)     # 64 channels: as before
    assert L.resolve_dtype('auto', 64, 64) == 'fp32_fft' and L.resolve_dtype('auto', 20, 28) == 'fp32'
    assert "mp_circuit_set_nhwc_loop" in L._SIGS


def test_facade_sizes_its_variables_from_k():
    M = pkg().hgru_module
    cc = M.ContextualCircuit(np.zeros((2, 7, 9, 25), np.float32), timesteps=C.T, SSF=15)
    shapes = {v.name.split("/")[-1]: tuple(v.shape) for v in cc.variable_table()}
    assert cc.k == 25 and shapes["p_r"] == (15, 15, 25, 25)
    assert shapes["i_r"] == shapes["o_r"] == (1, 1, 25, 25)
    for nm in ("i_b", "o_b", "beta", "nu", "gamma", "kappa", "omega", "lateral_bias"):
        assert shapes[nm] == (1, 1, 1, 25), nm
    w = cc.prepare_tensors()
    assert all(w[v.name].shape == tuple(v.shape) for v in cc.variable_table())


def test_oracle_images_are_independent():
    k, h, w, ssf, variant = C.BATCH
    X, O0, I0 = C.inputs(k, 3, h, w)
    whole = C.oracle(k, 3, h, w, ssf, variant)
    for i in range(3):
        one = C.oracle(k, i + 1, h, w, ssf, variant)      # images 0 .. i: the inputs are a prefix
        assert np.array_equal(C.inputs(k, i + 1, h, w)[0], X[:i + 1])
        assert np.array_equal(one[0][i], whole[0][i]) and np.array_equal(one[1][i], whole[1][i])
    import hgru_variants_ref as V
    wts = {n: a.astype(np.float64) for n, a in C.weights(k, ssf).items()}
    for i in range(3):
        O, I = V.variant_forward(X[i:i + 1].astype(np.float64), O0[i:i + 1].astype(np.float64),
                                 I0[i:i + 1].astype(np.float64), wts, C.aux_of(variant), C.T, scope=C.SCOPE)
        assert np.array_equal(O[0], whole[0][i]) and np.array_equal(I[0], whole[1][i])
