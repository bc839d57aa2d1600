"""Structural pin of the variant oracle to the reference's own code (CPU, no GPU); mirrors
``tests/test_hgru_structure.py``.

``tools/extract_hgru.py`` evaluates the reference's ``ContextualCircuit`` method bodies
(``hgru_module.py:9-959``) symbolically under each named variant's aux; the variant oracle
(``tests/hgru_variants_ref.py``) is run on symbolic tensors and every step's O_t and I_t are
compared by Merkle hash.  Also pinned: the initial I draw is a free input of O_T exactly for the
variants that read the previous I, and the variables the reference creates for an aux are the
facade's table for it.

``selu`` / ``leaky_relu`` have no op in ``tests/symbolic.py``: both sides build an opaque named node
for them, which pins where they are applied; their numerics are restated from TensorFlow's
documentation and unpinned (tests/hgru_variants_ref.py).

Where /root/reference is absent (the GPU box), the committed digests
(``tests/golden/hgru_variants_digest.json``, written by ``--regen`` below from the reference)
stand in for it.
"""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import hgru_variant_cases as C  # noqa: E402
import hgru_variants_ref as V  # noqa: E402
import symbolic as S  # noqa: E402
from oracle import hgru_ref as R  # noqa: E402
from test_hgru_structure import SymWeights, _pkg  # noqa: E402

DIGEST = os.path.join(ROOT, "tests", "golden", "hgru_variants_digest.json")
HAVE_REF = os.path.exists("/root/reference/hgru_module.py")
CASE = (2, 16, 32, 5, C.T)            # n, h, w, ssf, timesteps; hidden_init 'random'
HIDDEN_CASES = [("defaults", "zeros"), ("defaults", "identity"), ("mely_gru", "identity")]
SCOPE = "contextual_circuit"


@pytest.fixture
def symbolic_oracle(monkeypatch):
    monkeypatch.setattr(R, "conv2d_same", lambda x, w, stride=1: S.conv2d(x, w, stride, "SAME"))
    monkeypatch.setattr(R, "sigmoid", S.sigmoid)
    return V


def _key(name, hidden_init="random"):
    return name if hidden_init == "random" else f"{name}_{hidden_init}"


def _table(name):
    M = _pkg().hgru_module
    flags = M.variable_flags(M.merged_aux(C.VARIANTS[name]))
    return _pkg().weights.hgru_circuit_vars(k=64, ssf=CASE[3], timesteps=CASE[4], scope=SCOPE, **flags)


def oracle_circuit(V_, name, hidden_init, o0_name, i0_name):
    n, h, w, ssf, T = CASE
    X = S.inp("X", (n, h, w, 64))
    O0 = R.hidden_init_state(X, hidden_init, S.inp(o0_name, (n, h, w, 64)))
    I0 = R.hidden_init_state(X, hidden_init, S.inp(i0_name, (n, h, w, 64)))      # made like O0, 875-890
    return V_.variant_forward(X, O0, I0, SymWeights(_table(name)), C.VARIANTS[name], T, scope=SCOPE,
                              keep_steps=True)


def reference_digests():
    """{key: digest} of the reference's own expressions (needs /root/reference)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import extract_hgru as E
    n, h, w, ssf, T = CASE
    out = {}
    for name, hi in [(nm, "random") for nm in C.VARIANTS] + HIDDEN_CASES:
        it, res, circ = E.circuit(n, h, w, ssf, T, hidden_init=hi, store_states=True,
                                  aux_overrides=C.VARIANTS[name], pose_aux=False)
        O, weights, _ = res
        assert O.op == "transpose" and O.args[1] == (1, 0, 2, 3, 4), "store_states stacks [n, T, ...]"
        o_steps = O.args[0].args[0]
        i_steps = weights["store_I"].items
        out[_key(name, hi)] = dict(
            O_stack=[s.h for s in o_steps], I_stack=[s.h for s in i_steps],
            o0_input=f"rand#{it.rand_count - 1}", i0_input=f"rand#{it.rand_count - 2}",
            free=sorted(S.free_inputs(o_steps[-1])), weights=sorted(it.weights))
        it2, res2, _ = E.circuit(n, h, w, ssf, T, hidden_init=hi, store_states=False,
                                 aux_overrides=C.VARIANTS[name], pose_aux=False)
        assert res2[0].h == o_steps[-1].h
    return out


def _digest():
    with open(DIGEST) as f:
        return json.load(f)


@pytest.mark.parametrize("name,hidden_init", [(nm, "random") for nm in C.VARIANTS] + HIDDEN_CASES,
                         ids=lambda v: v)
def test_variant_oracle_matches_reference_structure(symbolic_oracle, name, hidden_init):
    d = _digest()[_key(name, hidden_init)]
    O, I, steps, isteps = oracle_circuit(symbolic_oracle, name, hidden_init, d["o0_input"], d["i0_input"])
    T = CASE[4]
    # DEFECT 13 (tests/test_hgru_structure.py): the reference's two TensorArrays trade places every
    # step, so its stacked "O" holds O_t where T-1-t is even and I_t elsewhere
    want_o = [(steps[t] if (T - 1 - t) % 2 == 0 else isteps[t]).h for t in range(T)]
    want_i = [(isteps[t] if (T - 1 - t) % 2 == 0 else steps[t]).h for t in range(T)]
    assert want_o == d["O_stack"], "per-step O_t / I_t differ from the reference's graph"
    assert want_i == d["I_stack"], "per-step I_t / O_t differ from the reference's graph"
    assert O.h == d["O_stack"][-1]
    assert sorted(S.free_inputs(O)) == d["free"]
    if hidden_init == "random":
        # the initial I draw reaches O_T exactly for the variants that read the previous I
        live = V.reads_previous_i(C.VARIANTS[name])
        assert (d["i0_input"] in d["free"]) == live
        assert live == _pkg().hgru_module.reads_previous_i(_pkg().hgru_module.merged_aux(C.VARIANTS[name]))
        assert d["o0_input"] in d["free"]


@pytest.mark.parametrize("name", list(C.VARIANTS))
def test_variable_set_is_the_facades_table(name):
    """the variables the reference's prepare_tensors creates for the aux are the facade's table"""
    d = _digest()[name]
    assert set(d["weights"]) == {v.name for v in _table(name)}


@pytest.mark.skipif(not HAVE_REF, reason="/root/reference not present (GPU box): digest only")
def test_digest_is_the_reference():
    assert reference_digests() == _digest()


if __name__ == "__main__" and "--regen" in sys.argv:
    json.dump(reference_digests(), open(DIGEST, "w"), indent=1, sort_keys=True)
    print("wrote", DIGEST)
