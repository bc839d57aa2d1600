"""Shared helpers for the parity tests: case inputs (regenerated from seeds) and error metrics."""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
import make_golden as MG  # noqa: E402

HGRU_POSE_AUX = {
    'recurrent_nl': 'tanh', 'rectify_weights': None, 'pre_batchnorm': False, 'gate_filter': 1,
    'xi': False, 'post_batchnorm': False, 'dense_connections': False, 'symmetric_weights': True,
    'symmetric_gate_weights': False, 'batch_norm': False, 'atrous_convolutions': False,
    'output_gru_gates': False, 'association_field': True, 'multiplicative_excitation': True,
    'gru_gates': True, 'gamma': True, 'adapation': True, 'trainable': True,
}

# fp32 parity gate of SURVEY.md 8d / BASELINE.md: ||out - ref||_inf / ||ref||_inf <= 1e-4
FP32_REL_TOL = 1e-4
# stated gates of the bf16 paths (bf16 cannot meet 1e-4): model outputs (pose, regressors;
# measured 6e-4 - 9e-4) and the raw per-step hGRU state maps, stored in bf16 (8-bit mantissa) and
# fed back through 8 steps without a head to average the rounding (measured up to 1.04e-2 of
# max|O_t|, 4.8e-3 on the circuit output)
BF16_REL_TOL = 5e-3
BF16_STATE_REL_TOL = 2e-2


def golden_meta():
    with open(os.path.join(GOLDEN, "golden.json")) as f:
        return json.load(f)


def golden_array(name, key):
    with np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False) as z:
        return z[key]


_REF_GRAPHS = {   # kind: (extract() arguments, attribute of tools/extract_dense_hier.py naming the source)
    "hier": (dict(heads=MG.HIER_HEADS), "REF_HIER"),
    "dense": (dict(heads=(69,)), "REF_DENSE"),
    "cnn": (dict(heads=(69,), cls="cnn_model_struct"), "REF_CNN"),
    "dense_hier": (dict(heads=MG.HIER_HEADS), "REF"),
}


def reference_graph(kind):
    """(ops, shapes) of the reference's ``kind`` regressor as tools/extract_dense_hier.py reads them
    from the reference's own build(): one record per op in build order (without the source line) and
    every tensor's static shape, as committed in tests/golden/<kind>_graph_ops.json.  Where the
    reference's sources are readable the extraction is run again and must equal the committed file."""
    with open(os.path.join(GOLDEN, f"{kind}_graph_ops.json")) as f:
        d = json.load(f)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import extract_dense_hier as X
    kw, src = _REF_GRAPHS[kind]
    if os.access(getattr(X, src), os.R_OK):
        ops, shapes = X.extract(path=getattr(X, src), **kw)
        assert [{k: v for k, v in o.items() if k != "line"} for o in ops] == d["ops"], kind
        assert shapes == d["shapes"], kind
    return d["ops"], d["shapes"]


def rel_inf(a, ref):
    a = np.asarray(a, np.float64)
    ref = np.asarray(ref, np.float64)
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30))


def pkg():
    return importlib.import_module("monkey-pose_amd")


if __name__ == "__main__" and "--regen-graphs" in sys.argv:   # needs the reference's sources
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import extract_dense_hier as X
    for kind, (kw, src) in _REF_GRAPHS.items():
        ops, shapes = X.extract(path=getattr(X, src), **kw)
        ops = [{k: v for k, v in o.items() if k != "line"} for o in ops]
        path = os.path.join(GOLDEN, f"{kind}_graph_ops.json")
        with open(path, "w") as f:   # one op per line
            f.write('{"source": %s,\n"ops": [\n' % json.dumps(
                f"tools/extract_dense_hier.py extract({kw}) on {os.path.basename(getattr(X, src))}"))
            f.write(",\n".join(json.dumps(o) for o in ops))
            f.write('\n],\n"shapes": %s}\n' % json.dumps(shapes))
        print("wrote", path, len(ops), "ops")
