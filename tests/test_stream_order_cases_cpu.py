"""CPU: the table of tests/stream_order_cases.py is complete.  Every function include/monkeypose.h
declares with a stream argument is classified exactly once -- ordered (with the GPU cases that hold it to
that), synchronous (with the reason) or diagnostic -- so a new export with a stream argument fails here until
someone classifies it; and every case has two different input sets and declares its outputs."""
import numpy as np

import stream_order_cases as SO

# the exports with a stream argument when this table was written: parsing the header finds at least these
KNOWN = {"mp_hgru_pose_fwd", "mp_hgru_pose_fwd_ex", "mp_hgru_pose_fwd_taps", "mp_hgru_circuit_fwd",
         "mp_hgru_circuit_fwd_ex", "mp_hgru_circuit_fwd_opts", "mp_hgru_circuit_fwd_var", "mp_dense_fwd", "mp_hier_fwd",
         "mp_attn_fwd", "mp_resize_bilinear", "mp_graph_fwd", "mp_crop3d_dev", "mp_crop3d_dev_ex",
         "mp_center_of_mass_dev", "mp_crop3d_dev_coms", "mp_center_of_mass_dev_dt", "mp_crop3d_dev_coms_dt",
         "mp_real_frames_dev", "mp_abs_joints_dev", "mp_rel_labels_dev", "mp_com_from_joints_dev", "mp_eval_reset_dev",
         "mp_eval_accumulate_dev", "mp_eval_summary_dev", "mp_overlay_dev", "mp_transform_joints_dev"}


def test_the_parser_finds_the_stream_prototypes():
    found = SO.stream_prototypes()
    assert len(found) == len(set(found))
    assert KNOWN <= set(found), sorted(KNOWN - set(found))


def test_the_parser_sees_a_new_export(tmp_path):
    with open(SO.HEADER) as f:
        text = f.read()
    marker = "int mp_info("
    assert marker in text
    new = "/* new */\nint mp_new_thing_dev(const float* x, int64_t n,\n                     float* out, void* stream);\n"
    p = tmp_path / "monkeypose.h"
    p.write_text(text.replace(marker, new + marker))
    found = SO.stream_prototypes(str(p))
    assert "mp_new_thing_dev" in found
    classes = set(SO.ORDERED) | set(SO.SYNCHRONOUS) | set(SO.DIAGNOSTIC)
    assert [f for f in found if f not in classes] == ["mp_new_thing_dev"]


def test_every_stream_export_is_classified_once():
    classes = {"ordered": set(SO.ORDERED), "synchronous": set(SO.SYNCHRONOUS), "diagnostic": set(SO.DIAGNOSTIC)}
    for fn in SO.stream_prototypes():
        where = [k for k, v in classes.items() if fn in v]
        assert len(where) == 1, f"{fn}: classify it in tests/stream_order_cases.py (found under {where})"
    exported = set(SO.exported_functions())
    for k, v in classes.items():
        assert v <= exported, (k, sorted(v - exported))
    assert not (classes["ordered"] & classes["synchronous"]) and not (classes["ordered"] & classes["diagnostic"])
    assert not (classes["synchronous"] & classes["diagnostic"])
    for fn, why in {**SO.SYNCHRONOUS, **SO.DIAGNOSTIC}.items():
        assert isinstance(why, str) and why.strip(), fn


def test_an_ordered_export_names_its_gpu_cases():
    for fn, names in SO.ORDERED.items():
        assert names, fn
        for n in names:
            assert n in SO.CASES, (fn, n)
            assert fn in SO.CASES[n]().covers
    assert SO.CHILD_CASE in SO.CASES and all(n in SO.CASES for n in SO.TWO_CONTEXTS)


def test_case_names_are_unique():
    names = [c.name for c in SO.all_cases()]
    assert len(names) == len(set(names)) == len(SO.CASES)


def test_every_case_has_two_input_sets_and_declares_its_outputs():
    for c in SO.all_cases():
        A, B = c.make(SO.SEED_A), c.make(SO.SEED_B)
        assert A and set(A) == set(B), c.name
        for k in A:
            assert isinstance(A[k], np.ndarray) and A[k].shape == B[k].shape and A[k].dtype == B[k].dtype, (c.name, k)
            assert np.isfinite(np.asarray(A[k], np.float64)).all() and np.isfinite(np.asarray(B[k], np.float64)).all(), \
                (c.name, k, "stale inputs are valid inputs")
        assert all(A[k].tobytes() != B[k].tobytes() for k in A), c.name
        assert c.outputs and len(set(c.outputs)) == len(c.outputs), c.name
        assert set(c.may_coincide) < set(c.outputs), c.name
        assert c.covers, c.name


def test_the_delay_is_within_the_issue_limits():
    assert 50.0 <= SO.DELAY_MS <= 1000.0 and SO.DELAY_BYTES >= 256 << 20
