"""GPU: the validation pass on the device -- MonkeyDetector.relative_labels_device /
calculateCoMfrom3DJoints, pose_evaluation.PoseEvaluator and the metric functions on CUDA tensors,
train_cnn_networks_hgru.prepare_data / ValidationPipeline / evaluate_tfrecord -- against the host
functions of the same package (which tests/test_eval_cpu.py pins to the reference and to numpy).

Per-frame values and counts are compared with np.array_equal(..., equal_nan=True): the device runs
numpy's float32 operations in numpy's order.  The float64 means over frames are compared within
1e-12 relative (n * 2^-53 for a sum of n <= 4096 non-negative doubles), and the mean error within
32 * 2^-24 relative of the float32 getMeanError_np (the float32 pairwise-sum bound for <= 4096
frames)."""
import warnings

import numpy as np
import pytest
import torch

from helpers import pkg

CAM = (365.456, 365.456, 256, 212, [800, 800, 1200], 200, 10000)
SCALE = (424, 512, 10000.)
F64_TOL = 1e-12
F32_MEAN_TOL = 32 * 2.0 ** -24
ERROR_CASES = [(1, 1), (3, 7), (5, 8), (4, 9), (7, 23), (2, 36), (3, 128), (257, 23), (1025, 23)]


def _md():
    return pkg().monkeydetector.MonkeyDetector(*CAM)


def _np_dist(lab, res):
    return pkg().pose_evaluation._joint_dist(lab, res)


def _np_frame_stats(dist):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # all-NaN rows
        return np.nanmean(dist, axis=1), np.nanmax(dist, axis=1)


def _just_above_five():
    """a float32 dz with sqrt(((3 * 3) + (4 * 4)) + dz * dz) == nextafter(5, inf) under numpy"""
    target = np.nextafter(np.float32(5), np.float32(np.inf))
    for dz in np.linspace(2.0e-3, 3.0e-3, 101, dtype=np.float32):
        d = _np_dist(np.array([[[3, 4, dz]]], np.float32), np.zeros((1, 1, 3), np.float32))
        if d[0, 0] == target:
            return dz
    raise AssertionError("no dz found")


def _error_inputs(n, J, seed):
    """labels / results [n, J, 3] float32 in mm with the edge rows the shape has room for"""
    rs = np.random.RandomState(seed)
    lab = rs.uniform(-500, 500, (n, J, 3)).astype(np.float32)
    res = (lab + rs.normal(0, 12, lab.shape)).astype(np.float32)
    if n >= 2 and J >= 2:
        res[0, J - 1, 1] = np.nan                  # a NaN joint (in the J % 8 tail)
        res[n - 1, 0, 0] = np.nan                  # and one in the first block of 8
    if n >= 3:
        lab[1] = np.nan                            # an all-NaN frame
        res[2] = lab[2]                            # labels equal to results: every distance 0
    if n >= 5:
        lab[3] = np.round(lab[3])
        res[3] = lab[3] + np.array([3, 4, 0], np.float32)        # every distance exactly 5.0
        lab[4] = np.round(lab[4])
        res[4] = lab[4] + np.array([3, 4, 0], np.float32)
        lab[4, 0] = 0
        res[4, 0] = np.array([3, 4, _just_above_five()], np.float32)   # one joint one step above 5.0
    return lab, res


def _check_against_numpy(ev_summary, frame_errors, lab, res, J):
    pe = pkg().pose_evaluation
    n = lab.shape[0]
    dist = _np_dist(lab, res)
    fmean, fmax = _np_frame_stats(dist)
    if frame_errors is not None:
        d, fm, fx = [t.cpu().numpy() for t in frame_errors]
        assert d.dtype == np.float32 and d.shape == (n, J)
        assert np.array_equal(d, dist, equal_nan=True)
        assert np.array_equal(fm, fmean, equal_nan=True)
        assert np.array_equal(fx, fmax, equal_nan=True)
    s = ev_summary
    assert s["frames"] == n and s["valid_frames"] == int((~np.isnan(fmean)).sum())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # nan* of all-NaN rows
        wmax = np.array([pe.getNumFramesWithinMaxDist(lab, res, t) / float(n) * 100. for t in range(100)])
        wmean = np.array([pe.getNumFramesWithinMeanDist(lab, res, t) / float(n) * 100. for t in range(100)])
    assert np.array_equal(s["within_max"], wmax) and np.array_equal(s["within_mean"], wmean)
    assert np.array_equal(np.rint(s["within_max"] * n / 100.), [(fmax <= t).sum() for t in range(100)])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        assert s["max_error"] == float(pe.getMaxError_np(lab, res))
        ref_mean = np.nanmean(fmean.astype(np.float64))
        ref_joint = np.nanmean(dist.astype(np.float64), axis=0)
        np32 = float(pe.getMeanError_np(lab, res))
    print(n, J, "mean_error", s["mean_error"], "float64 numpy", ref_mean, "float32 numpy", np32)
    assert abs(s["mean_error"] - ref_mean) <= F64_TOL * abs(ref_mean)
    assert np.array_equal(np.isnan(s["joint_mean"]), np.isnan(ref_joint))
    ok = ~np.isnan(ref_joint)
    assert np.all(np.abs(s["joint_mean"][ok] - ref_joint[ok]) <= F64_TOL * np.abs(ref_joint[ok]))
    assert abs(s["mean_error"] - np32) <= F32_MEAN_TOL * abs(np32)
    return dist, fmean, fmax


# ---------------------------------------------------------------- relative labels
def _on_boundary(c, target):
    lab = np.float32(c + target)
    for _ in range(64):
        d = np.float32(lab - c)
        if d == target:
            return lab
        lab = np.nextafter(lab, np.float32(np.inf) if d < target else np.float32(-np.inf))
    return None


@pytest.mark.gpu
@pytest.mark.parametrize("J", [23, 1])
def test_relative_labels_match_host(J):
    md = _md()
    n = 3
    rs = np.random.RandomState(3 + J)
    coms = np.array([[255.46593644951234, 200.2, 1500.1], [100.5, 300.25, 2345.678], [256.0, 212.0, 600.0]],
                    np.float64)
    c = md.uvdtoxyz(coms)                                         # float32 [3, 3]
    lab = (c[:, None, :] + rs.uniform(-700, 700, (n, J, 3))).astype(np.float32)
    lab[0, 0] = c[0]                                              # a label equal to the CoM xyz
    hits = 0
    for k in range(3):                                            # exactly on the boundary, then beyond it
        b = _on_boundary(c[1, k], np.float32(600. if k != 1 else -600.))
        if b is not None:
            lab[1, J - 1, k] = b
            hits += 1
    assert hits >= 2
    lab[2, J // 2] = c[2] + np.array([650., -650., np.nan], np.float32)   # clipped high, low, and a NaN
    host = md.relative_labels(lab, coms)
    assert host.dtype == np.float32 and (host == 1).any() and (host == -1).any() and np.isnan(host).sum() == 1
    assert not host[0, :3].any()
    got = md.relative_labels_device(torch.from_numpy(lab).cuda(), torch.from_numpy(coms).cuda())
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, 3 * J) and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), host, equal_nan=True)
    # [n, 3J] labels with num_joints, and a given output tensor
    out = torch.empty((n, 3 * J), dtype=torch.float32, device="cuda")
    got2 = md.relative_labels_device(torch.from_numpy(lab.reshape(n, 3 * J)).cuda(), torch.from_numpy(coms).cuda(),
                                     out=out, num_joints=J)
    assert got2.data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy(), host, equal_nan=True)


@pytest.mark.gpu
@pytest.mark.parametrize("J", [1, 23, 36])
def test_com_from_joints_matches_host(J):
    md = _md()
    rs = np.random.RandomState(J)
    j = np.concatenate([rs.uniform(-400, 400, (5, J, 2)), -rs.uniform(700, 2500, (5, J, 1))], axis=2).astype(np.float32)
    j[3, :, 2] = 0.0                                              # a joint mean of z == 0
    for scale in (SCALE, None):
        host = md.calculateCoMfrom3DJoints(j, scale=scale)
        got = md.calculateCoMfrom3DJoints_device(torch.from_numpy(j).cuda(), scale=scale)
        assert got.dtype == torch.float32 and tuple(got.shape) == (5, 3) and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), host, equal_nan=True)
        assert not np.isfinite(host[3, :2]).any()


# ---------------------------------------------------------------- joint errors
@pytest.mark.gpu
@pytest.mark.parametrize("case", ERROR_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_joint_errors_match_numpy(case):
    n, J = case
    pe = pkg().pose_evaluation
    lab, res = _error_inputs(n, J, 11 * n + J)
    ev = pe.PoseEvaluator(J)
    ev.update(torch.from_numpy(lab).cuda(), torch.from_numpy(res).cuda())
    dist, fmean, fmax = _check_against_numpy(ev.summary(), ev.last_frame_errors, lab, res, J)
    if n >= 5:
        above = np.nextafter(np.float32(5), np.float32(np.inf))
        assert fmax[3] == 5.0 and fmean[3] == 5.0 and fmax[4] == above and dist[4, 0] == above
        cnt = np.rint(ev.summary()["within_max"] * n / 100.)
        assert cnt[5] - cnt[4] >= 1                # frame 3 is within 5 mm (<=), not within 4
        assert cnt[5] == (fmax <= 5).sum() == (fmax < above).sum()       # frame 4 is not within 5 mm
    if n >= 3:
        assert np.isnan(fmean[1]) and np.isnan(fmax[1]) and fmean[2] == 0 and fmax[2] == 0


@pytest.mark.gpu
def test_metric_functions_on_cuda_tensors():
    pe = pkg().pose_evaluation
    lab, res = _error_inputs(7, 23, 5)
    L, R = torch.from_numpy(lab).cuda(), torch.from_numpy(res).cuda()
    dist = _np_dist(lab, res)
    fmean, fmax = _np_frame_stats(dist)
    ref = np.nanmean(fmean.astype(np.float64))
    for fn in (pe.getMeanError_np, pe.getMeanError_train):
        v = fn(L, R)
        assert isinstance(v, np.float64) and abs(v - ref) <= F64_TOL * ref
    assert pe.getMaxError_np(L, R) == pe.getMaxError(L, R) == float(np.nanmax(dist))
    per = pe.getMeanErrors_N(L, R)
    assert per.dtype == torch.float64 and np.array_equal(per.cpu().numpy(), fmean.astype(np.float64), equal_nan=True)
    assert pe.getMeanError(L[0], R[0]) == float(fmean[0])
    for t in (0, 5, 20, 60):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)      # numpy on the all-NaN frame
            want_max = pe.getNumFramesWithinMaxDist(lab, res, t)
            want_mean = pe.getNumFramesWithinMeanDist(lab, res, t)
        assert pe.getNumFramesWithinMaxDist(L, R, t) == want_max
        assert pe.getNumFramesWithinMeanDist(L, R, t) == want_mean
    jm = np.nanmean(dist[:, 4].astype(np.float64))
    assert abs(pe.getJointMeanError(L, R, 4) - jm) <= F64_TOL * jm
    assert abs(pe.getMean_np(L[:, 4], R[:, 4]) - jm) <= F64_TOL * jm
    # calc_com_error: one joint per frame
    T = pkg().train_cnn_networks_hgru
    a, b = lab[:, 5, :], res[:, 5, :]
    ce = float(np.nanmean(np.sqrt(np.square(a - b).sum(axis=1)).astype(np.float64)))
    assert abs(T.calc_com_error(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()) - ce) <= F64_TOL * ce
    assert abs(ce - float(T.calc_com_error(a, b))) <= F32_MEAN_TOL * ce


@pytest.mark.gpu
def test_normalised_inputs_equal_the_host_chain():
    """inputs normalised by cube_z / 2 with scale = 600: the reference's ``x * cube_z / 2.``"""
    pe = pkg().pose_evaluation
    lab, res = _error_inputs(7, 23, 9)
    ln, rn = (lab / np.float32(600)).astype(np.float32), (res / np.float32(600)).astype(np.float32)
    lh, rh = (ln * np.float32(1200)) / np.float32(2.), (rn * np.float32(1200)) / np.float32(2.)
    assert lh.dtype == np.float32
    ev = pe.PoseEvaluator(23)
    ev.update(torch.from_numpy(ln).cuda(), torch.from_numpy(rn).cuda(), scale=600.0)
    _check_against_numpy(ev.summary(), ev.last_frame_errors, lh, rh, 23)
    # [n, 3J] input is the same input
    ev2 = pe.PoseEvaluator(23)
    ev2.update(torch.from_numpy(ln.reshape(7, 69)).cuda(), torch.from_numpy(rn.reshape(7, 69)).cuda(), scale=600.0)
    assert ev2.summary_array().tobytes() == ev.summary_array().tobytes()


@pytest.mark.gpu
def test_streaming_batches_equal_the_whole_array():
    pe = pkg().pose_evaluation
    lab, res = _error_inputs(263, 23, 21)
    L, R = torch.from_numpy(lab).cuda(), torch.from_numpy(res).cuda()

    def run():
        ev = pe.PoseEvaluator(23)
        lo = 0
        for b in (5, 1, 257):
            ev.update(L[lo:lo + b], R[lo:lo + b])
            lo += b
        return ev, ev.summary_array()

    ev, a = run()
    _check_against_numpy(ev.summary(), None, lab, res, 23)
    assert tuple(ev.last_frame_errors[0].shape) == (257, 23)
    ev2, b = run()
    assert a.tobytes() == b.tobytes()
    assert ev._state.cpu().numpy().tobytes() == ev2._state.cpu().numpy().tobytes()
    # the float64 sums run in frame order: one batch of all 263 frames leaves the same bytes
    whole = pe.PoseEvaluator(23)
    whole.update(L, R)
    assert whole.summary_array().tobytes() == a.tobytes()
    # reset starts over
    ev.reset()
    ev.update(L[:5], R[:5])
    _check_against_numpy(ev.summary(), ev.last_frame_errors, lab[:5], res[:5], 23)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [0, 1, 256, 257, 1024])
def test_threshold_counts_for_many_thresholds(T):
    """the reset passes 256 thresholds per launch and every block of the accumulate owns 256: the
    sizes on both sides of those boundaries, fractional thresholds, and none at all"""
    pe = pkg().pose_evaluation
    lab, res = _error_inputs(37, 23, 13)
    thr = np.linspace(0.0, 60.0, T).astype(np.float32) if T > 1 else np.full(T, 12.5, np.float32)
    ev = pe.PoseEvaluator(23, thresholds=thr)
    ev.update(torch.from_numpy(lab).cuda(), torch.from_numpy(res).cuda())
    s = ev.summary()
    fmean, fmax = _np_frame_stats(_np_dist(lab, res))
    assert s["within_max"].shape == (T,) and np.array_equal(s["thresholds"], thr)
    assert np.array_equal(s["within_max"], (fmax[:, None] <= thr[None, :]).sum(axis=0) / float(37) * 100.)
    assert np.array_equal(s["within_mean"], (fmean[:, None] <= thr[None, :]).sum(axis=0) / float(37) * 100.)
    assert s["frames"] == 37 and s["max_error"] == float(np.nanmax(fmax))


# ---------------------------------------------------------------- prepare_data, the pipeline, a TFRecord
def _labels_around(md, n, J, seed):
    """labels [n, J, 3] in mm around the synthetic attention's CoM (212, 256, 1500 mm), +-700 mm"""
    c = md.uvdtoxyz(np.array([212., 256., 1500.]))
    rs = np.random.RandomState(seed)
    return (c + rs.uniform(-700, 700, (n, J, 3))).astype(np.float32)


@pytest.mark.gpu
def test_device_prepare_data_matches_host_and_keeps_status():
    P = pkg()
    T = P.train_cnn_networks_hgru
    md = _md()
    cfg = T.InferenceConfig()
    frames = P.weights.synth_frames(4, seed=5)
    tr = np.array([(0.5, 0.5, 0.15), (0.31, 0.77, 0.2), (0.5, 0.5, 0.0), (0.6, 0.3, 0.0731)], np.float32)
    lab = _labels_around(md, 4, 23, 2)
    good = [0, 1, 3]
    hp, hr = T.prepare_data(frames[good], lab[good], tr[good], md, cfg)
    fd, ld, td = torch.from_numpy(frames).cuda(), torch.from_numpy(lab).cuda(), torch.from_numpy(tr).cuda()
    patches, rel = T.prepare_data(fd, ld, td, md, cfg, check=False)          # a zero-depth CoM: status 1
    assert md.last_status.cpu().numpy().tolist() == [0, 0, 1, 0]
    assert np.array_equal(patches.cpu().numpy()[good], hp)
    assert np.array_equal(rel.cpu().numpy()[good], hr)
    assert tuple(rel.shape) == (4, 69) and np.isfinite(rel.cpu().numpy()).all()
    with pytest.raises(P._lib.MonkeyPoseError):
        T.prepare_data(fd, ld, td, md, cfg)


@pytest.fixture(scope="module")
def models():
    P = pkg()
    W, T = P.weights, P.train_cnn_networks_hgru
    attn = T.attn_model_struct()
    attn.load_weights(W.attn_synth_weights(seed=1234))
    pose = T.cnn_model_struct()
    pose.load_weights(W.synth_weights(W.cnn_vars(output_shape=69, crop=128), seed=77))
    return attn, pose


def _host_validation(md, out, coms, com_norm, lab):
    """the host evaluation the pipeline replaces: label half of prepare_data, numpy metrics"""
    rel = md.relative_labels(lab, coms)
    half = np.float32(md.cube[2] / 2.)
    n = lab.shape[0]
    L, R = (rel * half).reshape(n, -1, 3), (out * half).reshape(n, -1, 3)
    com2d = md.calculateCoMfrom3DJoints(lab, scale=SCALE)
    return rel, L, R, com2d[:, None, :], com_norm[:, None, :]


@pytest.mark.gpu
def test_validation_pipeline_matches_host_chain(models):
    P = pkg()
    T = P.train_cnn_networks_hgru
    attn, pose = models
    md = _md()
    frames = P.weights.synth_frames(4, seed=5)
    frames[2] = 0.0            # an all-zero depth frame: it crops like the others (the status follows the CoM)
    lab = _labels_around(md, 4, 23, 4)
    fd, ld = torch.from_numpy(frames).cuda(), torch.from_numpy(lab.reshape(4, 69)).cuda()
    out0, coms0, Ms0 = T.FramePosePipeline(attn, pose, md, check_crops=False).run(fd)
    status0 = md.last_status.cpu().numpy().copy()
    out0, coms0, Ms0 = out0.cpu().numpy(), coms0.cpu().numpy(), Ms0.cpu().numpy()
    com_norm = attn.out_put.cpu().numpy()
    pipe = T.ValidationPipeline(attn, pose, md, check_crops=False)
    out, rel, coms, Ms = pipe.run(fd, ld)
    assert np.array_equal(md.last_status.cpu().numpy(), status0)  # every frame keeps its status
    assert np.array_equal(out.cpu().numpy(), out0) and np.array_equal(coms.cpu().numpy(), coms0)
    assert np.array_equal(Ms.cpu().numpy(), Ms0)
    hrel, L, R, c_lab, c_res = _host_validation(md, out0, coms0, com_norm, lab)
    assert np.array_equal(rel.cpu().numpy(), hrel)
    assert (hrel == 1).any() and (hrel == -1).any()
    s = pipe.summary()
    _check_against_numpy(s["pose"], pipe.pose_eval.last_frame_errors, L, R, 23)
    _check_against_numpy(s["com"], pipe.com_eval.last_frame_errors, c_lab, c_res, 1)
    ce = float(T.calc_com_error(c_lab[:, 0], c_res[:, 0]))
    assert abs(s["com"]["mean_error"] - ce) <= F32_MEAN_TOL * ce
    # a second batch accumulates; reset starts over
    pipe.run(fd, ld)
    assert pipe.summary()["pose"]["frames"] == 8
    pipe.reset()
    pipe.run(fd, torch.from_numpy(lab).cuda())                    # [n, J, 3] labels
    s2 = pipe.summary()
    assert s2["pose"]["frames"] == 4 and s2["pose"]["mean_error"] == s["pose"]["mean_error"]
    assert np.array_equal(s2["pose"]["within_mean"], s["pose"]["within_mean"])


@pytest.mark.gpu
def test_validation_pipeline_failed_crops_keep_their_status(models):
    """A crop's status is a function of the attention CoM alone (an all-zero depth frame under a
    sound CoM crops with status 0, see the test above), so the failing frames come from an attention
    net whose depth output is negative: with check_crops=False the batch runs through, every frame
    keeps its non-zero status and is still counted; with check_crops=True the run raises."""
    P = pkg()
    W, T = P.weights, P.train_cnn_networks_hgru
    _, pose = models
    md = _md()
    w = W.attn_synth_weights(seed=1234)
    w["cnn/afc_out/afc_out_biases"] = np.array([0.5, 0.5, -0.15], np.float32)
    bad = T.attn_model_struct()
    bad.load_weights(w)
    frames = P.weights.synth_frames(2, seed=5)
    fd = torch.from_numpy(frames).cuda()
    ld = torch.from_numpy(_labels_around(md, 2, 23, 4)).cuda()
    pipe = T.ValidationPipeline(bad, pose, md, check_crops=False)
    out, rel, coms, Ms = pipe.run(fd, ld)
    assert (md.last_status.cpu().numpy() != 0).all()
    assert np.all(coms.cpu().numpy()[:, 2] < 0) and np.isfinite(out.cpu().numpy()).all()
    s = pipe.summary()
    assert s["pose"]["frames"] == 2 and s["com"]["frames"] == 2
    with pytest.raises(P._lib.MonkeyPoseError):
        T.ValidationPipeline(bad, pose, md, check_crops=True).run(fd, ld)


@pytest.mark.gpu
def test_evaluate_tfrecord_equals_evaluator_fed_the_batches(models, tmp_path):
    P = pkg()
    T, DL, pe = P.train_cnn_networks_hgru, P.data_loader, P.pose_evaluation
    attn, pose = models
    md = _md()
    frames_mm = P.weights.synth_frames(6, seed=8) * np.float32(10000.)
    lab = _labels_around(md, 6, 23, 6).reshape(6, 69)
    path = str(tmp_path / "val.tfrecord")
    DL.create_tf_record(frames_mm, lab, path)
    pipe = T.ValidationPipeline(attn, pose, md)
    s = T.evaluate_tfrecord(path, pipe, batch_size=2)
    assert s["pose"]["frames"] == 6 and s["com"]["frames"] == 6
    two = T.evaluate_tfrecord(path, pipe, batch_size=2, max_batches=2)
    assert two["pose"]["frames"] == 4
    ev, cev = pe.PoseEvaluator(23), pe.PoseEvaluator(1)
    pipe2 = T.ValidationPipeline(attn, pose, md)
    for i in range(0, 6, 2):
        fd = torch.from_numpy(frames_mm[i:i + 2]).cuda() / 10000.0
        ld = torch.from_numpy(lab[i:i + 2]).cuda()
        out, rel, _, _ = pipe2.run(fd, ld)
        ev.update(rel, out, scale=600.0)
        cev.update(md.calculateCoMfrom3DJoints(ld.reshape(2, 23, 3), scale=SCALE)[:, None, :],
                   attn.out_put[:, None, :])
    for key, e in (("pose", ev), ("com", cev)):
        r = e.summary()
        assert r["frames"] == 6
        for k in ("valid_frames", "mean_error", "max_error"):
            assert s[key][k] == r[k], (key, k)
        for k in ("joint_mean", "within_max", "within_mean"):
            assert np.array_equal(s[key][k], r[k]), (key, k)
    assert np.isfinite(s["pose"]["mean_error"]) and s["pose"]["mean_error"] > 0
