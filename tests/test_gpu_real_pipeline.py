"""GPU: train_cnn_networks_hgru.RealDataPipeline / eval_model_on_real_data -- raw camera frames as
stored (uint16 [w, h]) to absolute joints on the device -- against the chain it replaces, built from
components that predate it: the host preprocess (numpy), an upload of the float32 frames, the existing
FramePosePipeline.run and getAbsoluteCoordinates_device.  Bit for bit (np.array_equal).

The attention net's afc_out weights are zero and its biases a chosen CoM, so com_norm is that CoM for
every frame and the crops are valid whatever the synthetic weights would have predicted.  Where one
frame has to fail, afc_out's depth column reads two of the net's own afc_1 features (taken from the
device through an identity head) so that the three frames get three chosen depths."""
import functools

import numpy as np
import pytest
import torch

from helpers import pkg
from oracle import crop_ref as CR

CAM = (365.456, 365.456, 256, 212, [800, 800, 1200], 200, 10000)
W_AFC = "cnn/afc_out/afc_out_weights"
B_AFC = "cnn/afc_out/afc_out_biases"


@functools.lru_cache(maxsize=None)
def _raw():
    """three recorded frames as stored: uint16 [512, 424]"""
    out = np.stack([np.ascontiguousarray(CR.synth_frame(s).astype(np.uint16).T) for s in range(3)])
    assert out.shape == (3, 512, 424)
    out.setflags(write=False)
    return out


def _md():
    return pkg().monkeydetector.MonkeyDetector(*CAM)


@functools.lru_cache(maxsize=None)
def _attn_base():
    return pkg().weights.attn_synth_weights(seed=1234)


def _attn(bias, wz=None, out=3):
    """attention net with afc_out = zero weights (or the given depth column) and the given biases"""
    P = pkg()
    w = dict(_attn_base())
    if out == 3:
        w[W_AFC] = np.zeros((1024, 3), np.float32)
        if wz is not None:
            w[W_AFC][:, 2] = wz
        w[B_AFC] = np.asarray(bias, np.float32)
    else:                                   # an identity head: the output is afc_1's (normalised) features
        w[W_AFC] = np.eye(1024, dtype=np.float32)
        w[B_AFC] = np.zeros(1024, np.float32)
    a = P.train_cnn_networks_hgru.attn_model_struct()
    a.load_weights(w)
    return a


@pytest.fixture(scope="module")
def pose():
    P = pkg()
    W = P.weights
    m = P.train_cnn_networks_hgru.cnn_model_struct()
    m.load_weights(W.synth_weights(W.cnn_vars(output_shape=69, crop=128), seed=77))
    return m


def _parent_chain(attn, pose, raw, check=True):
    """host preprocessing -> upload -> FramePosePipeline.run -> getAbsoluteCoordinates_device"""
    P = pkg()
    T = P.train_cnn_networks_hgru
    md = _md()
    frames = P.monkeydetector.preprocess_real_frames(np.asarray(raw))            # numpy: the host function
    fd = torch.from_numpy(frames).cuda()
    out, coms, Ms = T.FramePosePipeline(attn, pose, md, check_crops=check).run(fd)
    status = md.last_status.cpu().numpy().copy()
    com_norm = attn.out_put.cpu().numpy().copy()
    xyz, uvd = md.getAbsoluteCoordinates_device(out, coms, 23)
    return [t.cpu().numpy().copy() for t in (xyz, uvd, coms, Ms)] + [com_norm], status


def _np(res):
    return [t.cpu().numpy().copy() for t in res]


@pytest.mark.gpu
def test_real_pipeline_equals_the_chain_it_replaces(pose):
    T = pkg().train_cnn_networks_hgru
    bias = (0.5, 0.5, 0.13)                                   # com = (212, 256, 1300 mm)
    ref, status = _parent_chain(_attn(bias), pose, _raw())
    assert not status.any()
    assert np.array_equal(ref[4], np.tile(np.float32(bias), (3, 1)))
    md = _md()
    pipe = T.RealDataPipeline(_attn(bias), pose, md)
    rd = torch.from_numpy(_raw().copy()).cuda()
    res = pipe.run(rd)
    assert [tuple(t.shape) for t in res] == [(3, 23, 3), (3, 23, 3), (3, 3), (3, 3, 3), (3, 3)]
    assert [t.dtype for t in res] == [torch.float32, torch.float32, torch.float64, torch.float64, torch.float32]
    assert all(t.is_cuda for t in res)
    ptrs = [t.data_ptr() for t in res[:2]]
    got = _np(res)
    for name, g, r in zip(("xyz", "uvd", "coms", "Ms", "com_norm"), got, ref):
        assert np.array_equal(g, r), name
    assert np.isfinite(got[0]).all() and len(np.unique(got[0][:, 0, 2])) == 3     # three different frames
    # the same shape and dtype again: into the same output buffers
    res2 = pipe.run(rd)
    assert [t.data_ptr() for t in res2[:2]] == ptrs
    for g, r in zip(_np(res2), ref):
        assert np.array_equal(g, r)
    # float32 raw frames: the same outputs
    resf = _np(pipe.run(torch.from_numpy(_raw().astype(np.float32)).cuda()))
    for g, r in zip(resf, ref):
        assert np.array_equal(g, r)
    # frame k of the batch equals the same frame run alone
    for k in range(3):
        alone = _np(pipe.run(rd[k:k + 1]))
        for name, g, r in zip(("xyz", "uvd", "coms", "Ms", "com_norm"), alone, ref):
            assert np.array_equal(g[0], r[k]), (k, name)
    with pytest.raises(TypeError):
        pipe.run(_raw())
    with pytest.raises(TypeError, match="host preprocess_real_frames"):
        pipe.run(torch.from_numpy(_raw().astype(np.int32)).cuda())


@pytest.mark.gpu
def test_real_pipeline_failed_frame_keeps_its_status(pose):
    P = pkg()
    T = P.train_cnn_networks_hgru
    md = _md()
    raw = _raw()
    rd = torch.from_numpy(raw.copy()).cuda()
    fd = torch.from_numpy(P.monkeydetector.preprocess_real_frames(raw)).cuda()
    feat = _attn(None, out=1024).build(fd, 1024).cpu().numpy().astype(np.float64)      # [3, 1024]
    want = np.array([0.13, -0.15, 0.14])                      # frame 1: a CoM behind the camera
    spread = np.argsort(-(feat.max(0) - feat.min(0)))[:32]
    best, sol = 0.0, None
    for a in spread:                                          # the best conditioned pair of features
        for b in spread:
            A = np.stack([feat[:, a], feat[:, b], np.ones(3)], axis=1)
            d = abs(np.linalg.det(A))
            if a < b and d > best:
                best, sol = d, (a, b, np.linalg.solve(A, want))
    assert sol is not None
    a, b, (wa, wb, bz) = sol
    wz = np.zeros(1024, np.float32)
    wz[a], wz[b] = wa, wb
    bias = (0.5, 0.5, bz)
    ref, status = _parent_chain(_attn(bias, wz), pose, raw, check=False)
    print("features", a, b, "com_norm z", ref[4][:, 2].tolist(), "status", status.tolist())
    assert status[0] == 0 and status[2] == 0 and status[1] != 0
    pipe = T.RealDataPipeline(_attn(bias, wz), pose, md, check_crops=False)
    got = _np(pipe.run(rd))
    assert np.array_equal(md.last_status.cpu().numpy(), status)
    for g, r in zip(got, ref):
        assert np.array_equal(g, r)
    # frames 0 and 2 are what they are without the failing frame between them
    pair = _np(pipe.run(torch.from_numpy(raw[[0, 2]].copy()).cuda()))
    assert not md.last_status.cpu().numpy().any()
    for g, p in zip(got, pair):
        assert np.array_equal(g[[0, 2]], p)
    with pytest.raises(P._lib.MonkeyPoseError, match="frame 1"):
        T.RealDataPipeline(_attn(bias, wz), pose, md, check_crops=True).run(rd)


@pytest.mark.gpu
def test_eval_model_on_real_data_over_a_directory(pose, tmp_path):
    T = pkg().train_cnn_networks_hgru
    raw = _raw()
    d = str(tmp_path) + "/"
    names = ["kinect_10.npy", "kinect_02.npy", "kinect_1.npy"]              # sorted: 02, 1, 10
    for k, name in enumerate(names):
        np.save(d + name, raw[k])
    order = [1, 2, 0]
    pipe = T.RealDataPipeline(_attn((0.5, 0.5, 0.13)), pose, _md())
    files, xyz, uvd, coms = T.eval_model_on_real_data(d, pipe, batch_size=2)
    assert [f[len(d):] for f in files] == [names[k] for k in order]
    assert xyz.shape == (3, 23, 3) and uvd.shape == (3, 23, 3) and coms.shape == (3, 3)
    sorted_raw = torch.from_numpy(raw[order].copy()).cuda()
    first = _np(pipe.run(sorted_raw[:2]))
    last = _np(pipe.run(sorted_raw[2:]))
    for got, k in ((xyz, 0), (uvd, 1), (coms, 2)):
        assert np.array_equal(got, np.concatenate([first[k], last[k]]))
    assert len(np.unique(xyz[:, 0, 2])) == 3
