"""GPU: uint16 depth frames on the device detector path -- MonkeyDetector.calculateCoM_device /
detect_crop_device and train_cnn_networks_hgru.DetectorPosePipeline fed torch.uint16 CUDA frames --
against the host MP_DEPTH_U16 functions of the same library (mp_center_of_mass, mp_crop3d_batch,
mp_crop3d_ex), which tests/test_crop.py and tests/test_crop_reference.py pin to the reference.
Every comparison is np.array_equal: a uint16 frame's sums are integers, its thresholds compare in
float64 and its near-plane clamp truncates, on the device as on the host."""
import functools

import numpy as np
import pytest
import torch

from helpers import pkg
from oracle import crop_ref as CR

CUBE = [800, 800, 1200]
CAMS = {"ref": (365.456, 365.456, 256, 212, CUBE, 200, 10000),
        "frac": (365.456, 365.456, 256, 212, CUBE, 200.5, 9999.5)}   # thresholds between two pixel values
EDGE_VALUES = (200, 201, 9999, 10000, 10001, 65535)
COM_CASES = [(3, 5, 7), (3, 8, 16), (3, 33, 47), (3, 100, 333), (2, 424, 512)]


def _md(cam):
    return pkg().monkeydetector.MonkeyDetector(*CAMS[cam])


@functools.lru_cache(maxsize=None)
def _frame(seed, h=424, w=512):
    f = CR.synth_frame(seed, h, w).astype(np.uint16)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _com_batch(n, h, w):
    """an all-zero frame; a frame with pixels at the thresholds, one step around them and at 65535;
    for n = 3 a plain synthetic frame.  5 x 7: frames 1 and 2 start 70 and 140 bytes in."""
    edge = _frame(11, h, w).copy().reshape(-1)
    for k, v in enumerate(EDGE_VALUES):
        edge[1 + 5 * k] = v
    frames = [np.zeros((h, w), np.uint16), edge.reshape(h, w)] + ([_frame(12, h, w)] if n == 3 else [])
    out = np.stack(frames)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _host_coms(cam, n, h, w):
    md = _md(cam)
    return np.stack([md.calculateCoM(f) for f in _com_batch(n, h, w)])


@pytest.mark.gpu
@pytest.mark.parametrize("case", COM_CASES, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}")
def test_device_com_of_uint16_frames_bit_exact_with_host(case):
    n, h, w = case
    fr = _com_batch(n, h, w)
    fd = torch.from_numpy(fr.copy()).cuda()
    assert fd.dtype == torch.uint16
    for cam in CAMS:
        got = _md(cam).calculateCoM_device(fd)
        assert got.dtype == torch.float64 and tuple(got.shape) == (n, 3) and got.is_cuda
        got, ref = got.cpu().numpy(), _host_coms(cam, n, h, w)
        print(cam, case, got.tolist(), ref.tolist())
        assert np.array_equal(got, ref)
        assert np.array_equal(got[0], np.zeros(3))       # the all-zero frame
        assert ref[1, 2] > 0
    # the two cameras disagree on the pixels at 200 and 10000, and it shows
    assert not np.array_equal(_host_coms("ref", n, h, w)[1], _host_coms("frac", n, h, w)[1])


@pytest.mark.gpu
def test_device_com_of_a_two_byte_aligned_view():
    n, h, w = 3, 33, 47
    fr = _com_batch(n, h, w)
    buf = np.zeros(n * h * w + 1, np.uint16)
    buf[0] = 4242                                         # in range: counted if the view were ignored
    buf[1:] = fr.reshape(-1)
    whole = torch.from_numpy(buf).cuda()
    view = whole[1:].view(n, h, w)
    assert view.data_ptr() == whole.data_ptr() + 2 and view.data_ptr() % 4 == 2 and view.is_contiguous()
    got = _md("ref").calculateCoM_device(view).cpu().numpy()
    assert np.array_equal(got, _host_coms("ref", n, h, w))


@pytest.mark.gpu
def test_uint16_com_is_not_the_float32_com_of_a_cast():
    md = _md("ref")
    fr = np.stack([_frame(s) for s in (1, 2, 3)])
    as_u16 = np.stack([md.calculateCoM(f) for f in fr])
    as_f32 = np.stack([md.calculateCoM(f.astype(np.float32)) for f in fr])
    print(as_u16[:, 2].tolist(), as_f32[:, 2].tolist())
    assert (as_u16[:, 2] != as_f32[:, 2]).all()          # exact integer sum vs float32 pairwise sum
    assert np.array_equal(as_u16[:, :2], as_f32[:, :2])
    got = md.calculateCoM_device(torch.from_numpy(fr).cuda()).cpu().numpy()
    assert np.array_equal(got, as_u16)


@functools.lru_cache(maxsize=None)
def _crop_case(n, h, w):
    """frames and given float64 CoMs of fractional depth: on the far wall around the body (the body's
    pixels lie before the near plane and are clamped to it), and boxes across the frame's borders"""
    frames = np.stack([_frame(20 + i, h, w) for i in range(n)])
    coms = []
    for i, f in enumerate(frames):
        ys, xs = np.nonzero((f > 0) & (f < 2000))
        by, bx = (ys.mean(), xs.mean()) if ys.size else (h / 2.0, w / 2.0)
        coms.append([(bx + 0.3, by + 0.6, 3500.25), (3.5, 5.25, 1100.7), (w - 2.2, h - 3.1, 3400.6),
                     (bx - 0.7, by + 0.2, 2950.9)][i % 4])
    frames.setflags(write=False)
    return frames, np.array(coms, np.float64)


@pytest.mark.gpu
@pytest.mark.parametrize("cam", list(CAMS))
@pytest.mark.parametrize("case", [(4, 424, 512), (2, 37, 53)], ids=["424x512", "37x53"])
def test_device_crop_of_uint16_frames_matches_host(case, cam):
    n, h, w = case
    md = _md(cam)
    frames, given = _crop_case(n, h, w)
    assert not np.array_equal(given, np.round(given))
    fd = torch.from_numpy(frames.copy()).cuda()
    f32_differs = False
    for coms in (given, None):
        hp, hM, hc = md.crop_batch(frames, coms=coms)
        fp, _, _ = md.crop_batch(frames.astype(np.float32), coms=hc)     # float32 rules, the same CoMs
        f32_differs |= not np.array_equal(hp, fp)
        cd = None if coms is None else torch.from_numpy(coms).cuda()
        patches, Ms, cout = md.detect_crop_device(fd, cd)
        assert patches.dtype == torch.float32 and tuple(patches.shape) == (n, 128, 128, 1)
        assert np.array_equal(cout.cpu().numpy(), hc)
        assert np.array_equal(Ms.cpu().numpy(), hM)
        assert np.array_equal(patches.cpu().numpy(), hp)
        assert not md.last_status.cpu().numpy().any()
        # docom=True against the host cropArea3D(docom=True) frame by frame
        patches, Ms, cout = md.detect_crop_device(fd, cd, docom=True)
        p, M, c = patches.cpu().numpy(), Ms.cpu().numpy(), cout.cpu().numpy()
        for i in range(n):
            crop, hM1, hc1 = md.cropArea3D(frames[i], None if coms is None else coms[i], docom=True)
            assert np.array_equal(c[i], hc1)
            assert np.array_equal(M[i], np.asarray(hM1))
            assert np.array_equal(p[i, ..., 0], crop / np.float32(md.maxDepth))
    assert f32_differs      # the truncating clamp is exercised: the float32 rules give other patches


@pytest.mark.gpu
def test_device_crop_uint16_zero_frame_status():
    P = pkg()
    md = _md("ref")
    frames, _ = _crop_case(4, 424, 512)
    batch = np.stack([frames[0], np.zeros_like(frames[0]), frames[1]])
    fd = torch.from_numpy(batch).cuda()
    hp, hM, hc = md.crop_batch(batch[[0, 2]], coms=None)
    for docom in (False, True):
        patches, Ms, coms = md.detect_crop_device(fd, check=False, docom=docom)
        assert md.last_status.cpu().numpy().tolist() == [0, 1, 0]
        p = patches.cpu().numpy()
        assert np.all(p[1] == 1.0)
        assert np.array_equal(coms.cpu().numpy()[1], np.zeros(3))
        if not docom:
            assert np.array_equal(p[[0, 2]], hp)
            assert np.array_equal(Ms.cpu().numpy()[[0, 2]], hM)
            assert np.array_equal(coms.cpu().numpy()[[0, 2]], hc)
    with pytest.raises(P._lib.MonkeyPoseError):
        md.detect_crop_device(fd)


def _host_joints(md, pose, coms):
    half = np.float32(md.cube[2] / 2.0)
    xs, us = [], []
    for i in range(pose.shape[0]):
        x, u = md.getAbsoluteCoordinates(pose[i].reshape(-1, 3) * half, coms[i])
        xs.append(np.asarray(x))
        us.append(np.asarray(u))
    return np.stack(xs), np.stack(us)


@pytest.mark.gpu
def test_detector_pipeline_on_uint16_frames_matches_host_chain():
    P = pkg()
    W = P.weights
    md = _md("ref")
    dev = torch.device("cuda", 0)
    n = 2
    wts = W.synth_weights(W.hgru_pose_vars(output_shape=69, timesteps=8, crop=64), seed=1234, timesteps=8)
    o0 = torch.from_numpy(W.synth_hidden((n, 32, 32, 64), seed=7)).to(dev)
    pm = P.hgru_pose.model()
    pm.load_weights(wts)
    pm.build(torch.zeros((n, 64, 64, 1), device=dev), 69, h2_init=o0)
    pipe = P.train_cnn_networks_hgru.DetectorPosePipeline(pm, md, dsize=64)

    def host_chain(frames):
        patches, Ms, coms = md.crop_batch(frames, coms=None, dsize=64)
        out = pm.forward(torch.from_numpy(patches).to(dev), h2_init=o0).cpu().numpy()
        xyz, uvd = _host_joints(md, out, coms)
        return xyz, uvd, coms, Ms

    fu = np.stack([_frame(1), _frame(2)])
    ff = fu.astype(np.float32)
    ref_u, ref_f = host_chain(fu), host_chain(ff)
    assert not np.array_equal(ref_u[2], ref_f[2])        # the two dtypes are told apart by their CoMs
    res = [t.cpu().numpy() for t in pipe.run(torch.from_numpy(fu).to(dev), h2_init=o0)]
    for g, r in zip(res, ref_u):
        assert np.array_equal(g, r)
    # float32 frames of the same shape next: the buffers are keyed by dtype, the float32 bits unchanged
    res = [t.cpu().numpy() for t in pipe.run(torch.from_numpy(ff).to(dev), h2_init=o0)]
    for g, r in zip(res, ref_f):
        assert np.array_equal(g, r)
    res = [t.cpu().numpy() for t in pipe.run(torch.from_numpy(fu).to(dev), h2_init=o0)]
    for g, r in zip(res, ref_u):
        assert np.array_equal(g, r)
