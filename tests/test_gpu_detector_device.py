"""GPU: the device-resident detector path -- MonkeyDetector.calculateCoM_device / detect_crop_device /
getAbsoluteCoordinates_device and train_cnn_networks_hgru.DetectorPosePipeline -- against the host
native functions of the same library (mp_center_of_mass, mp_crop3d_batch / mp_crop3d_ex, the numpy
getAbsoluteCoordinates), which the existing tests pin to the reference.  Every comparison is
np.array_equal: the device runs the host's float operations in the host's order."""
import functools

import numpy as np
import pytest
import torch

from helpers import pkg

CUBE = [800, 800, 1200]
CAMS = {"ref": (365.456, 365.456, 256, 212, CUBE, 200, 10000),
        "near": (365.456, 365.456, 256, 212, CUBE, 200, 2500)}   # far wall out of range: the CoM is on the body
SHAPES = [(1, 5), (8, 16), (8, 17), (37, 53), (100, 333), (424, 512)]
F10K = np.float32(10000.0)


def _md(cam):
    return pkg().monkeydetector.MonkeyDetector(*CAMS[cam])


@functools.lru_cache(maxsize=None)
def _frames_norm(n, seed, h=424, w=512):
    """normalised frames [n, h, w] (mm / 10000) and what the detector sees, frames * f32(10000)"""
    fn = np.ascontiguousarray(pkg().weights.synth_frames(n, seed=seed, h=h, w=w)[..., 0])
    return fn, fn * F10K


@functools.lru_cache(maxsize=None)
def _com_frames(h, w, max_depth):
    """three frames in mm: all zeros; pixels exactly at min_depth / max_depth and one float32 step
    outside each; fractional depths"""
    base = _frames_norm(3, 5, h, w)[1]
    z = np.zeros((h, w), np.float32)
    edge = base[1].copy().reshape(-1)
    vals = [np.float32(200), np.float32(max_depth), np.nextafter(np.float32(200), np.float32(0)),
            np.nextafter(np.float32(max_depth), np.float32(np.inf))]
    for k, v in enumerate(vals):
        edge[(k * 7) % edge.size if edge.size > 8 else k] = v
    frac = np.where(base[2] > 0, base[2] * np.float32(0.37) + np.float32(0.123), np.float32(0)).astype(np.float32)
    return np.stack([z, edge.reshape(h, w), frac])


@pytest.mark.gpu
@pytest.mark.parametrize("frame_scale", [1.0, 10000.0], ids=["mm", "normalised"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_com_bit_exact_with_host(shape, frame_scale):
    h, w = shape
    for cam in CAMS:
        md = _md(cam)
        fr = _com_frames(h, w, CAMS[cam][6])
        if frame_scale != 1.0:
            fr = fr / np.float32(frame_scale)
        seen = fr * np.float32(frame_scale)                      # the device's one float32 multiply
        got = md.calculateCoM_device(torch.from_numpy(fr).cuda(), frame_scale=frame_scale)
        assert got.dtype == torch.float64 and tuple(got.shape) == (3, 3) and got.is_cuda
        got = got.cpu().numpy()
        ref = np.stack([md.calculateCoM(f) for f in seen])
        print(cam, shape, frame_scale, got.tolist(), ref.tolist())
        assert np.array_equal(got, ref)
        assert np.array_equal(got[0], np.zeros(3))              # the all-zero frame
        if h * w > 8:
            assert ref[1, 2] > 0 and ref[2, 2] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("cam", list(CAMS))
@pytest.mark.parametrize("case", [(4, 5, 424, 512), (2, 9, 37, 53)], ids=["424x512", "37x53"])
def test_device_crop_own_com_matches_host(case, cam):
    n, seed, h, w = case
    md = _md(cam)
    fn, fmm = _frames_norm(n, seed, h, w)
    fd = torch.from_numpy(fn).cuda()
    patches, Ms, coms = md.detect_crop_device(fd, frame_scale=10000.0)
    hp, hM, hc = md.crop_batch(fmm, coms=None)
    assert np.array_equal(coms.cpu().numpy(), hc)
    assert np.array_equal(Ms.cpu().numpy(), hM)
    assert np.array_equal(patches.cpu().numpy(), hp)
    assert not md.last_status.cpu().numpy().any()
    # docom=True against the host cropArea3D(docom=True) frame by frame
    patches, Ms, coms = md.detect_crop_device(fd, frame_scale=10000.0, docom=True)
    p, M, c = patches.cpu().numpy(), Ms.cpu().numpy(), coms.cpu().numpy()
    for i in range(n):
        crop, hM1, hc1 = md.cropArea3D(fmm[i], None, docom=True)
        assert np.array_equal(c[i], hc1)
        assert np.array_equal(M[i], np.asarray(hM1))
        assert np.array_equal(p[i, ..., 0], crop / np.float32(md.maxDepth))


@pytest.mark.gpu
def test_device_crop_zero_frame_status():
    P = pkg()
    md = _md("near")
    fn, fmm = _frames_norm(4, 5)
    batch = np.stack([fn[0], np.zeros_like(fn[0]), fn[1]])
    fd = torch.from_numpy(batch).cuda()
    for docom in (False, True):
        patches, Ms, coms = md.detect_crop_device(fd, frame_scale=10000.0, check=False, docom=docom)
        st = md.last_status.cpu().numpy()
        assert st.tolist() == [0, 1, 0]
        p = patches.cpu().numpy()
        assert np.all(p[1] == 1.0)
        assert np.array_equal(coms.cpu().numpy()[1], np.zeros(3))
        if not docom:
            hp, hM, hc = md.crop_batch(fmm[:2], coms=None)
            assert np.array_equal(p[[0, 2]], hp)
            assert np.array_equal(Ms.cpu().numpy()[[0, 2]], hM)
            assert np.array_equal(coms.cpu().numpy()[[0, 2]], hc)
    with pytest.raises(P._lib.MonkeyPoseError):
        md.detect_crop_device(fd, frame_scale=10000.0)


@pytest.mark.gpu
def test_device_crop_given_float64_coms():
    md = _md("ref")
    fn, fmm = _frames_norm(4, 5)
    given = np.array([[255.46593644951234, 200.12345678901234, 1500.0000001234567],
                      [250.70000000000002, 190.29999999999998, 1234.5678901234567],
                      [300.00000000000006, 150.99999999999997, 999.99999999999989],
                      [128.1, 301.7, 3333.3333333333335]], np.float64)
    assert not np.array_equal(given, given.astype(np.float32).astype(np.float64))   # float32 cannot hold them
    fd = torch.from_numpy(fn).cuda()
    hp, hM, hc = md.crop_batch(fmm, coms=given)
    patches, Ms, coms = md.detect_crop_device(fd, coms=torch.from_numpy(given).cuda(), frame_scale=10000.0)
    assert np.array_equal(coms.cpu().numpy(), given) and np.array_equal(hc, given)
    assert np.array_equal(Ms.cpu().numpy(), hM)
    assert np.array_equal(patches.cpu().numpy(), hp)
    # frames already in mm: frame_scale = 1
    p1, M1, _ = md.detect_crop_device(torch.from_numpy(fmm).cuda(), coms=torch.from_numpy(given).cuda())
    assert np.array_equal(p1.cpu().numpy(), hp) and np.array_equal(M1.cpu().numpy(), hM)


def _host_joints(md, pose, coms):
    half = np.float32(md.cube[2] / 2.0)
    xs, us = [], []
    for i in range(pose.shape[0]):
        x, u = md.getAbsoluteCoordinates(pose[i].reshape(-1, 3) * half, coms[i])
        xs.append(np.asarray(x))
        us.append(np.asarray(u))
    return np.stack(xs), np.stack(us)


@pytest.mark.gpu
def test_device_abs_joints_match_host():
    md = _md("ref")
    rs = np.random.RandomState(0)
    pose = rs.uniform(-1.0, 1.0, (3, 69)).astype(np.float32)
    coms = np.array([[255.46593644951234, 200.2, 1500.1], [100.5, 300.25, 2345.678], [256.0, 212.0, 600.0]],
                    np.float64)
    pose[2, 5 * 3 + 2] = 1.0       # rel z = 600 on a CoM at depth 600: z == 0 exactly
    xyz, uvd = md.getAbsoluteCoordinates_device(torch.from_numpy(pose).cuda(), torch.from_numpy(coms).cuda())
    assert tuple(xyz.shape) == (3, 23, 3) and xyz.dtype == torch.float32 and uvd.is_cuda
    hx, hu = _host_joints(md, pose, coms)
    assert hx[2, 5, 2] == 0.0
    assert np.array_equal(xyz.cpu().numpy(), hx)
    assert np.array_equal(uvd.cpu().numpy(), hu)
    assert uvd.cpu().numpy()[2, 5].tolist() == [256.0, 212.0, 0.0]


@pytest.mark.gpu
def test_detector_pipeline_matches_host_chain():
    P = pkg()
    W = P.weights
    md = _md("near")
    dev = torch.device("cuda", 0)
    wts = W.synth_weights(W.hgru_pose_vars(output_shape=69, timesteps=8, crop=64), seed=1234, timesteps=8)
    o0 = torch.from_numpy(W.synth_hidden((3, 32, 32, 64), seed=7)).to(dev)
    pm = P.hgru_pose.model()
    pm.load_weights(wts)
    pm.build(torch.zeros((3, 64, 64, 1), device=dev), 69, h2_init=o0)
    pipe = P.train_cnn_networks_hgru.DetectorPosePipeline(pm, md, dsize=64, frame_scale=10000.0)

    def host_chain(fmm):
        patches, Ms, coms = md.crop_batch(fmm, coms=None, dsize=64)
        out = pm.forward(torch.from_numpy(patches).to(dev), h2_init=o0).cpu().numpy()
        xyz, uvd = _host_joints(md, out, coms)
        return xyz, uvd, coms, Ms

    def check(res, ref):
        for g, r in zip(res, ref):
            assert np.array_equal(g, r)

    fn, fmm = _frames_norm(4, 5)
    ref = host_chain(fmm[:3])
    res = [t.cpu().numpy() for t in pipe.run(torch.from_numpy(fn[:3]).to(dev), h2_init=o0)]
    check(res, ref)
    ptrs = [t.data_ptr() for t in pipe.run(torch.from_numpy(fn[:3]).to(dev), h2_init=o0)]
    # a non-default stream
    s = torch.cuda.Stream(device=dev)
    fd = torch.from_numpy(fn[:3]).to(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(s):
        out = pipe.run(fd, h2_init=o0)
        s.synchronize()
        res = [t.cpu().numpy() for t in out]
    check(res, ref)
    # new frames, the same batch shape: the buffers are reused and the result is still exact
    fn2, fmm2 = _frames_norm(3, 9)
    out = pipe.run(torch.from_numpy(fn2).to(dev), h2_init=o0)
    assert [t.data_ptr() for t in out] == ptrs
    check([t.cpu().numpy() for t in out], host_chain(fmm2))


@pytest.mark.gpu
def test_attention_crop_path_unchanged():
    """crop_batch_device (the float32 attention CoM form of the kernels the detector path now shares)
    on the inputs of the existing bit-exactness test: that test, run as it is."""
    import test_attn
    test_attn.test_device_crop_bit_exact_with_host_and_oracle()
