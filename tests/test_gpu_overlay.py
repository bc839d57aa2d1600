"""GPU: mp_overlay_dev through monkeydetector.render_overlays -- depth frames through a colour table
with joint markers and bones drawn on them -- against render_overlays_np, the numpy statement of the
rule in csrc/overlay_geom.hpp (tests/test_overlay_cpu.py holds that statement against the header and
against a brute-force loop).  Every comparison of pixels is np.array_equal on uint8.  Also
MonkeyDetector.transform_joints_device (joints in the crop's pixel space), the pipelines' render and
eval_model_on_real_data's overlay callback."""
import functools

import numpy as np
import pytest
import torch

from helpers import pkg
from oracle import crop_ref as CR

CAM = (365.456, 365.456, 256, 212, [800, 800, 1200], 200, 10000)
STYLES = (((0, 255, 0), (0, 160, 0), 3, 1), ((255, 0, 0), (200, 0, 200), 2, 3),
          ((0, 0, 255), (90, 90, 255), 0, 2), ((255, 255, 0), (200, 200, 0), 15, 15))
CHAIN = [(k, k + 1) for k in range(6)]                   # a chain over seven joints


def M():
    return pkg().monkeydetector


def _frames(kind, n, h, w, seed=0):
    rng = np.random.default_rng(1000 * seed + 31 * h + w)
    mm = rng.integers(0, 4000, (n, h, w))
    return mm.astype(np.uint16) if kind == "u16" else (mm / 7.0).astype(np.float32)


def _joints(n, S, J, h, w, seed=0):
    """random joints from a margin outside the frame to a margin past its far edge"""
    rng = np.random.default_rng(7 + seed)
    ju = np.empty((n, S, J, 3), np.float32)
    ju[..., 0] = rng.uniform(-6, w + 6, (n, S, J))
    ju[..., 1] = rng.uniform(-6, h + 6, (n, S, J))
    ju[..., 2] = rng.uniform(500, 3000, (n, S, J))
    return ju


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _both(fr, ju, **kw):
    got = M().render_overlays(_dev(fr), _dev(ju), **kw).cpu().numpy()
    ref = M().render_overlays_np(fr, ju, **kw)
    return got, ref


# (2, 33, 67): 3 h w is odd, so frame 1 of out starts on an odd byte and frame 1 of a uint16 input off a
# 4-byte boundary, with partial tiles on both edges; (3, 64, 128): whole tiles
SHAPES = [(1, 1, 1), (1, 7, 5), (2, 33, 67), (3, 64, 128), (2, 424, 512)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["u16", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_overlay_equals_numpy(kind, shape):
    n, h, w = shape
    fr = _frames(kind, n, h, w)
    ju = _joints(n, 2, 7, h, w)
    rng = (1000, 3000) if kind == "u16" else (1000 / 7.0, 3000 / 7.0)
    got, ref = _both(fr, ju, bones=CHAIN, depth_range=rng, lut="jet", styles=STYLES)
    assert got.shape == (n, h, w, 3) and got.dtype == np.uint8
    assert np.array_equal(got, ref)
    if h >= 33:
        plain = M().render_overlays_np(fr, ju[:, :, :0], depth_range=rng, lut="jet")
        assert (ref != plain).any()                       # something was drawn
    # a single set as [n, J, 3], default styles, markers only, the default table
    got, ref = _both(fr, ju[:, 1], depth_range=rng)
    assert np.array_equal(got, ref)


@pytest.mark.gpu
def test_colour_map_alone_for_every_uint16_value():
    fr = np.arange(65536, dtype=np.uint16).reshape(1, 256, 256)
    none = np.zeros((1, 1, 0, 3), np.float32)
    for rng in ((1000, 3000), (0, 65535), (3000, 1000), (0.5, 10000.25)):
        for lut in ("gray", "jet"):
            got, ref = _both(fr, none, depth_range=rng, lut=lut)
            assert np.array_equal(got, ref), (rng, lut)
    assert len(np.unique(ref.reshape(-1, 3), axis=0)) > 200
    # float32 frames with the values no uint16 has
    ff = fr.astype(np.float32)
    ff[0, 0, :6] = [np.nan, np.inf, -np.inf, -0.0, 1e30, -1e30]
    got, ref = _both(ff, none, depth_range=(1000, 3000), lut="jet")
    assert np.array_equal(got, ref)
    # a table of the caller's own, as a CUDA tensor
    table = np.random.default_rng(5).integers(0, 256, (256, 3)).astype(np.uint8)
    got = M().render_overlays(_dev(fr), _dev(none), depth_range=(1000, 3000), lut=_dev(table)).cpu().numpy()
    assert np.array_equal(got, M().render_overlays_np(fr, none, depth_range=(1000, 3000), lut=table))


@pytest.mark.gpu
def test_views_and_guard_bytes():
    n, h, w = 2, 33, 67
    fr = _frames("u16", n, h, w)
    ju = _joints(n, 2, 7, h, w)
    kw = dict(bones=CHAIN, depth_range=(1000, 3000), lut="jet", styles=STYLES)
    ref = M().render_overlays_np(fr, ju, **kw)
    nbytes = ref.size
    for off in (1, 2, 3, 16):
        buf = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        out = buf[off:off + nbytes]
        assert out.data_ptr() % 4 == off % 4
        got = M().render_overlays(_dev(fr), _dev(ju), out=out, **kw)
        assert got.data_ptr() == out.data_ptr()
        b = buf.cpu().numpy()
        assert np.array_equal(b[off:off + nbytes].reshape(ref.shape), ref), off
        assert (b[:off] == 0xA5).all() and (b[off + nbytes:] == 0xA5).all(), off      # the guard bytes
    # uint16 frames as a view starting at an odd element (2 bytes off a 4-byte boundary)
    wide = torch.zeros((fr.size + 3,), dtype=torch.uint16, device="cuda")
    view = wide[1:1 + fr.size].view(n, h, w)
    view.copy_(_dev(fr))
    assert view.data_ptr() % 4 == 2
    assert np.array_equal(M().render_overlays(view, _dev(ju), **kw).cpu().numpy(), ref)
    # float32 frames 4 bytes off a 16-byte boundary
    ff = fr.astype(np.float32)
    widef = torch.zeros((ff.size + 3,), dtype=torch.float32, device="cuda")
    viewf = widef[1:1 + ff.size].view(n, h, w)
    viewf.copy_(_dev(ff))
    assert viewf.data_ptr() % 16 == 4
    assert np.array_equal(M().render_overlays(viewf, _dev(ju), **kw).cpu().numpy(), ref)


@pytest.mark.gpu
def test_placement():
    h, w = 40, 150                                       # two tiles across, two down
    fr = np.full((1, h, w), 2000, np.uint16)
    nan = np.nan
    r = 4
    st = (((255, 0, 0), (0, 0, 255), r, 3),)
    kw = dict(depth_range=(1000, 3000), styles=st)
    base = M().render_overlays_np(fr, np.zeros((1, 1, 0, 3), np.float32), **kw)

    def run(pts, bones=None):
        ju = np.zeros((1, 1, len(pts), 3), np.float32)
        ju[0, 0, :, :2] = pts
        got, ref = _both(fr, ju, bones=bones, **kw)
        assert np.array_equal(got, ref)
        return got
    # markers at the four corners
    img = run([(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)])
    for x, y in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)):
        assert tuple(img[0, y, x]) == (255, 0, 0)
    # centred outside the frame by less than, exactly, and more than r
    assert (run([(-(r - 1), 20)]) != base).any()
    edge = run([(-r, 20)])
    assert tuple(edge[0, 20, 0]) == (255, 0, 0) and (edge != base).sum() == 3
    assert np.array_equal(run([(-(r + 1), 20)]), base)
    assert np.array_equal(run([(w - 1 + r + 1, 20), (20, h - 1 + r + 1), (20, -(r + 1))]), base)
    # a bone with one end 4,000 px outside: clipped, not dropped
    img = run([(10, 20), (4010, 25)], bones=[(0, 1)])
    assert tuple(img[0, 20, 60]) == (0, 0, 255) and tuple(img[0, 20, w - 1]) == (0, 0, 255)
    img = run([(-4000, -3000), (w + 100, h + 60)], bones=[(0, 1)])
    assert (img != base).any()
    # one end ineligible (past the range, or NaN): no bone, the other end's marker stays
    for bad in ((8192, 25), (-4097.5, 25), (nan, 25), (60, np.inf)):
        img = run([(10, 20), bad], bones=[(0, 1)])
        assert tuple(img[0, 20, 10]) == (255, 0, 0) and not (img == (0, 0, 255)).all(-1).any(), bad
    # a NaN-padded set: one real joint (say the CoM) and padding, next to a full set
    ju = np.full((1, 2, 5, 3), nan, np.float32)
    ju[0, 0, :, :2] = [(20, 10), (40, 12), (60, 30), (90, 20), (140, 35)]
    ju[0, 1, 0, :2] = (75, 20)
    got, ref = _both(fr, ju, bones=[(0, 1), (1, 2), (2, 3), (3, 4)], depth_range=(1000, 3000), styles=STYLES)
    assert np.array_equal(got, ref)
    assert tuple(got[0, 20, 75]) == STYLES[1][0]


@pytest.mark.gpu
def test_order_last_primitive_wins():
    h, w = 32, 32
    fr = np.full((1, h, w), 2000, np.uint16)
    st = (((10, 200, 10), (10, 90, 10), 2, 3), ((200, 10, 10), (90, 10, 10), 2, 3))
    ju = np.zeros((1, 2, 5, 3), np.float32)
    # each set: two bones crossing in (16, 16), then a marker on the crossing
    ju[0, :, :, :2] = [(6, 6), (26, 26), (6, 26), (26, 6), (16, 16)]
    bones = [(0, 1), (2, 3)]
    got, ref = _both(fr, ju, bones=bones, depth_range=(1000, 3000), styles=st)
    assert np.array_equal(got, ref)
    assert tuple(got[0, 16, 16]) == st[1][0]               # set 1's marker is last
    assert tuple(got[0, 20, 20]) == st[1][1]               # off the markers: set 1's bones over set 0's
    # without the crossing marker the later bone of the later set wins the crossing pixel
    got2, ref2 = _both(fr, ju[:, :, :4], bones=bones, depth_range=(1000, 3000), styles=st)
    assert np.array_equal(got2, ref2) and tuple(got2[0, 16, 16]) == st[1][1]
    # bones of different colours within one scene: two sets, each drawing one of the two bones
    jx = ju.copy()
    jx[0, 0, 2:4] = np.nan                                  # set 0 keeps the first bone
    jx[0, 1, 0:2] = np.nan                                  # set 1 keeps the second
    got3, ref3 = _both(fr, jx[:, :, :4], bones=bones, depth_range=(1000, 3000), styles=st)
    assert np.array_equal(got3, ref3) and tuple(got3[0, 16, 16]) == st[1][1]
    # the same scene with the styles swapped between the sets is a different image: order is seen
    swapped, ref4 = _both(fr, ju, bones=bones, depth_range=(1000, 3000), styles=st[::-1])
    assert np.array_equal(swapped, ref4)
    assert tuple(swapped[0, 16, 16]) == st[0][0] and not np.array_equal(swapped, got)


@pytest.mark.gpu
def test_crowding_the_list_worst_case():
    """128 joints x 4 sets and 256 bones all meeting one tile (the LDS list's 4 * (128 + 256) entries),
    then the same scene spread over the frame"""
    h, w = 48, 300
    fr = _frames("u16", 1, h, w)
    rng = np.random.default_rng(11)
    bones = np.stack([rng.integers(0, 128, 256), rng.integers(0, 128, 256)], axis=1)
    bones[:, 1] = np.where(bones[:, 1] == bones[:, 0], (bones[:, 0] + 1) % 128, bones[:, 1])
    st = tuple((tuple(rng.integers(0, 256, 3)), tuple(rng.integers(0, 256, 3)), int(r), int(t))
               for r, t in ((1, 1), (2, 2), (0, 1), (3, 3)))
    packed = np.zeros((1, 4, 128, 3), np.float32)
    packed[..., 0] = rng.uniform(130, 250, (1, 4, 128))    # all inside the tile x 128..255, y 0..31
    packed[..., 1] = rng.uniform(16.6, 23.4, (1, 4, 128))
    spread = np.zeros((1, 4, 128, 3), np.float32)
    spread[..., 0] = rng.uniform(0, w, (1, 4, 128))
    spread[..., 1] = rng.uniform(0, h, (1, 4, 128))
    for ju in (packed, spread):
        got, ref = _both(fr, ju, bones=bones, depth_range=(1000, 3000), lut="jet", styles=st)
        assert np.array_equal(got, ref)
    # every primitive of the packed scene lies in the tile at x 128..255, y 0..31
    ok, cen = M().overlay_centers(packed[..., :2])
    assert ok.all() and (cen[..., 0] >= 128).all() and (cen[..., 0] < 256).all()
    assert (cen[..., 1] >= 16).all() and (cen[..., 1] < 24).all()


@pytest.mark.gpu
def test_batch_invariance_and_repeatability():
    n, h, w = 3, 33, 140
    fr = _frames("f32", n, h, w)
    ju = _joints(n, 2, 7, h, w)
    kw = dict(bones=CHAIN, depth_range=(150, 420), lut="jet", styles=STYLES)
    fd, jd = _dev(fr), _dev(ju)
    a = M().render_overlays(fd, jd, **kw).cpu().numpy()
    b = M().render_overlays(fd, jd, stream=torch.cuda.current_stream().cuda_stream, **kw).cpu().numpy()
    assert a.tobytes() == b.tobytes()
    for i in range(n):
        alone = M().render_overlays(fd[i:i + 1], jd[i:i + 1], **kw).cpu().numpy()
        assert np.array_equal(alone[0], a[i]), i
    # [n, h, w, 1] frames, as the pipelines keep them
    assert np.array_equal(M().render_overlays(fd[..., None], jd, **kw).cpu().numpy(), a)


@pytest.mark.gpu
def test_device_call_rejects_bad_arguments():
    fd = torch.zeros((2, 8, 16), dtype=torch.uint16, device="cuda")
    jd = torch.zeros((2, 2, 5, 3), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        M().render_overlays(fd, jd, bones=[(0, 5)])
    with pytest.raises(ValueError):
        M().render_overlays(fd, jd, depth_range=(5, 5))
    with pytest.raises(ValueError):
        M().render_overlays(fd, jd, out=torch.zeros((10,), dtype=torch.uint8, device="cuda"))
    with pytest.raises(TypeError):
        M().render_overlays(fd, jd.cpu())
    with pytest.raises(TypeError):
        M().render_overlays(fd.to(torch.int32), jd)


# ---------------------------------------------------------------------- crop-space joints
@pytest.mark.gpu
def test_transform_joints_device():
    md = M().MonkeyDetector(*CAM)
    frames = np.stack([CR.synth_frame(s).astype(np.float32) for s in range(3)])
    _, Ms, coms = md.detect_crop_device(_dev(frames))
    Mh = Ms.cpu().numpy()
    rng = np.random.default_rng(3)
    ju = np.empty((3, 23, 3), np.float32)
    ju[..., 0] = rng.uniform(0, 512, (3, 23))
    ju[..., 1] = rng.uniform(0, 424, (3, 23))
    ju[..., 2] = rng.uniform(500, 3000, (3, 23))
    got = md.transform_joints_device(_dev(ju), Ms).cpu().numpy()
    # the expression, elementwise in float64 (no product fused into an add), rounded once
    u, v = ju[..., 0].astype(np.float64), ju[..., 1].astype(np.float64)
    t = [(u * Mh[:, i, 0, None] + v * Mh[:, i, 1, None]) + Mh[:, i, 2, None] for i in range(3)]
    want = np.stack([(t[0] / t[2]).astype(np.float32), (t[1] / t[2]).astype(np.float32), ju[..., 2]], axis=-1)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert np.isfinite(got).all() and np.ptp(got[..., 0]) > 10
    # the host getRelativeCoordinates forms t by a BLAS product, which may fuse or reorder its sums;
    # both are float64 evaluations rounded once to float32, so they agree to one float32 ulp
    for i in range(3):
        _, rel = md.getRelativeCoordinates(np.zeros((23, 3), np.float32), ju[i], coms[i].cpu().numpy(), Mh[i])
        ulp = np.spacing(np.abs(rel[:, :2]).astype(np.float32))
        assert (np.abs(got[i, :, :2] - rel[:, :2]) <= ulp).all()
        assert np.array_equal(got[i, :, 2], rel[:, 2])
    out = torch.empty((3 * 23 * 3,), dtype=torch.float32, device="cuda")
    again = md.transform_joints_device(_dev(ju), Ms, out=out)
    assert again.data_ptr() == out.data_ptr() and np.array_equal(again.cpu().numpy(), want)
    with pytest.raises(ValueError):
        md.transform_joints_device(_dev(ju), Ms[:2])


# ---------------------------------------------------------------------- the pipelines
W_AFC = "cnn/afc_out/afc_out_weights"
B_AFC = "cnn/afc_out/afc_out_biases"


@functools.lru_cache(maxsize=None)
def _raw():
    """three recorded frames as stored: uint16 [512, 424]"""
    out = np.stack([np.ascontiguousarray(CR.synth_frame(s).astype(np.uint16).T) for s in range(3)])
    out.setflags(write=False)
    return out


def _attn(bias):
    """attention net whose output is the chosen CoM for every frame (zero afc_out weights)"""
    P = pkg()
    w = dict(P.weights.attn_synth_weights(seed=1234))
    w[W_AFC] = np.zeros((1024, 3), np.float32)
    w[B_AFC] = np.asarray(bias, np.float32)
    a = P.train_cnn_networks_hgru.attn_model_struct()
    a.load_weights(w)
    return a


@pytest.fixture(scope="module")
def real_pipe():
    P = pkg()
    Wt, T = P.weights, P.train_cnn_networks_hgru
    m = T.cnn_model_struct()
    m.load_weights(Wt.synth_weights(Wt.cnn_vars(output_shape=69, crop=128), seed=77))
    return T.RealDataPipeline(_attn((0.5, 0.5, 0.13)), m, M().MonkeyDetector(*CAM))


@pytest.mark.gpu
def test_real_pipeline_render(real_pipe):
    pipe = real_pipe
    with pytest.raises(RuntimeError):
        type(pipe)(pipe.frame_pipeline.attn, pipe.frame_pipeline.pose, pipe.md).render()
    xyz, uvd, coms, Ms, com_norm = pipe.run(torch.from_numpy(_raw().copy()).cuda())
    frames = pipe._frames.cpu().numpy()                   # the pipeline's own gated, normalised frames
    assert frames.shape == (3, 424, 512, 1) and frames.dtype == np.float32
    uvd_h = uvd.cpu().numpy()
    bones = [(k, k + 1) for k in range(22)]
    img = pipe.render(bones=bones, lut="jet")
    assert img.is_cuda and tuple(img.shape) == (3, 424, 512, 3)
    ref = M().render_overlays_np(frames, uvd_h, bones=bones, depth_range=(0.1, 0.3), lut="jet")
    assert np.array_equal(img.cpu().numpy(), ref)
    plain = M().render_overlays_np(frames, uvd_h[:, :0], depth_range=(0.1, 0.3), lut="jet")
    assert (ref != plain).any()                           # the joints are in the picture
    # further sets (here the CoM as a NaN-padded set) are drawn over the results
    com_set = torch.full((3, 23, 3), float("nan"), device="cuda")
    com_set[:, 0] = coms.float()
    img2 = pipe.render(extra_sets=[com_set], depth_range=(0.05, 0.5))
    ref2 = M().render_overlays_np(frames, np.stack([uvd_h, com_set.cpu().numpy()], axis=1),
                                  depth_range=(0.05, 0.5))
    assert np.array_equal(img2.cpu().numpy(), ref2)


@pytest.mark.gpu
def test_frame_and_detector_pipeline_render(real_pipe):
    P = pkg()
    T = P.train_cnn_networks_hgru
    Wt = P.weights
    md = real_pipe.md
    mm = np.stack([CR.synth_frame(s).astype(np.uint16) for s in range(2)])
    pm = P.hgru_pose.model()
    pm.load_weights(Wt.synth_weights(Wt.hgru_pose_vars(output_shape=69, timesteps=8, crop=64), seed=1234, timesteps=8))
    o0 = _dev(Wt.synth_hidden((2, 32, 32, 64), seed=7))
    det = T.DetectorPosePipeline(pm, md, dsize=64)
    with pytest.raises(RuntimeError):
        det.render()
    xyz, uvd, coms, Ms = det.run(_dev(mm), h2_init=o0)
    img = det.render(depth_range=(1000, 3000))
    assert np.array_equal(img.cpu().numpy(),
                          M().render_overlays_np(mm, uvd.cpu().numpy(), depth_range=(1000, 3000)))
    fp = real_pipe.frame_pipeline
    fd = _dev((mm.astype(np.float32) / np.float32(10000.))[..., None])
    out, coms, Ms = fp.run(fd)
    _, uvd = md.getAbsoluteCoordinates_device(out, coms, 23)
    img = fp.render(uvd, lut="jet")
    assert np.array_equal(img.cpu().numpy(), M().render_overlays_np(fd.cpu().numpy(), uvd.cpu().numpy(), lut="jet"))


@pytest.mark.gpu
def test_eval_model_on_real_data_overlay_callback(real_pipe, tmp_path):
    T = pkg().train_cnn_networks_hgru
    raw = _raw()
    d = str(tmp_path) + "/"
    for k in range(3):
        np.save(d + f"kinect_{k}.npy", raw[k])
    plain = T.eval_model_on_real_data(d, real_pipe, batch_size=2)
    seen = []
    res = T.eval_model_on_real_data(d, real_pipe, batch_size=2,
                                    overlay=lambda files, rgb: seen.append((list(files), rgb.copy())))
    assert res[0] == plain[0]
    for a, b in zip(res[1:], plain[1:]):
        assert np.array_equal(a, b)
    assert [f for fs, _ in seen for f in fs] == plain[0]                 # every file once, in order
    assert [rgb.shape for _, rgb in seen] == [(2, 424, 512, 3), (1, 424, 512, 3)]
    frames = M().preprocess_real_frames(raw)
    ref = M().render_overlays_np(frames, plain[2], depth_range=(0.1, 0.3))
    assert np.array_equal(np.concatenate([rgb for _, rgb in seen]), ref)
