"""GPU: mp_png_encode_dev (csrc/k_png.hip) against mp_png_encode_host, byte for byte, on every case of
tests/png_cases.py -- tests/test_png_cpu.py holds the host's files to the pixels through zlib and PIL,
so equal bytes are right pixels.  Also: two calls agree, a picture's file does not depend on its
batch, nothing is written past a file's end or outside out, refusals touch nothing, the pipelines'
render_png decodes to render's pixels, and the call is ordered on the caller's stream."""
import functools

import numpy as np
import pytest
import torch

import png_cases as C
import stream_order_cases as SO
from helpers import pkg
from oracle import crop_ref as CR

SENTINEL = 0xA5
CAM = (365.456, 365.456, 256, 212, [800, 800, 1200], 200, 10000)


def _dev(name, sentinel=SENTINEL):
    """(buf, sizes) as numpy of the case through mp_png_encode_dev into a sentinel-filled buffer"""
    P = C.P()
    pic = C.picture(name)
    n, h, w, _ = pic.shape
    buf = torch.full((n, P.png_bound(h, w)), sentinel, dtype=torch.uint8, device="cuda")
    sizes = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    P.encode_png(torch.from_numpy(pic.copy()).cuda(), out=(buf, sizes))
    torch.cuda.synchronize()
    return buf.cpu().numpy(), sizes.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", C.NAMES)
def test_device_files_equal_the_host_files(name):
    ref, rs = C.host_files(name)
    buf, sizes = _dev(name)
    assert np.array_equal(sizes, rs)
    for i, s in enumerate(rs):
        assert buf[i, :s].tobytes() == ref[i, :s].tobytes(), f"picture {i}"
        assert (buf[i, s:] == SENTINEL).all(), f"picture {i}: bytes past the file's end were written"


@pytest.mark.gpu
def test_two_calls_agree_and_buffers_are_reused():
    P = C.P()
    pic = torch.from_numpy(C.picture("overlay-jet").copy()).cuda()
    b1, s1 = P.encode_png(pic)
    f1 = P.png_files(b1, s1)
    b2, s2 = P.encode_png(pic)
    assert b2.data_ptr() == b1.data_ptr() and s2.data_ptr() == s1.data_ptr()
    assert P.png_files(b2, s2) == f1
    ref, rs = C.host_files("overlay-jet")
    assert f1 == [ref[0, :rs[0]].tobytes()]
    assert np.array_equal(C.read_png(f1[0], 424, 512), C.picture("overlay-jet")[0])


class _N3Case(C.PngCase):
    SHAPE = (3, 20, 30, 3)                 # png_cases' n3


@pytest.mark.gpu
def test_two_encodes_on_two_streams_are_both_right():
    """stream_order_cases' hazards (late producer, immediate consumer, early release, back to back) for
    two calls of different pictures of one shape at once, each on a stream of its own into buffers of
    its own: the scratch is per stream too (tests/test_gpu_png16.py's test, with RGB pictures)"""
    preps = [SO.Prepared(_N3Case(draw)) for draw in (0, 1)]
    try:
        assert not np.array_equal(preps[0].A["rgb"], preps[1].A["rgb"])
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        report = SO.check_hazards(preps, streams, "two fresh streams")
        assert len(report) == 2 and all("conclusive" in r for r in report)
    finally:
        for p in preps:
            p.close()


@pytest.mark.gpu
def test_a_file_does_not_depend_on_its_batch():
    P = C.P()
    pic = torch.from_numpy(C.picture("n3").copy()).cuda()
    all3 = P.png_files(*P.encode_png(pic))
    for i in range(3):
        assert P.png_files(*P.encode_png(pic[i:i + 1])) == [all3[i]]


@pytest.mark.gpu
def test_odd_addresses_a_wider_stride_and_guards():
    P = C.P()
    lib = P._lib_png()
    pic = C.picture("n3")
    n, h, w, _ = pic.shape
    bound = P.png_bound(h, w)
    stride, guard = bound + 3, 64
    src = torch.zeros(pic.size + 1, dtype=torch.uint8, device="cuda")
    src[1:] = torch.from_numpy(pic.copy()).cuda().view(-1)
    dst = torch.full((guard + 1 + n * stride + guard,), SENTINEL, dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(n, dtype=torch.int64, device="cuda")
    work = torch.empty(lib.mp_png_work_bytes(n, h, w), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    assert lib.mp_png_encode_dev(src.data_ptr() + 1, n, h, w, dst.data_ptr() + guard + 1, stride, sizes.data_ptr(),
                                 work.data_ptr(), st) == 0
    torch.cuda.synchronize()
    ref, rs = C.host_files("n3")
    assert np.array_equal(sizes.cpu().numpy(), rs)
    d = dst.cpu().numpy()
    assert (d[:guard + 1] == SENTINEL).all() and (d[guard + 1 + n * stride:] == SENTINEL).all()
    body = d[guard + 1:guard + 1 + n * stride].reshape(n, stride)
    for i in range(n):
        assert body[i, :rs[i]].tobytes() == ref[i, :rs[i]].tobytes()
        assert (body[i, rs[i]:] == SENTINEL).all()


@pytest.mark.gpu
def test_refusals_leave_out_untouched():
    P = C.P()
    lib = P._lib_png()
    bound = P.png_bound(4, 4)
    pic = torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device="cuda")
    out = torch.full((bound,), SENTINEL, dtype=torch.uint8, device="cuda")
    sizes = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    work = torch.empty(lib.mp_png_work_bytes(1, 4, 4), dtype=torch.uint8, device="cuda")
    p, o, s, wk = pic.data_ptr(), out.data_ptr(), sizes.data_ptr(), work.data_ptr()
    for n, h, w, stride in ((0, 4, 4, bound), (65536, 4, 4, bound), (1, 0, 4, bound), (1, 4, 4097, 1 << 30),
                            (1, 4, 4, bound - 1)):
        assert lib.mp_png_encode_dev(p, n, h, w, o, stride, s, wk, None) == -5
    for args in ((None, 1, 4, 4, o, bound, s, wk), (p, 1, 4, 4, None, bound, s, wk), (p, 1, 4, 4, o, bound, None, wk),
                 (p, 1, 4, 4, o, bound, s, None), (p, 1, 4, 4, o, bound, s, wk + 4)):
        assert lib.mp_png_encode_dev(*args, None) == -1
    with pytest.raises(ValueError):
        P.encode_png(pic, out=(out.view(1, -1)[:, :bound - 1], sizes))
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all() and int(sizes.cpu()[0]) == -7


@functools.lru_cache(maxsize=None)
def _raw():
    """four recorded frames as stored: uint16 [512, 424]"""
    return np.stack([np.ascontiguousarray(CR.synth_frame(s).astype(np.uint16).T) for s in range(4)])


@pytest.mark.gpu
def test_pipelines_render_png(tmp_path):
    Pk = pkg()
    Wt, T, M, P = Pk.weights, Pk.train_cnn_networks_hgru, Pk.monkeydetector, Pk.png
    w = dict(Wt.attn_synth_weights(seed=1234))
    w["cnn/afc_out/afc_out_weights"] = np.zeros((1024, 3), np.float32)
    w["cnn/afc_out/afc_out_biases"] = np.asarray((0.5, 0.5, 0.13), np.float32)
    attn = T.attn_model_struct()
    attn.load_weights(w)
    pose = T.cnn_model_struct()
    pose.load_weights(Wt.synth_weights(Wt.cnn_vars(output_shape=69, crop=128), seed=77))
    md = M.MonkeyDetector(*CAM)
    pipe = T.RealDataPipeline(attn, pose, md)
    with pytest.raises(RuntimeError):
        pipe.render_png()
    bones = [(k, k + 1) for k in range(22)]
    xyz, uvd, coms, Ms, _ = pipe.run(torch.from_numpy(_raw().copy()).cuda())
    rgb = pipe.render(bones=bones, lut="jet").cpu().numpy()
    files = P.png_files(*pipe.render_png(bones=bones, lut="jet"))
    assert len(files) == 4
    for i, f in enumerate(files):
        assert np.array_equal(C.read_png(f, 424, 512), rgb[i])
    hb, hs = P.encode_png(rgb)                                   # and they are the host's files
    assert files == P.png_files(hb, hs)
    # FramePosePipeline takes the joints; DetectorPosePipeline draws its own
    fp = pipe.frame_pipeline
    f2 = P.png_files(*fp.render_png(uvd, bones=bones, lut="jet", depth_range=(0.1, 0.3)))
    assert f2 == files
    pm = Pk.hgru_pose.model()
    pm.load_weights(Wt.synth_weights(Wt.hgru_pose_vars(output_shape=69, timesteps=8, crop=64), seed=1234, timesteps=8))
    dp = T.DetectorPosePipeline(pm, md, dsize=64)
    with pytest.raises(RuntimeError):
        dp.render_png()
    mm = torch.from_numpy(np.stack([CR.synth_frame(s).astype(np.uint16) for s in range(2)])).cuda()
    dp.run(mm, h2_init=torch.from_numpy(Wt.synth_hidden((2, 32, 32, 64), seed=7)).cuda())
    f3 = P.png_files(*dp.render_png(depth_range=(1000, 3000)))
    ref3 = dp.render(depth_range=(1000, 3000)).cpu().numpy()
    assert len(f3) == 2 and all(np.array_equal(C.read_png(f, 424, 512), ref3[i]) for i, f in enumerate(f3))
    # eval_model_on_real_data hands the files to overlay_png, batch by batch
    for i, a in enumerate(_raw()[:3]):
        np.save(tmp_path / f"frame_{i}.npy", a)
    seen = []
    T.eval_model_on_real_data(str(tmp_path) + "/", pipe, batch_size=2, overlay_png=lambda fs, pngs: seen.append((fs, pngs)),
                              overlay_args=dict(bones=bones, lut="jet"))
    assert [len(p) for _, p in seen] == [2, 1]
    assert [p for _, ps in seen for p in ps] == files[:3]


@pytest.mark.gpu
@pytest.mark.parametrize("case", C.PNG_STREAM_CASES, ids=[c.name for c in C.PNG_STREAM_CASES])
def test_encode_is_ordered_on_its_stream(case):
    prep = SO.Prepared(case())
    try:
        for label, s in SO.caller_streams():
            report = SO.check_hazards([prep], [s], label)
            assert len(report) == 2 and all("conclusive" in r for r in report)
    finally:
        prep.close()
