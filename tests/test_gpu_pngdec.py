"""GPU: mp_png_decode_dev (csrc/k_pngdec.hip) against mp_png_decode_host, in pixels and statuses, on
every file of tests/pngdec_cases.py -- tests/test_pngdec_cpu.py holds the host to the writer's pixels, so
equal frames are right frames.  The refusal files go through in one call a shape: they are the ones the
sanitizer-built host program of the same rule has refused cleanly on the CPU; the corruption sweep stays
there.  Also: two calls agree, a frame does not depend on its batch, nothing outside out and status is
written, entry refusals touch nothing, encode -> decode on the device, the pipelines on decoded frames,
and the call is ordered on the caller's stream."""
import functools

import numpy as np
import pytest
import torch

import png_cases as PC
import pngdec_cases as C
import stream_order_cases as SO
from helpers import pkg

CAM = (365.456, 365.456, 256, 212, [800, 800, 1200], 200, 10000)
GOOD_GROUPS, BAD_GROUPS = C.groups(C.good()), C.groups(C.bad())


def _decode_dev(files, h, w, fmt):
    """(frames, status) as numpy of the files through decode_png on the device"""
    buf, sizes = C.P().pack_files(files)
    frames, status = C.P().decode_png(torch.from_numpy(buf).cuda(), torch.from_numpy(sizes).cuda(), h, w, format=fmt,
                                      check=False)
    torch.cuda.synchronize()
    fr = frames.cpu()
    return (fr.view(torch.int16).numpy().view(np.uint16) if fmt == "gray16" else fr.numpy()), status.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("group", range(len(GOOD_GROUPS)), ids=["%dx%d-%s" % k for k, _ in GOOD_GROUPS])
def test_device_equals_host_on_good_files(group):
    (h, w, fmt), names = GOOD_GROUPS[group]
    frames, status = _decode_dev([C.good()[n].data for n in names], h, w, fmt)
    ref = C.host_decoded("good")
    for i, n in enumerate(names):
        assert status[i] == ref[n][1] == 0, n
        assert np.array_equal(frames[i], ref[n][0]), n


@pytest.mark.gpu
@pytest.mark.parametrize("group", range(len(BAD_GROUPS)), ids=["%dx%d-%s" % k for k, _ in BAD_GROUPS])
def test_refusals_in_one_call(group):
    (h, w, fmt), names = BAD_GROUPS[group]
    good = C.write_png(C._pix("gpu-neighbour", h, w, fmt), fmt, filters=4)
    files = [good]
    for n in names:
        files += [C.bad()[n].data, good]
    frames, status = _decode_dev(files, h, w, fmt)
    ref = C.host_decoded("bad")
    assert not status[0::2].any() and all(np.array_equal(f, C._pix("gpu-neighbour", h, w, fmt)) for f in frames[0::2])
    for i, n in enumerate(names):
        assert status[1 + 2 * i] == ref[n][1] != 0, n
        assert not frames[1 + 2 * i].any(), n


@pytest.mark.gpu
def test_real_shape_frames():
    files, frames = C.real_frames()
    got, status = _decode_dev(files, 424, 512, "gray16")
    assert not status.any() and np.array_equal(got, frames)


@pytest.mark.gpu
def test_two_calls_agree_and_buffers_are_reused():
    P = C.P()
    files, frames = C.real_frames()
    buf, sizes = (torch.from_numpy(a).cuda() for a in P.pack_files(files[:2]))
    f1 = P.decode_png(buf, sizes, 424, 512)
    a = f1.cpu()
    f2 = P.decode_png(buf, sizes, 424, 512)
    assert f2.data_ptr() == f1.data_ptr() and f2.dtype == torch.uint16
    assert torch.equal(a.view(torch.int16), f2.cpu().view(torch.int16))
    assert np.array_equal(a.view(torch.int16).numpy().view(np.uint16), frames[:2])
    bad = torch.from_numpy(P.pack_files([files[0], files[1][:-20]])[0]).cuda()
    with pytest.raises(ValueError, match="file 1 .*status 1"):
        P.decode_png(bad, torch.tensor([len(files[0]), len(files[1]) - 20], device="cuda"), 424, 512)


@pytest.mark.gpu
def test_a_frame_does_not_depend_on_its_batch():
    names = [n for n, c in C.good().items() if (c.h, c.w, c.fmt) == (12, 13, "gray16")]
    files = [C.good()[n].data for n in names]
    all_, st = _decode_dev(files, 12, 13, "gray16")
    assert not st.any()
    for i, f in enumerate(files):
        one, s1 = _decode_dev([f], 12, 13, "gray16")
        assert s1[0] == 0 and np.array_equal(one[0], all_[i])


@pytest.mark.gpu
def test_odd_addresses_a_wider_stride_and_guards():
    lib = C.P()._lib_png()
    names = [n for n, c in C.good().items() if (c.h, c.w, c.fmt) == (12, 13, "rgb8")]
    files = [C.good()[n].data for n in names] + [C.bad()["filter-5"].data]      # the last one fails: wrong shape
    n, stride, guard = len(files), max(map(len, files)) + 5, 64
    src = np.full(guard + 1 + n * stride + guard, 0xA5, np.uint8)
    for i, f in enumerate(files):
        src[guard + 1 + i * stride:guard + 1 + i * stride + len(f)] = np.frombuffer(f, np.uint8)
    d_src = torch.from_numpy(src).cuda()
    sizes = torch.tensor([len(f) for f in files], dtype=torch.int64, device="cuda")
    image = 12 * 13 * 3
    out = torch.full((guard + 1 + n * image + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    status = torch.full((n + 2,), -7, dtype=torch.int32, device="cuda")
    work = torch.empty(lib.mp_png_decode_work_bytes(n, 12, 13, 2, stride), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    assert lib.mp_png_decode_dev(d_src.data_ptr() + guard + 1, stride, sizes.data_ptr(), n, 12, 13, 2,
                                 out.data_ptr() + guard + 1, status.data_ptr() + 4, work.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(d_src.cpu().numpy(), src)
    o = out.cpu().numpy()
    assert (o[:guard + 1] == 0xA5).all() and (o[guard + 1 + n * image:] == 0xA5).all()
    assert status.cpu().tolist() == [-7] + [0] * (n - 1) + [C.ST_MISMATCH, -7]
    body = o[guard + 1:guard + 1 + n * image].reshape(n, 12, 13, 3)
    for i, name in enumerate(names):
        assert np.array_equal(body[i], C.good()[name].pixels)
    assert not body[-1].any()


@pytest.mark.gpu
def test_entry_refusals_touch_nothing():
    lib = C.P()._lib_png()
    good = C.write_png(C._pix("entry", 4, 4, "gray16"), "gray16")
    files = torch.from_numpy(np.frombuffer(good, np.uint8).copy()).cuda()
    stride = files.numel()
    sizes = torch.tensor([stride], dtype=torch.int64, device="cuda")
    out = torch.full((34,), 0x5A, dtype=torch.uint8, device="cuda")
    status = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    work = torch.empty(lib.mp_png_decode_work_bytes(1, 4, 4, 0, stride) + 16, dtype=torch.uint8, device="cuda")
    f, s, o, t, wk = files.data_ptr(), sizes.data_ptr(), out.data_ptr(), status.data_ptr(), work.data_ptr()
    for n, h, w, fmt, sd in ((0, 4, 4, 0, stride), (65536, 4, 4, 0, stride), (1, 0, 4, 0, stride), (1, 4, 4097, 0, stride),
                             (1, 4, 4, 3, stride), (1, 4, 4, 0, 0), (1, 4, 4, 0, (1 << 30) + 1)):
        assert lib.mp_png_decode_dev(f, sd, s, n, h, w, fmt, o, t, wk, None) == -5
    for args in ((None, stride, s, 1, 4, 4, 0, o, t, wk), (f, stride, None, 1, 4, 4, 0, o, t, wk),
                 (f, stride, s, 1, 4, 4, 0, None, t, wk), (f, stride, s, 1, 4, 4, 0, o, None, wk),
                 (f, stride, s, 1, 4, 4, 0, o, t, None), (f, stride, s, 1, 4, 4, 0, o, t, wk + 4),
                 (f, stride, s, 1, 4, 4, 0, o + 1, t, wk), (f, stride, s, 1, 4, 4, 0, o, t + 2, wk)):
        assert lib.mp_png_decode_dev(*args, None) == -1
    with pytest.raises(ValueError):
        C.P().decode_png(files.view(1, -1), sizes, 4, 4, out=out[:32].view(1, 4, 8))
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x5A).all() and status.cpu().tolist() == [-7, -7]


@pytest.mark.gpu
def test_round_trip_on_the_device():
    P = C.P()
    pic = torch.from_numpy(PC.picture("overlay-jet").copy()).cuda()
    buf, sizes = P.encode_png(pic)
    got = P.decode_png(buf, sizes, 424, 512, format="rgb8")         # CUDA in, CUDA out: no host hop but the status
    assert got.is_cuda and torch.equal(got, pic)
    pic3 = torch.from_numpy(PC.picture("n3").copy()).cuda()
    assert torch.equal(P.decode_png(*P.encode_png(pic3), 20, 30, format="rgb8"), pic3)


@functools.lru_cache(maxsize=None)
def _frames_u16(n):
    from oracle import crop_ref as CR
    return np.stack([CR.synth_frame(s).astype(np.uint16) for s in range(n)])


@pytest.mark.gpu
def test_detector_pipeline_on_decoded_frames():
    Pk = pkg()
    Wt, T, M, P = Pk.weights, Pk.train_cnn_networks_hgru, Pk.monkeydetector, Pk.png
    pm = Pk.hgru_pose.model()
    pm.load_weights(Wt.synth_weights(Wt.hgru_pose_vars(output_shape=69, timesteps=8, crop=64), seed=1234, timesteps=8))
    dp = T.DetectorPosePipeline(pm, M.MonkeyDetector(*CAM), dsize=64)
    h2 = torch.from_numpy(Wt.synth_hidden((2, 32, 32, 64), seed=7)).cuda()
    files = C.real_frames()[0][:2]
    ref = [t.detach().cpu().numpy().copy() for t in dp.run(torch.from_numpy(_frames_u16(2).copy()).cuda(), h2_init=h2)]
    dec = P.decode_png_files(files, device="cuda")
    assert dec.dtype == torch.uint16 and tuple(dec.shape) == (2, 424, 512)
    got = [t.detach().cpu().numpy() for t in dp.run(dec, h2_init=h2)]
    assert len(got) == len(ref) == 4
    for a, b in zip(got, ref):
        assert a.tobytes() == b.tobytes()


@pytest.mark.gpu
def test_eval_model_on_real_data_reads_png_frames(tmp_path):
    Pk = pkg()
    Wt, T, M = Pk.weights, Pk.train_cnn_networks_hgru, Pk.monkeydetector
    w = dict(Wt.attn_synth_weights(seed=1234))
    w["cnn/afc_out/afc_out_weights"] = np.zeros((1024, 3), np.float32)
    w["cnn/afc_out/afc_out_biases"] = np.asarray((0.5, 0.5, 0.13), np.float32)
    attn = T.attn_model_struct()
    attn.load_weights(w)
    pose = T.cnn_model_struct()
    pose.load_weights(Wt.synth_weights(Wt.cnn_vars(output_shape=69, crop=128), seed=77))
    md = M.MonkeyDetector(*CAM)
    files = C.real_frames()[0][:3]
    for i, f in enumerate(files):
        (tmp_path / f"depth_{i:06d}.png").write_bytes(f)
    with pytest.raises(ValueError, match="transposed"):
        T.eval_model_on_real_data(str(tmp_path) + "/", T.RealDataPipeline(attn, pose, md))       # transposed=True
    pipe = T.RealDataPipeline(attn, pose, md, transposed=False)
    names, xyz, uvd, coms = T.eval_model_on_real_data(str(tmp_path) + "/", pipe, batch_size=2)
    assert [n.rsplit("/", 1)[1] for n in names] == [f"depth_{i:06d}.png" for i in range(3)]
    ref = [[], [], []]
    for i in (0, 2):
        res = pipe.run(torch.from_numpy(_frames_u16(3)[i:i + 2].copy()).cuda())
        for acc, t in zip(ref, res[:3]):
            acc.append(t.detach().cpu().numpy().copy())
    for got, want in zip((xyz, uvd, coms), ref):
        assert got.tobytes() == np.concatenate(want).tobytes()
    (tmp_path / "depth_000003.png").write_bytes(C.good()["fixed-small"].data)     # another shape: refused up front
    with pytest.raises(ValueError, match="share one shape"):
        T.eval_model_on_real_data(str(tmp_path) + "/", pipe, batch_size=2)


@pytest.mark.gpu
@pytest.mark.parametrize("case", C.PNGDEC_STREAM_CASES, ids=[c.name for c in C.PNGDEC_STREAM_CASES])
def test_decode_is_ordered_on_its_stream(case):
    prep = SO.Prepared(case())
    try:
        for label, s in SO.caller_streams():
            report = SO.check_hazards([prep], [s], label)
            assert len(report) == 2 and all("conclusive" in r for r in report)
    finally:
        prep.close()
