"""GPU: mp_png16_encode_dev (csrc/k_png16.hip) against mp_png16_encode_host, byte for byte, on every case
of tests/png16_cases.py -- tests/test_png16_cpu.py holds the host's files to the frames through PIL, zlib
and the library's decoder, so equal bytes are right pixels.  Also: nothing is written past a file's end
or outside out (an odd address, a wider stride), the device decoder reads the device encoder's files,
two encodes on two streams into separate buffers are both right and each is ordered on its stream,
tools/npy_to_png.py's directory gives eval_model_on_real_data the joints of the .npy directory, and
the RGB encoder still writes its host's bytes."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import png16_cases as C
import png_cases as PC
import stream_order_cases as SO
from helpers import ROOT, pkg
from oracle import crop_ref as CR

SENTINEL = 0xA5
CAM = (365.456, 365.456, 256, 212, [800, 800, 1200], 200, 10000)


def _u16(a):
    """a numpy uint16 array as a CUDA torch.uint16 tensor (a copy: the cases are read-only)"""
    return torch.from_numpy(np.array(a)).cuda()


def _dev(name):
    """(buf, sizes) as numpy of the case through mp_png16_encode_dev into a sentinel-filled buffer"""
    P = C.P()
    x = C.frames(name)
    n, h, w = x.shape
    buf = torch.full((n, P.depth_png_bound(h, w)), SENTINEL, dtype=torch.uint8, device="cuda")
    sizes = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    P.encode_depth_png(_u16(x), out=(buf, sizes))
    torch.cuda.synchronize()
    return buf.cpu().numpy(), sizes.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", C.NAMES)
def test_device_files_equal_the_host_files(name):
    ref, rs = C.host_files(name)
    buf, sizes = _dev(name)
    assert np.array_equal(sizes, rs)
    for i, s in enumerate(rs):
        assert buf[i, :s].tobytes() == ref[i, :s].tobytes(), f"frame {i}"
        assert (buf[i, s:] == SENTINEL).all(), f"frame {i}: bytes past the file's end were written"


@pytest.mark.gpu
def test_odd_addresses_a_wider_stride_and_guards():
    P = C.P()
    lib = P._lib_png()
    x = C.frames("n3")
    n, h, w = x.shape
    bound = P.depth_png_bound(h, w)
    stride, guard = bound + 3, 64
    src = torch.zeros(x.size + 1, dtype=torch.int16, device="cuda")           # frames at an address that is 2 mod 4
    src[1:] = torch.from_numpy(x.view(np.int16).copy()).cuda().view(-1)
    dst = torch.full((guard + 1 + n * stride + guard,), SENTINEL, dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(n, dtype=torch.int64, device="cuda")
    work = torch.empty(lib.mp_png16_work_bytes(n, h, w), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    assert lib.mp_png16_encode_dev(src.data_ptr() + 2, n, h, w, dst.data_ptr() + guard + 1, stride, sizes.data_ptr(),
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
    bound = P.depth_png_bound(4, 4)
    fr = torch.zeros((1, 4, 4), dtype=torch.uint16, device="cuda")
    out = torch.full((bound,), SENTINEL, dtype=torch.uint8, device="cuda")
    sizes = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    work = torch.empty(lib.mp_png16_work_bytes(1, 4, 4), dtype=torch.uint8, device="cuda")
    p, o, s, wk = fr.data_ptr(), out.data_ptr(), sizes.data_ptr(), work.data_ptr()
    for n, h, w, stride in ((0, 4, 4, bound), (65536, 4, 4, bound), (1, 0, 4, bound), (1, 4, 4097, 1 << 30),
                            (1, 4, 4, bound - 1)):
        assert lib.mp_png16_encode_dev(p, n, h, w, o, stride, s, wk, None) == -5
    for args in ((None, 1, 4, 4, o, bound, s, wk), (p, 1, 4, 4, None, bound, s, wk), (p, 1, 4, 4, o, bound, None, wk),
                 (p, 1, 4, 4, o, bound, s, None), (p, 1, 4, 4, o, bound, s, wk + 4), (p + 1, 1, 4, 4, o, bound, s, wk)):
        assert lib.mp_png16_encode_dev(*args, None) == -1
    with pytest.raises(ValueError):
        P.encode_depth_png(fr, out=(out.view(1, -1)[:, :bound - 1], sizes))
    with pytest.raises(TypeError):
        P.encode_depth_png(fr.view(torch.int16))
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all() and int(sizes.cpu()[0]) == -7


@pytest.mark.gpu
@pytest.mark.parametrize("name", C.NAMES)
def test_device_decode_of_device_encode_is_the_frame(name):
    P = C.P()
    x = C.frames(name)
    buf, sizes = P.encode_depth_png(_u16(x))
    got, status = P.decode_png(buf, sizes, x.shape[1], x.shape[2], check=False)
    assert not status.cpu().numpy().any()
    assert got.dtype == torch.uint16 and np.array_equal(got.cpu().numpy(), x)


@pytest.mark.gpu
def test_two_calls_agree_and_buffers_are_reused():
    P = C.P()
    x = _u16(C.frames("n3"))
    b1, s1 = P.encode_depth_png(x)
    f1 = P.png_files(b1, s1)
    b2, s2 = P.encode_depth_png(x)
    assert b2.data_ptr() == b1.data_ptr() and s2.data_ptr() == s1.data_ptr()
    assert P.png_files(b2, s2) == f1
    ref, rs = C.host_files("n3")
    assert f1 == [ref[i, :s].tobytes() for i, s in enumerate(rs)]
    for i in range(3):                                           # a file does not depend on its batch
        assert P.png_files(*P.encode_depth_png(x[i:i + 1])) == [f1[i]]


@pytest.mark.gpu
def test_two_encodes_on_two_streams_are_both_right():
    """stream_order_cases' hazards (late producer, immediate consumer, early release, back to back) for
    two calls of different frames at once, each on a stream of its own into buffers of its own"""
    preps = [SO.Prepared(C.Png16Case(draw)) for draw in (0, 1)]
    try:
        assert not np.array_equal(preps[0].A["frames"], preps[1].A["frames"])
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        report = SO.check_hazards(preps, streams, "two fresh streams")
        assert len(report) == 2 and all("conclusive" in r for r in report)
    finally:
        for p in preps:
            p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", C.PNG16_STREAM_CASES, ids=[c.name for c in C.PNG16_STREAM_CASES])
def test_encode_is_ordered_on_its_stream(case):
    prep = SO.Prepared(case())
    try:
        for label, s in SO.caller_streams():
            report = SO.check_hazards([prep], [s], label)
            assert len(report) == 2 and all("conclusive" in r for r in report)
    finally:
        prep.close()


@functools.lru_cache(maxsize=None)
def _raw():
    """four recorded frames as stored: uint16 [512, 424] (tests/test_gpu_real_pipeline.py's shape)"""
    return np.stack([np.ascontiguousarray(CR.synth_frame(s).astype(np.uint16).T) for s in range(4)])


def _tool():
    spec = importlib.util.spec_from_file_location("npy_to_png", os.path.join(ROOT, "tools", "npy_to_png.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
def test_npy_to_png_directory_gives_the_npy_directory_joints(tmp_path, capsys):
    Pk = pkg()
    Wt, T, M, P = Pk.weights, Pk.train_cnn_networks_hgru, Pk.monkeydetector, Pk.png
    src, dst, hostdst = tmp_path / "npy", tmp_path / "png", tmp_path / "png_host"
    src.mkdir()
    for i, a in enumerate(_raw()):
        np.save(src / f"frame_{i:02d}.npy", a)
    tool = _tool()
    assert tool.main([str(src), str(dst), "--batch", "3"]) == 0              # a batch of 3 and one of 1
    assert "4 frames" in capsys.readouterr().out
    names = sorted(os.listdir(dst))
    assert names == [f"depth_{i:06d}.png" for i in range(4)] + ["files.txt"]
    assert tool.main([str(src), str(hostdst), "--host"]) == 0                # the same bytes from the host
    for nme in names[:4]:
        assert (dst / nme).read_bytes() == (hostdst / nme).read_bytes()
    assert P.png_info((dst / names[0]).read_bytes()) == (424, 512, "gray16")
    assert np.array_equal(P.decode_png_files([str(dst / nme) for nme in names[:4]]), _raw().transpose(0, 2, 1))

    w = dict(Wt.attn_synth_weights(seed=1234))
    w["cnn/afc_out/afc_out_weights"] = np.zeros((1024, 3), np.float32)
    w["cnn/afc_out/afc_out_biases"] = np.asarray((0.5, 0.5, 0.13), np.float32)
    attn = T.attn_model_struct()
    attn.load_weights(w)
    pose = T.cnn_model_struct()
    pose.load_weights(Wt.synth_weights(Wt.cnn_vars(output_shape=69, crop=128), seed=77))
    md = M.MonkeyDetector(*CAM)
    ref = T.eval_model_on_real_data(str(src) + "/", T.RealDataPipeline(attn, pose, md), batch_size=3)
    got = T.eval_model_on_real_data(str(dst) + "/", T.RealDataPipeline(attn, pose, md, transposed=False), batch_size=3)
    assert len(ref[0]) == len(got[0]) == 4
    for a, b in zip(got[1:], ref[1:]):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("name", PC.NAMES)
def test_the_rgb_encoder_still_writes_its_host_files(name):
    P = C.P()
    pic = PC.picture(name)
    n, h, w, _ = pic.shape
    ref, rs = PC.host_files(name)
    buf = torch.full((n, P.png_bound(h, w)), SENTINEL, dtype=torch.uint8, device="cuda")
    sizes = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    P.encode_png(torch.from_numpy(pic.copy()).cuda(), out=(buf, sizes))
    torch.cuda.synchronize()
    buf, sizes = buf.cpu().numpy(), sizes.cpu().numpy()
    assert np.array_equal(sizes, rs)
    for i, s in enumerate(rs):
        assert buf[i, :s].tobytes() == ref[i, :s].tobytes() and (buf[i, s:] == SENTINEL).all()
