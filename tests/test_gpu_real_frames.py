"""GPU: mp_real_frames_dev through monkeydetector.preprocess_real_frames -- recorded camera frames
(uint16 or float32, stored [w, h] or already [h, w]) -> transpose, depth gate, one float32 division
by the maximum depth -- against the host function of the same name (vectorised numpy, pinned to the
reference's lines in tests/test_real_frames_cpu.py).  Every comparison is of the float32 bit
patterns: each operation is exactly specified, so there is no tolerance."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from helpers import pkg

EDGE = (0, 999, 1000, 1001, 2999, 3000, 3001, 9999, 10000, 65535)
TILE = 64
# (n, w, h): one pixel; odd frames (uint16 frames 1 and 2 start 70 and 140 bytes in); one off a tile
# edge each way; every uint16 value once; the camera's shape
CASES = [(1, 1, 1), (3, 7, 5), (2, 65, 63), (2, 63, 65), (1, 256, 256), (2, 512, 424)]
MP_ERR_ARG, MP_ERR_SHAPE = -1, -5


def _edge_values(kind):
    vals = [float(v) for v in EDGE]
    if kind == "f32":
        vals += [np.nan, np.inf, -np.inf, -0.0, float(np.nextafter(np.float32(1000), np.float32(0))),
                 float(np.nextafter(np.float32(3000), np.float32(1e9)))]
    return np.array(vals, np.float64).astype(np.uint16 if kind == "u16" else np.float32)


def _marks(d):
    """first and last index, and one either side of every tile boundary"""
    m = {0, d - 1}
    for t in range(TILE, d + 1, TILE):
        m.update(v for v in (t - 1, t, t + 1) if v < d)
    return sorted(m)


@functools.lru_cache(maxsize=None)
def _raw(kind, n, d1, d2):
    dt = np.uint16 if kind == "u16" else np.float32
    if (n, d1, d2) == (1, 256, 256):
        out = np.random.RandomState(3).permutation(65536).astype(dt).reshape(1, 256, 256)
        if kind == "u16":
            assert np.array_equal(np.sort(out.reshape(-1)), np.arange(65536))
            out.setflags(write=False)
            return out
    else:
        out = np.random.RandomState(n * 1000 + d1).randint(500, 3600, size=(n, d1, d2)).astype(dt)
    vals = _edge_values(kind)
    for f in range(n):      # the edge values along the first / last row and column and every tile border
        for r in _marks(d1):
            out[f, r, :] = np.resize(np.roll(vals, r + f), d2)
        for c in _marks(d2):
            out[f, :, c] = np.resize(np.roll(vals, c + 3 + f), d1)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _host(kind, n, d1, d2, transposed, gate=(1000, 3000), fill=10000, max_depth=10000.):
    out = pkg().monkeydetector.preprocess_real_frames(_raw(kind, n, d1, d2), transposed, gate, fill, max_depth)
    out.setflags(write=False)
    return out


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("transposed", [True, False], ids=["stored", "plain"])
@pytest.mark.parametrize("kind", ["u16", "f32"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_device_preprocess_bit_exact_with_host(case, kind, transposed):
    P = pkg().monkeydetector
    n, d1, d2 = case
    raw = _raw(kind, n, d1, d2)
    rd = torch.from_numpy(raw.copy()).cuda()
    assert rd.dtype == (torch.uint16 if kind == "u16" else torch.float32)
    got = P.preprocess_real_frames(rd, transposed=transposed)
    h, w = (d2, d1) if transposed else (d1, d2)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (n, h, w, 1) and got.is_contiguous()
    ref = _host(kind, n, d1, d2, transposed)
    g = _bits(got)
    bad = np.argwhere(g != _bits(ref))
    print(case, kind, transposed, "mismatches:", len(bad), bad[:5].tolist())
    assert np.array_equal(g, _bits(ref))
    if case == (1, 256, 256) and kind == "u16":            # the division, for all 65536 inputs
        assert np.unique(raw).size == 65536
        plain = P.preprocess_real_frames(rd, transposed=transposed, gate=None)
        assert np.array_equal(_bits(plain), _bits(_host(kind, n, d1, d2, transposed, None)))
        assert np.unique(plain.cpu().numpy()).size == 65536


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_device_preprocess_gate_options(kind):
    P = pkg().monkeydetector
    n, d1, d2 = 2, 65, 63
    rd = torch.from_numpy(_raw(kind, n, d1, d2).copy()).cuda()
    for tr in (True, False):
        for gate, fill, md in ((None, 10000, 10000.), ((999, 3001), 7, 10000.), ((1001, 2999), 0, 4096.),
                               ((0, 65535), 1, 3.)):
            got = P.preprocess_real_frames(rd, tr, gate, fill, md)
            assert np.array_equal(_bits(got), _bits(_host(kind, n, d1, d2, tr, gate, fill, md))), (tr, gate, fill, md)
    if kind == "f32":       # a fractional float gate and a negative fill
        below = float(np.nextafter(np.float32(1000), np.float32(0)))
        got = P.preprocess_real_frames(rd, True, (below, 3000.0001), -2.5)
        assert np.array_equal(_bits(got), _bits(_host(kind, n, d1, d2, True, (below, 3000.0001), -2.5)))


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(3, 7, 5), (2, 65, 63)], ids=lambda c: "x".join(map(str, c)))
def test_device_preprocess_of_a_two_byte_aligned_view(case):
    """uint16 frames from an address that is no multiple of 4, and an output 4 bytes off a 16-byte
    boundary: the scalar paths"""
    P = pkg().monkeydetector
    n, d1, d2 = case
    raw = _raw("u16", n, d1, d2)
    buf = np.full(raw.size + 1, 2000, np.uint16)
    buf[1:] = raw.reshape(-1)
    whole = torch.from_numpy(buf).cuda()
    view = whole[1:].view(n, d1, d2)
    assert view.data_ptr() % 4 == 2 and view.is_contiguous()
    obuf = torch.full((raw.size + 2,), -1.0, dtype=torch.float32, device="cuda")
    for tr in (True, False):
        got = P.preprocess_real_frames(view, transposed=tr)
        assert np.array_equal(_bits(got), _bits(_host("u16", n, d1, d2, tr)))
        obuf.fill_(-1.0)
        out = obuf[1:-1]
        assert out.data_ptr() % 16 == 4
        got = P.preprocess_real_frames(view, transposed=tr, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert np.array_equal(_bits(got), _bits(_host("u16", n, d1, d2, tr)))
        assert obuf[0].item() == -1.0 and obuf[-1].item() == -1.0          # nothing written around it


@pytest.mark.gpu
def test_device_preprocess_out_reuse_and_views():
    P = pkg().monkeydetector
    n, d1, d2 = 2, 65, 63
    a = torch.from_numpy(_raw("u16", n, d1, d2).copy()).cuda()
    b = torch.from_numpy(_raw("f32", n, d1, d2).copy()).cuda()
    out = torch.empty((n, d2, d1, 1), dtype=torch.float32, device="cuda")
    r1 = P.preprocess_real_frames(a, out=out)
    assert r1.data_ptr() == out.data_ptr()
    assert np.array_equal(_bits(out), _bits(_host("u16", n, d1, d2, True)))
    r2 = P.preprocess_real_frames(b, out=out, stream=torch.cuda.current_stream().cuda_stream)
    assert r2.data_ptr() == out.data_ptr()
    assert np.array_equal(_bits(out), _bits(_host("f32", n, d1, d2, True)))
    for bad in (torch.empty((n, d2, d1), dtype=torch.float64, device="cuda"),
                torch.empty((n, d2, d1 + 1), dtype=torch.float32, device="cuda"),
                torch.empty((n, d2, 2 * d1), dtype=torch.float32, device="cuda")[:, :, ::2],
                torch.empty((n, d2, d1), dtype=torch.float32)):
        with pytest.raises(ValueError):
            P.preprocess_real_frames(a, out=bad)
    # a single [w, h] frame
    one = P.preprocess_real_frames(a[1])
    assert tuple(one.shape) == (1, d2, d1, 1)
    assert np.array_equal(_bits(one), _bits(_host("u16", n, d1, d2, True))[1:2])
    # non-contiguous views give the result of their contiguous copy
    for t, kind in ((a, "u16"), (b, "f32")):
        tv = t.transpose(1, 2)                          # [n, h, w] seen through strides
        assert not tv.is_contiguous()
        got = P.preprocess_real_frames(tv, transposed=False)
        assert np.array_equal(_bits(got), _bits(_host(kind, n, d1, d2, True)))
        wide = torch.from_numpy(np.concatenate([_raw(kind, n, d1, d2)] * 2, axis=2)).cuda()[:, :, :d2]
        assert not wide.is_contiguous()
        got = P.preprocess_real_frames(wide)
        assert np.array_equal(_bits(got), _bits(_host(kind, n, d1, d2, True)))


@pytest.mark.gpu
def test_device_preprocess_rejects_bad_arguments_before_any_launch():
    P = pkg()
    M = P.monkeydetector
    good = torch.from_numpy(np.zeros((2, 6, 4), np.uint16)).cuda()
    for dt in (torch.int32, torch.float64, torch.float16, torch.uint8, torch.int16):
        with pytest.raises(TypeError, match="host preprocess_real_frames"):
            M.preprocess_real_frames(torch.zeros((2, 6, 4), dtype=dt, device="cuda"))
    for shape in ((6,), (2, 6, 4, 1), (0, 6, 4), (2, 0, 4)):
        with pytest.raises(ValueError):
            M.preprocess_real_frames(torch.zeros(shape, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="65535"):
        M.preprocess_real_frames(torch.from_numpy(np.zeros((65536, 1, 1), np.uint16)).cuda())
    with pytest.raises(TypeError, match="CUDA"):
        M.preprocess_real_frames(torch.from_numpy(np.zeros((2, 6, 4), np.uint16)))
    for kw in (dict(gate=(-1, 3000)), dict(gate=(1000, 65536)), dict(fill=65536), dict(gate=(1000.5, 3000)),
               dict(max_depth=0.0), dict(max_depth=float("nan")), dict(gate=(1000,))):
        with pytest.raises(ValueError):
            M.preprocess_real_frames(good, **kw)
    # the C entry itself: MP_ERR_ARG / MP_ERR_SHAPE before any launch
    lib = M._lib_crop()
    out = torch.full((2 * 6 * 4,), -1.0, dtype=torch.float32, device="cuda")
    r, o, vp = good.data_ptr(), out.data_ptr(), ctypes.c_void_p

    def call(raw=r, dt=M.DEPTH_U16, n=2, h=4, w=6, tr=1, gate=1, lo=1000., hi=3000., fill=10000., md=10000., dst=o):
        return lib.mp_real_frames_dev(vp(raw), dt, n, h, w, tr, gate, lo, hi, fill, md, vp(dst), vp(0))

    bad_arg = [dict(raw=None), dict(dst=None), dict(dt=2), dict(dt=-1), dict(raw=r + 1), dict(dt=M.DEPTH_F32, raw=r + 2),
               dict(dst=o + 2), dict(tr=2), dict(gate=-1), dict(lo=-1.), dict(hi=65536.), dict(fill=0.5),
               dict(lo=float("nan")), dict(md=0.), dict(md=float("nan")), dict(md=1e-60)]
    bad_shape = [dict(n=0), dict(n=65536), dict(h=0), dict(w=-3), dict(h=1 << 20, w=1 << 11), dict(h=1 << 62, w=4)]
    for kw in bad_arg:
        assert call(**kw) == MP_ERR_ARG, kw
        assert lib.mp_last_error()
    for kw in bad_shape:
        assert call(**kw) == MP_ERR_SHAPE, kw
    torch.cuda.synchronize()
    assert (out == -1.0).all().item()                      # nothing was launched
    assert call(gate=0, lo=-1., fill=0.5) == 0             # without a gate its numbers are not read
    torch.cuda.synchronize()
    assert (out == 0.0).all().item()
    assert call() == 0
    torch.cuda.synchronize()
    assert (out == 1.0).all().item()                       # zeros are gated to the fill: 10000 / 10000
