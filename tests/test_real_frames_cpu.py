"""CPU: the host half of the real-data evaluation (eval_model_on_real_data, reference
train_cnn_networks_hgru.py:342-419) -- monkeydetector.preprocess_real_frames on numpy arrays against
the reference's lines written out here, the float32 / float64 crop-route equivalence that
RealDataPipeline's docstring states (through oracle.crop_ref), and eval_model_on_real_data's file
handling with a stub pipeline.  Every comparison is exact: np.array_equal, and the bit patterns
where a frame holds NaN or -0.0."""
import functools

import numpy as np
import pytest
import torch

from helpers import pkg
from oracle import crop_ref as CR

EDGE = (0, 999, 1000, 1001, 2999, 3000, 3001, 9999, 10000, 65535)


def _f32_edges():
    below = np.nextafter(np.float32(1000), np.float32(0))
    above = np.nextafter(np.float32(3000), np.float32(1e9))
    assert np.float32(999.99994) == below and np.float32(3000.0002) == above
    return [np.nan, np.inf, -np.inf, -0.0, below, above]


def _reference(raw_frame, lo=1000, hi=3000, fill=10000, max_depth=10000., gate=True, transposed=True):
    """lines 388-392 and 359 for one stored frame: the feed is a float32 placeholder"""
    im = np.transpose(raw_frame.copy()) if transposed else raw_frame.copy()
    if gate:
        im[(im < lo)] = fill
        im[(im > hi)] = fill
    im = np.asarray([im])
    with np.errstate(all="ignore"):
        return im.astype(np.float32)[..., None] / np.float32(max_depth)


def _bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


@functools.lru_cache(maxsize=None)
def _raw(kind, n=3, w=7, h=5):
    """n stored frames [w, h] of synthetic depth with the edge values planted in every frame"""
    rs = np.random.RandomState(5)
    vals = list(EDGE)
    if kind == "f32":
        vals += _f32_edges()
    if kind == "f64":
        vals += [999.9999999, 3000.0000001, 1e300, np.nan]
    dt = {"u16": np.uint16, "f32": np.float32, "f64": np.float64}[kind]
    out = rs.randint(500, 3600, size=(n, w, h)).astype(dt)
    flat = out.reshape(n, -1)
    for f in range(n):
        pos = rs.permutation(w * h)[:len(vals)]
        with np.errstate(all="ignore"):
            flat[f, pos] = np.array(vals, np.float64).astype(dt)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("kind", ["u16", "f32", "f64"])
def test_host_preprocess_equals_the_reference_lines(kind):
    P = pkg().monkeydetector
    raw = _raw(kind)
    got = P.preprocess_real_frames(raw)
    assert got.dtype == np.float32 and got.shape == (3, 5, 7, 1) and got.flags.c_contiguous
    ref = np.concatenate([_reference(f) for f in raw])
    assert np.array_equal(_bits(got), _bits(ref))
    one = P.preprocess_real_frames(raw[1])                # a single [w, h] frame
    assert one.shape == (1, 5, 7, 1) and np.array_equal(_bits(one), _bits(ref[1:2]))
    assert P.MonkeyDetector.preprocess_real_frames is P.preprocess_real_frames
    # what the gate did to the planted values
    vals = np.unique(got[np.isfinite(got)])
    assert np.float32(1.0) in vals and np.float32(0.1) in vals and np.float32(0.3) in vals
    assert not ((vals < np.float32(0.1)) | ((vals > np.float32(0.3)) & (vals < np.float32(1.0)))).any()
    if kind == "f32":
        assert np.isnan(got).sum() == 3 and not np.isinf(got).any()      # NaN passes, +-inf is gated
    assert raw.flags.writeable is False                   # the input is left alone


@pytest.mark.parametrize("kind", ["u16", "f32", "f64"])
def test_host_preprocess_options(kind):
    P = pkg().monkeydetector
    raw = _raw(kind)
    for kw in (dict(gate=None), dict(gate=(999, 3001), fill=7), dict(gate=(1001, 2999), fill=0, max_depth=4096.),
               dict(transposed=False), dict(transposed=False, gate=None, max_depth=3.)):
        got = P.preprocess_real_frames(raw, **kw)
        g = kw.get("gate", (1000, 3000))
        ref = np.concatenate([_reference(f, *(g or (0, 0)), kw.get("fill", 10000), kw.get("max_depth", 10000.),
                                         gate=g is not None, transposed=kw.get("transposed", True)) for f in raw])
        assert got.shape == ref.shape, kw
        assert np.array_equal(_bits(got), _bits(ref)), kw
    if kind == "f32":     # a float gate compares against f32(lo): the neighbour below 1000 passes lo = itself
        below = float(np.nextafter(np.float32(1000), np.float32(0)))
        got = P.preprocess_real_frames(raw, gate=(below, 3000))
        assert (got == np.float32(below) / np.float32(10000)).any()
        with np.errstate(all="ignore"):
            ref = np.concatenate([_reference(f, np.float32(below)) for f in raw])
        assert np.array_equal(_bits(got), _bits(ref))
        neg0 = P.preprocess_real_frames(raw, gate=None)
        assert (_bits(neg0) == 0x80000000).sum() == 3      # -0.0 / 10000 keeps its sign


def test_host_preprocess_argument_errors():
    P = pkg().monkeydetector
    u, f = _raw("u16"), _raw("f32")
    for bad in (dict(gate=(-1, 3000)), dict(gate=(1000, 65536)), dict(fill=70000), dict(gate=(1000.5, 3000)),
                dict(gate=(1000,)), dict(gate=1000), dict(gate=("a", 3)), dict(max_depth=0.), dict(max_depth=float("nan")),
                dict(max_depth=1e-60)):
        with pytest.raises(ValueError):
            P.preprocess_real_frames(u, **bad)
    P.preprocess_real_frames(f, gate=(1000.5, 3000), fill=-1)        # fine for float frames
    P.preprocess_real_frames(u, gate=None, fill=70000)               # no gate: fill is not used
    for shape in ((7,), (2, 3, 4, 5), (0, 4, 4), (2, 0, 3)):
        with pytest.raises(ValueError):
            P.preprocess_real_frames(np.zeros(shape, np.uint16))
    with pytest.raises(TypeError):
        P.preprocess_real_frames(np.zeros((2, 3, 4), np.complex64))
    with pytest.raises(ValueError):
        P.preprocess_real_frames(u, out=np.zeros(3))
    # tensors: the dtype error names the host function, a CPU tensor is no device input; no GPU is touched
    with pytest.raises(TypeError, match="preprocess_real_frames"):
        P.preprocess_real_frames(torch.zeros((2, 3, 4), dtype=torch.int32))
    with pytest.raises(TypeError, match="CUDA"):
        P.preprocess_real_frames(torch.zeros((2, 3, 4), dtype=torch.float32))
    with pytest.raises(ValueError):
        P.preprocess_real_frames(torch.zeros((2, 3, 4, 1), dtype=torch.float32))
    with pytest.raises(ValueError):
        P.preprocess_real_frames(torch.zeros((2, 3, 4), dtype=torch.uint16), gate=(1000, 65536))


def test_uint16_values_through_the_float32_product():
    """f32(v / 10000) * 10000 is not v for 9152 uint16 values, yet / 10000 again lands on the same
    float32 for all of them (the number RealDataPipeline's docstring quotes)"""
    f32 = np.float32
    v = np.arange(65536, dtype=np.uint16)
    norm = v.astype(f32) / f32(10000)
    back = norm * f32(10000)
    assert int((back != v).sum()) == 9152
    assert np.array_equal(back / f32(10000), norm)


@pytest.mark.parametrize("seed", range(10))
def test_float32_crop_route_equals_the_float64_route(seed):
    """The reference crops from float64 (im / 10000.) * 10000. (399, 68); the pipeline crops from the
    float32 normalised frame times 10000 in float32.  Equal patches and M for these frames."""
    P = pkg().monkeydetector
    md = CR.MonkeyDetectorRef()
    raw = np.ascontiguousarray(CR.synth_frame(seed).astype(np.uint16).T)         # stored [w, h]
    im = np.transpose(raw.copy())
    im[(im < 1000)] = 10000
    im[(im > 3000)] = 10000
    ys, xs = np.nonzero(im < 2000)                                                # the body
    assert ys.size > 1000
    com = np.array([xs.mean(), ys.mean(), im[ys, xs].mean()])
    scale = [424, 512, 10000.]
    tr = (com / scale).astype(np.float32)                                         # the attention output
    # float64 route, as the reference runs it
    crop, M64, _, _ = md.cropArea3D((im / 10000.) * 10000., com=tr * scale)
    patch64 = (np.expand_dims(crop, axis=2) / 10000.)
    assert patch64.dtype == np.float32
    # float32 route: the host preprocessing, then prepare_data_test on the normalised frame
    norm = P.preprocess_real_frames(raw)
    patches, Ms, _ = CR.prepare_data_test(norm, tr[None], md)
    assert np.array_equal(patches[0], patch64[..., 0])
    assert np.array_equal(Ms[0], np.asarray(M64))
    body = (patch64 > 0) & (patch64 < 1)
    assert body.sum() > 1000 and (patch64 == 0).any()       # the body in the cube, the gated wall behind it


class _StubPipeline:
    """records its batches; returns the same three buffers every call, like the real pipeline"""

    def __init__(self):
        self.batches = []
        self.buf = None

    def run(self, raw):
        n = raw.shape[0]
        self.batches.append((n, raw.dtype, tuple(raw.shape[1:])))
        if self.buf is None or self.buf[0].shape[0] != n:
            self.buf = (torch.empty((n, 2, 3)), torch.empty((n, 2, 3)), torch.empty((n, 3), dtype=torch.float64))
        tag = raw.reshape(n, -1)[:, 0].to(torch.float64)
        self.buf[0][:] = tag[:, None, None].float()
        self.buf[1][:] = -tag[:, None, None].float()
        self.buf[2][:] = tag[:, None] * 2
        return self.buf + (None, None)


def test_eval_model_on_real_data_files_and_batches(tmp_path):
    T = pkg().train_cnn_networks_hgru
    d = str(tmp_path) + "/"
    order = ["f_10", "f_2", "f_033", "f_1", "f_9"]          # written in this order, tagged 0..4
    for k, name in enumerate(order):
        a = np.full((6, 4), 100 + k, np.uint16)
        np.save(d + name + ".npy", a)
    (tmp_path / "notes.txt").write_text("not a frame")
    stub = _StubPipeline()
    files, xyz, uvd, coms = T.eval_model_on_real_data(d, stub, batch_size=2, device="cpu")
    want = sorted(order)
    assert [f[len(d):-4] for f in files] == want == ["f_033", "f_1", "f_10", "f_2", "f_9"]
    assert stub.batches == [(2, torch.uint16, (6, 4)), (2, torch.uint16, (6, 4)), (1, torch.uint16, (6, 4))]
    tags = np.array([100 + order.index(n) for n in want], np.float64)
    assert xyz.shape == (5, 2, 3) and uvd.shape == (5, 2, 3) and coms.shape == (5, 3) and coms.dtype == np.float64
    assert np.array_equal(xyz[:, 0, 0], tags) and np.array_equal(uvd[:, 1, 2], -tags)
    assert np.array_equal(coms[:, 0], 2 * tags)
    # one batch holds them all
    stub2 = _StubPipeline()
    _, xyz2, _, _ = T.eval_model_on_real_data(d, stub2, batch_size=8, device="cpu")
    assert stub2.batches == [(5, torch.uint16, (6, 4))] and np.array_equal(xyz2, xyz)
    # a frame of another shape, then of another dtype: a clear error, before any batch is run
    np.save(d + "f_5.npy", np.zeros((4, 6), np.uint16))
    stub3 = _StubPipeline()
    with pytest.raises(ValueError, match="f_5.npy"):
        T.eval_model_on_real_data(d, stub3, batch_size=2, device="cpu")
    assert stub3.batches == []
    np.save(d + "f_5.npy", np.zeros((6, 4), np.float32))
    with pytest.raises(ValueError, match="share one shape and dtype"):
        T.eval_model_on_real_data(d, stub3, batch_size=2, device="cpu")
    np.save(d + "f_5.npy", np.zeros((6, 4), np.uint16))
    assert len(T.eval_model_on_real_data(d, stub3, batch_size=4, device="cpu")[0]) == 6
    with pytest.raises(ValueError):
        T.eval_model_on_real_data(str(tmp_path / "empty") + "/", stub3, device="cpu")
    with pytest.raises(ValueError):
        T.eval_model_on_real_data(d, stub3, batch_size=0, device="cpu")
