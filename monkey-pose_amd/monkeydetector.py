"""Drop-in for ``/root/reference/monkeydetector.py`` / ``tf_monkeydetector.py`` (inference geometry).

``MonkeyDetector(fx, fy, ux, uy, cube, d1, d2).cropArea3D(dpt, com)`` -> (crop, M, com) runs in
native code (``mp_crop3d`` in libmonkeypose.so, host C++, bit-exact integer bounds / sizes /
offsets / nearest-neighbour indices); ``crop_batch`` is the reference's per-frame loop
(``prepare_data_test``, train_cnn_networks_hgru.py:61-74) in one call, producing the normalised
model input directly.  The small joint-coordinate transforms are vectorised numpy.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import _lib


class _Camera(ctypes.Structure):
    _fields_ = [("fx", ctypes.c_double), ("fy", ctypes.c_double), ("ux", ctypes.c_double),
                ("uy", ctypes.c_double), ("cube", ctypes.c_double * 3),
                ("min_depth", ctypes.c_double), ("max_depth", ctypes.c_double)]


_CROP_SIGS = {
    "mp_center_of_mass": (ctypes.c_int, [ctypes.POINTER(_Camera), ctypes.c_void_p, ctypes.c_int,
                                         ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]),
    "mp_crop3d": (ctypes.c_int, [ctypes.POINTER(_Camera), ctypes.c_void_p, ctypes.c_int, ctypes.c_int64,
                                 ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "mp_crop3d_ex": (ctypes.c_int, [ctypes.POINTER(_Camera), ctypes.c_void_p, ctypes.c_int, ctypes.c_int64,
                                    ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p,
                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "mp_crop3d_batch": (ctypes.c_int, [ctypes.POINTER(_Camera), ctypes.c_void_p, ctypes.c_int,
                                       ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
                                       ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_int]),
    "mp_crop3d_dev": (ctypes.c_int, [ctypes.POINTER(_Camera), ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                     ctypes.c_int64, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_void_p]),
    "mp_crop3d_dev_ex": (ctypes.c_int, [ctypes.POINTER(_Camera), ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                        ctypes.c_int64, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "mp_center_of_mass_dev_work": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64]),
    "mp_center_of_mass_dev": (ctypes.c_int, [ctypes.POINTER(_Camera), ctypes.c_void_p, ctypes.c_int64,
                                             ctypes.c_int64, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "mp_crop3d_dev_coms": (ctypes.c_int, [ctypes.POINTER(_Camera), ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                          ctypes.c_int64, ctypes.c_float, ctypes.c_void_p, ctypes.c_int,
                                          ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p]),
    # the same two calls by frame dtype (MP_DEPTH_F32 forwards; MP_DEPTH_U16: uint16 mm frames)
    "mp_center_of_mass_dev_work_dt": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int64, ctypes.c_int64,
                                                        ctypes.c_int64]),
    "mp_center_of_mass_dev_dt": (ctypes.c_int, [ctypes.POINTER(_Camera), ctypes.c_void_p, ctypes.c_int,
                                                ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_float,
                                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                                ctypes.c_void_p]),
    "mp_crop3d_dev_coms_dt": (ctypes.c_int, [ctypes.POINTER(_Camera), ctypes.c_void_p, ctypes.c_int, ctypes.c_int64,
                                             ctypes.c_int64, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p,
                                             ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "mp_abs_joints_dev": (ctypes.c_int, [ctypes.POINTER(_Camera), ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    # recorded camera frames -> the attention net's input (k_real.hip)
    "mp_real_frames_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int64,
                                          ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                          ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_void_p,
                                          ctypes.c_void_p]),
    # joint overlays and crop-space joints (k_overlay.hip)
    "mp_overlay_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                      ctypes.c_float, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "mp_transform_joints_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                               ctypes.c_void_p, ctypes.c_void_p]),
    # the validation pass on the device (k_eval.hip)
    "mp_rel_labels_dev": (ctypes.c_int, [ctypes.POINTER(_Camera), ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "mp_com_from_joints_dev": (ctypes.c_int, [ctypes.POINTER(_Camera), ctypes.c_void_p, ctypes.c_int64,
                                              ctypes.c_int64, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                              ctypes.c_void_p, ctypes.c_void_p]),
    "mp_eval_state_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64]),
    "mp_eval_work_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int64]),
    "mp_eval_reset_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
                                         ctypes.c_void_p]),
    "mp_eval_accumulate_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                              ctypes.c_int64, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p,
                                              ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_void_p]),
    "mp_eval_summary_len": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64]),
    "mp_eval_summary_dev": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
                                           ctypes.c_void_p]),
}

MAX_EVAL_JOINTS = 128       # eval_plan.hpp MAX_JOINTS: numpy's pairwise sum is one leaf up to there
MAX_EVAL_THRESHOLDS = 1024
MAX_DEV_FRAMES = 65535
DEPTH_F32, DEPTH_U16 = 0, 1    # monkeypose.h MP_DEPTH_*

_CROP_MSG = {1: "CoM depth is zero or not finite (no valid pixel in range?)", 2: "empty crop",
             3: "degenerate bounds", 4: "resize target is empty"}


def _lib_crop():
    lib = _lib.load()
    if not getattr(lib, "_crop_bound", False):
        for name, (res, args) in _CROP_SIGS.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        lib._crop_bound = True
    return lib


def _p(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


def _real_gate(gate, fill, max_depth, np_dtype):
    """(lo, hi, fill) as scalars of ``np_dtype`` (``None`` without a gate) and f32(max_depth); an
    integer dtype takes whole numbers in its own range, since the gate runs in the frame's dtype."""
    md = np.float32(max_depth)
    if not (md != 0) or np.isnan(md):
        raise ValueError(f"max_depth must be a non-zero number, got {max_depth!r}")
    if gate is None:
        return None, md
    try:
        lo, hi = gate
    except (TypeError, ValueError):
        raise ValueError(f"gate must be (lo, hi) or None, got {gate!r}") from None
    dt = np.dtype(np_dtype)
    vals = []
    for name, v in (("gate[0]", lo), ("gate[1]", hi), ("fill", fill)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f"{name} must be a real number, got {v!r}")
        if dt.kind in "ui":
            info = np.iinfo(dt)
            if not (float(v) == int(v) and info.min <= int(v) <= info.max):
                raise ValueError(f"{name} must be an integer in [{info.min}, {info.max}] for {dt} frames "
                                 f"(the gate runs in the frames' own dtype), got {v!r}")
            vals.append(dt.type(int(v)))
        else:
            with np.errstate(all="ignore"):
                vals.append(dt.type(v))
    return tuple(vals), md


def preprocess_real_frames(raw, transposed=True, gate=(1000, 3000), fill=10000, max_depth=10000., stream=None,
                           out=None):
    """The preprocessing of ``eval_model_on_real_data`` (train_cnn_networks_hgru.py:388-392, 359) for
    a batch of recorded frames: ``np.transpose`` of each frame as stored (``transposed``: ``raw`` is
    [n, w, h] or a single [w, h]; else [n, h, w]), ``im[im < lo] = fill; im[im > hi] = fill`` in the
    frames' own dtype (``gate=(lo, hi)``; ``None``: no gate), the cast to float32 (the placeholder)
    and one float32 division by ``f32(max_depth)``.  Returns [n, h, w, 1] float32, the attention
    net's input.

    A numpy array (any real dtype) runs vectorised numpy on the host -- the CPU oracle of the
    kernel.  A CUDA tensor, ``torch.uint16`` (the camera's own millimetres, uploaded as they are) or
    ``torch.float32``, runs ``mp_real_frames_dev`` on the current stream (or ``stream``) into
    ``out`` (a contiguous CUDA float32 tensor of n * h * w elements, else a new one) and returns a
    CUDA tensor with the bits of the host function; a non-contiguous view is made contiguous first.
    A float NaN passes the gate and +-inf is gated, as numpy's comparisons decide; a uint16 gate and
    fill are whole numbers in [0, 65535].  Shapes, the frame limit and the argument ranges are
    checked before any GPU call."""
    if isinstance(raw, np.ndarray) or not hasattr(raw, "is_cuda"):
        if stream is not None or out is not None:
            raise ValueError("stream= and out= belong to the device path (a CUDA tensor in)")
        a = np.asarray(raw)
        if a.dtype.kind not in "uif":
            raise TypeError(f"frames must have a real dtype, got {a.dtype}")
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3 or 0 in a.shape:
            raise ValueError(f"raw must be [n, w, h] or [w, h], got {a.shape}")
        g, md = _real_gate(gate, fill, max_depth, a.dtype)
        im = np.transpose(a, (0, 2, 1)) if transposed else a
        with np.errstate(all="ignore"):
            if g is not None:
                im = np.where((im < g[0]) | (im > g[1]), g[2], im)     # = the two masked assignments
            return np.ascontiguousarray(im.astype(np.float32)[..., None] / md)
    import torch
    if raw.dim() == 2:
        raw = raw[None]
    if raw.dim() != 3 or 0 in raw.shape:
        raise ValueError(f"raw must be [n, w, h] or [w, h], got {tuple(raw.shape)}")
    n, d1, d2 = raw.shape
    h, w = (d2, d1) if transposed else (d1, d2)
    if n > MAX_DEV_FRAMES:
        raise ValueError(f"at most {MAX_DEV_FRAMES} frames a call, got {n}")
    if h * w > 1 << 30:
        raise ValueError(f"a frame has at most 2^30 pixels, got {h} x {w}")
    if raw.dtype not in (torch.uint16, torch.float32):
        raise TypeError(f"CUDA frames must be torch.uint16 or torch.float32, got {raw.dtype}: convert them, or "
                        "pass a numpy array to run the host preprocess_real_frames")
    u16 = raw.dtype == torch.uint16
    g, md = _real_gate(gate, fill, max_depth, np.uint16 if u16 else np.float32)
    if not raw.is_cuda:
        raise TypeError("raw must be a CUDA (ROCm) tensor or a numpy array")
    if out is None:
        out = torch.empty((n, h, w, 1), dtype=torch.float32, device=raw.device)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == raw.device
              and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == n * h * w):
        raise ValueError(f"out must be a contiguous CUDA float32 tensor of {n * h * w} elements on {raw.device}")
    r = raw.detach().contiguous()
    st = _lib.current_stream(r.device) if stream is None else stream
    lo, hi, fl = (0.0, 0.0, 0.0) if g is None else (float(v) for v in g)
    _lib.check(_lib_crop().mp_real_frames_dev(ctypes.c_void_p(r.data_ptr()), DEPTH_U16 if u16 else DEPTH_F32, n, h, w,
                                              1 if transposed else 0, 0 if g is None else 1, lo, hi, fl,
                                              float(max_depth), ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(st)))
    return out.view(n, h, w, 1)


# ---------------------------------------------------------------------- joint overlays
# The drawing rule is csrc/overlay_geom.hpp (the kernel's text); render_overlays_np states it in numpy.
OVERLAY_MAX_HW, OVERLAY_MAX_SETS, OVERLAY_MAX_JOINTS, OVERLAY_MAX_BONES = 4096, 4, 128, 256
OVERLAY_MAX_RADIUS, OVERLAY_MAX_THICK = 15, 15
OVERLAY_C_MIN, OVERLAY_C_MAX = -4096, 8191

# per set (marker RGB, bone RGB, marker radius, bone thickness): set 0 (e.g. labels) green, set 1
# (e.g. results) red, then blue and yellow
DEFAULT_OVERLAY_STYLES = (((0, 255, 0), (0, 160, 0), 3, 1), ((255, 0, 0), (200, 0, 0), 3, 1),
                          ((0, 128, 255), (0, 96, 200), 3, 1), ((255, 255, 0), (200, 200, 0), 3, 1))


class _OverlaySetStyle(ctypes.Structure):
    _fields_ = [("marker_rgb", ctypes.c_uint8 * 3), ("radius", ctypes.c_uint8),
                ("bone_rgb", ctypes.c_uint8 * 3), ("thickness", ctypes.c_uint8)]


class OverlayStyle(ctypes.Structure):
    """``mp_overlay_style`` (include/monkeypose.h)."""
    _fields_ = [("struct_size", ctypes.c_uint64), ("sets", _OverlaySetStyle * 4)]


def overlay_lut(name="gray"):
    """The [256, 3] uint8 colour table ``name``.  ``'gray'``: entry k is (k, k, k).  ``'jet'``: the
    piecewise-linear blue - cyan - yellow - red map, with x = k / 255 in float64:
    ``r = clip(1.5 - |4x - 3|, 0, 1)``, ``g = clip(1.5 - |4x - 2|, 0, 1)``,
    ``b = clip(1.5 - |4x - 1|, 0, 1)``, each stored as ``rint(255 c)``."""
    k = np.arange(256)
    if name == "gray":
        return np.repeat(k.astype(np.uint8)[:, None], 3, axis=1)
    if name == "jet":
        x = k / 255.0
        rgb = [np.clip(1.5 - np.abs(4.0 * x - c), 0.0, 1.0) for c in (3.0, 2.0, 1.0)]
        return np.rint(255.0 * np.stack(rgb, axis=1)).astype(np.uint8)
    raise ValueError(f"unknown colour table {name!r}: 'gray' or 'jet'")


def _overlay_lut_array(lut):
    if isinstance(lut, str):
        return overlay_lut(lut)
    a = np.asarray(lut)
    if a.dtype != np.uint8 or a.shape != (256, 3):
        raise ValueError(f"lut must be a name or a [256, 3] uint8 table, got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a)


def _overlay_scene(n, h, w, jshape, bones, depth_range, styles):
    """The checks shared by ``render_overlays`` and ``render_overlays_np``, all before any GPU call ->
    (S, J, bones [nb, 2] int32, f32 lo, f32 hi, styles as S tuples)."""
    if n <= 0 or h <= 0 or w <= 0:
        raise ValueError(f"frames must be a non-empty [n, h, w], got {(n, h, w)}")
    if h > OVERLAY_MAX_HW or w > OVERLAY_MAX_HW:
        raise ValueError(f"h and w are at most {OVERLAY_MAX_HW}, got {h} x {w}")
    if n > MAX_DEV_FRAMES:
        raise ValueError(f"at most {MAX_DEV_FRAMES} frames a call, got {n}")
    jshape = tuple(jshape)
    if len(jshape) == 3:
        jshape = (jshape[0], 1) + jshape[1:]
    if len(jshape) != 4 or jshape[0] != n or jshape[3] != 3:
        raise ValueError(f"joints_uvd must be [{n}, S, J, 3] or [{n}, J, 3], got {jshape}")
    S, J = jshape[1], jshape[2]
    if not 1 <= S <= OVERLAY_MAX_SETS:
        raise ValueError(f"1 to {OVERLAY_MAX_SETS} joint sets, got {S}")
    if J > OVERLAY_MAX_JOINTS:
        raise ValueError(f"at most {OVERLAY_MAX_JOINTS} joints a set, got {J}")
    if bones is None:
        b = np.zeros((0, 2), np.int32)
    else:
        b = np.asarray(bones)
        if b.size == 0:
            b = np.zeros((0, 2), np.int32)
        if b.dtype.kind not in "ui" or b.ndim != 2 or b.shape[1] != 2:
            raise ValueError(f"bones must be [nb, 2] integer index pairs, got {b.dtype} {b.shape}")
        if len(b) > OVERLAY_MAX_BONES:
            raise ValueError(f"at most {OVERLAY_MAX_BONES} bones, got {len(b)}")
        if len(b) and (b.min() < 0 or b.max() >= J):
            raise ValueError(f"a bone index is outside 0..{J - 1}")
        b = np.ascontiguousarray(b, dtype=np.int32)
    try:
        lo, hi = depth_range
        with np.errstate(all="ignore"):
            lo, hi = np.float32(lo), np.float32(hi)
    except (TypeError, ValueError):
        raise ValueError(f"depth_range must be (lo, hi), got {depth_range!r}") from None
    if not (np.isfinite(lo) and np.isfinite(hi)) or lo == hi:
        raise ValueError(f"depth_range must be two finite float32 values that differ, got {depth_range!r}")
    st = DEFAULT_OVERLAY_STYLES if styles is None else tuple(styles)
    if len(st) < S:
        raise ValueError(f"{S} joint sets need {S} styles, got {len(st)}")
    out = []
    for s in st[:S]:
        try:
            m, c, r, th = s
            m, c = tuple(int(v) for v in m), tuple(int(v) for v in c)
            r, th = int(r), int(th)
        except (TypeError, ValueError):
            raise ValueError(f"a style is (marker_rgb, bone_rgb, radius, thickness), got {s!r}") from None
        if len(m) != 3 or len(c) != 3 or not all(0 <= v <= 255 for v in m + c):
            raise ValueError(f"style colours are three values in 0..255, got {s!r}")
        if not 0 <= r <= OVERLAY_MAX_RADIUS or not 1 <= th <= OVERLAY_MAX_THICK:
            raise ValueError(f"radius is 0..{OVERLAY_MAX_RADIUS} and thickness 1..{OVERLAY_MAX_THICK}, got {s!r}")
        out.append((m, c, r, th))
    return S, J, b, lo, hi, out


def overlay_color_index(d, lo, hi):
    """The colour-table index of frame values ``d`` (float32 array): ``x = (d - lo) / (hi - lo)`` in
    float32, 0 if ``not x >= 0`` (also NaN), 255 if ``x >= 1``, else ``int(x * 255 + 0.5)``."""
    f32 = np.float32
    with np.errstate(all="ignore"):
        x = (np.asarray(d, f32) - f32(lo)) / (f32(hi) - f32(lo))
        mid = (x >= 0) & ~(x >= 1)
        k = np.zeros(x.shape, np.int64)
        k[x >= 1] = 255
        k[mid] = (x[mid] * f32(255.) + f32(0.5)).astype(np.int64)
    return k


def overlay_centers(uv):
    """(eligible, centres int64) of joint coordinates ``uv`` [..., 2] float32: ``floor(u + 0.5)`` in
    float32; eligible iff both centres are in [-4096, 8191] (NaN and +-inf are not)."""
    with np.errstate(all="ignore"):
        f = np.floor(np.asarray(uv, np.float32) + np.float32(0.5))
        ok = ((f >= OVERLAY_C_MIN) & (f <= OVERLAY_C_MAX)).all(axis=-1)
        c = np.where(ok[..., None], f, 0).astype(np.int64)
    return ok, c


def overlay_disc_mask(X, Y, cu, cv, r):
    return (X - cu) ** 2 + (Y - cv) ** 2 <= r * r


def overlay_bone_mask(X, Y, P, Q, th):
    """int64 coverage of the bone P -> Q, ``th`` thick, at pixel grids X, Y (the caps are the markers')"""
    dx, dy = int(Q[0]) - int(P[0]), int(Q[1]) - int(P[1])
    L2 = dx * dx + dy * dy
    ex, ey = X.astype(np.int64) - int(P[0]), Y.astype(np.int64) - int(P[1])
    s = ex * dx + ey * dy
    c = ex * dy - ey * dx
    return (L2 > 0) & (0 <= s) & (s <= L2) & (4 * c * c <= th * th * L2)


def render_overlays_np(frames, joints_uvd, bones=None, depth_range=None, lut="gray", styles=None):
    """``render_overlays`` in numpy on host arrays -- the statement of the drawing rule the kernel is
    tested against (float32 colour arithmetic, int64 coverage, vectorised per primitive over its
    bounding box).  Returns [n, h, w, 3] uint8."""
    fr = np.asarray(frames)
    if fr.ndim == 4 and fr.shape[-1] == 1:
        fr = fr[..., 0]
    if fr.ndim != 3:
        raise ValueError(f"frames must be [n, h, w] or [n, h, w, 1], got {fr.shape}")
    if fr.dtype not in (np.uint16, np.float32):
        raise TypeError(f"frames must be uint16 or float32, got {fr.dtype}")
    n, h, w = fr.shape
    ju = np.asarray(joints_uvd)
    if ju.dtype != np.float32:
        raise TypeError(f"joints_uvd must be float32, got {ju.dtype}")
    if depth_range is None:
        depth_range = (0, 10000) if fr.dtype == np.uint16 else (0.0, 1.0)
    S, J, b, lo, hi, st = _overlay_scene(n, h, w, ju.shape, bones, depth_range, styles)
    table = _overlay_lut_array(lut)
    ju = ju.reshape(n, S, J, 3)
    out = table[overlay_color_index(fr.astype(np.float32), lo, hi)]
    ok, cen = overlay_centers(ju[..., :2])

    def paint(img, x0, x1, y0, y1, mask_of, rgb):
        x0, x1, y0, y1 = max(x0, 0), min(x1, w - 1), max(y0, 0), min(y1, h - 1)
        if x0 > x1 or y0 > y1:
            return
        Y, X = np.mgrid[y0:y1 + 1, x0:x1 + 1]
        img[y0:y1 + 1, x0:x1 + 1][mask_of(X, Y)] = rgb

    for i in range(n):
        for s in range(S):
            m_rgb, b_rgb, r, th = st[s]
            for a, q in b:
                if ok[i, s, a] and ok[i, s, q]:
                    P, Q = cen[i, s, a], cen[i, s, q]
                    paint(out[i], min(P[0], Q[0]) - th, max(P[0], Q[0]) + th, min(P[1], Q[1]) - th,
                          max(P[1], Q[1]) + th, lambda X, Y: overlay_bone_mask(X, Y, P, Q, th), b_rgb)
            for j in range(J):
                if ok[i, s, j]:
                    cu, cv = cen[i, s, j]
                    paint(out[i], cu - r, cu + r, cv - r, cv + r,
                          lambda X, Y: overlay_disc_mask(X, Y, cu, cv, r), m_rgb)
    return out


_LUT_CACHE = {}


def render_overlays(frames, joints_uvd, bones=None, depth_range=None, lut="gray", styles=None, stream=None,
                    out=None):
    """Depth frames through a colour table with joint markers and bones drawn on them, on the device
    (``mp_overlay_dev``, one streaming kernel on the current stream or ``stream``): what the
    reference's ``plt.imshow(frame); plt.scatter(uvd)`` and ``save_result_image`` show.

    frames       CUDA [n, h, w] or [n, h, w, 1], ``torch.uint16`` or ``torch.float32``; h, w <= 4096
    joints_uvd   CUDA float32 [n, S, J, 3] or [n, J, 3] (one set); u, v are read.  1 <= S <= 4,
                 J <= 128.  A joint whose rounded centre is outside [-4096, 8191] (NaN too) is not
                 drawn and draws no bone: pad a short set with NaN
    bones        [nb, 2] index pairs into 0..J-1 (host), nb <= 256; ``None``: markers only
    depth_range  (lo, hi) of the colour table in the frames' units, as float32; default (0, 10000)
                 for uint16 frames and (0, 1) for float32 frames
    lut          ``'gray'``, ``'jet'`` (``overlay_lut``), a [256, 3] uint8 array or CUDA tensor
    styles       per set (marker_rgb, bone_rgb, radius 0..15, thickness 1..15);
                 ``DEFAULT_OVERLAY_STYLES``
    out          a contiguous CUDA uint8 tensor of n * h * w * 3 elements at any byte offset
    Returns CUDA uint8 [n, h, w, 3], the bytes of ``render_overlays_np``.  Set s + 1 is drawn over set
    s, joints over bones, the last primitive wins; no blending, text or anti-aliasing.  Everything is
    checked before any GPU call."""
    import torch
    if not isinstance(frames, torch.Tensor) or not isinstance(joints_uvd, torch.Tensor):
        raise TypeError("frames and joints_uvd must be CUDA (ROCm) tensors (numpy: render_overlays_np)")
    if frames.dim() == 4 and frames.shape[-1] == 1:
        frames = frames[..., 0]
    if frames.dim() != 3:
        raise ValueError(f"frames must be [n, h, w] or [n, h, w, 1], got {tuple(frames.shape)}")
    if frames.dtype not in (torch.uint16, torch.float32):
        raise TypeError(f"frames must be torch.uint16 or torch.float32, got {frames.dtype}")
    if joints_uvd.dtype != torch.float32:
        raise TypeError(f"joints_uvd must be torch.float32, got {joints_uvd.dtype}")
    u16 = frames.dtype == torch.uint16
    n, h, w = frames.shape
    if depth_range is None:
        depth_range = (0, 10000) if u16 else (0.0, 1.0)
    S, J, b, lo, hi, st = _overlay_scene(n, h, w, joints_uvd.shape, bones, depth_range, styles)
    if isinstance(lut, torch.Tensor):
        if lut.dtype != torch.uint8 or tuple(lut.shape) != (256, 3):
            raise ValueError(f"lut must be [256, 3] uint8, got {lut.dtype} {tuple(lut.shape)}")
        table = None
    else:
        table = _overlay_lut_array(lut)
    if out is not None and not (isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and out.is_contiguous()
                                and out.numel() == n * h * w * 3):
        raise ValueError(f"out must be a contiguous CUDA uint8 tensor of {n * h * w * 3} elements")
    if not (frames.is_cuda and joints_uvd.is_cuda and (out is None or out.is_cuda)
            and (table is not None or lut.is_cuda)):
        raise TypeError("frames, joints_uvd (and out, lut) must be CUDA (ROCm) tensors")
    dev = frames.device
    if table is not None:
        key = (table.tobytes(), dev)
        lut = _LUT_CACHE.get(key)
        if lut is None:
            lut = _LUT_CACHE[key] = torch.from_numpy(table).to(dev)
    style = OverlayStyle(struct_size=ctypes.sizeof(OverlayStyle))
    for s, (m, c, r, th) in enumerate(st):
        style.sets[s].marker_rgb[:] = m
        style.sets[s].bone_rgb[:] = c
        style.sets[s].radius, style.sets[s].thickness = r, th
    fr = frames.detach().contiguous()
    ju = joints_uvd.detach().contiguous()
    lt = lut.detach().contiguous()
    if out is None:
        out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
    stp = _lib.current_stream(dev) if stream is None else stream
    _lib.check(_lib_crop().mp_overlay_dev(ctypes.c_void_p(fr.data_ptr()), DEPTH_U16 if u16 else DEPTH_F32, n, h, w,
                                          float(lo), float(hi), ctypes.c_void_p(lt.data_ptr()),
                                          ctypes.c_void_p(ju.data_ptr() if J else None), S, J,
                                          _p(b) if len(b) else None, len(b), ctypes.byref(style),
                                          ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(stp)))
    return out.view(n, h, w, 3)


class MonkeyDetector(object):
    """``MonkeyDetector`` (monkeydetector.py:21-63)."""

    preprocess_real_frames = staticmethod(preprocess_real_frames)
    render_overlays = staticmethod(render_overlays)
    render_overlays_np = staticmethod(render_overlays_np)

    RESIZE_BILINEAR = 0
    RESIZE_CV2_NN = 1
    RESIZE_CV2_LINEAR = 2

    def __init__(self, fx, fy, ux, uy, cube, d1, d2, importer=None):
        if len(cube) != 3:
            raise ValueError("Volume must be 3D")
        self.maxDepth = d2
        self.minDepth = d1
        self.fx, self.fy, self.ux, self.uy = fx, fy, ux, uy
        self.cube = cube
        self.resizeMethod = self.RESIZE_CV2_NN

    def _cam(self) -> _Camera:
        return _Camera(float(self.fx), float(self.fy), float(self.ux), float(self.uy),
                       (ctypes.c_double * 3)(*[float(c) for c in self.cube]), float(self.minDepth),
                       float(self.maxDepth))

    @staticmethod
    def _frame(dpt, ndim=2):
        """(contiguous array, MP_DEPTH_* code): uint16 frames keep their numpy semantics (exact CoM
        sum, truncating near-plane clamp); anything else is computed as float32 like the
        reference's float32 frames."""
        a = np.asarray(dpt)
        if a.ndim != ndim:
            raise NotImplementedError(f"expected {ndim}-D single-channel depth, got shape {a.shape}")
        if a.dtype == np.uint16:
            return np.ascontiguousarray(a), 1
        return np.ascontiguousarray(a, dtype=np.float32), 0

    # ------------------------------------------------------------------ native
    def calculateCoM(self, dpt):
        """monkeydetector.py:66-83 (float32 frame in mm; a uint16 frame is converted exactly)."""
        f, dt = self._frame(dpt)
        com = np.zeros(3, np.float64)
        cam = self._cam()
        _lib.check(_lib_crop().mp_center_of_mass(ctypes.byref(cam), _p(f), dt, f.shape[0], f.shape[1], _p(com)))
        return com

    def cropArea3D(self, dpt, com=None, dsize=(128, 128), docom=False):
        """monkeydetector.py:261-334 -> (crop [dsize] float32 mm, M 3x3 numpy matrix, com);
        ``docom=True`` runs the second refinement (287-300): a CoM of the first crop, a second crop
        around it, and the refined CoM returned."""
        if self.resizeMethod != self.RESIZE_CV2_NN:
            raise NotImplementedError("only RESIZE_CV2_NN (the reference default) is implemented")
        if len(dsize) != 2 or dsize[0] != dsize[1]:
            raise ValueError("dsize must be a square 2D bounding box")
        f, dt = self._frame(dpt)
        out = np.empty((dsize[0], dsize[1]), np.float32)
        M = np.zeros(9, np.float64)
        com_out = np.zeros(3, np.float64)
        info = np.zeros(8, np.int32)
        c = None if com is None else np.ascontiguousarray(np.asarray(com, np.float64).reshape(3))
        cam = self._cam()
        _lib.check(_lib_crop().mp_crop3d_ex(ctypes.byref(cam), _p(f), dt, f.shape[0], f.shape[1],
                                            None if c is None else _p(c), 1 if docom else 0, dsize[0], _p(out),
                                            _p(M), _p(com_out), _p(info)))
        self.last_crop_info = dict(bounds=tuple(int(v) for v in info[:4]), sz=(int(info[4]), int(info[5])),
                                   offset=(int(info[6]), int(info[7])))
        return out, np.asmatrix(M.reshape(3, 3)), com_out

    def crop_batch(self, frames, coms=None, dsize=128, nthreads=None, out=None):
        """Per-frame crop of ``prepare_data_test`` (train_cnn_networks_hgru.py:61-74) in one native
        call: returns (patches [n, dsize, dsize, 1] = crop / maxDepth, Ms [n, 3, 3], coms [n, 3]).
        ``out``: a C-contiguous float32 [n, dsize, dsize, 1] array the patches are written into (and
        returned as ``patches``), e.g. a reused or pinned staging buffer."""
        fr, dt = self._frame(frames, ndim=3)
        n = fr.shape[0]
        if out is None:
            patches = np.empty((n, dsize, dsize, 1), np.float32)
        else:
            if not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags.c_contiguous
                    and out.shape == (n, dsize, dsize, 1)):
                raise ValueError(f"out must be a C-contiguous float32 array of shape {(n, dsize, dsize, 1)}")
            patches = out
        Ms = np.empty((n, 9), np.float64)
        com_out = np.empty((n, 3), np.float64)
        c = None if coms is None else np.ascontiguousarray(np.asarray(coms, np.float64).reshape(n, 3))
        nt = nthreads or min(16, len(os.sched_getaffinity(0)))
        cam = self._cam()
        _lib.check(_lib_crop().mp_crop3d_batch(ctypes.byref(cam), _p(fr), dt, n, fr.shape[1], fr.shape[2],
                                               None if c is None else _p(c), dsize, _p(patches), _p(Ms),
                                               _p(com_out), int(nt)))
        return patches, Ms.reshape(n, 3, 3), com_out

    def crop_batch_device(self, frames, com_norm, com_scale=(424, 512, 10000.), frame_scale=10000.,
                          dsize=128, check=True, stream=None, docom=False):
        """``prepare_data_test`` (train_cnn_networks_hgru.py:61-74) on the GPU for a batch, with
        ``tr_res`` = the attention output still on the device (``mp_crop3d_dev``, one launch):

        frames     CUDA [n, h, w] or [n, h, w, 1] fp32 as fed to the attention net (image / max depth)
        com_norm   CUDA [n, 3] fp32 attention output; com = com_norm * com_scale (float64)
        returns    (patches CUDA [n, dsize, dsize, 1] = crop / maxDepth, Ms CUDA [n, 3, 3] f64,
                    coms CUDA [n, 3] f64); with ``check`` the per-frame status is read back (one
                    sync) and a failed frame raises like the host ``cropArea3D``.  ``docom``: the
                    second CoM refinement of ``cropArea3D(docom=True)`` per frame, on the device."""
        import torch
        if not (isinstance(frames, torch.Tensor) and frames.is_cuda and isinstance(com_norm, torch.Tensor)
                and com_norm.is_cuda):
            raise TypeError("frames and com_norm must be CUDA (ROCm) tensors")
        if frames.dim() == 4:
            if frames.shape[-1] != 1:
                raise ValueError("frames must be single-channel")
            frames = frames[..., 0]
        if frames.dim() != 3:
            raise ValueError(f"frames must be [n, h, w], got {tuple(frames.shape)}")
        fr = frames.detach().float().contiguous()
        n, h, w = fr.shape
        cn = com_norm.detach().float().contiguous().view(n, 3)
        dev = fr.device
        patches = torch.empty((n, dsize, dsize, 1), dtype=torch.float32, device=dev)
        Ms = torch.empty((n, 3, 3), dtype=torch.float64, device=dev)
        coms = torch.empty((n, 3), dtype=torch.float64, device=dev)
        status = torch.empty((n,), dtype=torch.int32, device=dev)
        scale = (ctypes.c_double * 3)(*[float(v) for v in com_scale])   # host array (read at the call)
        st = _lib.current_stream(dev) if stream is None else stream
        cam = self._cam()
        _lib.check(_lib_crop().mp_crop3d_dev_ex(ctypes.byref(cam), ctypes.c_void_p(fr.data_ptr()), n, h, w,
                                                float(frame_scale), ctypes.c_void_p(cn.data_ptr()),
                                                ctypes.cast(scale, ctypes.c_void_p), 1 if docom else 0, int(dsize),
                                             ctypes.c_void_p(patches.data_ptr()), ctypes.c_void_p(Ms.data_ptr()),
                                             ctypes.c_void_p(coms.data_ptr()), ctypes.c_void_p(status.data_ptr()),
                                             ctypes.c_void_p(st)))
        self.last_status = status
        if check:
            bad = torch.nonzero(status).flatten().tolist()
            if bad:
                code = int(status[bad[0]].item())
                raise _lib.MonkeyPoseError(-1, f"frame {bad[0]}: cropArea3D: {_CROP_MSG.get(code, code)}")
        return patches, Ms, coms

    # ------------------------------------------------------------------ detector path on the device
    @staticmethod
    def _dev_frames(frames, coms=None, frame_scale=1.0):
        """``frames`` ([n, h, w] or [n, h, w, 1]) as (a contiguous CUDA [n, h, w] tensor, its
        MP_DEPTH_* code): a ``torch.uint16`` tensor (the camera's own millimetres) stays uint16 and
        keeps its numpy semantics as on the host (``_frame``), every other dtype is computed as
        fp32.  The shapes (also of ``coms`` [n, 3], when given) are checked first, then that uint16
        frames come with ``frame_scale`` 1 (they have no normalised form), then the device, all
        before any GPU call."""
        import torch
        if not isinstance(frames, torch.Tensor):
            raise TypeError("frames must be a CUDA (ROCm) tensor")
        if frames.dim() == 4:
            if frames.shape[-1] != 1:
                raise ValueError("frames must be single-channel")
            frames = frames[..., 0]
        if frames.dim() != 3 or 0 in frames.shape:
            raise ValueError(f"frames must be [n, h, w], got {tuple(frames.shape)}")
        if isinstance(coms, torch.Tensor) and tuple(coms.shape) != (frames.shape[0], 3):
            raise ValueError(f"coms must be [{frames.shape[0]}, 3], got {tuple(coms.shape)}")
        u16 = frames.dtype == torch.uint16
        if u16 and float(frame_scale) != 1.0:
            raise ValueError(f"uint16 frames are millimetres: frame_scale must be 1, got {frame_scale}")
        if not frames.is_cuda:
            raise TypeError("frames must be a CUDA (ROCm) tensor")
        if u16:
            return frames.detach().contiguous(), DEPTH_U16
        return frames.detach().float().contiguous(), DEPTH_F32

    @staticmethod
    def _dev_coms(coms, n):
        import torch
        if not isinstance(coms, torch.Tensor):
            raise TypeError("coms must be a CUDA (ROCm) tensor")
        if tuple(coms.shape) != (n, 3):
            raise ValueError(f"coms must be [{n}, 3], got {tuple(coms.shape)}")
        if not coms.is_cuda:
            raise TypeError("coms must be a CUDA (ROCm) tensor")
        return coms.detach().double().contiguous()

    def _detect_buffers(self, n, h, w, dsize, dev, dt=DEPTH_F32):
        """output and scratch tensors of one detector batch of frames of dtype code ``dt``
        (``DetectorPosePipeline`` keeps them)"""
        import torch
        nbytes = int(_lib_crop().mp_center_of_mass_dev_work_dt(dt, n, h, w))
        return dict(
            work=torch.empty((max(nbytes, 8),), dtype=torch.uint8, device=dev), work_bytes=nbytes,
            coms0=torch.empty((n, 3), dtype=torch.float64, device=dev),
            patches=torch.empty((n, dsize, dsize, 1), dtype=torch.float32, device=dev),
            Ms=torch.empty((n, 3, 3), dtype=torch.float64, device=dev),
            coms=torch.empty((n, 3), dtype=torch.float64, device=dev),
            status=torch.empty((n,), dtype=torch.int32, device=dev))

    def _com_into(self, fr, frame_scale, coms, work, work_bytes, st, dt=DEPTH_F32):
        n, h, w = fr.shape
        cam = self._cam()
        _lib.check(_lib_crop().mp_center_of_mass_dev_dt(ctypes.byref(cam), ctypes.c_void_p(fr.data_ptr()), dt, n, h,
                                                        w, float(frame_scale), ctypes.c_void_p(coms.data_ptr()),
                                                        ctypes.c_void_p(work.data_ptr()), work_bytes,
                                                        ctypes.c_void_p(st)))

    def _crop_coms_into(self, fr, frame_scale, coms_in, dsize, docom, b, st, dt=DEPTH_F32):
        n, h, w = fr.shape
        cam = self._cam()
        _lib.check(_lib_crop().mp_crop3d_dev_coms_dt(ctypes.byref(cam), ctypes.c_void_p(fr.data_ptr()), dt, n, h, w,
                                                     float(frame_scale), ctypes.c_void_p(coms_in.data_ptr()),
                                                     1 if docom else 0, int(dsize),
                                                     ctypes.c_void_p(b["patches"].data_ptr()),
                                                     ctypes.c_void_p(b["Ms"].data_ptr()),
                                                     ctypes.c_void_p(b["coms"].data_ptr()),
                                                     ctypes.c_void_p(b["status"].data_ptr()), ctypes.c_void_p(st)))

    def _check_status(self, status):
        import torch
        self.last_status = status
        bad = torch.nonzero(status).flatten().tolist()   # the one sync of a checked call
        if bad:
            code = int(status[bad[0]].item())
            raise _lib.MonkeyPoseError(-1, f"frame {bad[0]}: cropArea3D: {_CROP_MSG.get(code, code)}")

    def calculateCoM_device(self, frames, frame_scale=1.0, stream=None):
        """``calculateCoM`` (monkeydetector.py:66-83) of every frame of a CUDA batch [n, h, w] (or
        [n, h, w, 1]) in one asynchronous call (``mp_center_of_mass_dev_dt``): a CUDA [n, 3] float64
        tensor, each row the bits of ``calculateCoM(frame * frame_scale)`` (``frame_scale`` 1 for
        frames in mm, 10000 for normalised frames).  ``torch.uint16`` frames (mm, ``frame_scale`` 1)
        give the bits of ``calculateCoM`` of the uint16 frame; any other dtype is computed as fp32."""
        fr, dt = self._dev_frames(frames, frame_scale=frame_scale)
        import torch
        n, h, w = fr.shape
        nbytes = int(_lib_crop().mp_center_of_mass_dev_work_dt(dt, n, h, w))
        work = torch.empty((max(nbytes, 8),), dtype=torch.uint8, device=fr.device)
        coms = torch.empty((n, 3), dtype=torch.float64, device=fr.device)
        st = _lib.current_stream(fr.device) if stream is None else stream
        self._com_into(fr, frame_scale, coms, work, nbytes, st, dt)
        return coms

    def detect_crop_device(self, frames, coms=None, frame_scale=1.0, dsize=128, docom=False, check=True,
                           stream=None, _buffers=None):
        """``crop_batch`` on the GPU: ``cropArea3D(frame * frame_scale, com)`` / maxDepth per frame
        with ``coms`` a CUDA [n, 3] float64 tensor taken as it is (``mp_crop3d_dev_coms_dt``), or
        ``None`` for the detector's own ``calculateCoM`` on the device first.  Returns (patches CUDA
        [n, dsize, dsize, 1], Ms CUDA [n, 3, 3] f64, coms CUDA [n, 3] f64) with the outputs, status
        codes and ``check`` semantics of ``crop_batch_device``.  ``torch.uint16`` frames (mm,
        ``frame_scale`` 1) give the bits of ``crop_batch`` / ``cropArea3D`` of the uint16 frames."""
        fr, dt = self._dev_frames(frames, coms, frame_scale)
        n, h, w = fr.shape
        cin = None if coms is None else self._dev_coms(coms, n)
        b = _buffers if _buffers is not None else self._detect_buffers(n, h, w, int(dsize), fr.device, dt)
        st = _lib.current_stream(fr.device) if stream is None else stream
        if cin is None:
            cin = b["coms0"]
            self._com_into(fr, frame_scale, cin, b["work"], b["work_bytes"], st, dt)
        self._crop_coms_into(fr, frame_scale, cin, dsize, docom, b, st, dt)
        self.last_status = b["status"]
        if check:
            self._check_status(b["status"])
        return b["patches"], b["Ms"], b["coms"]

    def getAbsoluteCoordinates_device(self, pose, coms, num_joints=23, stream=None, out=None):
        """``getAbsoluteCoordinates`` (monkeydetector.py:356-360) for a batch on the GPU
        (``mp_abs_joints_dev``): ``pose`` CUDA [n, num_joints * 3] fp32 normalised by cube_z / 2 (a
        regressor's output), ``coms`` CUDA [n, 3] f64 -> (xyz mm, uvd), CUDA fp32 [n, num_joints, 3]."""
        import torch
        J = int(num_joints)
        if not isinstance(pose, torch.Tensor):
            raise TypeError("pose must be a CUDA (ROCm) tensor")
        if pose.dim() != 2 or pose.shape[0] == 0 or pose.shape[1] != 3 * J:
            raise ValueError(f"pose must be [n, {3 * J}], got {tuple(pose.shape)}")
        n = pose.shape[0]
        if isinstance(coms, torch.Tensor) and tuple(coms.shape) != (n, 3):
            raise ValueError(f"coms must be [{n}, 3], got {tuple(coms.shape)}")
        if not pose.is_cuda:
            raise TypeError("pose must be a CUDA (ROCm) tensor")
        c = self._dev_coms(coms, n)
        p = pose.detach().float().contiguous()
        if out is None:
            out = (torch.empty((n, J, 3), dtype=torch.float32, device=p.device),
                   torch.empty((n, J, 3), dtype=torch.float32, device=p.device))
        xyz, uvd = out
        st = _lib.current_stream(p.device) if stream is None else stream
        cam = self._cam()
        _lib.check(_lib_crop().mp_abs_joints_dev(ctypes.byref(cam), ctypes.c_void_p(p.data_ptr()), n, J,
                                                 ctypes.c_void_p(c.data_ptr()), ctypes.c_void_p(xyz.data_ptr()),
                                                 ctypes.c_void_p(uvd.data_ptr()), ctypes.c_void_p(st)))
        return xyz, uvd

    def transform_joints_device(self, joints_uvd, Ms, stream=None, out=None):
        """The uvd half of ``getRelativeCoordinates`` (monkeydetector.py:341-354) for a batch on the
        GPU (``mp_transform_joints_dev``): joints in the crop's pixel space, which is what
        ``save_result_image`` draws on the 128 x 128 patch.  ``joints_uvd`` CUDA [n, J, 3] fp32,
        ``Ms`` CUDA [n, 3, 3] f64 (the crops' transforms) -> CUDA [n, J, 3] fp32.  Per joint, in
        float64 and not fused: ``t_i = (u * M_i0 + v * M_i1) + M_i2``, ``u' = f32(t_0 / t_2)``,
        ``v' = f32(t_1 / t_2)``, ``d' = d``.  The host function forms ``t`` by a BLAS product, which
        may fuse or reorder, so the two can differ in the last float32 bit."""
        import torch
        if not isinstance(joints_uvd, torch.Tensor) or not isinstance(Ms, torch.Tensor):
            raise TypeError("joints_uvd and Ms must be CUDA (ROCm) tensors")
        if joints_uvd.dim() != 3 or joints_uvd.shape[2] != 3 or 0 in joints_uvd.shape:
            raise ValueError(f"joints_uvd must be [n, joints, 3], got {tuple(joints_uvd.shape)}")
        n, J = joints_uvd.shape[0], joints_uvd.shape[1]
        if tuple(Ms.shape) != (n, 3, 3):
            raise ValueError(f"Ms must be [{n}, 3, 3], got {tuple(Ms.shape)}")
        if not (joints_uvd.is_cuda and Ms.is_cuda):
            raise TypeError("joints_uvd and Ms must be CUDA (ROCm) tensors")
        ju = joints_uvd.detach().float().contiguous()
        m = Ms.detach().double().contiguous()
        if out is None:
            out = torch.empty((n, J, 3), dtype=torch.float32, device=ju.device)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32
                  and out.is_contiguous() and out.numel() == n * J * 3):
            raise ValueError(f"out must be a contiguous CUDA float32 tensor of {n * J * 3} elements")
        st = _lib.current_stream(ju.device) if stream is None else stream
        _lib.check(_lib_crop().mp_transform_joints_dev(ctypes.c_void_p(ju.data_ptr()), ctypes.c_void_p(m.data_ptr()),
                                                       n, J, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(st)))
        return out.view(n, J, 3)

    # ------------------------------------------------------------------ labels (validation pass)
    @staticmethod
    def _dev_labels(labels, name="labels", num_joints=None, shape_only=False):
        """``labels`` [n, J, 3] (or [n, 3J] with ``num_joints``) as a contiguous fp32 CUDA [n, J, 3]
        tensor; the shape is checked first, then the device, both before any GPU call
        (``shape_only``: the reshaped tensor after the shape checks alone)."""
        import torch
        if not isinstance(labels, torch.Tensor):
            raise TypeError(f"{name} must be a CUDA (ROCm) tensor")
        if labels.dim() == 2 and num_joints is not None and labels.shape[1] == 3 * int(num_joints):
            labels = labels.reshape(labels.shape[0], int(num_joints), 3)
        if labels.dim() != 3 or labels.shape[2] != 3 or 0 in labels.shape:
            raise ValueError(f"{name} must be [n, joints, 3], got {tuple(labels.shape)}")
        if labels.shape[1] > MAX_EVAL_JOINTS:
            raise ValueError(f"{name}: at most {MAX_EVAL_JOINTS} joints, got {labels.shape[1]}")
        if labels.shape[0] > MAX_DEV_FRAMES:
            raise ValueError(f"{name}: at most {MAX_DEV_FRAMES} frames a call, got {labels.shape[0]}")
        if shape_only:
            return labels
        if not labels.is_cuda:
            raise TypeError(f"{name} must be a CUDA (ROCm) tensor")
        return labels.detach().float().contiguous()

    def calculateCoMfrom3DJoints(self, jnts, scale=None, stream=None, out=None):
        """``tfMonkeyDetector.calculateCoMfrom3DJoints`` (tf_monkeydetector.py:66-71) of labels
        [n, J, 3] in mm, then the driver's normalisation ``/ scale`` (train_cnn_networks_hgru.py:166,
        ``scale = (orig0, orig1, max_depth)``; ``None``: the plain uvd) -> [n, 3] float32.

        All float32: the mean over the joints is ``labels.mean(axis=1)`` (a sequential sum in joint
        order, divided by f32(J)); then TF's ``xyztouvd``, ``u = f32(ux) - (x / z) * f32(fx)``,
        ``v = f32(uy) + (y / z) * f32(fy)``, ``d = -z`` with no ``z == 0`` guard (inf / NaN propagate
        as in TF); then ``/ f32(scale[k])``.  numpy in -> these operations on the host (the CPU oracle
        of the kernel); a CUDA tensor in -> ``mp_com_from_joints_dev``, the same bits.  TF's own
        ``reduce_mean`` order over the joints is PARITY UNPINNED (no TensorFlow here); every other
        operation is elementwise."""
        sc = (1.0, 1.0, 1.0) if scale is None else tuple(float(v) for v in scale)
        if len(sc) != 3:
            raise ValueError("scale must have three entries (u, v, d)")
        if isinstance(jnts, np.ndarray) or not hasattr(jnts, "is_cuda"):
            j = np.asarray(jnts, np.float32)
            if j.ndim != 3 or j.shape[2] != 3 or 0 in j.shape:
                raise ValueError(f"jnts must be [n, joints, 3], got {j.shape}")
            f32 = np.float32
            with np.errstate(divide="ignore", invalid="ignore"):
                m = j.mean(axis=1, dtype=np.float32)
                u = f32(self.ux) - (m[:, 0] / m[:, 2]) * f32(self.fx)
                v = f32(self.uy) + (m[:, 1] / m[:, 2]) * f32(self.fy)
                d = -m[:, 2]
                return np.stack([u / f32(sc[0]), v / f32(sc[1]), d / f32(sc[2])], axis=1).astype(np.float32)
        import torch
        lab = self._dev_labels(jnts, "jnts")
        n, J = lab.shape[0], lab.shape[1]
        if out is None:
            out = torch.empty((n, 3), dtype=torch.float32, device=lab.device)
        st = _lib.current_stream(lab.device) if stream is None else stream
        cam = self._cam()
        _lib.check(_lib_crop().mp_com_from_joints_dev(ctypes.byref(cam), ctypes.c_void_p(lab.data_ptr()), n, J,
                                                      sc[0], sc[1], sc[2], ctypes.c_void_p(out.data_ptr()),
                                                      ctypes.c_void_p(st)))
        return out

    calculateCoMfrom3DJoints_device = calculateCoMfrom3DJoints

    def relative_labels(self, labels_xyz, coms):
        """The label half of ``prepare_data`` (train_cnn_networks_hgru.py:52-56) on the host: labels
        [n, J, 3] float32 in mm, coms [n, 3] (u, v, d) -> [n, 3J] float32 =
        ``clip((label - uvdtoxyz(com)) / f32(cube_z / 2), -1, 1)`` (``getRelativeCoordinates``'s
        rel_xyz; rel_uvd is plot-only in the reference and not produced)."""
        lab = np.asarray(labels_xyz, np.float32)
        n = lab.shape[0]
        lab = lab.reshape(n, -1, 3)
        c = self.uvdtoxyz(np.asarray(coms, np.float64).reshape(n, 3))          # float64 ops, one rounding
        rel = (lab - c[:, None, :]) / np.float32(self.cube[2] / 2.)
        return np.clip(rel, np.float32(-1), np.float32(1)).reshape(n, -1)

    def relative_labels_device(self, labels_xyz, coms, stream=None, out=None, num_joints=None):
        """``relative_labels`` on the GPU (``mp_rel_labels_dev``): ``labels_xyz`` CUDA [n, J, 3] fp32 in
        mm (or [n, 3J] with ``num_joints``), ``coms`` CUDA [n, 3] f64 (the crop's coms) -> CUDA
        [n, 3J] fp32, the bits of the host function; asynchronous, a NaN label stays NaN."""
        import torch
        lab = self._dev_labels(labels_xyz, "labels_xyz", num_joints, shape_only=True)
        n, J = lab.shape[0], lab.shape[1]
        if isinstance(coms, torch.Tensor) and tuple(coms.shape) != (n, 3):
            raise ValueError(f"coms must be [{n}, 3], got {tuple(coms.shape)}")
        lab = self._dev_labels(lab, "labels_xyz")
        c = self._dev_coms(coms, n)
        if out is None:
            out = torch.empty((n, 3 * J), dtype=torch.float32, device=lab.device)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32
                  and out.is_contiguous() and out.numel() == n * 3 * J):
            raise ValueError(f"out must be a contiguous CUDA float32 tensor of {n * 3 * J} elements")
        st = _lib.current_stream(lab.device) if stream is None else stream
        cam = self._cam()
        _lib.check(_lib_crop().mp_rel_labels_dev(ctypes.byref(cam), ctypes.c_void_p(lab.data_ptr()), n, J,
                                                 ctypes.c_void_p(c.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                                 ctypes.c_void_p(st)))
        return out

    # ------------------------------------------------------------------ geometry (host numpy)
    def comToBounds(self, com, size):
        """monkeydetector.py:162-175."""
        zstart = com[2] - size[2] / 2.
        zend = com[2] + size[2] / 2.
        xstart = int(np.floor((com[0] * com[2] / self.fx - size[0] / 2.) / com[2] * self.fx))
        xend = int(np.floor((com[0] * com[2] / self.fx + size[0] / 2.) / com[2] * self.fx))
        ystart = int(np.floor((com[1] * com[2] / self.fy - size[1] / 2.) / com[2] * self.fy))
        yend = int(np.floor((com[1] * com[2] / self.fy + size[1] / 2.) / com[2] * self.fy))
        return xstart, xend, ystart, yend, zstart, zend

    def xyztouvd(self, jnts_xyz):
        """monkeydetector.py:85-112 / tf_monkeydetector.py:116-141 (float32 output; z == 0 maps to the
        principal point).  The reference's scalar arithmetic under NumPy 1.x: ``x / z`` in the joints'
        own dtype (float32 / float32 is a float32 division), then ``* fx`` and ``ux -`` in float64
        (a float32 scalar with a Python float promotes), one rounding to float32 on the store."""
        j = np.asarray(jnts_xyz)
        one = j.ndim == 1
        j = np.atleast_2d(j)
        if j.dtype.kind != "f":
            j = j.astype(np.float64)
        out = np.zeros((j.shape[0], 3), np.float32)
        z = j[:, 2]
        nz = z != 0.
        out[~nz, 0], out[~nz, 1] = self.ux, self.uy
        qx = (j[nz, 0] / z[nz]).astype(np.float64)
        qy = (j[nz, 1] / z[nz]).astype(np.float64)
        out[nz, 0] = self.ux - qx * self.fx
        out[nz, 1] = qy * self.fy + self.uy
        out[nz, 2] = -z[nz]
        return out[0] if one else out

    def xyztouvd_np(self, jnts_xyz):
        return self.xyztouvd(jnts_xyz)

    def uvdtoxyz(self, jnts_uvd):
        """monkeydetector.py:114-131."""
        u = np.asarray(jnts_uvd)
        one = u.ndim == 1
        u = np.atleast_2d(u).astype(np.float64)
        out = np.empty((u.shape[0], 3), np.float32)
        out[:, 0] = (self.ux - u[:, 0]) * u[:, 2] / (-self.fx)
        out[:, 1] = (u[:, 1] - self.uy) * u[:, 2] / (-self.fy)
        out[:, 2] = -u[:, 2]
        return out[0] if one else out

    def calcCoMRenders(self, jnts):
        assert jnts.ndim == 2, 'input must be the 3D coordinates of all monkey joints'
        return np.sum(jnts, axis=0) / jnts.shape[0]

    @staticmethod
    def transformPoint2D(pt, M):
        p = np.asarray(M, np.float64).reshape(3, 3) @ np.array([pt[0], pt[1], 1.0])
        return np.array([p[0] / p[2], p[1] / p[2]])

    def getRelativeCoordinates(self, jnts_xyz, jnts_uvd, com_uvd, M):
        """monkeydetector.py:341-354."""
        rel_xyz = jnts_xyz - self.uvdtoxyz(com_uvd)
        Mm = np.asarray(M, np.float64).reshape(3, 3)
        uv1 = np.c_[np.asarray(jnts_uvd, np.float64)[:, :2], np.ones(len(jnts_uvd))]
        t = uv1 @ Mm.T
        rel_uvd = np.zeros((len(jnts_uvd), 3), np.float32)
        rel_uvd[:, 0] = t[:, 0] / t[:, 2]
        rel_uvd[:, 1] = t[:, 1] / t[:, 2]
        rel_uvd[:, 2] = np.asarray(jnts_uvd)[:, 2]
        return rel_xyz, rel_uvd

    def getAbsoluteCoordinates(self, rel_jnts_xyz, com_uvd):
        """monkeydetector.py:356-360 / tf_monkeydetector.py:387-391 (A19 post-step)."""
        r = rel_jnts_xyz
        c = np.asarray(com_uvd)
        if (isinstance(r, np.ndarray) and r.dtype == np.float32 and r.ndim == 2 and r.shape[1] == 3
                and c.shape == (3,) and c.dtype.kind == "f"):
            # one joint set per frame (the config-5 loop): uvdtoxyz of the CoM as Python float64
            # scalars (the same IEEE double operations numpy runs elementwise), one float32 rounding
            # each, then xyztouvd's operations on whole columns when no joint has z == 0
            u0, u1, u2 = float(c[0]), float(c[1]), float(c[2])
            cxyz = np.array([(self.ux - u0) * u2 / (-self.fx), (u1 - self.uy) * u2 / (-self.fy), -u2], np.float32)
            jnts_xyz = r + cxyz
            z = jnts_xyz[:, 2]
            if z.all():
                q = (jnts_xyz[:, :2] / z[:, None]).astype(np.float64)
                uvd = np.empty((r.shape[0], 3), np.float32)
                uvd[:, 0] = self.ux - q[:, 0] * self.fx
                uvd[:, 1] = q[:, 1] * self.fy + self.uy
                uvd[:, 2] = -z
                return jnts_xyz, uvd
            return jnts_xyz, self.xyztouvd(jnts_xyz)
        jnts_xyz = rel_jnts_xyz + self.uvdtoxyz(com_uvd)
        return jnts_xyz, self.xyztouvd(jnts_xyz)


# tf_monkeydetector.tfMonkeyDetector shares this inference API (tf_monkeydetector.py:21-391)
tfMonkeyDetector = MonkeyDetector
