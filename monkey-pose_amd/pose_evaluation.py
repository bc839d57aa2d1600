"""Pose metrics of ``/root/reference/pose_evaluation.py`` ([frames, joints, 3] in mm), on numpy arrays
(host) and on CUDA tensors (the HIP kernels of ``csrc/k_eval.hip``).

The reference's evaluation runs on the host after the forward (train_hier_networks.py:323,
train_dense_networks.py:208, train_dense_hier_networks.py:324 call ``getMeanError_np``); the numpy
paths are the same NaN-aware reductions, checked against the reference's own functions executed on
the same inputs (tests/golden/make_crop_fixtures.py, tests/test_crop_reference.py).

CUDA tensors in: the joint distances ``sqrt(((dx * dx) + (dy * dy)) + dz * dz)`` and the per-frame
``nanmean`` / ``nanmax`` over the joints run on the device in numpy's float32 operation order (bit
for bit), the sums over frames in float64; the functions return Python floats / float64 values.
``PoseEvaluator`` is the streaming form: a state in device memory updated per batch without a host
sync, read by ``summary()`` alone.

NaN rule: every device function is NaN-aware like the ``_np`` ones (a NaN joint is left out of its
frame's mean and maximum, an all-NaN frame out of the mean over frames).  The reference's
``getMeanError_train`` / ``getMeanError`` / ``getMeanErrors_N`` / ``getMaxError`` are TensorFlow
reductions, which would propagate a NaN; the two differ only on inputs that hold a NaN.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib


def _is_cuda(x):
    return hasattr(x, "is_cuda") and not isinstance(x, np.ndarray)


def _joint_dist(labels, results, axis=2):
    d = np.asarray(labels) - np.asarray(results)
    return np.sqrt(np.square(d).sum(axis=axis))


class PoseEvaluator:
    """A streaming evaluator in device memory (``mp_eval_*``): ``update(labels, results, scale)`` per
    batch (asynchronous: two launches, no host sync), ``summary()`` once.

    ``num_joints`` <= 128; ``thresholds``: up to 1024 distances in mm for the "fraction of frames
    within distance" curves of ``pose_evaluation.main`` (136-186, ``range(0, 100)`` there).
    ``update``: ``labels`` / ``results`` CUDA [n, J, 3] (or [n, 3J]) fp32, both multiplied by the
    float32 ``scale`` first -- 1 for mm, ``cube_z / 2`` for values normalised like a regressor's
    output (``x * cube_z / 2.`` in the reference gives the same bits).
    ``summary()`` -> dict: ``frames``, ``valid_frames`` (frames whose mean is not NaN),
    ``mean_error`` (getMeanError_np; with J = 1, calc_com_error), ``max_error`` (getMaxError_np),
    ``joint_mean`` [J] (getJointMeanError), ``thresholds`` [T], ``within_max`` / ``within_mean`` [T]
    in percent of all frames.  It is the one place that syncs.
    ``last_frame_errors``: (dist [n, J], frame_mean [n], frame_max [n]) CUDA fp32 of the last batch."""

    def __init__(self, num_joints, thresholds=range(100), device=None):
        from .monkeydetector import MAX_EVAL_JOINTS, MAX_EVAL_THRESHOLDS
        self.J = int(num_joints)
        self.thresholds = np.ascontiguousarray(np.asarray(list(thresholds), np.float32).reshape(-1))
        self.T = int(self.thresholds.size)
        if not 1 <= self.J <= MAX_EVAL_JOINTS:
            raise ValueError(f"num_joints must be 1..{MAX_EVAL_JOINTS}, got {self.J}")
        if self.T > MAX_EVAL_THRESHOLDS:
            raise ValueError(f"at most {MAX_EVAL_THRESHOLDS} thresholds, got {self.T}")
        self.device = device
        self._state = None
        self._work = None
        self.last_frame_errors = None

    def _lib(self):
        from .monkeydetector import _lib_crop
        return _lib_crop()

    def _ensure(self, dev):
        import torch
        if self._state is None:
            lib = self._lib()
            nbytes = int(lib.mp_eval_state_bytes(self.J, self.T))
            self.device = dev
            self._state = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
            self._summary = torch.empty((int(lib.mp_eval_summary_len(self.J, self.T)),), dtype=torch.float64,
                                        device=dev)
            self._reset_on(_lib.current_stream(dev))

    def _reset_on(self, st):
        _lib.check(self._lib().mp_eval_reset_dev(ctypes.c_void_p(self._state.data_ptr()), self.J, self.T,
                                                 self.thresholds.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(st)))

    def reset(self, stream=None):
        if self._state is not None:
            self._reset_on(_lib.current_stream(self.device) if stream is None else stream)
        self.last_frame_errors = None

    def update(self, labels, results, scale=1.0, stream=None):
        import torch
        from .monkeydetector import MonkeyDetector
        if not (isinstance(labels, torch.Tensor) and isinstance(results, torch.Tensor)):
            raise TypeError("labels and results must be CUDA (ROCm) tensors")
        lab = MonkeyDetector._dev_labels(labels, "labels", self.J, shape_only=True)
        res = MonkeyDetector._dev_labels(results, "results", self.J, shape_only=True)
        if lab.shape[1] != self.J:
            raise ValueError(f"labels must have {self.J} joints, got {lab.shape[1]}")
        if tuple(res.shape) != tuple(lab.shape):
            raise ValueError(f"results must match labels {tuple(lab.shape)}, got {tuple(res.shape)}")
        lab = MonkeyDetector._dev_labels(lab, "labels")
        res = MonkeyDetector._dev_labels(res, "results")
        if res.device != lab.device:
            raise ValueError("labels and results must be on the same device")
        if self.device is not None and self._state is not None and lab.device != self._state.device:
            raise ValueError("the evaluator's state is on another device")
        n = lab.shape[0]
        dev = lab.device
        self._ensure(dev)
        lib = self._lib()
        wb = int(lib.mp_eval_work_bytes(n, self.J))
        if self._work is None or self._work.numel() < wb:
            self._work = torch.empty((wb,), dtype=torch.uint8, device=dev)
        dist = torch.empty((n, self.J), dtype=torch.float32, device=dev)
        fmean = torch.empty((n,), dtype=torch.float32, device=dev)
        fmax = torch.empty((n,), dtype=torch.float32, device=dev)
        st = _lib.current_stream(dev) if stream is None else stream
        _lib.check(lib.mp_eval_accumulate_dev(ctypes.c_void_p(self._state.data_ptr()), ctypes.c_void_p(lab.data_ptr()),
                                              ctypes.c_void_p(res.data_ptr()), n, self.J, self.T, float(scale),
                                              ctypes.c_void_p(self._work.data_ptr()), wb,
                                              ctypes.c_void_p(dist.data_ptr()), ctypes.c_void_p(fmean.data_ptr()),
                                              ctypes.c_void_p(fmax.data_ptr()), ctypes.c_void_p(st)))
        self.last_frame_errors = (dist, fmean, fmax)
        return self

    def summary_array(self, stream=None):
        """the flat float64 array of ``mp_eval_summary_dev`` as numpy (one sync)"""
        if self._state is None:
            raise RuntimeError("PoseEvaluator.summary() before any update()")
        st = _lib.current_stream(self.device) if stream is None else stream
        _lib.check(self._lib().mp_eval_summary_dev(ctypes.c_void_p(self._state.data_ptr()), self.J, self.T,
                                                   ctypes.c_void_p(self._summary.data_ptr()), ctypes.c_void_p(st)))
        return self._summary.cpu().numpy()

    def summary(self, stream=None):
        a = self.summary_array(stream)
        J, T = self.J, self.T
        return dict(frames=int(a[0]) if a[0] == a[0] else -1, valid_frames=int(a[1]) if a[1] == a[1] else -1,
                    mean_error=float(a[2]), max_error=float(a[3]), joint_mean=a[4:4 + J].copy(),
                    thresholds=self.thresholds.copy(), within_max=a[4 + J:4 + J + T].copy(),
                    within_mean=a[4 + J + T:4 + J + 2 * T].copy())


def _device_eval(labels, results, thresholds=()):
    """one batch through a fresh PoseEvaluator: (evaluator, summary)"""
    import torch
    if not (isinstance(labels, torch.Tensor) and isinstance(results, torch.Tensor)):
        raise TypeError("labels and results must both be CUDA (ROCm) tensors (or both numpy arrays)")
    if labels.dim() != 3:
        raise ValueError(f"labels must be [frames, joints, 3], got {tuple(labels.shape)}")
    ev = PoseEvaluator(labels.shape[1], thresholds)
    ev.update(labels, results)
    return ev, ev.summary()


def _count(s, key):
    return int(round(float(s[key][0]) * s["frames"] / 100.))


def getMeanError_np(labels, results):
    """Mean over frames of the mean joint distance (pose_evaluation.py:10-15)."""
    if _is_cuda(labels) or _is_cuda(results):
        return np.float64(_device_eval(labels, results)[1]["mean_error"])
    return np.nanmean(np.nanmean(_joint_dist(labels, results), axis=1))


def getMaxError_np(labels, results):
    """Largest joint distance (pose_evaluation.py:18-24)."""
    if _is_cuda(labels) or _is_cuda(results):
        return np.float64(_device_eval(labels, results)[1]["max_error"])
    return np.nanmax(_joint_dist(labels, results))


def getMean_np(labels, results):
    """Mean joint distance per joint over a [frames, 3] pair (pose_evaluation.py:26-28)."""
    if _is_cuda(labels) or _is_cuda(results):
        if labels.dim() != 2:
            raise ValueError(f"labels must be [frames, 3], got {tuple(labels.shape)}")
        return np.float64(_device_eval(labels[:, None, :], results[:, None, :])[1]["joint_mean"][0])
    return np.nanmean(_joint_dist(labels, results, axis=1), axis=0)


def getNumFramesWithinMaxDist(labels, results, dist):
    """Frames whose worst joint is within ``dist`` mm (pose_evaluation.py:63-69)."""
    if _is_cuda(labels) or _is_cuda(results):
        return _count(_device_eval(labels, results, [dist])[1], "within_max")
    return (np.nanmax(_joint_dist(labels, results), axis=1) <= dist).sum()


def getNumFramesWithinMeanDist(labels, results, dist):
    """Frames whose mean joint distance is within ``dist`` mm (pose_evaluation.py:72-78)."""
    if _is_cuda(labels) or _is_cuda(results):
        return _count(_device_eval(labels, results, [dist])[1], "within_mean")
    return (np.nanmean(_joint_dist(labels, results), axis=1) <= dist).sum()


def getJointMeanError(labels, results, jointID):
    """Mean distance of one joint over the frames (pose_evaluation.py:81-88)."""
    if _is_cuda(labels) or _is_cuda(results):
        return np.float64(_device_eval(labels, results)[1]["joint_mean"][jointID])
    lab, res = np.asarray(labels), np.asarray(results)
    return np.nanmean(np.sqrt(np.square(lab[:, jointID, :] - res[:, jointID, :]).sum(axis=1)))


def _same_shape(labels, results):
    if tuple(labels.shape) != tuple(results.shape):
        raise AssertionError(f"labels {tuple(labels.shape)} and results {tuple(results.shape)} differ")


def getMeanError_train(labels, results):
    """pose_evaluation.py:30-36 on [B, J, 3]: the mean over frames of the mean joint distance
    (NaN-aware, see the module docstring)."""
    _same_shape(labels, results)
    return getMeanError_np(labels, results)


def getMeanError(labels, results):
    """pose_evaluation.py:38-44 on one frame [J, 3]: the mean joint distance."""
    _same_shape(labels, results)
    if _is_cuda(labels) or _is_cuda(results):
        if labels.dim() != 2:
            raise ValueError(f"labels must be [joints, 3], got {tuple(labels.shape)}")
        return np.float64(_device_eval(labels[None], results[None])[1]["mean_error"])
    return np.nanmean(_joint_dist(labels, results, axis=1), axis=0)


def getMeanErrors_N(labels, results):
    """pose_evaluation.py:46-52 on [B, J, 3]: the mean joint distance of every frame, [B] (a CUDA
    float64 tensor for CUDA input)."""
    _same_shape(labels, results)
    if _is_cuda(labels) or _is_cuda(results):
        ev, _ = _device_eval(labels, results)
        return ev.last_frame_errors[1].double()
    return np.nanmean(_joint_dist(labels, results), axis=1)


def getMaxError(labels, results):
    """pose_evaluation.py:54-60 on [B, J, 3]: the largest joint distance."""
    _same_shape(labels, results)
    return getMaxError_np(labels, results)
