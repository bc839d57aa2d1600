"""Drop-in for the inference pieces of ``/root/reference/train_cnn_networks_hgru.py``: the attention
(centre-of-mass) regressor and the frame -> CoM -> crop -> pose chain of its ``test_model`` loop.

* ``attn_model_struct().build(images, num_dims)`` -> ``.out_put`` [N, num_dims]
  (train_cnn_networks_hgru.py:422-525): ``mp_attn_fwd`` -- TF1 bilinear resize to 128x128, five
  conv + max-pool + BN stages, afc_1 + relu + BN, afc_out, on the generic implicit-GEMM conv /
  split-K FC kernels (fp32 MFMA).
* ``prepare_data_test(images, tr_res, md, config)`` (61-74): with CUDA tensors it crops every
  frame on the GPU in one launch (``mp_crop3d_dev``), bit-exact with the host ``cropArea3D``
  integers, and the patches never leave the device; with numpy arrays it runs the native host
  crop (``mp_crop3d_batch``).
* ``FramePosePipeline``: ``test_model``'s per-batch body (284-321) -- attention, device crop,
  hGRU pose regressor -- as one device-resident call.
* ``prepare_data(images, labels, tr_res, md, config)`` (41-59): ``prepare_data_test`` plus the label
  half (relative labels, ``mp_rel_labels_dev``); ``calc_com_error`` (36-39); ``ValidationPipeline``
  / ``evaluate_tfrecord``: the validation pass of ``train_model`` (160-173, 229-237) for labelled
  batches -- attention, crop + relative labels, pose, joint errors and metrics accumulated in device
  memory (``pose_evaluation.PoseEvaluator``), no host round trip.
* ``RealDataPipeline`` / ``eval_model_on_real_data`` (342-419): recorded camera frames as stored
  (uint16 or float32, [w, h]) -> transpose, depth gate, / image_max_depth on the device
  (``mp_real_frames_dev``) -> the ``FramePosePipeline`` calls -> absolute joints.  The pipelines'
  ``render`` draws the joints on the frames on the device (``monkeydetector.render_overlays``): the
  picture the reference's loops end with.
* ``cnn_model_struct().build(crops, num_classes)`` -> ``.out_put`` [N, num_classes]
  (train_cnn_networks_hgru.py:626-760): the regressor the reference's driver builds for
  validation (169), ``test_model`` (291) and ``eval_model_on_real_data`` (363) -- five conv +
  max-pool stages and four FCs, recorded op for op and run on the native layer-graph runtime.

Training (``train_model``: TFRecord queues, Adam, l2 losses) is outside the inference path.
``train_mode`` must be falsy: the reference's ``test_model`` builds the attention net with
``train_mode=True`` (dropout 0.7 and batch-statistics BN at test time, 287); that is a training
graph and raises here, as for the other facades.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from . import _lib
from . import weights as W
from ._regressor import GraphRegressorBase, RegressorBase


@dataclass
class InferenceConfig:
    """The ``config.py`` fields the inference chain reads (config.py:31-51)."""
    image_orig_size: List[int] = field(default_factory=lambda: [424, 512, 1])
    image_target_size: List[int] = field(default_factory=lambda: [128, 128, 1])
    image_max_depth: float = 10000.
    num_joints: int = 23
    num_dims: int = 3

    @property
    def num_classes(self) -> int:
        return self.num_joints * self.num_dims


class attn_model_struct(RegressorBase):
    """``attn_model_struct`` (train_cnn_networks_hgru.py:422-525), inference."""

    MODEL_KIND = _lib.MP_MODEL_ATTN

    def __init__(self, trainable=True):
        super().__init__(trainable)
        self._BATCH_NORM_DECAY = 0.997
        self._BATCH_NORM_EPSILON = 1e-5

    def build(self, depth, output_shape, batch_norm=None, train_mode=None):
        """``depth`` CUDA [N, H, W, 1] fp32 normalised frames (images / image_max_depth); any H, W
        (resized to 128 x 128).  Sets and returns ``.out_put`` [N, output_shape]."""
        depth = self._check_input(depth, batch_norm, train_mode)
        self.output_shape = int(output_shape)
        table = W.attn_vars(output_shape=self.output_shape)
        self._ctx = self._context(self.output_shape, table, depth.device.index or 0)
        return self.forward(depth)

    def forward(self, depth, out=None):
        import torch
        depth = depth.detach().float().contiguous()
        if out is None:
            out = torch.empty((depth.shape[0], self.output_shape), dtype=torch.float32, device=depth.device)
        self._ctx.attn_fwd(depth, out, _lib.current_stream(depth.device))
        self.out_put = out
        return out


class cnn_model_struct(GraphRegressorBase):
    """``cnn_model_struct`` (train_cnn_networks_hgru.py:626-760), inference: conv_1 .. conv_5 (3x3,
    conv_5 5x5; relu(conv2d SAME + b)) each with a 2x2 max pool, fc_1 .. fc_3 + relu, fc_4.  The
    reference's driver builds it for the validation / test crops (169, 291, 363).  ``build``
    records the reference's calls (``record``, op for op against the reference's AST in
    tests/test_cnn_model.py) and runs them on the layer-graph runtime (the f16x3 halo / tap-skipping
    convs fused with their max pools, split-K FCs)."""

    OUTPUT_ATTRS = ("out_put",)

    def record(self, h, w, output_shape):
        """The graph of build (639-673)."""
        g = self._new_graph(h, w)
        c, put = self.conv_layer, self._set
        prev = g.input                                                                       # 641
        for i, (name, k, cin, cout) in enumerate(W.CNN_CONV_SPECS, 1):                       # 642-656
            put(f"conv{i}", c(prev, cin, cout, name, filter_size=k))
            prev = put(f"pool{i}", self.max_pool(getattr(self, f"conv{i}"), f"pool_{i}"))
        flat = 1
        for s in self.pool5.shape:
            flat *= s
        r1 = self._relu_fc("fc1", "relu1", self.pool5, flat, 1024, "fc_1")                     # 658-661
        r2 = self._relu_fc("fc2", "relu2", r1, 1024, 1024, "fc_2")                            # 663-666
        r3 = self._relu_fc("fc3", "relu3", r2, 1024, 1024, "fc_3")                            # 668-671
        f4 = put("fc4", self.fc_layer(r3, 1024, int(output_shape), "fc_4"))                   # 672
        put("out_put", g.identity(f4))                                                        # 673
        return g

    def build(self, depth, output_shape, batch_norm=None, train_mode=None):
        """``depth`` CUDA [N, H, W, 1] fp32 crops (crop / 10000); sets and returns ``.out_put``
        [N, output_shape] (joint-major, / (cube_z / 2), as hgru_pose)."""
        return self._graph_build(depth, (output_shape,), batch_norm, train_mode)

    def forward(self, depth):
        return self._graph_forward(depth)


def prepare_data_test(image_np, tr_res, md, config, dsize: Optional[int] = None):
    """``prepare_data_test`` (train_cnn_networks_hgru.py:61-74): returns (patches [N, 128, 128, 1]
    = cropArea3D(image * max_depth, tr_res * [orig0, orig1, max_depth]) / max_depth, coms, Ms).

    CUDA tensors in -> everything stays on the device (``coms`` [N, 3] and ``Ms`` [N, 3, 3] float64
    tensors); numpy in -> the native host crop, ``coms`` / ``Ms`` as lists like the reference."""
    import torch
    dsize = int(dsize or config.image_target_size[0])
    scale = (float(config.image_orig_size[0]), float(config.image_orig_size[1]), float(config.image_max_depth))
    if isinstance(image_np, torch.Tensor) and image_np.is_cuda:
        patches, Ms, coms = md.crop_batch_device(image_np, tr_res, com_scale=scale,
                                                 frame_scale=float(config.image_max_depth), dsize=dsize)
        return patches, coms, Ms
    fr = np.asarray(image_np, np.float32)
    if fr.ndim == 4:
        fr = fr[..., 0]
    frames_mm = fr * np.float32(config.image_max_depth)
    coms_in = np.asarray(tr_res, np.float32).reshape(-1, 3) * np.array(scale)
    patches, Ms, coms = md.crop_batch(frames_mm, coms=coms_in, dsize=dsize)
    if float(md.maxDepth) != float(config.image_max_depth):
        raise ValueError("md.maxDepth must equal config.image_max_depth for the host batch crop")
    return patches, list(coms), [np.asmatrix(m) for m in Ms]


def _is_cuda(x):
    return hasattr(x, "is_cuda") and not isinstance(x, np.ndarray) and x.is_cuda


def prepare_data(image_np, image_label_shaped, tr_res, md, config, show=False, check=True):
    """``prepare_data`` (train_cnn_networks_hgru.py:41-59): returns (patches [N, 128, 128, 1] =
    cropArea3D(image * max_depth, tr_res * [orig0, orig1, max_depth]) / max_depth, rel_labels
    [N, 3J] = clip(getRelativeCoordinates(label, com).xyz / (cube_z / 2), -1, 1)), float32 holding
    the reference's values.  The batch is ``image_np.shape[0]`` (the reference's
    ``config.train_batch`` only sizes its arrays).

    CUDA tensors in -> ``crop_batch_device`` and ``mp_rel_labels_dev``, nothing leaves the device
    (``check``: read the crop status back, the one sync); numpy in -> the native host crop and the
    host label half.  ``show=True`` (the reference's plot of every crop) raises."""
    if show:
        raise NotImplementedError("show=True plots every crop in the reference; plotting is out of scope")
    if _is_cuda(image_np):
        patches, rel, _, _ = _prepare_data_device(image_np, image_label_shaped, tr_res, md, config, check)
        return patches, rel
    patches, coms, _ = prepare_data_test(image_np, tr_res, md, config)
    lab = np.asarray(image_label_shaped, np.float32)
    if lab.shape[0] != patches.shape[0]:
        raise ValueError(f"{patches.shape[0]} frames but {lab.shape[0]} label rows")
    return patches, md.relative_labels(lab, np.stack(coms))


def _prepare_data_device(frames, labels, tr_res, md, config, check):
    """prepare_data on the device -> (patches, rel_labels, coms [n, 3] f64, Ms [n, 3, 3] f64)"""
    n = frames.shape[0]
    J = int(getattr(config, "num_joints", 0)) or None
    lab = md._dev_labels(labels, "image_label_shaped", J)     # raises before any GPU call
    if lab.shape[0] != n:
        raise ValueError(f"{n} frames but {lab.shape[0]} label rows")
    scale = (float(config.image_orig_size[0]), float(config.image_orig_size[1]), float(config.image_max_depth))
    patches, Ms, coms = md.crop_batch_device(frames, tr_res, com_scale=scale,
                                             frame_scale=float(config.image_max_depth),
                                             dsize=int(config.image_target_size[0]), check=check)
    return patches, md.relative_labels_device(lab, coms), coms, Ms


def calc_com_error(labels, predictions):
    """``calc_com_error`` (train_cnn_networks_hgru.py:36-39): the mean over the batch of the
    distance between [n, 3] (u, v, d) rows; numpy in -> float32 numpy, CUDA tensors in -> the
    device evaluator with one joint (float64)."""
    assert tuple(labels.shape) == tuple(predictions.shape)
    from . import pose_evaluation as PE
    if _is_cuda(labels) or _is_cuda(predictions):
        if labels.dim() != 2 or labels.shape[1] != 3:
            raise ValueError(f"labels must be [n, 3], got {tuple(labels.shape)}")
        return PE.getMeanError_np(labels[:, None, :], predictions[:, None, :])
    lab, pred = np.asarray(labels), np.asarray(predictions)
    return np.nanmean(np.sqrt(np.square(lab - pred).sum(axis=1)), axis=0)


class FramePosePipeline:
    """``test_model``'s per-batch body (train_cnn_networks_hgru.py:284-321) on one GPU:
    frames -> attention CoM -> device crop -> hGRU pose, no host round trip in between.

    ``run(frames)`` returns (pose output [N, num_classes] normalised by cube_z / 2, coms [N, 3],
    Ms [N, 3, 3]); the caller maps to millimetres with ``md.getAbsoluteCoordinates`` as the
    reference does."""

    def __init__(self, attn: attn_model_struct, pose_model, md, config: Optional[InferenceConfig] = None,
                 check_crops: bool = True):
        self.attn, self.pose, self.md = attn, pose_model, md
        self.config = config or InferenceConfig()
        self.check_crops = check_crops
        self._last_frames = None

    def run(self, frames, h2_init=None):
        cfg = self.config
        self._last_frames = frames
        com_norm = self.attn.build(frames, cfg.num_dims)
        patches, Ms, coms = self.md.crop_batch_device(
            frames, com_norm, com_scale=(cfg.image_orig_size[0], cfg.image_orig_size[1], cfg.image_max_depth),
            frame_scale=float(cfg.image_max_depth), dsize=cfg.image_target_size[0], check=self.check_crops)
        kw = {} if h2_init is None else {"h2_init": h2_init}    # cnn_model_struct has no hidden state
        out = self.pose.build(patches, cfg.num_classes, **kw)
        return out, coms, Ms

    def render(self, joints_uvd, **kw):
        """The frames of the last ``run`` with ``joints_uvd`` (CUDA [n, J, 3] or [n, S, J, 3], e.g. the
        uvd of ``md.getAbsoluteCoordinates_device``) drawn on them: ``monkeydetector.render_overlays``
        and its keywords -> CUDA uint8 [n, h, w, 3]."""
        from .monkeydetector import render_overlays
        if self._last_frames is None:
            raise RuntimeError("render() draws the frames of the last run(): call run() first")
        return render_overlays(self._last_frames, joints_uvd, **kw)

    def render_png(self, joints_uvd, **render_kw):
        """``render(...)`` followed by ``png.encode_png`` on the same stream: the pictures as finished PNG
        files in device memory -> (buf [n, png_bound(h, w)] uint8, sizes [n] int64), CUDA tensors reused by
        the next call of the same shape; ``png.png_files(buf, sizes)`` copies the files to the host."""
        return _render_png(self, dict(render_kw, joints_uvd=joints_uvd))


class ValidationPipeline:
    """The validation pass of ``train_model`` (train_cnn_networks_hgru.py:160-173, 229-237) and of
    ``test_model``'s loop for a labelled batch on one GPU: frames + labels -> attention CoM -> device
    crop + relative labels (``prepare_data``) -> pose regressor -> joint error in mm, accumulated in
    two device-resident evaluators (``pose_evaluation.PoseEvaluator``):

    * ``pose``: rel_labels against the pose output, both at scale ``cube_z / 2`` --
      ``getMeanError_train(val_crop_labels_shaped, val_results_shaped)`` (171-173);
    * ``com`` (one joint): ``calculateCoMfrom3DJoints(labels) / (orig0, orig1, max_depth)`` against
      the attention output -- ``calc_com_error(val_com2d, attn_val_results_shaped)`` (165-167).

    ``run(frames, labels, h2_init=None)``: ``frames`` CUDA [n, h, w, 1] fp32 normalised as for
    ``FramePosePipeline``, ``labels`` CUDA [n, 3J] or [n, J, 3] fp32 in mm -> (out [n, 3J],
    rel_labels [n, 3J], coms [n, 3] f64, Ms [n, 3, 3] f64).  Nothing leaves the device; the only
    sync is the crop status read when ``check_crops`` is set.  ``summary()`` ->
    ``{"pose": {...}, "com": {...}}`` (``PoseEvaluator.summary``); ``reset()`` starts over."""

    def __init__(self, attn: attn_model_struct, pose_model, md, config: Optional[InferenceConfig] = None,
                 thresholds=range(100), check_crops: bool = True):
        from .pose_evaluation import PoseEvaluator
        self.attn, self.pose, self.md = attn, pose_model, md
        self.config = config or InferenceConfig()
        self.check_crops = bool(check_crops)
        self.pose_eval = PoseEvaluator(self.config.num_joints, thresholds)
        self.com_eval = PoseEvaluator(1, thresholds)

    def run(self, frames, labels, h2_init=None):
        import torch
        cfg, md = self.config, self.md
        if not (isinstance(frames, torch.Tensor) and frames.is_cuda):
            raise TypeError("frames must be a CUDA (ROCm) tensor")
        lab = md._dev_labels(labels, "labels", cfg.num_joints)          # shape, then device: before any GPU call
        if lab.shape[1] != cfg.num_joints or lab.shape[0] != frames.shape[0]:
            raise ValueError(f"labels must be [{frames.shape[0]}, {cfg.num_joints}, 3], got {tuple(lab.shape)}")
        com_norm = self.attn.build(frames, cfg.num_dims)
        patches, rel, coms, Ms = _prepare_data_device(frames, lab, com_norm, md, cfg, self.check_crops)
        kw = {} if h2_init is None else {"h2_init": h2_init}
        if getattr(self.pose, "_ctx", None) is None:
            out = self.pose.build(patches, cfg.num_classes, **kw)
        else:
            out = self.pose.forward(patches, **kw)
        self.pose_eval.update(rel, out, scale=float(md.cube[2]) / 2.0)
        scale = (cfg.image_orig_size[0], cfg.image_orig_size[1], cfg.image_max_depth)
        com2d = md.calculateCoMfrom3DJoints(lab, scale=scale)
        self.com_eval.update(com2d[:, None, :], com_norm[:, None, :cfg.num_dims])
        return out, rel, coms, Ms

    def summary(self):
        return {"pose": self.pose_eval.summary(), "com": self.com_eval.summary()}

    def reset(self):
        self.pose_eval.reset()
        self.com_eval.reset()


def evaluate_tfrecord(tfrecord_file, pipeline: ValidationPipeline, batch_size, max_batches=None, device=None):
    """One epoch of ``data_loader.inputs(tfrecord_file, shuffle=False, device=...)`` (frames in mm as
    the reference's records hold them, labels [3J] in mm) through ``pipeline`` (reset first):
    frames / image_max_depth as the driver feeds them (161), then ``pipeline.run``.  Returns
    ``pipeline.summary()``; a partial last batch is dropped as ``shuffle_batch`` does."""
    import torch
    from . import data_loader as DL
    cfg = pipeline.config
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    pipeline.reset()
    done = 0
    for frames, labels in DL.inputs(tfrecord_file, 1, cfg.image_orig_size, [cfg.num_classes], int(batch_size),
                                    shuffle=False, device=dev):
        if max_batches is not None and done >= int(max_batches):
            break
        pipeline.run(frames / float(cfg.image_max_depth), labels)
        done += 1
    if done == 0:
        raise ValueError(f"{tfrecord_file}: fewer records than one batch of {batch_size}")
    return pipeline.summary()


def _render_png(pipeline, render_kw):
    """``pipeline.render(**render_kw)`` followed by ``png.encode_png`` on the same stream"""
    from .png import encode_png
    return encode_png(pipeline.render(**render_kw), stream=render_kw.get("stream"))


def _render_sets(frames, uvd, extra_sets, kw):
    """``render_overlays`` of ``frames`` with ``uvd`` as set 0 and ``extra_sets`` drawn over it"""
    import torch
    from .monkeydetector import render_overlays
    sets = [uvd] + list(extra_sets or [])
    if any(not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(uvd.shape) for t in sets):
        raise ValueError(f"every extra joint set must be a tensor of shape {tuple(uvd.shape)} (pad with NaN)")
    joints = uvd if len(sets) == 1 else torch.stack([t.to(uvd.dtype) for t in sets], dim=1)
    return render_overlays(frames, joints, **kw)


class DetectorPosePipeline:
    """SURVEY config 5 for a batch, device-resident: ``MonkeyDetector``'s own ``calculateCoM`` of
    every frame (``mp_center_of_mass_dev_dt``) -> device crop around those float64 CoMs
    (``mp_crop3d_dev_coms_dt``) -> the pose forward -> absolute joints (``mp_abs_joints_dev``), all on
    the current stream with no host round trip; the only sync is the status read when
    ``check_crops`` is set.  The batch counterpart of ``StreamPosePipeline`` (same bits per frame).

    ``pose_model``: a pose regressor with ``build(patches, num_classes, h2_init=)`` /
    ``forward(patches, h2_init=)`` (``hgru_pose.model``).  ``frame_scale``: 1 for frames in mm,
    10000 for frames normalised by the maximum depth.  ``run(frames, h2_init=None)`` with ``frames``
    CUDA [n, h, w] or [n, h, w, 1], fp32 or ``torch.uint16`` (the camera's own millimetres, with
    ``frame_scale`` 1: half the bytes to upload, the host's uint16 semantics) -> (xyz [n, J, 3] mm,
    uvd [n, J, 3], coms [n, 3] f64, Ms [n, 3, 3] f64), CUDA tensors reused by the next call of the
    same batch shape and frame dtype."""

    def __init__(self, pose_model, md, dsize: int = 128, num_joints: int = 23, docom: bool = False,
                 frame_scale: float = 1.0, check_crops: bool = True):
        self.pose, self.md = pose_model, md
        self.dsize, self.num_joints = int(dsize), int(num_joints)
        self.docom, self.frame_scale, self.check_crops = bool(docom), float(frame_scale), bool(check_crops)
        self._key, self._buf, self._out = None, None, None
        self._last = None

    def render(self, extra_sets=None, **kw):
        """The frames given to the last ``run`` with its uvd joints drawn on them
        (``monkeydetector.render_overlays`` and its keywords) -> CUDA uint8 [n, h, w, 3].
        ``extra_sets``: further CUDA [n, J, 3] joint sets drawn over them (pad a short one with NaN)."""
        if self._last is None:
            raise RuntimeError("render() draws the frames of the last run(): call run() first")
        return _render_sets(self._last[0], self._last[1], extra_sets, kw)

    def render_png(self, **render_kw):
        """``render(...)`` followed by ``png.encode_png`` on the same stream: the pictures as finished PNG
        files in device memory -> (buf [n, png_bound(h, w)] uint8, sizes [n] int64), CUDA tensors reused by
        the next call of the same shape; ``png.png_files(buf, sizes)`` copies the files to the host."""
        return _render_png(self, render_kw)

    def run(self, frames, h2_init=None):
        import torch
        md = self.md
        # shape, uint16 scale, then device: raises before any GPU call
        fr, dt = md._dev_frames(frames, frame_scale=self.frame_scale)
        n, h, w = fr.shape
        key = (n, h, w, fr.device, dt)
        if key != self._key:
            self._buf = md._detect_buffers(n, h, w, self.dsize, fr.device, dt)
            self._out = tuple(torch.empty((n, self.num_joints, 3), dtype=torch.float32, device=fr.device)
                              for _ in range(2))
            self._key = key
        patches, Ms, coms = md.detect_crop_device(fr, None, frame_scale=self.frame_scale, dsize=self.dsize,
                                                  docom=self.docom, check=self.check_crops, _buffers=self._buf)
        nc = self.num_joints * 3
        if getattr(self.pose, "_ctx", None) is None:
            out = self.pose.build(patches, nc, h2_init=h2_init)
        else:
            out = self.pose.forward(patches, h2_init=h2_init)
        xyz, uvd = md.getAbsoluteCoordinates_device(out, coms, self.num_joints, out=self._out)
        self._last = (fr, uvd)
        return xyz, uvd, coms, Ms


class RealDataPipeline:
    """``eval_model_on_real_data``'s per-frame body (train_cnn_networks_hgru.py:385-407) for a batch
    of recorded camera frames on one GPU: raw frames as stored -> transpose, gate, / image_max_depth
    (``monkeydetector.preprocess_real_frames``, ``mp_real_frames_dev``) -> the calls of
    ``FramePosePipeline.run`` (attention CoM, device crop, pose regressor) -> absolute joints
    (``md.getAbsoluteCoordinates_device``).  Nothing leaves the device; the only sync is the crop
    status read when ``check_crops`` is set.

    ``run(raw, h2_init=None)``: ``raw`` CUDA [n, w, h] (``transposed``, as the recordings are stored;
    else [n, h, w]), ``torch.uint16`` (the camera's millimetres, uploaded as they are) or
    ``torch.float32`` -> (xyz [n, J, 3] mm, uvd [n, J, 3], coms [n, 3] f64, Ms [n, 3, 3] f64,
    com_norm [n, 3] the attention output).  The frame buffer and xyz / uvd are reused by the next call
    of the same batch shape and dtype.  Any ``n``: the reference runs one frame per step, and a frame's
    results here do not depend on the batch it is in.

    The crop input.  The reference crops from float64, ``(im / 10000.) * 10000.`` (399, 68); here the
    crop reads the float32 normalised frame times ``frame_scale = image_max_depth`` in float32, like
    ``FramePosePipeline``.  For gated uint16 frames (``oracle.crop_ref.synth_frame`` seeds 0..9, a CoM
    over the body pixels rounded through float32) both routes give equal float32 patches and ``M``
    (tests/test_real_frames_cpu.py): ``f32(v / 10000) * 10000`` differs from ``v`` for 9152 of the
    65536 uint16 values, but the final ``/ 10000`` lands on the same float32.  The routes can differ
    only where ``zstart`` or ``zend`` of a crop falls within a float32 ulp of a pixel value; nothing
    more is claimed."""

    def __init__(self, attn: attn_model_struct, pose_model, md, config: Optional[InferenceConfig] = None,
                 gate=(1000, 3000), fill=10000, transposed: bool = True, check_crops: bool = True):
        self.config = config or InferenceConfig()
        self.md = md
        self.gate, self.fill, self.transposed = gate, fill, bool(transposed)
        self.frame_pipeline = FramePosePipeline(attn, pose_model, md, self.config, check_crops)
        self._key, self._frames, self._out = None, None, None
        self._drawn = False

    def run(self, raw, h2_init=None):
        import torch
        from .monkeydetector import preprocess_real_frames
        cfg = self.config
        if not isinstance(raw, torch.Tensor):
            raise TypeError("raw must be a CUDA (ROCm) tensor")
        key = (tuple(raw.shape), raw.dtype, raw.device)
        # shape, dtype, gate and device are checked in there, before any GPU call
        frames = preprocess_real_frames(raw, self.transposed, self.gate, self.fill, cfg.image_max_depth,
                                        out=self._frames if key == self._key else None)
        if key != self._key:
            n = frames.shape[0]
            self._frames = frames
            self._out = tuple(torch.empty((n, cfg.num_joints, 3), dtype=torch.float32, device=frames.device)
                              for _ in range(2))
            self._key = key
        out, coms, Ms = self.frame_pipeline.run(frames, h2_init)
        xyz, uvd = self.md.getAbsoluteCoordinates_device(out, coms, cfg.num_joints, out=self._out)
        self._drawn = True
        return xyz, uvd, coms, Ms, self.frame_pipeline.attn.out_put

    def render(self, bones=None, depth_range=None, extra_sets=None, **kw):
        """The picture the reference's loop ends with (``plt.imshow(im); plt.scatter(uvd)``, 409-415),
        on the device: the last ``run``'s frames -- the gated, normalised float32 buffer kept here --
        with its uvd joints drawn on them (``monkeydetector.render_overlays`` and its keywords) ->
        CUDA uint8 [n, h, w, 3].  ``depth_range`` defaults to the gate in the frames' units,
        ``(lo, hi) / image_max_depth`` ((0, 1) without a gate).  ``extra_sets``: further CUDA
        [n, J, 3] joint sets drawn over the results (pad a short one, such as a CoM, with NaN)."""
        if not self._drawn:
            raise RuntimeError("render() draws the frames of the last run(): call run() first")
        if depth_range is None:
            md = float(self.config.image_max_depth)
            depth_range = (0.0, 1.0) if self.gate is None else (self.gate[0] / md, self.gate[1] / md)
        return _render_sets(self._frames, self._out[1], extra_sets, dict(kw, bones=bones, depth_range=depth_range))

    def render_png(self, **render_kw):
        """``render(...)`` followed by ``png.encode_png`` on the same stream: the pictures as finished PNG
        files in device memory -> (buf [n, png_bound(h, w)] uint8, sizes [n] int64), CUDA tensors reused by
        the next call of the same shape; ``png.png_files(buf, sizes)`` copies the files to the host."""
        return _render_png(self, render_kw)


def eval_model_on_real_data(real_data_dir, pipeline, batch_size=16, device=None, overlay=None, overlay_args=None,
                            overlay_png=None):
    """``eval_model_on_real_data`` (train_cnn_networks_hgru.py:342-419) over a directory of recorded
    frames: the files ``sorted(glob(real_data_dir + '*.npy'))`` (the reference's pattern: the directory
    ends in its separator), each loaded on the host, stacked ``batch_size`` at a time, uploaded as they
    are (uint16 stays uint16) and run through ``pipeline.run`` (a ``RealDataPipeline``).  Returns
    (files, xyz [N, J, 3] mm, uvd [N, J, 3], coms [N, 3] f64) as numpy arrays in file order.  The last,
    partial batch is run too: every file is a result.  All frames of a directory share one shape and
    one dtype, ``uint16`` or ``float32``; anything else raises.

    The reference's plot of every frame (409-415) is ``overlay``: a callback called once per batch with
    ``(files, rgb)``, the batch's file names and ``pipeline.render(**overlay_args)`` copied to the host
    as a numpy uint8 [n, h, w, 3] array (the depth frame through a colour table, the joints drawn on
    it).  ``None``: nothing is drawn; the four returned values are the same either way.

    ``overlay_png`` is the same picture as a finished file: a callback called once per batch with
    ``(files, pngs)``, ``pngs`` a list of ``bytes``, one PNG file a frame, encoded on the device
    (``pipeline.render_png(**overlay_args)``): only the compressed bytes cross to the host.

    A directory with no ``.npy`` file but ``*.png`` frames (the reference importer's ``depth_*.png``)
    is read as PNG files: every file's IHDR is checked up front (one shape, one of gray16 / gray8), and
    each batch's files are uploaded as they are and decoded on the device (``png.decode_png``), so only
    the compressed bytes cross.  PNG frames are [h, w]: a pipeline built with ``transposed=True``
    raises ``ValueError`` before any frame is run."""
    import glob
    import torch
    files = sorted(glob.glob(real_data_dir + '*.npy'))
    pngs = [] if files else sorted(glob.glob(real_data_dir + '*.png'))
    if not files and not pngs:
        raise ValueError(f"no .npy frames match {real_data_dir + '*.npy'!r}")
    batch_size = int(batch_size)
    if batch_size <= 0:
        raise ValueError(f"batch_size must be positive, got {batch_size}")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if pngs:
        return _eval_png_frames(pngs, pipeline, batch_size, dev, overlay, overlay_args, overlay_png)
    first = None
    for f in files:                              # the headers alone, before any frame is run
        a = np.load(f, mmap_mode="r", allow_pickle=False)
        if first is None:
            if a.ndim != 2 or a.dtype not in (np.uint16, np.float32):
                raise ValueError(f"{f}: expected a 2-D uint16 or float32 frame, got {a.dtype} {a.shape} "
                                 "(run other dtypes through the host preprocess_real_frames)")
            first = (a.shape, a.dtype)
        elif (a.shape, a.dtype) != first:
            raise ValueError(f"{f}: frame is {a.dtype} {a.shape}, but {files[0]} is {first[1]} {first[0]}; "
                             "all frames of a directory must share one shape and dtype")
        del a
    xyz, uvd, coms = [], [], []
    for i in range(0, len(files), batch_size):
        batch = np.stack([np.load(f, allow_pickle=False) for f in files[i:i + batch_size]])
        res = pipeline.run(torch.from_numpy(batch).to(dev))
        for acc, t in zip((xyz, uvd, coms), res[:3]):
            acc.append(t.detach().cpu().numpy().copy())     # a copy: the pipeline reuses its buffers
        if overlay is not None:
            overlay(files[i:i + batch_size], pipeline.render(**(overlay_args or {})).cpu().numpy())
        if overlay_png is not None:
            from .png import png_files
            overlay_png(files[i:i + batch_size], png_files(*pipeline.render_png(**(overlay_args or {}))))
    return files, np.concatenate(xyz), np.concatenate(uvd), np.concatenate(coms)


def _eval_png_frames(files, pipeline, batch_size, dev, overlay, overlay_args, overlay_png):
    """eval_model_on_real_data over PNG frames: IHDRs first, then batch by batch upload -> decode -> run"""
    import torch
    from . import png
    if getattr(pipeline, "transposed", False):
        raise ValueError("PNG frames are stored [h, w]: build the pipeline with transposed=False")
    first = None
    for f in files:                              # the IHDRs alone, before any frame is run
        with open(f, "rb") as fh:
            try:
                info = png.png_info(fh.read(33))
            except ValueError as e:
                raise ValueError(f"{f}: {e}") from None
        if first is None:
            if info[2] not in ("gray16", "gray8"):
                raise ValueError(f"{f}: expected a 16- or 8-bit grayscale PNG frame, not interlaced")
            first = info
        elif info != first:
            raise ValueError(f"{f}: frame is {info[2]} {info[:2]}, but {files[0]} is {first[2]} {first[:2]}; "
                             "all frames of a directory must share one shape and format")
    h, w, fmt = first
    xyz, uvd, coms = [], [], []
    for i in range(0, len(files), batch_size):
        names = files[i:i + batch_size]
        try:
            frames = png.decode_png_files(names, device=dev, format=fmt)
        except ValueError as e:
            raise ValueError(f"{names[0]} ... {names[-1]}: {e}") from None
        if frames.shape[1:] != (h, w):
            raise ValueError(f"{names[0]}: decoded {tuple(frames.shape[1:])}, expected {(h, w)}")
        res = pipeline.run(frames if fmt == "gray16" else frames.to(torch.uint16))
        for acc, t in zip((xyz, uvd, coms), res[:3]):
            acc.append(t.detach().cpu().numpy().copy())     # a copy: the pipeline reuses its buffers
        if overlay is not None:
            overlay(names, pipeline.render(**(overlay_args or {})).cpu().numpy())
        if overlay_png is not None:
            overlay_png(names, png.png_files(*pipeline.render_png(**(overlay_args or {}))))
    return files, np.concatenate(xyz), np.concatenate(uvd), np.concatenate(coms)


class StreamPosePipeline:
    """SURVEY config 5, one depth frame per call: the host CoM crop of ``MonkeyDetector`` (native
    ``mp_crop3d_batch``) -> the hGRU pose forward at batch 1 -> absolute joints
    (``getAbsoluteCoordinates``, monkeydetector.py:356-360).  The reference's frame loop
    (train_cnn_networks_hgru.py:284-321 with the detector's ``cropArea3D`` in place of the attention
    net) minus the per-call allocations: the crop is written straight into a reused host buffer, one
    H2D and one D2H bracket the forward on the current stream.  ``pinned=True`` stages through pinned
    memory with asynchronous copies and waits on that stream alone; it measured no faster than the
    default pageable blocking copies at batch 1 (1.103 vs 1.097 ms p50, DESIGN.md §3a'').

    ``pose_model``: a built ``hgru_pose.model`` (weights loaded); ``h2_init``: an optional fixed
    [1, dsize / 2, dsize / 2, 64] CUDA hidden state (else the model's own hidden init).
    ``run(frame_mm)`` -> (joints_xyz [num_joints, 3] mm, joints_uvd [num_joints, 3], com_uvd [3])."""

    def __init__(self, pose_model, md, h2_init=None, dsize: int = 128, num_joints: int = 23, device=None,
                 pinned: bool = False):
        import torch
        self.pose, self.md, self.h2_init = pose_model, md, h2_init
        self.dsize, self.num_joints = int(dsize), int(num_joints)
        dev = torch.device(device) if device is not None else (
            h2_init.device if h2_init is not None else torch.device("cuda", torch.cuda.current_device()))
        self.pinned = bool(pinned)   # False: pageable staging, blocking copies (the copies' own waits)
        self._x_host = torch.empty((1, self.dsize, self.dsize, 1), dtype=torch.float32)
        if self.pinned:
            self._x_host = self._x_host.pin_memory()
        self._x_np = self._x_host.numpy()
        self._x_dev = torch.empty((1, self.dsize, self.dsize, 1), dtype=torch.float32, device=dev)
        self._y_host = torch.empty((1, self.num_joints * 3), dtype=torch.float32)
        if self.pinned:
            self._y_host = self._y_host.pin_memory()
        self._y_dev = torch.empty((1, self.num_joints * 3), dtype=torch.float32, device=dev)
        self._half_z = float(md.cube[2]) / 2.0
        self._dev = dev
        # with a given O0 the built context is called directly (no per-call façade work)
        self._direct = h2_init is not None and getattr(pose_model, "_ctx", None) is not None
        if self._direct:
            self._h2 = h2_init.detach().float().contiguous()

    def run(self, frame_mm, com=None, nthreads: int = 1):
        import torch
        ts = torch.cuda.current_stream(self._dev)   # the copies and the forward on the caller's stream
        _, _, coms = self.md.crop_batch(np.asarray(frame_mm, np.float32)[None], None if com is None else [com],
                                        dsize=self.dsize, nthreads=nthreads, out=self._x_np)
        self._x_dev.copy_(self._x_host, non_blocking=self.pinned)
        if self._direct:
            self.pose._ctx.pose_fwd(self._x_dev, self._h2, self._y_dev, ts.cuda_stream)
            out = self._y_dev
        else:
            out = self.pose.forward(self._x_dev, h2_init=self.h2_init)
        self._y_host.copy_(out, non_blocking=self.pinned)
        if self.pinned:
            ts.synchronize()
        rel = self._y_host.numpy().reshape(self.num_joints, 3) * np.float32(self._half_z)
        xyz, uvd = self.md.getAbsoluteCoordinates(rel, coms[0])
        return xyz, uvd, coms[0]
