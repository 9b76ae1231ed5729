"""Training targets on the device: the collated batch the reference's dataset builds per image on the host
(dataset/generic_dataset.py:206-239, 441-687, dataset/datasets/nuscenes.py:348-391), for B images at once in three launches
(cf_targets_build, csrc/cf_targets.hip; semantics: include/cf_hip.h).

    ann = pack_annotations(anns)                                   # host: lists of the reference's annotation dicts -> padded tables
    batch = build_targets(ann, trans_out, calib, config, pc_dep=pc_dep, device="cuda")
    outputs = model(images, pc_hm=batch["pc_hm"], pc_dep=pc_dep, calib=calib)     # model.train() on a frozen trunk
    total, losses = GenericLoss(config, 10)(outputs, batch)

What comes before the annotation loop is train_inputs.py: `draw_augmentation` (getAugmentParam, the flip draw and the two affine
matrices: `trans_out` is its `getAffineTransform(center, scale, rotation, [out_w, out_h])`), `flip_annotations` on the dicts before
they are packed, `augment_images` (warp, flip, colour augmentation) and `radar_to_pc_dep(flip=...)`.  The caller still loads the
image bytes, the radar sweeps and the annotation dicts, and does lidar points and `prev` frames.
"""
import ctypes

import numpy as np
import torch

from . import _lib

# columns of the float64 table (cf_targets_args.ann)
_BBOX, _TRUNC, _AMODAL, _VEL, _VEL_MIN, _ALPHA, _DEPTH, _DIM, _LOC, _YAW = 0, 4, 5, 7, 10, 11, 12, 13, 16, 19
_FRUSTUM_KEYS = (("dimension", _lib.TGT_HAS_DIMENSION), ("alpha", _lib.TGT_HAS_ALPHA), ("depth", _lib.TGT_HAS_DEPTH))


def _get(node, name, default=None):
    try:
        return node[name] if isinstance(node, dict) else getattr(node, name)
    except (KeyError, AttributeError):
        return default


def _frustum(config):
    return bool(_get(config.DATASET, "RADAR_PC", False)) and bool(_get(config.MODEL, "FRUSTUM", False))


class PackedAnnotations:
    """`table` (B, max_objs, 20) float64, `itable` (B, max_objs, 3) int32 (class id after the class map, attributes, presence
    bits of the optional keys), `counts` (B) int32.  `to(device)` gives a copy on the device; a copy whose contents are
    overwritten in place (`copy_`) feeds a captured `build_targets` with new annotations."""

    def __init__(self, table, itable, counts):
        self.table, self.itable, self.counts = table, itable, counts

    @property
    def max_objs(self):
        return int(self.table.shape[1])

    @property
    def device(self):
        return self.table.device

    def to(self, device, non_blocking=False):
        return PackedAnnotations(*(t.to(device, non_blocking=non_blocking) for t in (self.table, self.itable, self.counts)))

    def copy_(self, other):
        for dst, src in ((self.table, other.table), (self.itable, other.itable), (self.counts, other.counts)):
            dst.copy_(src, non_blocking=True)
        return self


def pack_annotations(anns, class_ids=None, max_objs=128, config=None, num_classes=10):
    """Host only.  `anns`: a list (B) of lists of the reference's annotation dicts (convert_nuScenes.py): `bbox` [x, y, w, h] in
    source pixels, `category_id`, `truncated`, optionally `amodal_center`, `attributes`, `velocity_cam`, `alpha`, `depth`,
    `dimension`, `location`, `yaw`.  Only the first `max_objs` annotations of an image are kept, before any filtering
    (generic_dataset.py:209).  `class_ids` maps category_id -> class id; default: the identity on 1..num_classes
    (nuscenes.py:50).  With `config` given and radar + frustum association on, an annotation of a kept class that lacks
    `dimension`, `alpha` or `depth` raises ValueError (the reference raises KeyError inside addInstance)."""
    if not 1 <= int(max_objs) <= _lib.CF_TARGETS_MAX_OBJS:
        raise ValueError(f"pack_annotations: max_objs must be in 1..{_lib.CF_TARGETS_MAX_OBJS}, got {max_objs}")
    if class_ids is None:
        class_ids = {i + 1: i + 1 for i in range(int(num_classes))}
    need = _frustum(config) if config is not None else False
    B, M = len(anns), int(max_objs)
    table = np.zeros((B, M, _lib.CF_TARGETS_F), np.float64)
    itable = np.zeros((B, M, 3), np.int32)
    counts = np.zeros((B,), np.int32)
    for b, image in enumerate(anns):
        counts[b] = min(len(image), M)
        for i, ann in enumerate(image[:M]):
            row, bits = table[b, i], 0
            cid = int(class_ids[ann["category_id"]])
            row[_BBOX:_BBOX + 4] = ann["bbox"]
            row[_TRUNC] = ann["truncated"]
            if "amodal_center" in ann:
                row[_AMODAL:_AMODAL + 2], bits = ann["amodal_center"][:2], bits | _lib.TGT_HAS_AMODAL
            if "attributes" in ann:
                itable[b, i, 1], bits = int(ann["attributes"]), bits | _lib.TGT_HAS_ATTRIBUTES
            if "velocity_cam" in ann:
                row[_VEL:_VEL + 3], row[_VEL_MIN] = list(ann["velocity_cam"])[:3], min(ann["velocity_cam"])
                bits |= _lib.TGT_HAS_VELOCITY
            if "alpha" in ann:
                row[_ALPHA], bits = ann["alpha"], bits | _lib.TGT_HAS_ALPHA
            if "depth" in ann:
                depth = ann["depth"]
                row[_DEPTH] = depth[0] if isinstance(depth, (list, tuple)) else depth
                bits |= _lib.TGT_HAS_DEPTH
            if "dimension" in ann:
                row[_DIM:_DIM + 3], bits = ann["dimension"], bits | _lib.TGT_HAS_DIMENSION
            if "location" in ann:
                row[_LOC:_LOC + 3], bits = ann["location"], bits | _lib.TGT_HAS_LOCATION
            if "yaw" in ann:
                row[_YAW], bits = ann["yaw"], bits | _lib.TGT_HAS_YAW
            itable[b, i, 0], itable[b, i, 2] = cid, bits
            if need and not (cid > num_classes or cid <= -999):
                missing = [k for k, bit in _FRUSTUM_KEYS if not bits & bit]
                if missing:
                    raise ValueError(f"pack_annotations: image {b}, annotation {i} lacks {missing}: the ground-truth frustum "
                                     "association (DATASET.RADAR_PC + MODEL.FRUSTUM) needs dimension, alpha and depth")
    return PackedAnnotations(torch.from_numpy(table), torch.from_numpy(itable), torch.from_numpy(counts))


def _check_config(config):
    pyramid = _get(config.MODEL, "PYRAMID_OUT_SIZE")
    out_hw = tuple(int(v) for v in config.MODEL.OUTPUT_SIZE)
    if pyramid is not None and (len(pyramid) != 1 or tuple(int(v) for v in pyramid[0]) != out_hw):
        raise NotImplementedError("build_targets on the HIP path: one output layer of MODEL.OUTPUT_SIZE only "
                                  f"(MODEL.PYRAMID_OUT_SIZE = {list(pyramid)})")
    if _get(config.DATASET, "ONE_HOT_PC", False):
        raise NotImplementedError("build_targets on the HIP path: DATASET.ONE_HOT_PC is not implemented")
    rep = _get(config.DATASET, "HEATMAP_REP", "2d")
    if rep not in ("2d", "3d"):
        raise ValueError(f"Invalid heatmap representation: {rep}")
    return out_hw, rep


def build_targets(ann, trans_out, calib, config, pc_dep=None, scale_factor=1.0, num_classes=10, device=None):
    """-> the reference's collated batch with a leading B (keys, dtypes and shapes of `initReturn`; a key exists only for the heads
    in `config.heads`): heatmap0 (B,C,h,w), classIds i64, mask, truncMask, widthHeight, reg, amodal_offset, dimension, depth
    (B,M,1), rotbin i64, rotres, nuscenes_att, nuscenes_att_mask, velocity, pc_hm (B,3,h,w), calib, pc_dep (handed through) and
    target = {bboxes, scores, centers, heatCenters, bboxes3d, rotation, nuscenes_att, velocity}.

    `ann`: pack_annotations' tables; `trans_out` (B,2,3) float64, source image -> output map; `calib` (B,3,4) fp32; `pc_dep`
    (B,3,h,w) fp32 on the device, required with DATASET.RADAR_PC (never written: without MODEL.FRUSTUM pc_hm is a normalised copy);
    `scale_factor`: a scalar or (B).  Tables, `trans_out`, `calib` and `scale_factor` may live on the host when `device` names the
    GPU: they are uploaded.  Everything is enqueued on the current stream with no host synchronisation; with device-resident inputs
    the call can be captured in a HIP graph.  Tensors that end up on the CPU raise CfHipError: there is no CPU path."""
    (h, w), rep = _check_config(config)
    heads = set(config.heads)
    radar = bool(_get(config.DATASET, "RADAR_PC", False))
    frustum = _frustum(config)
    if radar and pc_dep is None:
        raise ValueError("build_targets: DATASET.RADAR_PC is set, pc_dep (B,3,h,w) is required")
    B, M, C = int(ann.table.shape[0]), ann.max_objs, int(num_classes)
    if frustum and ann.device.type == "cpu":                       # (tables already on the device were checked when packed)
        it = ann.itable
        live = (torch.arange(M)[None, :] < ann.counts[:, None]) & ~((it[..., 0] > C) | (it[..., 0] <= -999))
        need = _lib.TGT_HAS_DIMENSION | _lib.TGT_HAS_ALPHA | _lib.TGT_HAS_DEPTH
        if bool((live & ((it[..., 2] & need) != need)).any()):
            raise ValueError("build_targets: the ground-truth frustum association (DATASET.RADAR_PC + MODEL.FRUSTUM) needs "
                             "dimension, alpha and depth on every annotation of a kept class")
    if device is None:
        device = pc_dep.device if torch.is_tensor(pc_dep) else ann.device
    device = torch.device(device)
    if device.type != "cuda" or (radar and pc_dep.device.type != "cuda"):
        raise _lib.CfHipError("build_targets: the targets are built on the GPU; CPU tensors have no path here "
                              "(pass device='cuda' to upload host tables)")

    def dev(t, dtype, shape, name):
        t = torch.as_tensor(t)
        if t.dtype != dtype:
            raise TypeError(f"build_targets: {name} must be {dtype}, got {t.dtype}")
        if tuple(t.shape) != shape:
            raise ValueError(f"build_targets: {name} must have shape {shape}, got {tuple(t.shape)}")
        return t.to(device, non_blocking=True).contiguous()

    table = dev(ann.table, torch.float64, (B, M, _lib.CF_TARGETS_F), "ann.table")
    itable = dev(ann.itable, torch.int32, (B, M, 3), "ann.itable")
    counts = dev(ann.counts, torch.int32, (B,), "ann.counts")
    trans = dev(trans_out, torch.float64, (B, 2, 3), "trans_out")
    calib_d = dev(calib, torch.float32, (B, 3, 4), "calib")
    scale = torch.as_tensor(scale_factor, dtype=torch.float64)
    scale = (scale.expand(B) if scale.dim() == 0 else scale).to(device, non_blocking=True).contiguous()
    if tuple(scale.shape) != (B,):
        raise ValueError(f"build_targets: scale_factor must be a scalar or have shape ({B},)")
    if radar:
        pc_dep = dev(pc_dep, torch.float32, (B, 3, h, w), "pc_dep")

    f32 = dict(dtype=torch.float32, device=device)
    new = lambda *shape, **kw: torch.empty(shape, **{**f32, **kw})      # (every element is written by the launches)
    batch = {"heatmap0": new(B, C, h, w), "classIds": new(B, M, dtype=torch.int64), "mask": new(B, M), "truncMask": new(B, M),
             "widthHeight": new(B, M, 2)}
    target = {"bboxes": new(B, M, 4), "scores": new(B, M), "centers": new(B, M, 2), "heatCenters": new(B, M, 2),
              "bboxes3d": new(B, M, 8, 3)}
    for head, n in (("reg", 2), ("dimension", 3), ("amodal_offset", 2)):            # generic_dataset.py:475-485
        if head in heads:
            batch[head] = new(B, M, n)
    if {f"depth{i if i else ''}" for i in range(5)} & heads:
        batch["depth"] = new(B, M, 1)
    if {f"rotation{i if i else ''}" for i in range(5)} & heads:
        batch["rotbin"], batch["rotres"] = new(B, M, 2, dtype=torch.int64), new(B, M, 2)
        target["rotation"] = new(B, M, 8)
    for head, n in (("nuscenes_att", 8), ("velocity", 3)):                          # nuscenes.py:374-391
        if head in heads:
            batch[head], target[head] = new(B, M, n), new(B, M, n)
    if "nuscenes_att" in heads:
        batch["nuscenes_att_mask"] = new(B, M, 8)
    if radar and frustum:
        batch["pc_hm"] = new(B, 3, h, w)

    lib = _lib.load()
    a = _lib.TargetsArgs()
    a.ann, a.iann, a.counts, a.trans, a.calib, a.scale = (t.data_ptr() for t in (table, itable, counts, trans, calib_d, scale))
    a.pc_dep = _lib.ptr(pc_dep) if frustum else None
    a.B, a.M, a.C, a.h, a.w = B, M, C, h, w
    a.flags = ((_lib.TGT_REP3D if rep == "3d" else 0) | (_lib.TGT_NORM2D if _get(config.MODEL, "NORM_2D", False) else 0) |
               (_lib.TGT_WRITE_DEPTH if {"depth", "depth2"} & heads else 0) | (_lib.TGT_WRITE_ROT if "rotation" in heads else 0) |
               (_lib.TGT_FRUSTUM if frustum else 0))
    a.max_pc_dist = float(_get(config.DATASET, "MAX_PC_DIST", 60.0))
    for field, key in (("heat", "heatmap0"), ("cls", "classIds"), ("mask", "mask"), ("trunc_mask", "truncMask"),
                       ("wh", "widthHeight"), ("reg", "reg"), ("amodal_offset", "amodal_offset"), ("dimension", "dimension"),
                       ("depth", "depth"), ("rotbin", "rotbin"), ("rotres", "rotres"), ("att", "nuscenes_att"),
                       ("att_mask", "nuscenes_att_mask"), ("velocity", "velocity")):
        setattr(a, field, _lib.ptr(batch.get(key)))
    a.pc_hm = _lib.ptr(batch.get("pc_hm")) if frustum else None
    for field, key in (("t_bboxes", "bboxes"), ("t_scores", "scores"), ("t_centers", "centers"), ("t_heat_centers", "heatCenters"),
                       ("t_bboxes3d", "bboxes3d"), ("t_rotation", "rotation"), ("t_att", "nuscenes_att"), ("t_velocity", "velocity")):
        setattr(a, field, _lib.ptr(target.get(key)))
    ws_bytes = lib.cf_targets_workspace_bytes(B, M)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=device)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws_bytes
    with torch.cuda.device(device):
        _lib.check(lib.cf_targets_build(ctypes.byref(a), _lib.stream_ptr()), "cf_targets_build")
        if radar and not frustum:
            # generic_dataset.py:229-238: a copy of pc_dep whose channel 0 is 1 - x / MAX_PC_DIST; the caller's map is not touched
            pc_hm = pc_dep.clone()
            _lib.check(lib.cf_pc_hm_direct(pc_hm.data_ptr(), B, h, w, a.max_pc_dist, None, None, _lib.stream_ptr()),
                       "cf_pc_hm_direct")
            batch["pc_hm"] = pc_hm
    batch["calib"] = calib_d
    if radar:
        batch["pc_dep"] = pc_dep
    batch["target"] = target
    return batch
