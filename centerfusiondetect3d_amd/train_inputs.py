"""Training inputs on the device: what the reference dataset's `__getitem__` does to the IMAGE of a training item
(dataset/generic_dataset.py:141-190, 326-439, utils/image.py:112-142), for B frames at once (cf_augment_images,
csrc/cf_augment.hip; semantics: include/cf_hip.h).

    params = draw_augmentation(config, B, (Hs, Ws), rng, generator)            # host: the random draws and both matrices
    images = augment_images(frames, params, config.MODEL.INPUT_SIZE)           # (B,3,inH,inW) fp32, on the GPU
    pc_dep = radar_to_pc_dep(sweeps, K, (Ws, Hs), calib, params.trans_out, out_hw, flip=params.flip)
    ann = pack_annotations([flip_annotations(a, f, Ws, config) for a, f in zip(anns, params.flip.tolist())])
    batch = build_targets(ann, params.trans_out, calib, config, pc_dep=pc_dep, scale_factor=params.scale_factor)

so a training step needs only the raw bytes, the raw radar sweeps and the annotation tables from the host.  The warp is
preProcessImages' (OpenCV's fixed point), with the frame's own matrix and, for a flipped frame, of the mirrored source; the
colour chain is torchvision's ToTensor -> RandomOrder(ColorJitter brightness / contrast / saturation) -> lightingAug ->
Normalize in fp32.  tests/train_inputs_ref.py states it on the CPU; the device result equals it bit for bit.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .pointcloud import getAffineTransform
from .preprocess import NUSCENES_MEAN, NUSCENES_STD, invert_affine
from .targets import _get

BRIGHTNESS, CONTRAST, SATURATION = 0, 1, 2       # values of `order`: the positions in the reference's ColorJitter list
JITTER = 0.4                                     # ColorJitter(x=0.4): the factor is uniform in [1 - 0.4, 1 + 0.4]
# utils/image.py:122-133
_EIG_VAL = (0.2141788, 0.01817699, 0.00341571)
_EIG_VEC = ((-0.58752847, -0.69563484, 0.41340352), (-0.5832747, 0.00994535, -0.81221408), (-0.56089297, 0.71832671, 0.41158938))


class AugmentParams:
    """The augmentation of B frames: `center` (B,2) f32, `scale` (B,2) f64 (the scale handed to getAffineTransform, the factor
    included; both columns equal with DATASET.MAX_CROP), `scale_factor` (B) f64, `rotate` (B) f64 degrees, `flip` (B) bool,
    `order` (B,3) i32 (a permutation of BRIGHTNESS, CONTRAST, SATURATION), `factor` (B,3) f32 indexed by the operation,
    `lighting` (B,3) f32 (added to the channels), `trans_in` / `trans_out` (B,2,3) f64: source image -> network input / output
    map.  Validated on the host when built.  `to(device)` gives a copy on the device; a copy whose contents are overwritten in
    place (`copy_`) feeds a captured `augment_images` with new parameters."""

    FIELDS = (("center", torch.float32, (2,)), ("scale", torch.float64, (2,)), ("scale_factor", torch.float64, ()),
              ("rotate", torch.float64, ()), ("flip", torch.bool, ()), ("order", torch.int32, (3,)), ("factor", torch.float32, (3,)),
              ("lighting", torch.float32, (3,)), ("trans_in", torch.float64, (2, 3)), ("trans_out", torch.float64, (2, 3)))

    def __init__(self, center, scale, scale_factor, rotate, flip, order, factor, lighting, trans_in, trans_out):
        given = dict(center=center, scale=scale, scale_factor=scale_factor, rotate=rotate, flip=flip, order=order, factor=factor,
                     lighting=lighting, trans_in=trans_in, trans_out=trans_out)
        B = None
        for name, dtype, tail in self.FIELDS:
            t = given[name]
            t = t if torch.is_tensor(t) else torch.as_tensor(np.asarray(t))
            t = t.to(dtype)
            if B is None:
                B = int(t.shape[0]) if t.dim() else 1
            if tuple(t.shape) != (B, *tail):
                raise ValueError(f"AugmentParams: {name} must have shape {(B, *tail)}, got {tuple(t.shape)}")
            setattr(self, name, t.contiguous())
        self._validate()
        # the (B,6) dst -> src maps cf_augment_images reads: cv::warpAffine's inversion of trans_in, on the host
        self.map_in = torch.from_numpy(np.stack([invert_affine(m) for m in self.trans_in.cpu().numpy()], 0)).to(self.trans_in.device)

    def _validate(self):
        order = self.order.cpu().numpy()
        if not (np.sort(order, axis=1) == np.arange(3)).all():
            raise ValueError(f"AugmentParams: every row of order must be a permutation of 0, 1, 2, got {order.tolist()}")
        factor = self.factor.cpu().numpy()
        if not (np.isfinite(factor).all() and (factor >= 0).all()):
            raise ValueError("AugmentParams: the colour factors must be finite and >= 0")
        if not np.isfinite(self.lighting.cpu().numpy()).all():
            raise ValueError("AugmentParams: lighting must be finite")
        for name in ("trans_in", "trans_out"):
            m = getattr(self, name).cpu().numpy()
            det = m[:, 0, 0] * m[:, 1, 1] - m[:, 0, 1] * m[:, 1, 0]
            if not (np.isfinite(m).all() and (det != 0).all()):
                raise ValueError(f"AugmentParams: {name} holds a matrix that is not invertible")

    @property
    def B(self):
        return int(self.flip.shape[0])

    @property
    def device(self):
        return self.flip.device

    def _names(self):
        return [f[0] for f in self.FIELDS] + ["map_in"]

    def to(self, device, non_blocking=False):
        new = object.__new__(AugmentParams)
        for name in self._names():
            setattr(new, name, getattr(self, name).to(device, non_blocking=non_blocking))
        return new

    def copy_(self, other):
        for name in self._names():
            getattr(self, name).copy_(getattr(other, name), non_blocking=True)
        return self


def _border(border, size):
    """generic_dataset.py:310-324"""
    i = 1
    while size - border // i <= border // i:
        i *= 2
    return border // i


def draw_augmentation(config, B, src_hw, rng, generator=None, train=True):
    """Host only: the random part of B training items and both affine matrices -> AugmentParams (on the host).

    `rng` (a numpy RandomState) is consumed per frame in the reference's order, so with the same state the draws, the centre,
    the scale and the matrices are the reference's own (generic_dataset.py:141-166, 326-372; utils/image.py:135-140):
      1. getAugmentParam: with DATASET.RANDOM_CROP choice(arange(0.6, 1.4, 0.1)) and two randint for the centre, otherwise the
         clipped randn for DATASET.SCALE and two for DATASET.SHIFT, added in place to the float32 centre (DATASET.MAX_CROP: the
         scale is max(H, W), otherwise the float32 pair (W, H));
      2. random() against DATASET.ROTATE, and a clipped randn when it falls below;
      3. random() against DATASET.FLIP;
      4. three normal() for the lighting: 0.1 * alpha, then torch.mm(eig_vec, eig_val * alpha) on the CPU as lightingAug
         evaluates it (the kernel only adds the three numbers).
    `order` (a random permutation) and `factor` (uniform in [0.6, 1.4]) come from the torch `generator`.  The reference draws
    them inside torchvision, from Python's `random` (RandomOrder) and torch's global stream (ColorJitter): this part has the
    same distribution but NOT the same stream.  `train=False` (a split without "train" upstream): identity parameters - no flip,
    no rotation, scale factor 1, factors 1, lighting 0, nothing drawn."""
    Hs, Ws = int(src_hw[0]), int(src_hw[1])
    ds = config.DATASET
    inH, inW = (int(v) for v in config.MODEL.INPUT_SIZE)
    outH, outW = (int(v) for v in config.MODEL.OUTPUT_SIZE)
    eig_val = torch.tensor(_EIG_VAL).unsqueeze(1)
    eig_vec = torch.tensor(_EIG_VEC)
    out = {k: [] for k in ("center", "scale", "scale_factor", "rotate", "flip", "order", "factor", "lighting", "trans_in",
                           "trans_out")}
    for _ in range(int(B)):
        center = np.array([Ws / 2.0, Hs / 2.0], dtype=np.float32)
        scale = max(Hs, Ws) * 1.0 if _get(ds, "MAX_CROP", True) else np.array([Ws, Hs], dtype=np.float32)
        scale_factor, rotate, flip = 1, 0, False
        lighting = torch.zeros(3)
        if train:
            if _get(ds, "RANDOM_CROP", False):
                scale_factor = rng.choice(np.arange(0.6, 1.4, 0.1))
                w_border, h_border = _border(128, Ws), _border(128, Hs)
                center[0] = rng.randint(low=w_border, high=Ws - w_border)
                center[1] = rng.randint(low=h_border, high=Hs - h_border)
            else:
                if not np.isscalar(scale):
                    raise ValueError("draw_augmentation: the SCALE / SHIFT branch adds scale * shift to one coordinate of the "
                                     "centre and needs the scalar scale of DATASET.MAX_CROP (the reference fails here as well)")
                sf, shift = _get(ds, "SCALE", 0), _get(ds, "SHIFT", 0.2)
                scale_factor = np.clip(rng.randn() * sf + 1, 1 - sf, 1 + sf)
                center[0] += scale * np.clip(rng.randn() * shift, -2 * shift, 2 * shift)
                center[1] += scale * np.clip(rng.randn() * shift, -2 * shift, 2 * shift)
            rot = _get(ds, "ROTATE", 0)
            if rng.random_sample() < rot:
                rotate = np.clip(rng.randn() * rot, -rot * 2, rot * 2)
            scale *= scale_factor
            flip = bool(rng.random_sample() < _get(ds, "FLIP", 0.5))
            alpha = torch.empty((3, 1), dtype=torch.float32)
            for i in range(3):
                alpha[i] = rng.normal()
            alpha *= 0.1
            lighting = torch.mm(eig_vec, eig_val * alpha).reshape(3)
            order = torch.randperm(3, generator=generator).to(torch.int32)
            factor = (torch.rand(3, generator=generator, dtype=torch.float64) * (2 * JITTER) + (1 - JITTER)).to(torch.float32)
        else:
            order, factor = torch.arange(3, dtype=torch.int32), torch.ones(3)
        out["center"].append(torch.from_numpy(center.copy()))
        out["scale"].append(torch.from_numpy(np.broadcast_to(np.asarray(scale, np.float64), (2,)).copy()))
        out["scale_factor"].append(float(scale_factor))
        out["rotate"].append(float(rotate))
        out["flip"].append(flip)
        out["order"].append(order)
        out["factor"].append(factor)
        out["lighting"].append(lighting)
        out["trans_in"].append(torch.from_numpy(getAffineTransform(center, scale, rotate, [inW, inH])))
        out["trans_out"].append(torch.from_numpy(getAffineTransform(center, scale, rotate, [outW, outH])))
    stack = lambda v: torch.stack(v, 0) if torch.is_tensor(v[0]) else torch.from_numpy(np.asarray(v))
    return AugmentParams(**{k: stack(v) for k, v in out.items()})


def flip_annotations(anns, flip, width, config):
    """Host: `flipAnnotations` (generic_dataset.py:374-412) on one image's annotation dicts, before `pack_annotations`.  With
    `flip` false the list is returned as it is; otherwise the dicts are updated IN PLACE, as the reference does: the box
    [width - x - 1 - w, y, w, h]; `alpha` mirrored only with a `rotation` head; the amodal centre's x only with an
    `amodal_offset` head.  Velocities are never touched: the reference's caller passes
    `getattr(img_info, "velocity_trans_matrix", None)` on a dict, which is always None, so its velocity branch never runs."""
    if not flip:
        return anns
    heads = config.heads
    for ann in anns:
        bbox = ann["bbox"]
        ann["bbox"] = [width - bbox[0] - 1 - bbox[2], bbox[1], bbox[2], bbox[3]]
        if "rotation" in heads and "alpha" in ann:
            ann["alpha"] = np.pi - ann["alpha"] if ann["alpha"] > 0 else -np.pi - ann["alpha"]
        if "amodal_offset" in heads and "amodal_center" in ann:
            ann["amodal_center"][0] = width - ann["amodal_center"][0] - 1
    return anns


def augment_images(frames, params, input_size, colour=True, mean=NUSCENES_MEAN, std=NUSCENES_STD, out=None, device=None):
    """frames: as preProcessImages takes them - a list of (H, W, 3) uint8 ndarrays / tensors of one size, or a (B, H, W, 3) uint8
    tensor (host or device), channels as stored (BGR from cv2.imread; nothing is reordered).  params: AugmentParams (host or
    device; uploaded when on the host).  -> (B, 3, inH, inW) fp32 on the device.  `colour=False` is the dataset's path without
    DATASET.COLOR_AUG: warp (and flip), / 255, Normalize, in fp32.  Enqueued on the current stream, no host synchronisation;
    with device-resident inputs and `out` the call can be captured in a HIP graph (the workspace is a torch allocation).
    A CPU target raises CfHipError: there is no CPU path."""
    if isinstance(frames, (list, tuple)):
        frames = torch.stack([torch.as_tensor(np.ascontiguousarray(f) if isinstance(f, np.ndarray) else f) for f in frames], 0)
    else:
        frames = torch.as_tensor(frames)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError(f"frames must be (B, H, W, 3) uint8, got {tuple(frames.shape)} {frames.dtype}")
    if not isinstance(params, AugmentParams):
        raise TypeError("augment_images: params must be an AugmentParams")
    if device is None:
        device = frames.device if frames.is_cuda else (params.device if params.device.type == "cuda" else
                                                       torch.device("cuda", torch.cuda.current_device()))
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.CfHipError("augment_images runs on the GPU: the HIP path has no CPU fallback")
    B, Hs, Ws, _ = frames.shape
    if params.B != B:
        raise ValueError(f"augment_images: {B} frames but parameters for {params.B}")
    inH, inW = int(input_size[0]), int(input_size[1])
    frames = frames.to(device, non_blocking=True).contiguous()
    p = params if params.device == device else params.to(device, non_blocking=True)
    mean_c = (C.c_float * 3)(*np.asarray(mean, np.float32).reshape(3).tolist())
    std_c = (C.c_float * 3)(*np.asarray(std, np.float32).reshape(3).tolist())
    if out is None:
        out = torch.empty((B, 3, inH, inW), device=device, dtype=torch.float32)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B, 3, inH, inW) or out.device != device or not out.is_contiguous():
        raise ValueError(f"augment_images: out must be a contiguous ({B}, 3, {inH}, {inW}) float32 tensor on {device}")
    lib = _lib.load()
    ws_bytes = lib.cf_augment_workspace_bytes(B, inH, inW) if colour else 0
    ws = torch.empty(ws_bytes // 8 + 1, dtype=torch.float64, device=device) if colour else None
    with torch.cuda.device(device):
        _lib.check(lib.cf_augment_images(frames.data_ptr(), B, Hs, Ws, p.map_in.data_ptr(), p.flip.data_ptr(), p.order.data_ptr(),
                                         p.factor.data_ptr(), p.lighting.data_ptr(), mean_c, std_c, int(bool(colour)), inH, inW,
                                         out.data_ptr(), _lib.ptr(ws), ws_bytes, _lib.stream_ptr()), "cf_augment_images")
    return out
