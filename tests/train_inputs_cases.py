"""Seeded inputs of the training-input tests (tests/test_train_inputs_cpu.py, tests/test_gpu_train_inputs.py): frames,
augmentation parameters, and the CPU reference result of each call (tests/train_inputs_ref.py), computed once per process.

Every call is (frames (B,Hs,Ws,3) uint8, AugmentParams, (inH, inW), colour).  The shapes are the smallest at which the kernels of
csrc/cf_augment.hip can still go wrong: more than one 1024-pixel block per frame, a last block that is not full, sizes that are
no multiple of the block, the wave or four, and one frame (`c`) whose grey mean is summed over 22 blocks."""
import functools

import numpy as np
import torch

from centerfusiondetect3d_amd import AugmentParams, getAffineTransform
from centerfusiondetect3d_amd.preprocess import NUSCENES_MEAN, NUSCENES_STD
from tests import train_inputs_ref as ref

ORDERS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
MARGIN = 2.0 ** -40          # least relative distance of a reference contrast mean from an fp32 rounding boundary


def frames_for(seed, B, Hs, Ws, band=None):
    """smooth structure + noise, so that bilinear taps differ; `band`: rows (lo, hi) of every frame set to 200..255"""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:Hs, 0:Ws]
    out = []
    for b in range(B):
        base = 110 + 70 * np.sin(x / (5.0 + b) + rs.uniform(0, 3))[..., None] * np.cos(y / (7.0 + b))[..., None]
        img = base + rs.uniform(-60, 60, (Hs, Ws, 3)) + rs.uniform(-25, 25, 3)
        if band is not None:
            img[band[0]:band[1]] = rs.uniform(200, 256, (band[1] - band[0], Ws, 3))
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return np.stack(out)


def params_for(Hs, Ws, in_hw, specs):
    """specs: per frame dict(shift=(dx, dy) source pixels, sf, rotate, flip, order, factor (3), lighting (3))"""
    inH, inW = in_hw
    rows = {k: [] for k in ("center", "scale", "scale_factor", "rotate", "flip", "order", "factor", "lighting", "trans_in", "trans_out")}
    for s in specs:
        center = np.array([Ws / 2.0 + s.get("shift", (0, 0))[0], Hs / 2.0 + s.get("shift", (0, 0))[1]], np.float32)
        sf, rot = s.get("sf", 1.0), s.get("rotate", 0.0)
        scale = max(Hs, Ws) * 1.0 * sf
        rows["center"].append(center); rows["scale"].append([scale, scale]); rows["scale_factor"].append(sf)
        rows["rotate"].append(rot); rows["flip"].append(bool(s.get("flip", False))); rows["order"].append(list(s.get("order", (0, 1, 2))))
        rows["factor"].append(np.asarray(s.get("factor", (1, 1, 1)), np.float32))
        rows["lighting"].append(np.asarray(s.get("lighting", (0, 0, 0)), np.float32))
        rows["trans_in"].append(getAffineTransform(center, scale, rot, [inW, inH]))
        rows["trans_out"].append(getAffineTransform(center, scale, rot, [inW // 4, inH // 4]))
    return AugmentParams(**{k: np.asarray(v) for k, v in rows.items()})


def _spec(rs, order, **kw):
    s = dict(order=order, factor=rs.uniform(0.6, 1.4, 3), lighting=rs.standard_normal(3) * 0.03, shift=tuple(rs.uniform(-4, 4, 2)),
             sf=float(rs.uniform(0.8, 1.2)))
    s.update(kw)
    return s


@functools.lru_cache(maxsize=None)
def calls(name):
    """-> a list of (frames, params, in_hw, colour)"""
    if name == "a":                                      # B=3, 37x53 -> 24x40: mixed flips, three orders; and colour off
        rs = np.random.RandomState(401)
        fr = frames_for(41, 3, 37, 53)
        p = params_for(37, 53, (24, 40), [_spec(rs, ORDERS[1], flip=True), _spec(rs, ORDERS[3], flip=False, rotate=-4.0),
                                           _spec(rs, ORDERS[4], flip=True)])
        return [(fr, p, (24, 40), True), (fr, p, (24, 40), False)]
    if name == "b":                                      # B=2, 90x160 -> 44x80: all six orders; shift, clamps at both ends
        rs = np.random.RandomState(402)
        fr = frames_for(42, 2, 90, 160, band=(30, 62))
        out = []
        for i in range(3):
            # a third of the output lies outside the source (border zeros enter the mean); brightness 1.4 on the bright band
            # binds the upper clamp; 0.6 factors with negative lighting take the chain below 0 before the normalisation
            s0 = _spec(rs, ORDERS[2 * i], shift=(53.0, 3.0), sf=1.0, factor=(1.4, float(rs.uniform(0.6, 1.4)), float(rs.uniform(0.6, 1.4))))
            s1 = _spec(rs, ORDERS[2 * i + 1], shift=(-5.0, 30.0), sf=1.0, flip=True, factor=(0.6, 0.6, 0.6), lighting=(-0.21, -0.16, -0.18))
            out.append((fr, params_for(90, 160, (44, 80), [s0, s1]), (44, 80), True))
        return out
    if name == "c":                                      # B=1, 225x400 -> 112x200: 7 degrees with flip, 22 blocks
        rs = np.random.RandomState(403)
        fr = frames_for(43, 1, 225, 400)
        return [(fr, params_for(225, 400, (112, 200), [_spec(rs, ORDERS[5], rotate=7.0, flip=True, sf=0.9)]), (112, 200), True)]
    if name == "d":                                      # 64x96 -> 31x45: no size is a multiple of anything
        rs = np.random.RandomState(404)
        fr = frames_for(44, 2, 64, 96)
        return [(fr, params_for(64, 96, (31, 45), [_spec(rs, ORDERS[3], flip=True, rotate=2.5), _spec(rs, ORDERS[0])]), (31, 45), True)]
    raise KeyError(name)


NAMES = ("a", "b", "c", "d")


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> per call (out (B,3,inH,inW) float32, [the float64 contrast mean of each frame]); computed once, never written to"""
    res = []
    for frames, p, in_hw, colour in calls(name):
        means = []
        out = ref.augment_images(frames, p, in_hw, NUSCENES_MEAN, NUSCENES_STD, colour=colour, means=means)
        out.setflags(write=False)
        res.append((out, means))
    return res


def batch_of_five():
    """frame `c` in slot 3 of a B=5 batch of other frames and parameters"""
    (fc, pc, in_hw, _), = calls("c")
    rs = np.random.RandomState(405)
    others = frames_for(45, 5, 225, 400)
    specs = [_spec(rs, ORDERS[i], flip=bool(i & 1), rotate=float(rs.uniform(-10, 10))) for i in range(5)]
    p = params_for(225, 400, in_hw, specs)
    others[3] = fc[0]
    for name, _, _ in AugmentParams.FIELDS:
        getattr(p, name)[3] = getattr(pc, name)[0]
    p.map_in[3] = pc.map_in[0]
    return others, p, in_hw
