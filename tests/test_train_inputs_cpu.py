"""CPU: the host side of the training inputs (centerfusiondetect3d_amd.train_inputs, getAffineTransform with a rotation) against
tests/golden/train_inputs.npz - what the reference's own getAugmentParam, flip draw, getAffineTransform, lightingAug and
flipAnnotations returned under np.random.seed (tests/golden/make_golden_train_inputs.py) - and the properties the GPU parity test
(tests/test_gpu_train_inputs.py) rests on: its cases bind the clamps and the border, and every contrast mean of the reference
lies far enough from an fp32 rounding boundary for a float64 sum in another order to round alike."""
import copy
import ctypes as C
import glob
import os

import numpy as np
import pytest
import torch

from tests import train_inputs_cases as cases
from tests import train_inputs_ref as ref
from tests.golden import make_golden_train_inputs as gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "train_inputs.npz")))


def _config(golden, name):
    from centerfusiondetect3d_amd import config as cfgmod
    inH, inW = (int(v) for v in golden[f"{name}/in_input_size"])
    cfg = cfgmod.centerfusion_middle_config((inH, inW))
    assert tuple(cfg.MODEL.OUTPUT_SIZE) == (inH // 4, inW // 4)
    for k in ("RANDOM_CROP", "MAX_CROP", "SCALE", "SHIFT", "ROTATE", "FLIP"):
        cfg.DATASET[k] = golden[f"{name}/in_{k}"].item()
    return cfg


@pytest.mark.parametrize("name", list(gen.AUGMENT_CASES))
def test_draw_augmentation_equals_the_reference_draws(golden, name):
    from centerfusiondetect3d_amd import draw_augmentation
    n = len(golden[f"{name}/out_flip"])
    rng = np.random.RandomState(int(golden[f"{name}/in_seed"]))
    p = draw_augmentation(_config(golden, name), n, tuple(golden[f"{name}/in_src_hw"]), rng, torch.Generator().manual_seed(1))
    for k in ("center", "scale", "scale_factor", "rotate", "flip", "lighting", "trans_in", "trans_out"):
        got, want = getattr(p, k).numpy(), golden[f"{name}/out_{k}"]
        assert got.dtype == want.dtype and np.array_equal(got, want), k
    # the part with its own stream: permutations, factors in [0.6, 1.4], and the same generator state gives the same draw
    assert (np.sort(p.order.numpy(), 1) == np.arange(3)).all()
    assert float(p.factor.min()) >= 0.6 and float(p.factor.max()) <= 1.4 and p.factor.unique().numel() > n
    q = draw_augmentation(_config(golden, name), n, tuple(golden[f"{name}/in_src_hw"]),
                          np.random.RandomState(int(golden[f"{name}/in_seed"])), torch.Generator().manual_seed(1))
    assert torch.equal(p.order, q.order) and torch.equal(p.factor, q.factor) and torch.equal(p.map_in, q.map_in)


def test_draw_augmentation_eval_is_the_identity(golden):
    from centerfusiondetect3d_amd import draw_augmentation, getAffineTransform
    cfg = _config(golden, "shift_scale_rotate")
    rng = np.random.RandomState(3)
    state = rng.get_state()[1].copy()
    p = draw_augmentation(cfg, 2, (900, 1600), rng, train=False)
    assert np.array_equal(rng.get_state()[1], state)                                   # nothing drawn
    assert not p.flip.any() and not p.rotate.any() and (p.scale_factor == 1).all() and (p.factor == 1).all() and not p.lighting.any()
    want = getAffineTransform(np.array([800, 450], np.float32), 1600.0, 0, [800, 448])
    assert np.array_equal(p.trans_in[1].numpy(), want)


def test_get_affine_transform_with_rotation_and_pair_scale(golden):
    from centerfusiondetect3d_amd import getAffineTransform
    seen_rot = seen_pair = 0
    for name, (_, n, _, (inH, inW), over) in gen.AUGMENT_CASES.items():
        for i in range(n):
            center, scale, rot = golden[f"{name}/out_center"][i], golden[f"{name}/out_scale"][i], float(golden[f"{name}/out_rotate"][i])
            # what the reference hands over: a float64 scalar with MAX_CROP, the float32 pair (W, H) * factor without
            for arg in [scale[0] if over["MAX_CROP"] else scale.astype(np.float32)]:
                for key, wh in (("trans_in", [inW, inH]), ("trans_out", [inW // 4, inH // 4])):
                    assert np.array_equal(getAffineTransform(center, arg, rot, wh), golden[f"{name}/out_{key}"][i]), (name, i, key)
            seen_rot += rot != 0
            seen_pair += not over["MAX_CROP"]
    assert seen_rot >= 10 and seen_pair >= 8


def test_get_affine_transform_unchanged_at_rotation_zero():
    """the matrices the reference made for the inference fixtures committed earlier (rotation 0, scalar scale)"""
    from centerfusiondetect3d_amd import getAffineTransform
    paths = sorted(glob.glob(os.path.join(GOLDEN, "pillar_*.npz")))
    assert len(paths) >= 8
    for path in paths:
        g = np.load(path)
        H, W = (int(v) for v in g["in_out_hw"])
        assert np.array_equal(getAffineTransform(g["in_center"], float(g["in_scale"]), 0, [W, H]), g["in_trans_out"]), path


@pytest.mark.parametrize("heads", ["allheads", "fewheads"])
def test_flip_annotations_equals_the_reference(golden, heads):
    from centerfusiondetect3d_amd import config as cfgmod, flip_annotations
    cfg = cfgmod.centerfusion_middle_config((448, 800))
    assert "rotation" in cfg.heads and "amodal_offset" in cfg.heads
    if heads == "fewheads":
        cfg.heads = {k: v for k, v in cfg.heads.items() if k not in ("rotation", "amodal_offset")}
    anns = gen.annotation_case()
    assert all(np.array_equal(v, golden[f"anns/in_{k}"], equal_nan=True) for k, v in gen.ann_arrays(anns, "").items())
    same = flip_annotations(copy.deepcopy(anns), False, 1600, cfg)
    assert same == anns
    got = gen.ann_arrays(flip_annotations(copy.deepcopy(anns), True, int(golden["anns/in_width"]), cfg), "")
    for k, v in got.items():
        assert np.array_equal(v, golden[f"anns/out_{heads}_{k}"], equal_nan=True), k
    assert np.array_equal(got["velocity"], golden["anns/in_velocity"])                 # never touched, as upstream
    assert not np.array_equal(got["bbox"], golden["anns/in_bbox"])


def test_augment_params_refuses_bad_tables():
    from centerfusiondetect3d_amd import AugmentParams
    (_, p, _, _), = cases.calls("c")
    good = {name: getattr(p, name).clone() for name, _, _ in AugmentParams.FIELDS}
    assert torch.equal(AugmentParams(**good).map_in, p.map_in)

    def bad(**kw):
        return {**good, **kw}

    with pytest.raises(ValueError, match="permutation"):
        AugmentParams(**bad(order=torch.tensor([[0, 1, 1]])))
    with pytest.raises(ValueError, match="permutation"):
        AugmentParams(**bad(order=torch.tensor([[1, 2, 3]])))
    for f in ([1.0, -0.1, 1.0], [1.0, float("nan"), 1.0], [float("inf"), 1.0, 1.0]):
        with pytest.raises(ValueError, match="factors"):
            AugmentParams(**bad(factor=torch.tensor([f])))
    singular = torch.tensor([[[1.0, 2.0, 3.0], [2.0, 4.0, 5.0]]], dtype=torch.float64)
    for name in ("trans_in", "trans_out"):
        with pytest.raises(ValueError, match="invertible"):
            AugmentParams(**bad(**{name: singular}))
    with pytest.raises(ValueError, match="shape"):
        AugmentParams(**bad(lighting=torch.zeros(2, 3)))
    # to / copy_ carry every field
    q = p.to("cpu")
    q.copy_(AugmentParams(**bad(lighting=torch.ones(1, 3))))
    assert torch.equal(q.lighting, torch.ones(1, 3)) and torch.equal(q.map_in, p.map_in)


def test_augment_images_has_no_cpu_path():
    from centerfusiondetect3d_amd import _lib, augment_images
    (fr, p, in_hw, _), = cases.calls("c")
    with pytest.raises(_lib.CfHipError, match="no CPU fallback"):
        augment_images(torch.from_numpy(fr), p, in_hw, device="cpu")


def test_entry_point_refuses_bad_arguments_without_gpu():
    """cf_augment_images checks everything before its first launch: these calls never reach the device"""
    from centerfusiondetect3d_amd import _lib
    lib = _lib.load()
    f3 = C.c_float * 3
    mean, std, zero = f3(0.4, 0.4, 0.4), f3(0.3, 0.3, 0.3), f3(0.3, 0.0, 0.3)
    p = 4096                                                            # a non-null, 8-byte aligned stand-in: never dereferenced
    call = lambda B=1, Hs=8, Ws=8, Hd=8, Wd=8, std=std, colour=1, ws=p, ws_bytes=1 << 40, order=p, src=p: lib.cf_augment_images(
        src, B, Hs, Ws, p, p, order, p, p, mean, std, colour, Hd, Wd, p, ws, ws_bytes, None)
    err = lambda: lib.cf_last_error()
    assert call(src=None) == -22 and b"null buffer" in err()
    assert call(order=None) == -22 and b"colour needs order" in err()
    assert call(B=0) == -22 and b"bad geometry" in err()
    for kw in (dict(Hs=32768), dict(Ws=32768), dict(Hd=32768), dict(Wd=32768)):
        assert call(**kw) == -22 and b"too large for the fixed-point map" in err()
    assert call(std=zero) == -22 and b"std[1] is zero" in err()
    assert call(ws=None) == -22 and b"workspace" in err()
    assert call(ws=p + 4) == -22 and b"aligned" in err()
    need = lib.cf_augment_workspace_bytes(2, 31, 45)
    assert need == 2 * 2 * 8 + 2 * 31 * 45 * 4                         # two 1024-pixel blocks per frame
    assert call(B=2, Hd=31, Wd=45, ws_bytes=need - 1) == -22 and b"needed" in err()
    # the grid limit: B * ceil(Hd * Wd / 1024) <= 2^31 - 1
    assert call(B=4096, Hd=32767, Wd=32767, colour=0) == -22 and b"exceeds the grid limit" in err()


@pytest.mark.parametrize("name", cases.NAMES)
def test_reference_means_are_clear_of_fp32_rounding_boundaries(name):
    n = 0
    for (out, means), (frames, p, _, colour) in zip(cases.reference(name), cases.calls(name)):
        assert np.isfinite(out).all()
        assert len(means) == (len(frames) if colour else 0)
        for m in means:
            assert 0.0 < m < 1.0 and ref.mean_margin(m) >= cases.MARGIN, (name, m, ref.mean_margin(m))
            n += 1
    assert n >= 1


def test_case_b_binds_the_border_and_both_clamps():
    """what the issue asks of case (b): a third of the output outside the source, the upper clamp on about a third of the pixels
    of the bright frame, and the chain below zero before the normalisation on the other"""
    from centerfusiondetect3d_amd.preprocess import NUSCENES_MEAN, NUSCENES_STD
    orders = set()
    for (out, _), (frames, p, in_hw, _) in zip(cases.reference("b"), cases.calls("b")):
        orders |= {tuple(o) for o in p.order.tolist()}
        w0 = ref.warp_u8(frames[0], p.trans_in[0].numpy(), in_hw, False)
        outside = (w0 == 0).all(-1).mean()
        assert 0.28 <= outside <= 0.40, outside
        t = torch.from_numpy(w0.transpose(2, 0, 1).copy()).to(torch.float32).div(255)
        for k in p.order[0].tolist():                                   # the chain up to the brightness step
            f = float(p.factor[0, k])
            if k == ref.BRIGHTNESS:
                break
            t = ref.adjust_contrast(t, f) if k == ref.CONTRAST else ref.adjust_saturation(t, f)
        assert f == float(np.float32(1.4))
        above = float((f * t > 1.0).float().mean())                     # pixels on which brightness' upper clamp binds
        assert 0.2 <= above <= 0.45, above
        t1 = out[1] * NUSCENES_STD.reshape(3, 1, 1) + NUSCENES_MEAN.reshape(3, 1, 1)
        assert (t1 < 0).mean() > 0.02
    assert orders == set(cases.ORDERS)


def test_reference_colour_off_is_the_fp32_dataset_path():
    (fr, p, in_hw, _), (_, _, _, colour) = cases.calls("a")
    assert not colour
    out = cases.reference("a")[1][0]
    from centerfusiondetect3d_amd.preprocess import NUSCENES_MEAN, NUSCENES_STD
    for b in range(3):
        w = ref.warp_u8(fr[b], p.trans_in[b].numpy(), in_hw, bool(p.flip[b]))
        want = ((w.astype(np.float32) / 255.0 - NUSCENES_MEAN) / NUSCENES_STD).transpose(2, 0, 1)      # generic_dataset.py:431-436
        assert want.dtype == np.float32 and np.array_equal(out[b], want)
