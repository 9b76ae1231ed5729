"""GPU: the training inputs on the device (centerfusiondetect3d_amd.train_inputs, cf_augment_images; radar_to_pc_dep(flip=...)).

Image parity is BIT equality with tests/train_inputs_ref.py (the numpy flip, oracle.preprocess_ref.warp_affine_u8 and the
torchvision chain in torch-CPU fp32) on the calls of tests/train_inputs_cases.py.  Every operation of the chain is one IEEE fp32
operation on both sides; the only quantity computed differently is the contrast mean, a float64 sum whose order differs.  A
float64 sum of n <= 22400 terms in [0, 1] carries a relative error below n * 2^-53 < 2^-38.5 in the worst case and around
sqrt(n) * 2^-53 ~ 2^-45.8 in practice; `_margins` below asserts that every reference mean of the committed seeds lies at least
2^-40 (relative) from an fp32 rounding boundary, so both sums round to the same fp32."""
import os

import numpy as np
import pytest
import torch

from tests import train_inputs_cases as cases
from tests import train_inputs_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X box"
    from centerfusiondetect3d_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "train_inputs.npz")))


@pytest.fixture(scope="module")
def _margins():
    """the premise of bit equality, checked on the CPU for the committed seeds"""
    for name in cases.NAMES:
        for _, means in cases.reference(name):
            for m in means:
                assert ref.mean_margin(m) >= cases.MARGIN, (name, m)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def run(dev, frames, p, in_hw, colour=True, **kw):
    from centerfusiondetect3d_amd import augment_images
    return augment_images(torch.from_numpy(frames).to(dev), p, in_hw, colour=colour, **kw)


@pytest.mark.parametrize("name", cases.NAMES)
def test_images_equal_the_cpu_reference_bit_for_bit(dev, _margins, name):
    for i, ((frames, p, in_hw, colour), (want, _)) in enumerate(zip(cases.calls(name), cases.reference(name))):
        got = run(dev, frames, p, in_hw, colour).cpu().numpy()
        assert got.shape == want.shape and got.dtype == np.float32
        diff = bits(got) != bits(want)
        print(f"{name}[{i}] colour={colour}: {int(diff.sum())} of {diff.size} words differ, "
              f"max |d| = {float(np.abs(got.astype(np.float64) - want).max()):.3g}")
        assert not diff.any(), (name, i, int(diff.sum()), np.argwhere(diff)[:5].tolist())


def test_frame_alone_equals_its_slot_in_a_batch_and_runs_repeat(dev, _margins):
    (fc, pc, in_hw, _), = cases.calls("c")
    want = cases.reference("c")[0][0]
    alone = run(dev, fc, pc, in_hw)
    frames, p, _ = cases.batch_of_five()
    pd = p.to(dev)                                                     # device-resident parameters
    batch = run(dev, frames, pd, in_hw)
    again = run(dev, frames, pd, in_hw, out=torch.full_like(batch, float("nan")))
    assert torch.equal(batch[3], alone[0])
    assert torch.equal(batch.view(torch.int32), again.view(torch.int32))
    assert np.array_equal(bits(batch[3].cpu().numpy()), bits(want[0]))
    assert not torch.equal(batch[2], batch[3]) and bool(torch.isfinite(batch).all())


def test_identity_parameters_give_preprocess_images_bytes(dev):
    from centerfusiondetect3d_amd import config as cfgmod, draw_augmentation, preProcessImages
    from centerfusiondetect3d_amd.preprocess import NUSCENES_MEAN, NUSCENES_STD
    frames = torch.from_numpy(cases.frames_for(46, 2, 90, 160)).to(dev)
    cfg = cfgmod.centerfusion_middle_config((44, 80))
    p = draw_augmentation(cfg, 2, (90, 160), np.random.RandomState(0), train=False)
    from centerfusiondetect3d_amd import augment_images
    a = augment_images(frames, p, (44, 80), colour=False)
    b = preProcessImages(frames, (44, 80))
    mean = torch.from_numpy(NUSCENES_MEAN).to(dev).reshape(1, 3, 1, 1)
    std = torch.from_numpy(NUSCENES_STD).to(dev).reshape(1, 3, 1, 1)
    to_bytes = lambda t: torch.round((t * std + mean) * 255).to(torch.int32)
    ba, bb = to_bytes(a), to_bytes(b)
    assert torch.equal(ba, bb) and int(ba.min()) >= 0 and int(ba.max()) <= 255 and ba.unique().numel() > 100
    assert float((a - b).abs().max()) < 1e-6                           # fp32 chain against the detector's float64 one


def test_radar_flip_equals_the_reference(dev, golden):
    from centerfusiondetect3d_amd import radar_to_pc_dep
    n = 4
    g = lambda i, k: golden[f"radar/{i}/{k}"]
    raws = [g(i, "in_radar_pc") for i in range(n)]
    calib = np.stack([g(i, "in_calib") for i in range(n)])
    trans = np.stack([g(i, "in_trans_out") for i in range(n)])
    flip = np.array([bool(g(i, "in_flip")) for i in range(n)])
    assert flip.any() and not flip.all()
    img_wh = tuple(int(v) for v in golden["radar/in_img_wh"])
    out_hw = tuple(int(v) for v in golden["radar/in_out_hw"])
    args = (raws, calib[:, :, :3], img_wh, calib, trans, out_hw)
    pc_dep = radar_to_pc_dep(*args, device=dev, flip=torch.from_numpy(flip))
    for i in range(n):
        assert np.array_equal(pc_dep[i].cpu().numpy(), g(i, "out_pc_dep")), i
    # the flipped point lists themselves: the reference keeps the points that also survive the output-map keep mask, in order
    from centerfusiondetect3d_amd import ops
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    for i in np.flatnonzero(flip):
        raw = raws[i]
        p2, p3, cnt = ops.radar_ingest(t(raw[None]), t(np.array([raw.shape[1]], np.int32)), t(calib[i:i + 1, :, :3].copy()), img_wh, 60.0, 0.0, False)
        m = int(cnt[0])
        x3 = p3[0, :, :m].cpu().numpy() * np.where(np.isin(np.arange(18), (0, 8)), -1.0, 1.0)[:, None]
        ref3, j = g(i, "out_pc_3d"), 0
        for k in range(m):                                              # (the reference's pc_2d is in output-map pixels: pc_dep holds it)
            if j < ref3.shape[1] and np.array_equal(x3[:, k], ref3[:, j]):
                j += 1
        assert j == ref3.shape[1] == int(g(i, "out_pc_n")) and (ref3[0] != 0).any() and (ref3[8] != 0).any()
    # flip=None is today's path: the same call without the argument, and an all-false mask
    plain = radar_to_pc_dep(*args, device=dev)
    none = radar_to_pc_dep(*args, device=dev, flip=None)
    off = radar_to_pc_dep(*args, device=dev, flip=np.zeros(n, bool))
    assert torch.equal(plain, none) and torch.equal(plain, off)
    for i in np.flatnonzero(~flip):
        assert torch.equal(plain[i], pc_dep[i])
    for i in np.flatnonzero(flip):
        assert not torch.equal(plain[i], pc_dep[i])
    # a device-resident (B,2,3) matrix tensor, as AugmentParams.to(device) holds it
    assert torch.equal(radar_to_pc_dep(raws, calib[:, :, :3], img_wh, calib, t(trans), out_hw, device=dev, flip=t(flip)), pc_dep)


def test_end_to_end_training_step_from_raw_inputs(dev):
    """augment_images -> radar_to_pc_dep(flip) -> flip_annotations / build_targets -> model.train() forward -> GenericLoss ->
    backward at a 64 x 96 input, on the frozen-backbone model of tests/test_gpu_targets.py"""
    from centerfusiondetect3d_amd import (GenericLoss, augment_images, build_targets, config as cfgmod, draw_augmentation,
                                          flip_annotations, getModel, pack_annotations, radar_to_pc_dep)
    from tests import targets_cases as tc
    from tests.golden import cases_dataset as cd
    torch.manual_seed(12)
    cfg = cfgmod.centerfusion_middle_config((64, 96))
    cfg.MODEL.FREEZE_BACKBONE = True
    cfg.DATASET.ROTATE, cfg.DATASET.SCALE, cfg.DATASET.SHIFT, cfg.DATASET.FLIP = 0.5, 0.2, 0.05, 0.5
    cfgmod.update_loss_weights(cfg)
    B, Hs, Ws = 2, 150, 225
    p = draw_augmentation(cfg, B, (Hs, Ws), np.random.RandomState(8), torch.Generator().manual_seed(5))
    assert p.flip.tolist() == [True, False]                              # (the seed gives one of each)
    images = augment_images(cases.frames_for(47, B, Hs, Ws), p, cfg.MODEL.INPUT_SIZE, device=dev)
    assert tuple(images.shape) == (B, 3, 64, 96) and bool(torch.isfinite(images).all())
    radar = dict(cd.radar_cases())
    calib = np.repeat(radar["n150"]["calib"][None], B, 0).astype(np.float64)
    calib[:, :2] *= Ws / 1600.0                                          # the 1600-wide intrinsics on a 225-wide frame
    raws = [radar["n150"]["radar_pc"], radar["n300_zoff"]["radar_pc"]]
    pc_dep = radar_to_pc_dep(raws, calib[:, :, :3], (Ws, Hs), calib, p.trans_out, (16, 24), device=dev, flip=p.flip)
    assert int((pc_dep[:, 0] != 0).sum()) > 0
    rs = np.random.RandomState(22)
    anns = []
    for b in range(B):
        T = p.trans_out[b].numpy()
        image = tc._random_image(rs, tc.matrix(24, src_w=float(Ws)), 16, 24, 4)
        for a in image:
            a["depth"] = float(rs.uniform(10.0, 38.0))
        anns.append(flip_annotations(image, bool(p.flip[b]), Ws, cfg))
    ann = pack_annotations(anns, max_objs=16, config=cfg)
    calib32 = torch.from_numpy(calib.astype(np.float32))
    batch = build_targets(ann, p.trans_out, calib32, cfg, pc_dep=pc_dep, scale_factor=p.scale_factor, device=dev)
    m = getModel(cfg).to(dev).train()
    y = m(images, pc_hm=batch["pc_hm"], pc_dep=pc_dep, calib=batch["calib"])
    total, _ = GenericLoss(cfg, int(cfg.DATASET.NUM_CLASSES)).train()(y, batch)
    total.backward()
    assert bool(torch.isfinite(total))
    grads = [q.grad for n, q in m.named_parameters() if n.startswith("detectHead_0.")]
    assert grads and all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    assert any(float(g.abs().max()) > 0 for g in grads)


def test_bad_arguments_are_refused(dev):
    from centerfusiondetect3d_amd import _lib, augment_images
    (fr, p, in_hw, _), = cases.calls("c")
    frames = torch.from_numpy(fr).to(dev)
    with pytest.raises(ValueError, match="uint8"):
        augment_images(frames.float(), p, in_hw)
    with pytest.raises(ValueError, match="uint8"):
        augment_images(frames[0], p, in_hw)
    with pytest.raises(ValueError, match="uint8"):
        augment_images(frames[..., :2], p, in_hw)
    with pytest.raises(ValueError, match="parameters for 1"):
        augment_images(torch.cat([frames, frames]), p, in_hw)
    with pytest.raises(TypeError):
        augment_images(frames, {"flip": p.flip}, in_hw)
    with pytest.raises(ValueError, match="out must be"):
        augment_images(frames, p, in_hw, out=torch.empty((1, 3, 112, 200), dtype=torch.float64, device=dev))
    with pytest.raises(_lib.CfHipError, match=r"std\[2\] is zero"):
        augment_images(frames, p, in_hw, std=(0.3, 0.3, 0.0))
    with pytest.raises(_lib.CfHipError, match="no CPU fallback"):
        augment_images(frames, p, in_hw, device="cpu")
    with pytest.raises(ValueError, match="flip must have shape"):
        from centerfusiondetect3d_amd import radar_to_pc_dep
        radar_to_pc_dep([np.zeros((18, 3))], np.eye(3), (1600, 900), np.zeros((1, 3, 4)), np.eye(3)[:2], (112, 200), device=dev,
                        flip=np.zeros(2, bool))
