"""GPU: `ret["depthmaps"]` - the normalised uint8 maps of the reference's Detector.post_process (detector.py:351-393) from one
device launch (cf_depth_maps), against the bytes the reference's own method produced (tests/golden/make_golden_depthmaps.py).

Sub, div and mul in fp32, each rounded, then truncation: reproducible exactly, so every non-flat image must equal the
reference's uint8 bit for bit.  A flat image is 0 / 0 in the reference (numpy's cast of NaN is implementation-defined): here it
is DEFINED as all zeros, and only that is tested for it."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.golden import cases, cases_dataset as cd
from tests.golden.make_golden_depthmaps import FIXTURE, UNC_FIXTURE, DEPTH_KEYS

CASES = ("unc", "neg", "k255", "flat")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, FIXTURE))


def _inputs(g, golden_dir, case):
    if case == "unc":
        u = np.load(os.path.join(golden_dir, UNC_FIXTURE))
        return {k: u[f"out_{k}"] for k in ("depthMap", "pc_hm_out", "pc_hm_in")}
    pre = f"in_{case}_"
    return {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)}


def _expect(g, case, key):
    ref, flat = g[f"ref_{case}_{key}"].copy(), g[f"flat_{case}_{key}"]
    ref[flat] = 0                                                  # our definition of the 0 / 0 images
    return ref


class _Cfg:                                                        # the two fields Detector.depth_maps reads
    def __init__(self, hw):
        self.MODEL = type("M", (), {"OUTPUT_SIZE": hw})


@pytest.mark.parametrize("case", CASES)
def test_depth_maps_equal_the_reference_bytes(dev, golden, golden_dir, case):
    from centerfusiondetect3d_amd import Detector, ops
    g = golden
    maps = _inputs(g, golden_dir, case)
    out = {k: torch.from_numpy(v).to(dev) for k, v in maps.items()}
    before = {k: v.clone() for k, v in out.items()}
    B, _, H, W = next(iter(maps.values())).shape
    det = Detector.__new__(Detector)                               # (depth_maps reads config and device only: no model is built)
    det.config, det.device = _Cfg((H, W)), dev
    dm = det.depth_maps([out])
    want = ["depth"] + [k for k in ("pc_hm_out", "pc_hm_in") if k in maps]
    assert list(dm.keys()) == want
    for k in want:
        assert isinstance(dm[k], np.ndarray) and dm[k].dtype == np.uint8 and dm[k].shape == (B, H, W), k
        exp = _expect(g, case, k)
        bad = int((dm[k] != exp).sum())
        print(f"[depthmaps] {case}/{k}: {bad} of {exp.size} bytes differ; flat images {g[f'flat_{case}_{k}'].astype(int).tolist()}")
        assert np.array_equal(dm[k], exp), (case, k)
    for k in out:
        assert torch.equal(out[k], before[k]), k                   # the model's maps are only read (the zeroing happens on the fly)
    # the operator alone, and the maps as channel-0 VIEWS of a wider tensor (how the model hands out pc_hm_in): read in place
    src = next(k for k in DEPTH_KEYS if k in maps)
    one = ops.depth_maps([out[src]])
    assert one.shape == (1, B, H, W) and one.is_cuda and np.array_equal(one[0].cpu().numpy(), dm["depth"])
    wide = torch.full((B, 3, H, W), 1e9, device=dev)
    wide[:, :1] = out[src]
    view = wide[:, :1]
    assert not view.is_contiguous() or B == 1
    assert np.array_equal(ops.depth_maps([view])[0].cpu().numpy(), dm["depth"])
    # a pointer that is only 4-byte aligned takes the one-pixel path: the same bytes
    store = torch.zeros(B * H * W + 4, device=dev)
    off = store[1:1 + B * H * W].view(B, 1, H, W)
    off.copy_(out[src])
    assert off.data_ptr() % 16 != 0
    assert np.array_equal(ops.depth_maps([off])[0].cpu().numpy(), dm["depth"])


def test_flat_images_are_zero_and_the_rest_of_the_batch_is_not(dev, golden, golden_dir):
    from centerfusiondetect3d_amd import ops
    g = golden
    maps = _inputs(g, golden_dir, "flat")
    got = ops.depth_maps([torch.from_numpy(maps[k]).to(dev) for k in ("depth", "pc_hm_in")]).cpu().numpy()
    assert not got[0, 1].any() and not got[1, 2].any()
    for m, b in ((0, 0), (0, 2), (1, 0), (1, 1)):
        assert got[m, b].max() == 255 and got[m, b].min() == 0
    with pytest.raises(Exception, match="depth_maps"):
        ops.depth_maps([torch.zeros(2, 2, 4, 4, device=dev)])      # (B,1,H,W) maps only


@pytest.mark.parametrize("shape", [(1, 33, 41), (2, 112, 200), (1, 224, 400)], ids=lambda s: "x".join(map(str, s)))
def test_more_than_one_pass_per_workgroup(dev, shape):
    """Images larger than one sweep of the workgroup, odd sizes (the one-pixel path) and multiples of four (the 16-byte path),
    against the same three fp32 operations in numpy (what the reference executes)."""
    from centerfusiondetect3d_amd import ops
    B, H, W = shape
    x = np.random.RandomState(B * H + W).uniform(-3, 60, (B, 1, H, W)).astype(np.float32)
    z = x[:, 0].copy()
    z[0, 0] = 0
    z[0, :, 0] = 0
    lo, hi = z.min(axis=(1, 2), keepdims=True), z.max(axis=(1, 2), keepdims=True)
    want = (((z - lo) / (hi - lo)) * 255).astype(np.uint8)
    got = ops.depth_maps([torch.from_numpy(x).to(dev)])[0].cpu().numpy()
    assert np.array_equal(got, want)


def test_detector_run_returns_depthmaps_only_when_asked(dev):
    from centerfusiondetect3d_amd import Detector, centerfusion_middle_config, ops
    H, W, B = 128, 160, 2
    det = Detector(centerfusion_middle_config((H, W)), device=dev)
    det.model.load_state_dict(cases.tuned_state_dict(radar=True, seed=0), strict=True)
    calib = np.concatenate([cd.NUSC_K, np.zeros((3, 1))], axis=1)
    rs = np.random.RandomState(40)
    frames = torch.from_numpy(rs.randint(0, 256, (B, 900, 1600, 3)).astype(np.uint8))
    infos = [dict(calib=calib.tolist(), camera_intrinsic=cd.NUSC_K.tolist(), width=1600, height=900)] * B
    sweeps = [cd._sweep(np.random.RandomState(400 + b), 60 + 20 * b) for b in range(B)]
    with torch.no_grad():
        plain = det.run(frames, infos, sweeps)
        ret = det.run(frames, infos, sweeps, depthmaps=True)
    assert set(plain.keys()) == {"outputs", "post", "metas", "img_infos", "detects", "predictBoxes"}
    assert set(ret.keys()) == set(plain.keys()) | {"depthmaps"}
    assert torch.equal(ret["post"], plain["post"])
    dm = ret["depthmaps"]
    assert list(dm.keys()) == ["depth", "pc_hm_out", "pc_hm_in"]
    for k, v in dm.items():
        assert isinstance(v, np.ndarray) and v.dtype == np.uint8 and v.shape == (B, H // 4, W // 4), k
    out = ret["outputs"][0]
    assert np.array_equal(dm["depth"], ops.depth_maps([out["depthMap"]])[0].cpu().numpy())
    assert np.array_equal(dm["pc_hm_in"], ops.depth_maps([out["pc_hm_in"]])[0].cpu().numpy())
    # the raw depthMap may be negative everywhere (it is with these weights), so the zeroed row and column of image 0 are not
    # byte 0 but the byte of the value 0.0: restate the three fp32 operations on the host and compare every byte
    z = out["depthMap"][:, 0].cpu().numpy().copy()
    z[0, 0] = 0
    z[0, :, 0] = 0
    lo, hi = z.min(axis=(1, 2), keepdims=True), z.max(axis=(1, 2), keepdims=True)
    assert (hi > lo).all()
    assert np.array_equal(dm["depth"], (((z - lo) / (hi - lo)) * 255).astype(np.uint8))
    edge = np.concatenate([dm["depth"][0, 0], dm["depth"][0, :, 0]])
    assert dm["depth"].max() == 255 and (edge == edge[0]).all()                     # image 0: one byte along row 0 and column 0
    assert len(np.unique(dm["depth"][1, 0])) > 1 and len(np.unique(dm["depth"][1, :, 0])) > 1    # image 1 is not zeroed
    same =det.depth_maps(ret["outputs"])
    assert all(np.array_equal(same[k], dm[k]) for k in dm)
    with torch.no_grad():
        timed = det.run(frames, infos, sweeps, stage_times=True, depthmaps=True)
        piped = list(det.run_pipelined(iter([(frames, infos, sweeps)] * 2), depthmaps=True))
        piped_plain = list(det.run_pipelined(iter([(frames, infos, sweeps)])))
    assert timed["postprocess"] > 0.0 and all(np.array_equal(timed["depthmaps"][k], dm[k]) for k in dm)
    assert len(piped) == 2 and all(np.array_equal(p["depthmaps"][k], dm[k]) for p in piped for k in dm)
    assert "depthmaps" not in piped_plain[0]
    bad = dict(out, depthMap=out["depthMap"][:, :, :-1])
    with pytest.raises(ValueError, match="OUTPUT_SIZE|expected"):
        det.depth_maps([bad])
