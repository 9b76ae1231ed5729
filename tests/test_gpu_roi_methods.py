"""GPU: DATASET.PC_ROI_METHOD "points" and "heatmap" (cf_radar_roi_expand) against fixtures produced by the reference's own
processPointCloud (tests/golden/make_golden_roi_methods.py): painted set and values bit for bit, the keep mask and the
transformed coordinates as well; and the method travelling from the config through `Detector.run`."""
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
METHODS = ("points", "heatmap")
FIXTURES = [(m, p) for m in METHODS for p in sorted(glob.glob(os.path.join(GOLDEN, f"roi_{m}_*.npz")))]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def test_fixture_set_covers_what_it_must():
    for m in METHODS:
        gs = [np.load(p) for mm, p in FIXTURES if mm == m]
        assert len(gs) >= 4
        assert any(int(g["n_border_points"]) > 0 for g in gs) and any(int(g["n_near"]) > 0 for g in gs)
        assert any(int(g["n_shared_pixels"]) > 1 for g in gs)
        for g in gs:                                               # tie-free in depth, ascending: painting order = depth order
            assert (np.diff(g["in_pc_2d"][2]) > 0).all()


@pytest.mark.parametrize("method,path", FIXTURES, ids=[os.path.basename(p)[:-4] for _, p in FIXTURES])
def test_roi_expand_bit_exact_vs_reference_golden(dev, method, path):
    from centerfusiondetect3d_amd import ops, pointcloud
    g = np.load(path)
    H, W = (int(v) for v in g["in_out_hw"])
    ref = g["out_depth_map"]
    pc_dep = pointcloud.process_point_cloud_batch([g["in_pc_2d"]], [g["in_pc_3d"]], g["in_calib"][None], g["in_trans_out"],
                                                  (H, W), device=dev, roi_method=method)
    got = pc_dep[0].cpu().numpy()
    assert got.shape == ref.shape and got.dtype == ref.dtype
    assert np.array_equal(got != 0, ref != 0)
    assert np.array_equal(got, ref)
    n = g["in_pc_2d"].shape[1]
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
    _, keep, xy = ops.radar_roi_expand(t(g["in_pc_2d"][None], torch.float64), t(g["in_pc_3d"][None], torch.float64),
                                       t(np.array([n]), torch.int32), t(g["in_calib"][None], torch.float64),
                                       t(g["in_trans_out"][None], torch.float64), (H, W), method, want_aux=True)
    kb = keep[0].cpu().numpy().astype(bool)
    assert kb.sum() == g["out_pc_2d"].shape[1]
    assert np.array_equal(xy[0].cpu().numpy()[:, kb], g["out_pc_2d"][:2])


@pytest.mark.parametrize("method", METHODS)
def test_roi_expand_batched_ragged(dev, method):
    """The 112 x 200 fixtures of a method as ONE ragged batch, frame by frame equal to the single-frame results."""
    from centerfusiondetect3d_amd import pointcloud
    gs = [np.load(p) for m, p in FIXTURES if m == method and tuple(np.load(p)["in_out_hw"]) == (112, 200)]
    assert len(gs) >= 3
    pc_dep = pointcloud.process_point_cloud_batch([g["in_pc_2d"] for g in gs], [g["in_pc_3d"] for g in gs],
                                                  np.stack([g["in_calib"] for g in gs]), gs[0]["in_trans_out"], (112, 200),
                                                  device=dev, roi_method=method)
    for b, g in enumerate(gs):
        assert np.array_equal(pc_dep[b].cpu().numpy(), g["out_depth_map"]), b


def test_pillars_keyword_is_the_default_path(dev):
    from centerfusiondetect3d_amd import pointcloud
    g = np.load(os.path.join(GOLDEN, "pillar_n200.npz"))
    H, W = (int(v) for v in g["in_out_hw"])
    a = pointcloud.process_point_cloud_batch([g["in_pc_2d"]], [g["in_pc_3d"]], g["in_calib"][None], g["in_trans_out"], (H, W),
                                             device=dev)
    b = pointcloud.process_point_cloud_batch([g["in_pc_2d"]], [g["in_pc_3d"]], g["in_calib"][None], g["in_trans_out"], (H, W),
                                             device=dev, roi_method="pillars")
    assert torch.equal(a, b) and np.array_equal(a[0].cpu().numpy(), g["out_depth_map"])


def test_detector_run_uses_the_configured_method(dev):
    from centerfusiondetect3d_amd import Detector, centerfusion_middle_config, getModel, pointcloud
    from tests.golden import cases
    H, W = 128, 160
    cfg = centerfusion_middle_config((H, W))
    cfg.DATASET.PC_ROI_METHOD = "points"
    m = getModel(cfg)
    m.load_state_dict(cases.tuned_state_dict(radar=True, seed=0), strict=True)
    det = Detector(cfg, model=m, device=dev)
    rs = np.random.RandomState(7)
    frame = rs.randint(0, 256, (900, 1600, 3), dtype=np.uint8)
    K3 = np.array([[1266.417203046554, 0.0, 816.2670197447984], [0.0, 1266.417203046554, 491.50706579294757], [0.0, 0.0, 1.0]])
    calib = np.concatenate([K3, np.zeros((3, 1))], axis=1)
    n = 120
    sweep = np.zeros((18, n))
    sweep[2] = rs.uniform(2.0, 58.0, n)
    sweep[0] = rs.uniform(-0.5, 0.5, n) * sweep[2]
    sweep[1] = rs.uniform(-1.0, 1.0, n)
    sweep[8], sweep[9] = rs.normal(0, 5, n), rs.normal(0, 5, n)
    info = {"calib": calib.tolist(), "camera_intrinsic": K3.tolist(), "width": 1600, "height": 900}
    images, pc_dep, metas, calibs = det.pre_process([frame], [info], [sweep.copy()])
    kw = dict(max_dist=60.0, z_offset=0.0, pillar_dims=tuple(cfg.DATASET.PILLAR_DIMS), device=dev)
    args = ([sweep.copy()], K3[None], (1600, 900), calib[None], metas[0]["transMatOutput"], (H // 4, W // 4))
    points = pointcloud.radar_to_pc_dep(*args, roi_method="points", **kw)
    pillars = pointcloud.radar_to_pc_dep(*args, **kw)
    assert torch.equal(pc_dep, points) and not torch.equal(pc_dep, pillars)
    assert 0 < int((points[0, 0] != 0).sum()) <= n < int((pillars[0, 0] != 0).sum())
    ret = det.run(frame, info, sweep.copy())
    assert torch.equal(ret["outputs"][0]["pc_hm_in"], points[:, :1])
    assert ret["post"].shape[0] == 1
