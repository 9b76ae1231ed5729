"""CPU: the host-side contract of the two radar configurations added beside pillars + frustum - middle fusion with
MODEL.FRUSTUM = False (the model constructs, same parameters) and DATASET.PC_ROI_METHOD "points" / "heatmap" (method
validation before the device is touched, a config without the key means pillars) - and the argument validation of the two new
entry points.  No compute calls (no GPU here)."""
import ctypes

import numpy as np
import pytest
import torch


def _cfg(frustum, size=(128, 160)):
    from centerfusiondetect3d_amd import centerfusion_middle_config
    c = centerfusion_middle_config(size)
    c.MODEL.FRUSTUM = frustum
    return c


def test_model_without_frustum_constructs_with_the_same_parameters():
    from centerfusiondetect3d_amd import getModel
    m0, m1 = getModel(_cfg(True)), getModel(_cfg(False))
    assert m1.isRadarEnabled and m1.fusionStrategy == "middle" and not m1.isFrustumEnabled and m0.isFrustumEnabled
    sd0, sd1 = m0.state_dict(), m1.state_dict()
    assert list(sd0.keys()) == list(sd1.keys())
    assert all(sd0[k].shape == sd1[k].shape for k in sd0)
    assert sd1["detectHead_0.depth2.0.weight"].shape[1] == 67          # cat(feat, pc_hm): 64 + 1 + 2 channels


def test_the_other_constructor_guards_stay():
    from centerfusiondetect3d_amd import getModel
    c = _cfg(False)
    c.DATASET.ONE_HOT_PC = True
    with pytest.raises(NotImplementedError, match="ONE_HOT_PC"):
        getModel(c)
    c = _cfg(False)
    c.MODEL.FUSION_STRATEGY = "early"
    with pytest.raises(NotImplementedError):
        getModel(c)


@pytest.mark.parametrize("bad", ["nonsense", "Pillars", None, ""])
def test_unknown_roi_method_raises_before_the_device(bad, monkeypatch):
    from centerfusiondetect3d_amd import ops, pointcloud

    def boom(*a, **k):
        raise AssertionError("the device was touched")
    for name in ("radar_ingest", "pillar_expand", "radar_roi_expand"):
        monkeypatch.setattr(ops, name, boom)
    sweep = np.zeros((18, 3)); sweep[2] = 10.0
    with pytest.raises(ValueError, match=f"Invalid PC_ROI_METHOD: {bad}"):
        pointcloud.radar_to_pc_dep([sweep], np.eye(3), (1600, 900), np.zeros((1, 3, 4)), np.zeros((2, 3)), (112, 200),
                                   roi_method=bad)
    with pytest.raises(ValueError, match="Invalid PC_ROI_METHOD"):
        pointcloud.process_point_cloud_batch([np.zeros((3, 1))], [np.zeros((18, 1))], np.zeros((1, 3, 4)), np.zeros((2, 3)),
                                             (112, 200), roi_method=bad)


@pytest.mark.parametrize("method", [None, "pillars", "points", "heatmap"])
def test_detector_hands_the_configured_method_on_and_no_key_means_pillars(method, monkeypatch):
    from centerfusiondetect3d_amd import detector
    cfg = _cfg(True, (448, 800))
    if method is None:
        del cfg.DATASET["PC_ROI_METHOD"]
    else:
        cfg.DATASET.PC_ROI_METHOD = method
    seen = {}

    def fake_radar(*a, **k):
        seen.update(k)
        return "pc_dep"
    monkeypatch.setattr(detector, "radar_to_pc_dep", fake_radar)
    monkeypatch.setattr(detector, "preProcessImages", lambda *a, **k: "images")
    d = detector.Detector.__new__(detector.Detector)
    d.config, d.device, d.mean, d.std = cfg, torch.device("cpu"), detector.NUSCENES_MEAN, detector.NUSCENES_STD
    info = {"calib": np.eye(3, 4).tolist(), "camera_intrinsic": np.eye(3).tolist(), "width": 1600, "height": 900}
    images, pc_dep, metas, calibs = d.pre_process([np.zeros((900, 1600, 3), np.uint8)], [info], [np.zeros((18, 0))])
    assert pc_dep == "pc_dep" and seen["roi_method"] == (method or "pillars")


def test_new_entry_points_validate_their_arguments_without_gpu():
    from centerfusiondetect3d_amd import _lib
    lib = _lib.load()
    assert lib.cf_abi_version() == 7
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    assert lib.cf_pc_hm_direct(None, 1, 4, 4, 60.0, None, None, None) == -22
    assert b"cf_pc_hm_direct" in lib.cf_last_error() and b"null" in lib.cf_last_error()
    assert lib.cf_pc_hm_direct(p, 0, 4, 4, 60.0, None, None, None) == -22
    assert lib.cf_pc_hm_direct(p, 1, -1, 4, 60.0, None, None, None) == -22
    assert b"geometry" in lib.cf_last_error()
    assert lib.cf_pc_hm_direct(p, 1, 4, 4, 0.0, None, None, None) == -22
    assert b"max_pc_dist" in lib.cf_last_error()
    assert lib.cf_pc_hm_direct(p, 1, 4, 4, 60.0, p + 4, None, None) == -22
    assert b"aligned" in lib.cf_last_error()
    d = (ctypes.c_double * 64)()
    q = ctypes.addressof(d)
    args = lambda **o: [o.get("pc_2d", q), q, q, o.get("B", 1), o.get("max_n", 4), o.get("n_rows", 18), q, q, 112, 200,
                        o.get("method", 1), p, None, None, None]
    assert lib.cf_radar_roi_expand(*args(pc_2d=None)) == -22
    assert b"cf_radar_roi_expand" in lib.cf_last_error()
    assert lib.cf_radar_roi_expand(*args(B=0)) == -22
    assert lib.cf_radar_roi_expand(*args(max_n=100000)) == -22
    assert lib.cf_radar_roi_expand(*args(n_rows=9)) == -22
    for bad in (0, 3, -1):
        assert lib.cf_radar_roi_expand(*args(method=bad)) == -22
        assert b"method" in lib.cf_last_error()
