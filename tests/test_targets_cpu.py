"""CPU side of the training-target builder (centerfusiondetect3d_amd.targets): `pack_annotations` (presence bits, truncation to
max_objs, the class map, the ValueError of the frustum keys), the ctypes mirror of cf_targets_args against the C compiler, the
refusals of `build_targets` before any device is touched, and the invariants of the fixture tests/golden/targets_cases.npz that the
GPU tests compare against (keys, dtypes and shapes of the reference's initReturn; mask.sum() equals the rows drawn)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import targets_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "targets_cases.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(FIXTURE))


def _pack(case, **kw):
    from centerfusiondetect3d_amd import pack_annotations
    return pack_annotations(case["anns"], class_ids=case["class_ids"], max_objs=case["max_objs"], **kw)


def test_pack_flags_truncation_and_class_map():
    from centerfusiondetect3d_amd import _lib
    case = tc.build("skips")
    p = _pack(case)
    assert p.table.dtype == torch.float64 and tuple(p.table.shape) == (2, 8, _lib.CF_TARGETS_F)
    assert p.itable.dtype == torch.int32 and tuple(p.itable.shape) == (2, 8, 3)
    assert p.counts.tolist() == [8, 2]                                  # 11 annotations, the first max_objs = 8 kept
    bits = [_lib.TGT_HAS_AMODAL, _lib.TGT_HAS_ATTRIBUTES, _lib.TGT_HAS_VELOCITY, _lib.TGT_HAS_ALPHA, _lib.TGT_HAS_DEPTH,
            _lib.TGT_HAS_DIMENSION, _lib.TGT_HAS_LOCATION, _lib.TGT_HAS_YAW]
    for i in range(8):                                                  # annotation i lacks optional key i and nothing else
        assert int(p.itable[0, i, 2]) == 255 & ~bits[i]
    assert int(p.itable[0, 2, 0]) == 11 and int(p.itable[0, 5, 0]) == -999      # the class map, not the category id
    assert int(p.itable[0, 3, 0]) == 4
    a = case["anns"][0][0]
    assert p.table[0, 0, :4].tolist() == a["bbox"] and float(p.table[0, 0, 4]) == a["truncated"]
    assert p.table[0, 0, 13:16].tolist() == a["dimension"] and float(p.table[0, 0, 19]) == a["yaw"]
    assert float(p.table[1, 0, 10]) == -1000.5                          # min(velocity_cam) travels with the row
    assert not p.table[1, 2:].any() and not p.itable[1, 2:].any()
    # the default class map is the identity on 1..num_classes: category 11 is not in it
    from centerfusiondetect3d_amd import pack_annotations
    with pytest.raises(KeyError):
        pack_annotations(case["anns"])
    with pytest.raises(ValueError, match="max_objs"):
        pack_annotations(case["anns"], max_objs=129)


def test_pack_refuses_missing_frustum_keys():
    """radar + frustum: the reference raises KeyError inside addInstance; here it is a ValueError at packing time"""
    from centerfusiondetect3d_amd import build_targets, pack_annotations
    case = tc.build("skips")
    cfg = tc.config_for(tc.build("basic"))
    with pytest.raises(ValueError, match="dimension, alpha and depth"):
        _pack(case, config=cfg)
    _pack(case, config=tc.config_for(case))                             # camera only: nothing is required
    anns = [[dict(a) for a in case["anns"][1]]]
    del anns[0][1]["alpha"]
    with pytest.raises(ValueError, match="alpha"):
        pack_annotations(anns, config=cfg)
    anns[0][1]["category_id"] = 11                                      # a skipped class needs nothing
    pack_annotations(anns, class_ids=case["class_ids"], config=cfg)
    # build_targets looks again when the tables are still on the host
    p = pack_annotations([[dict(a) for a in case["anns"][1]][:1] + [{k: v for k, v in case["anns"][1][1].items() if k != "depth"}]])
    with pytest.raises(ValueError, match="dimension, alpha and depth"):
        build_targets(p, torch.zeros(1, 2, 3, dtype=torch.float64), torch.zeros(1, 3, 4), cfg,
                      pc_dep=torch.zeros(1, 3, 28, 50), device="cuda")


def test_targets_struct_layout_matches_c(tmp_path):
    from centerfusiondetect3d_amd import _lib
    fields = ["ann", "pc_dep", "B", "flags", "max_pc_dist", "heat", "rotbin", "pc_hm", "t_bboxes", "t_velocity", "workspace",
              "workspace_bytes"]
    prog = tmp_path / "szt.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cf_hip.h"\nint main(){printf("%zu", sizeof(cf_targets_args));'
                    + "".join(f'printf(" %zu", offsetof(cf_targets_args, {f}));' for f in fields)
                    + 'printf(" %d %d %d\\n", CF_TARGETS_MAX_OBJS, CF_TARGETS_F, CF_TARGETS_DESC_BYTES);return 0;}')
    exe = tmp_path / "szt"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    A = _lib.TargetsArgs
    lib = _lib.load()
    assert got == [ctypes.sizeof(A)] + [getattr(A, f).offset for f in fields] + \
        [_lib.CF_TARGETS_MAX_OBJS, _lib.CF_TARGETS_F, lib.cf_targets_workspace_bytes(1, 1)]
    assert lib.cf_targets_workspace_bytes(16, 128) == 16 * 128 * got[-1] and lib.cf_targets_workspace_bytes(0, 128) == 0


def test_entry_point_validates_before_the_device():
    from centerfusiondetect3d_amd import _lib
    lib = _lib.load()
    a = _lib.TargetsArgs()
    assert lib.cf_targets_build(ctypes.byref(a), None) == -22 and b"cf_targets_build" in lib.cf_last_error()
    a.B, a.M, a.C, a.h, a.w = 1, 129, 10, 28, 50
    assert lib.cf_targets_build(ctypes.byref(a), None) == -22 and b"M <= 128" in lib.cf_last_error()
    a.M = 128
    assert lib.cf_targets_build(ctypes.byref(a), None) == -22 and b"null input table" in lib.cf_last_error()
    assert lib.cf_targets_build(None, None) == -22


def test_build_targets_refusals():
    from centerfusiondetect3d_amd import _lib, build_targets
    case = tc.build("empty_b1")
    cfg = tc.config_for(case)
    p = _pack(case)
    trans, calib, pc = torch.from_numpy(case["trans"]), torch.from_numpy(case["calib"]), torch.from_numpy(case["pc_dep"])
    with pytest.raises(_lib.CfHipError, match="GPU"):
        build_targets(p, trans, calib, cfg, pc_dep=pc)                  # CPU tensors: there is no CPU path
    with pytest.raises(_lib.CfHipError, match="GPU"):
        build_targets(p, trans, calib, tc.config_for(tc.build("borders")))
    with pytest.raises(ValueError, match="pc_dep"):
        build_targets(p, trans, calib, cfg, device="cuda")
    cfg.MODEL.PYRAMID_OUT_SIZE = [cfg.MODEL.OUTPUT_SIZE, (14, 25)]
    with pytest.raises(NotImplementedError, match="one output layer"):
        build_targets(p, trans, calib, cfg, pc_dep=pc)
    cfg.MODEL.PYRAMID_OUT_SIZE = [cfg.MODEL.OUTPUT_SIZE]
    cfg.DATASET.ONE_HOT_PC = True
    with pytest.raises(NotImplementedError, match="ONE_HOT_PC"):
        build_targets(p, trans, calib, cfg, pc_dep=pc)
    cfg.DATASET.ONE_HOT_PC = False
    cfg.DATASET.HEATMAP_REP = "4d"
    with pytest.raises(ValueError, match="heatmap representation"):
        build_targets(p, trans, calib, cfg, pc_dep=pc)


def expected_keys(case):
    """{fixture key: (dtype, shape without B)} - initReturn of generic_dataset.py:441-493 and nuscenes.py:348-391"""
    cfg = tc.config_for(case)
    heads, M, (h, w) = set(cfg.heads), case["max_objs"], case["out_hw"]
    f, i = np.float32, np.int64
    keys = {"heatmap0": (f, (tc.NUM_CLASSES, h, w)), "classIds": (i, (M,)), "mask": (f, (M,)), "truncMask": (f, (M,)),
            "widthHeight": (f, (M, 2)), "reg": (f, (M, 2)), "dimension": (f, (M, 3)), "amodal_offset": (f, (M, 2)),
            "depth": (f, (M, 1)), "rotbin": (i, (M, 2)), "rotres": (f, (M, 2)), "nuscenes_att": (f, (M, 8)),
            "nuscenes_att_mask": (f, (M, 8)), "velocity": (f, (M, 3)),
            "target.bboxes": (f, (M, 4)), "target.scores": (f, (M,)), "target.centers": (f, (M, 2)),
            "target.heatCenters": (f, (M, 2)), "target.bboxes3d": (f, (M, 8, 3)), "target.rotation": (f, (M, 8)),
            "target.nuscenes_att": (f, (M, 8)), "target.velocity": (f, (M, 3))}
    assert {"reg", "dimension", "amodal_offset", "depth", "rotation", "nuscenes_att", "velocity"} <= heads
    if case["radar"]:
        keys["pc_hm"] = (f, (3, h, w))
    return keys


@pytest.mark.parametrize("name", tc.NAMES)
def test_fixture_invariants(golden, name):
    case = tc.build(name)
    B = len(case["anns"])
    want = expected_keys(case)
    have = {k.split("/out_")[1] for k in golden if k.startswith(name + "/out_")}
    assert have == set(want)
    for k, (dtype, shape) in want.items():
        v = golden[f"{name}/out_{k}"]
        assert v.dtype == dtype and v.shape == (B,) + shape, (k, v.dtype, v.shape)
    for k in ("trans", "calib", "scale") + (("pc_dep",) if case["radar"] else ()):
        assert np.array_equal(golden[f"{name}/in_{k}"], case[k]), k     # the fixture was made from these very cases
    out = lambda k: golden[f"{name}/out_{k}"]
    mask = out("mask")
    drawn = (out("widthHeight") != 0).all(-1)
    assert mask.sum() == drawn.sum() and np.array_equal(mask != 0, drawn)
    assert set(np.unique(mask)) <= {0.0, 1.0}
    # a heat-map peak of exactly 1 at every drawn row's integer centre, in its class
    hc, cls = out("target.heatCenters"), out("classIds")
    for b, m in zip(*np.nonzero(mask)):
        assert out("heatmap0")[b, cls[b, m], int(hc[b, m, 1]), int(hc[b, m, 0])] == 1.0
    assert not out("target.scores").any() and not out("target.nuscenes_att").any() and not out("target.velocity").any()
    for k in want:                                                      # a skipped row is zero in every per-object array
        if k not in ("heatmap0", "pc_hm"):
            assert not out(k)[mask == 0].any(), k
    if name == "skips":
        assert mask[0].tolist() == [1, 1, 0, 1, 1, 0, 1, 1] and mask[1].tolist() == [1, 1, 0, 0, 0, 0, 0, 0]
        assert not out("velocity")[1, 0].any() and out("velocity")[1, 1].any()
        assert not out("nuscenes_att_mask")[1, 1].any()
    if name == "borders":
        assert mask[0, :8].tolist() == [1, 1, 1, 1, 1, 1, 0, 1]         # the zero-width box between two valid rows
        assert int((out("heatmap0")[0, 5] != 0).sum()) == 1             # the radius-0 object: its centre pixel alone
    if name == "rep3d_norm2d":
        hcx, hcy = hc[0, :5, 0], hc[0, :5, 1]
        assert hcx[1] == 0.0 and hcx[2] == 49.0 and hcy[2] == 27.0 and hcy[4] == 27.0       # clipped amodal centres
        assert float(out("widthHeight")[0, :5].max()) < 1.0             # NORM_2D
    if name == "full":
        assert mask.sum() == 128
    if name.startswith("empty"):
        assert not mask[0].any() and not out("heatmap0")[0].any() and not out("pc_hm")[0].any()
    if name == "nofrustum":
        pc = case["pc_dep"]
        assert np.array_equal(out("pc_hm")[:, 1:], pc[:, 1:]) and np.array_equal(out("pc_hm")[:, 0] == 1.0, pc[:, 0] == 0)
