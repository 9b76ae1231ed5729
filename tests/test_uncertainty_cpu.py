"""The `uncertainty` head (TRAIN.UNCERTAINTY_LOSS) and `depthmaps`, everything that needs no GPU: the derived head, the parameter
tree against the reference's (fixture of tests/golden/make_golden_uncertainty.py), the additive exports and their argument
checks, the public signatures, and the fixtures' own discriminating power."""
import ctypes
import inspect
import os

import numpy as np
import pytest

from tests.golden.make_golden_uncertainty import uncertainty_state_dict, FIXTURE, B, H, W, K
from tests.golden.make_golden_depthmaps import FIXTURE as DM_FIXTURE


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, FIXTURE))


def _cfg(size=(H, W)):
    from centerfusiondetect3d_amd import centerfusion_middle_config
    from centerfusiondetect3d_amd.config import update_heads
    c = centerfusion_middle_config(size)
    c.TRAIN.UNCERTAINTY_LOSS = True
    return update_heads(c)


def test_config_derives_the_head():
    c = _cfg()
    assert c.heads["uncertainty"] == 1 and list(c.head_conv["uncertainty"]) == [256]
    assert list(c.heads)[-1] == "uncertainty"                      # config/utils.py:100-102: after depth2 / rotation2
    from centerfusiondetect3d_amd import centerfusion_middle_config
    assert "uncertainty" not in centerfusion_middle_config((H, W)).heads


def test_state_dict_keys_and_shapes_equal_the_references(golden):
    from centerfusiondetect3d_amd import getModel
    m = getModel(_cfg())
    sd = m.state_dict()
    ref = dict(zip((str(k) for k in golden["sd_keys"]), (str(s) for s in golden["sd_shapes"])))
    assert {k: ",".join(str(int(n)) for n in v.shape) for k, v in sd.items()} == ref
    for k, shape in (("0.weight", (256, 64, 3, 3)), ("0.bias", (256,)), ("2.weight", (1, 256, 1, 1)), ("2.bias", (1,))):
        assert tuple(sd[f"detectHead_0.uncertainty.{k}"].shape) == shape
    assert len(sd) == len(getModel(_base_cfg()).state_dict()) + 4
    m.load_state_dict(uncertainty_state_dict(0), strict=True)


def _base_cfg():
    from centerfusiondetect3d_amd import centerfusion_middle_config
    return centerfusion_middle_config((H, W))


def test_new_exports_exist_and_reject_null_arguments():
    from centerfusiondetect3d_amd import _lib
    lib = _lib.load()
    assert lib.cf_abi_version() == 7
    d = _lib.DecodeArgs()
    assert lib.cf_decode_gather_unc(None, None, None) == -22
    assert b"uncertainty" in lib.cf_last_error()
    assert lib.cf_decode_gather_unc(ctypes.byref(d), 16, None) == -22     # (a non-null map: the struct's buffers are checked next)
    assert b"cf_decode_gather_unc: null buffer" in lib.cf_last_error()
    assert lib.cf_decode_post_unc(ctypes.byref(d), None, None, None, None, None) == -22
    assert b"uncertainty" in lib.cf_last_error()
    assert lib.cf_decode_post_unc(ctypes.byref(d), 16, None, None, None, None) == -22
    assert b"cf_decode_post_unc: null buffer" in lib.cf_last_error()
    # the siblings answer as before
    assert lib.cf_decode_gather(ctypes.byref(d), None) == -22 and b"cf_decode_gather: null buffer" in lib.cf_last_error()
    assert lib.cf_decode_post(ctypes.byref(d), None, None, None, None) == -22
    assert b"cf_decode_post: null buffer" in lib.cf_last_error()
    assert lib.cf_depth_maps(None, None, 1, 1, 4, 4, None, None) == -22 and b"maps" in lib.cf_last_error()
    one = (_lib._f * 1)(None)
    assert lib.cf_depth_maps(one, None, 1, 1, 4, 4, None, None) == -22 and b"out" in lib.cf_last_error()
    assert lib.cf_depth_maps(one, None, 1, 1, 4, 4, 16, None) == -22 and b"maps[0]" in lib.cf_last_error()
    one[0] = 16
    assert lib.cf_depth_maps(one, None, _lib.CF_DEPTH_MAPS_MAX + 1, 1, 4, 4, 16, None) == -22 and b"n_maps" in lib.cf_last_error()
    assert lib.cf_depth_maps(one, None, 1, 0, 4, 4, 16, None) == -22 and b"geometry" in lib.cf_last_error()
    short = (ctypes.c_long * 1)(15)
    assert lib.cf_depth_maps(one, short, 1, 2, 4, 4, 16, None) == -22 and b"batch_strides" in lib.cf_last_error()


def test_public_signatures():
    from centerfusiondetect3d_amd import ops
    from centerfusiondetect3d_amd.detector import Detector
    for fn in (Detector.run, Detector.run_pipelined):
        p = inspect.signature(fn).parameters["depthmaps"]
        assert p.default is False
    assert callable(Detector.depth_maps) and callable(ops.depth_maps)
    for fn in (ops.decode_gather, ops.decode_post):
        assert inspect.signature(fn).parameters["uncertainty"].default is None


def test_decode_no_longer_refuses_the_head_on_the_host_side():
    """_peaks_and_maps used to raise before any launch; what it raises now for host tensors is the library's 'no CPU path'."""
    import torch
    from centerfusiondetect3d_amd import _lib, fusionDecode
    out = {"heatmap": torch.zeros(1, 10, 4, 4), "uncertainty": torch.zeros(1, 1, 4, 4)}
    with pytest.raises(_lib.CfHipError, match="device tensors"):
        fusionDecode([out], outputSize=(4, 4), K=4)


def test_uncertainty_fixture_discriminates(golden):
    g = golden
    assert g["det_scores"].shape == (B, K) and g["det_scores"].dtype == np.float32
    w = np.exp(-np.exp(g["peak_u"].astype(np.float64)))
    assert ((w.max(1) / w.min(1)) >= 2.0).all()                                   # the weights matter ...
    assert (g["det_scores"][:, 1:] > g["det_scores"][:, :-1]).any()               # ... and a re-sorting decode would differ
    assert (g["ctl_scores"][:, 1:] <= g["ctl_scores"][:, :-1]).all()
    for k in g.files:
        if k.startswith("det_") and k != "det_scores":
            assert np.array_equal(g[k], g["ctl_" + k[4:]]), k
    f64 = g["ctl_scores"].astype(np.float64) * w
    assert np.array_equal(f64, g["score_f64"])
    e = float((np.abs(g["det_scores"].astype(np.float64) - f64) / f64).max())
    assert e == float(g["e_ref"]) and 0 < e < 1e-6
    # u really is the head's map at the peak pixels
    xs = np.rint(g["ctl_centers"][..., 0] * (W // 4)).astype(int)
    ys = np.rint(g["ctl_centers"][..., 1] * (H // 4)).astype(int)
    for b in range(B):
        assert np.array_equal(g["out_uncertainty"][b, 0, ys[b], xs[b]], g["peak_u"][b])


def test_depthmaps_fixture_holds_its_cases(golden_dir, golden):
    d = np.load(os.path.join(golden_dir, DM_FIXTURE))
    assert [str(c) for c in d["cases"]] == ["unc", "neg", "k255", "flat"]
    assert d["ref_unc_depth"].shape == (B, H // 4, W // 4) and d["ref_unc_depth"].dtype == np.uint8
    # image 0's border is one value (the zeroed one), image 1's is not
    assert len(np.unique(np.concatenate([d["ref_unc_depth"][0, 0], d["ref_unc_depth"][0, :, 0]]))) == 1
    assert len(np.unique(np.concatenate([d["ref_unc_depth"][1, 0], d["ref_unc_depth"][1, :, 0]]))) > 1
    neg = d["in_neg_depth"]
    assert neg.shape == (3, 1, 5, 7) and (neg < 0).any()
    assert neg[0, 0].argmax() == 3 and d["ref_neg_depth"][0, 0, 3] != 255 and d["ref_neg_depth"][1, 0, 2] == 255
    assert int(d["ref_k255_depth"].max()) == 255
    assert d["flat_flat_depth"].tolist() == [False, True, False] and d["flat_flat_pc_hm_in"].tolist() == [False, False, True]
