"""GPU: the `uncertainty` head (TRAIN.UNCERTAINTY_LOSS = True) against the fixture the reference's own forward + fusionDecode
produced (tests/golden/make_golden_uncertainty.py).

Decode of GIVEN maps (the reference's own, uploaded: no model error enters): every field except `scores` bit for bit, the rows
in the reference's order (NOT sorted again by the weighted score); `scores` = score * exp(-exp(u)) against the reference's fp32
values with the relative bound 4 * e_ref, e_ref being the reference's own largest relative distance from the float64 evaluation
(stored in the fixture: two chained exp calls of two math libraries may differ by an ulp or two each, and the inner difference
is amplified by e^u).  Each measured deviation is printed before it is asserted.

Model level: our forward on the fixture's weights and inputs against every stored map under tests/test_gpu_model.py's criterion
(`_assert_maps_close`, RTOL / ATOL_FLOOR: imported, not restated), for both head arithmetics, and Detector.process end to end."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.golden.make_golden_uncertainty import uncertainty_inputs, uncertainty_state_dict, FIXTURE, B, H, W, K
from tests.test_gpu_model import _assert_maps_close, RTOL, ATOL_FLOOR          # noqa: F401  (the criterion in use)

OUT_HW = (H // 4, W // 4)
F64_BOUND = 5.0          # in units of e_ref, for comparisons with a float64 evaluation (see test_cached_peaks_are_never_weighted_in_place)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, FIXTURE))


def _maps(g, dev, batch=slice(None), drop=()):
    return {str(k): torch.from_numpy(g[f"out_{k}"][batch]).to(dev) for k in g["key_order"]
            if str(k) != "calib" and str(k) not in drop}


def _rel(scores, ref):
    ref = np.asarray(ref, np.float64)
    return float((np.abs(np.asarray(scores, np.float64) - ref) / np.abs(ref)).max())


def _check_scores(got, g, what, batch=slice(None)):
    bound = 4.0 * float(g["e_ref"])
    dev32 = _rel(got, g["det_scores"][batch])
    dev64 = _rel(got, g["score_f64"][batch])
    print(f"[uncertainty] {what}: max rel. deviation from the reference's fp32 scores {dev32:.3e} (bound 4 * e_ref = {bound:.3e}), "
          f"from float64 {dev64:.3e} (the reference's own: e_ref = {float(g['e_ref']):.3e})")
    assert dev32 <= bound, (what, dev32, bound)


def _cfg():
    from centerfusiondetect3d_amd import centerfusion_middle_config
    from centerfusiondetect3d_amd.config import update_heads
    c = centerfusion_middle_config((H, W))
    c.TRAIN.UNCERTAINTY_LOSS = True
    return update_heads(c)


def _model(dev, **flags):
    from centerfusiondetect3d_amd import getModel
    m = getModel(_cfg())
    for k, v in flags.items():
        setattr(m, k, v)
    m.load_state_dict(uncertainty_state_dict(0), strict=True)
    return m.to(dev).eval()


# ------------------------------------------------------------------------------------------------ decode of given maps
def test_fusion_decode_weights_the_scores_and_keeps_the_order(dev, golden):
    from centerfusiondetect3d_amd import fusionDecode
    g = golden
    maps = _maps(g, dev)
    det = fusionDecode([maps], outputSize=OUT_HW, K=K, norm2d=False)
    ref_keys = {k[4:] for k in g.files if k.startswith("det_")}
    assert set(det.keys()) == ref_keys
    for k in sorted(ref_keys - {"scores"}):                       # the index path: bit for bit, rows in the reference's order
        assert det[k].shape == g[f"det_{k}"].shape, k
        assert np.array_equal(det[k].cpu().numpy(), g[f"det_{k}"]), k
    s = det["scores"].cpu().numpy()
    assert s.shape == (B, K) and s.dtype == np.float32
    _check_scores(s, g, "fusionDecode")
    assert (s[:, 1:] > s[:, :-1]).any()                           # not sorted again
    assert "rotation2" not in maps and "rotation" in maps and "uncertainty" in maps
    again = fusionDecode([maps], outputSize=OUT_HW, K=K, norm2d=False)["scores"]          # the same dict twice
    assert torch.equal(again, det["scores"])


def test_packed_decodes_agree_and_a_dict_without_the_key_is_the_control(dev, golden):
    from centerfusiondetect3d_amd import fusionDecode, ops
    from centerfusiondetect3d_amd.decode import decode_packed, decode_post_packed, unpack_detections
    from centerfusiondetect3d_amd.postprocess import inverse_affine
    g = golden
    _, _, calib = uncertainty_inputs()
    tinv = torch.from_numpy(inverse_affine(np.array([800.0, 450.0], np.float32), 1600.0, (OUT_HW[1], OUT_HW[0]))).to(dev)
    det, present = decode_packed([_maps(g, dev)], outputSize=OUT_HW, K=K)
    assert det.shape == (B, K, 33)
    _check_scores(det[..., 0].cpu().numpy(), g, "decode_packed")
    post, det2 = decode_post_packed([_maps(g, dev)], calib.to(dev), tinv, outputSize=OUT_HW, K=K, want_det=True)
    assert post.shape == (B, K, 54)
    assert torch.equal(det2, det) and torch.equal(post[..., 0], det[..., 0])            # one kernel body: the same bits
    # without the key: the control, bit for bit - through every entry
    ctl, _ = decode_packed([_maps(g, dev, drop=("uncertainty",))], outputSize=OUT_HW, K=K)
    for k, v in unpack_detections(ctl, present).items():
        assert np.array_equal(v.cpu().numpy(), g[f"ctl_{k}"]), k
    assert torch.equal(ctl[..., 1:], det[..., 1:])                                      # only column 0 differs
    post_ctl = decode_post_packed([_maps(g, dev, drop=("uncertainty",))], calib.to(dev), tinv, outputSize=OUT_HW, K=K)
    assert np.array_equal(post_ctl[..., 0].cpu().numpy(), g["ctl_scores"])
    assert torch.equal(post_ctl[..., 1:], post[..., 1:])
    d = fusionDecode([_maps(g, dev, drop=("uncertainty",))], outputSize=OUT_HW, K=K)
    assert np.array_equal(d["scores"].cpu().numpy(), g["ctl_scores"])
    # the operator refuses a map of another shape instead of reading out of bounds
    m = _maps(g, dev)
    s, i, c = ops.topk_peaks(m["heatmap"], K, nms=True)
    with pytest.raises(Exception, match="uncertainty"):
        ops.decode_gather(s, i, c, {}, *OUT_HW, OUT_HW, uncertainty=m["uncertainty"][:, :, :-1])


def test_batch_of_one(dev, golden):
    """B = 1: the reference's `.squeeze()` gives (K,) there and broadcasts back to (1, K); image 1 of the fixture alone."""
    from centerfusiondetect3d_amd import fusionDecode
    g = golden
    det = fusionDecode([_maps(g, dev, batch=slice(1, 2))], outputSize=OUT_HW, K=K)
    assert det["scores"].shape == (1, K)
    for k in ("classIds", "centers", "bboxes", "depth", "velocity"):
        assert np.array_equal(det[k].cpu().numpy(), g[f"det_{k}"][1:2]), k
    _check_scores(det["scores"].cpu().numpy(), g, "B = 1", batch=slice(1, 2))


# ------------------------------------------------------------------------------------------------------- model level
@pytest.fixture(scope="module")
def forward(dev):
    """One forward per head arithmetic, shared (the outputs are not modified by the tests that only read them)."""
    x, pc_dep, calib = uncertainty_inputs()
    out = {}
    for name, flags in (("heads_bf16", dict()), ("exact_fp32_heads", dict(heads_bf16=False))):
        m = _model(dev, **flags)
        with torch.no_grad():
            out[name] = (m, m(x.to(dev), pc_dep=pc_dep.to(dev), calib=calib.to(dev)))
    return out


@pytest.mark.parametrize("arith", ["heads_bf16", "exact_fp32_heads"])
def test_forward_matches_the_reference_maps(forward, golden, arith):
    g = golden
    m, out = forward[arith]
    assert isinstance(out, list) and len(out) == 1
    y = out[0]
    assert list(y.keys()) == [str(k) for k in g["key_order"]]
    assert tuple(y["uncertainty"].shape) == (B, 1) + OUT_HW
    for k, v in y.items():
        if k != "calib":
            _assert_maps_close(v, g[f"out_{k}"], f"{arith} {k}")
    launched = [st[0].__name__ for plan in m._all_plans() for st in plan.steps if st and not isinstance(st[0], str)]
    if arith == "heads_bf16":
        assert launched.count("cf_head_fused") == 2                # eight primary heads in the one fused launch, then the secondary
    assert any("uncertainty" in p.primary and len(p.primary) == 8 for p in m._all_plans())


def test_range_guard_covers_the_head(dev):
    m = _model(dev)
    x, pc_dep, calib = uncertainty_inputs()
    m.check_ranges(x.to(dev), pc_dep.to(dev), calib.to(dev))       # the shadow forward runs all eight primary heads
    r = m.measure_ranges(x.to(dev), pc_dep.to(dev), calib.to(dev))
    assert any("heads.primary" in str(k) or "uncertainty" in str(k) for k in r), sorted(map(str, r))[:8]


def test_cached_peaks_are_never_weighted_in_place(dev, golden, forward):
    """The forward attaches the decoder's peaks to the heat map tensor; every decode of that tensor reuses those score
    buffers.  Twice the same outputs -> twice the same weighted scores; a heat map written after the forward -> the peaks are
    recomputed (the checksum guard) and then weighted."""
    from centerfusiondetect3d_amd import fusionDecode
    x, pc_dep, calib = uncertainty_inputs()
    m = forward["heads_bf16"][0]
    with torch.no_grad():
        out = m(x.to(dev), pc_dep=pc_dep.to(dev), calib=calib.to(dev))
    heat = out[0]["heatmap"]
    cached = getattr(heat, "_cf_peaks", None)
    assert cached is not None, "the forward no longer carries the decoder's peaks: this test would show nothing"
    raw = cached[2].clone()
    a = fusionDecode(out, outputSize=OUT_HW, K=K)
    assert torch.equal(cached[2], raw)                             # the shared buffer still holds the raw scores
    b = fusionDecode(out, outputSize=OUT_HW, K=K)
    assert torch.equal(a["scores"], b["scores"]) and torch.equal(a["classIds"], b["classIds"])
    u = out[0]["uncertainty"]
    pix = cached[3].long()
    want = raw.double() * torch.exp(-torch.exp(torch.gather(u.reshape(B, -1), 1, pix).double()))
    e = _rel(a["scores"].cpu().numpy(), want.cpu().numpy())
    # against FLOAT64 there is no fp32 reference in between: the reference's own distance from float64 (e_ref) plus ours from the
    # reference (4 * e_ref, the bound above) - the model's u at its peaks lies in the fixture's range (same weights, same inputs)
    print(f"[uncertainty] model's own maps: max rel. deviation from float64 {e:.3e} (bound 5 * e_ref = {F64_BOUND * float(golden['e_ref']):.3e})")
    assert e <= F64_BOUND * float(golden["e_ref"])
    assert bool((a["scores"] < raw).all())                         # weighted at all (exp(-exp(u)) < 1)
    # in-place write after the forward: one pixel far above every peak, in image 1, at a pixel with a known u
    with torch.no_grad():
        heat[1, 3, 17, 23] = 0.999
    c = fusionDecode(out, outputSize=OUT_HW, K=K)
    assert float(c["classIds"][1, 0]) == 3.0
    assert np.array_equal(c["centers"][1, 0].cpu().numpy(), np.array([23 / OUT_HW[1], 17 / OUT_HW[0]], np.float32))
    want0 = float(np.float64(np.float32(0.999)) * np.exp(-np.exp(np.float64(float(u[1, 0, 17, 23])))))
    assert abs(float(c["scores"][1, 0]) - want0) <= F64_BOUND * float(golden["e_ref"]) * want0
    assert torch.equal(c["scores"][0], a["scores"][0])             # image 0 is untouched
    d = fusionDecode(out, outputSize=OUT_HW, K=K)
    assert torch.equal(c["scores"], d["scores"])


def test_detector_process_end_to_end(dev, golden, forward):
    from centerfusiondetect3d_amd import Detector
    from centerfusiondetect3d_amd.postprocess import unpack_post
    x, pc_dep, calib = uncertainty_inputs()
    m = forward["heads_bf16"][0]
    det = Detector(_cfg(), model=m, device=dev)
    meta = {"center": np.array([800.0, 450.0], np.float32), "scale": 1600.0}
    outputs, post = det.process(x.to(dev), calib.to(dev), pc_dep.to(dev), meta)
    assert post.shape == (B, K, 54) and "uncertainty" in outputs[0]
    fields = {k: v.cpu() for k, v in unpack_post(post).items()}
    raw = outputs[0]["heatmap"]._cf_peaks[2]
    assert bool((fields["scores"] < raw.cpu()).all()) and bool((fields["scores"] > 0).all())
    boxes = det.merge_outputs(fields)                              # `score > -1` and everything behind it: no special case
    assert len(boxes) == B and all(len(b) > 0 for b in boxes)
