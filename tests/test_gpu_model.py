"""GPU parity, module level: DLASeg.forward + fusionDecode on the HIP path against (a) the golden
vectors produced by the reference's own forward and (b) the CPU oracle, through the drop-in
boundary `model(images, pc_dep=, calib=) -> [dict]`.

Tolerance (north star "within 1e-3 relative fp32"): per element
    |got - ref| <= 1e-3*|ref| + A*max|ref|,      A = max(2e-4, 3*e32 + 2e-5)
where e32 is MEASURED in the test itself: the max-norm error of the fp32 oracle (= the reference's own
fp32 arithmetic) against the same oracle evaluated in float64 on the same inputs.  Why e32 enters: `ref`
is an fp32 evaluation, and two correct fp32 evaluations of this network can differ by the sum of their
own errors - the DCN neck amplifies rounding ~100x at samples that sit on a cell or image border, so
e32 is ~1e-5 at small sizes and up to ~1e-4 in the worst of ~10^6 elements at 448x800.  The HIP path is
separately held to |hip - fp64| <= 2*e32 + 2e-5 and RMS <= max(1.25x the fp32 oracle's, 5e-5 of the output's RMS)
(test_accuracy_anchored_on_float64 on the bench configuration itself; test_accuracy_gate_holds_on_every_weight_draw on four draws), which gives 3*e32 + 2e-5 against
`ref` by the triangle inequality.  Where no float64 run is made the floor A = 2e-4 applies.  Both numbers
(observed error, allowed A) are printed (pytest -s).  The index path (top-k, painted pixel set) must be
identical."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import model_ref, decode_ref
from tests.golden import cases

RTOL = 1e-3
ATOL_FLOOR = 2e-4
# The float64-anchored gate (test_accuracy_anchored_on_float64, test_accuracy_gate_holds_on_every_weight_draw), per output,
# errors against the float64 oracle, r = RMS error / RMS of the output, e = worst element / max |output|:
#     r_hip <= max(1.25 * r_fp32 + 2e-6, 5e-5)     and     e_hip <= 2 * e_fp32 + 2e-5
# i.e. EITHER as close to float64 as the reference's own fp32 arithmetic (the fp32 oracle) within 25 %, OR - on draws where
# the fp32 oracle itself happens to be right to ~1e-5 and any other correct arithmetic shows beside it - inside an absolute
# floor of 5e-5 of the output's RMS, 20 x inside the north star's 1e-3.  The floor does not depend on the draw; the ratio
# does (0.8-1.8 over weight seeds 0-3 for BOTH head arithmetics: docs/experiments/r5_heads_mx_numerics.txt).
GATE_RMS_RATIO, GATE_RMS_FLOOR = 1.25, 5e-5


def _gate(k, r_gpu, r_cpu, e_gpu, e_cpu):
    assert r_gpu <= max(GATE_RMS_RATIO * r_cpu + 2e-6, GATE_RMS_FLOOR), (k, r_gpu, r_cpu)
    assert e_gpu <= 2.0 * e_cpu + 2e-5, (k, e_gpu, e_cpu)


def _atol(e32=None):
    return ATOL_FLOOR if e32 is None else max(ATOL_FLOOR, 3.0 * e32 + 2e-5)


def _fp32_noise(sd, x, pc_dep, calib, radar, ref32=None):
    """{output: max-norm error of the fp32 oracle against the float64 oracle} on these inputs.  The float64
    run shares the fp32 run's frustum map (discrete decisions), so only arithmetic differs."""
    from oracle import frustum_ref
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    with torch.no_grad():
        r32 = ref32 if ref32 is not None else model_ref.forward(sd, x, pc_dep=pc_dep, calib=calib, radar=radar)[0]
        hm = frustum_ref.pc_frustum_heatmap(r32, pc_dep, calib, 100, 60.0) if radar else None
        r64 = model_ref.forward(sd64, x.double(), pc_dep=pc_dep.double() if radar else None, calib=calib,
                                radar=radar, pc_hm_override=hm)[0]
    noise = {}
    for k, t in r64.items():
        if k == "calib":
            continue
        noise[k] = float((r32[k].double() - t).abs().max()) / (float(t.abs().max()) + 1e-300)
    return noise, r32, r64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _model(radar, dev, input_size):
    from centerfusiondetect3d_amd import getModel, centerfusion_middle_config, centernet_config
    cfg = (centerfusion_middle_config if radar else centernet_config)(input_size)
    m = getModel(cfg)
    m.load_state_dict(cases.tuned_state_dict(radar=radar, seed=0), strict=True)
    return m.to(dev).eval()


def _assert_maps_close(got, ref, name, e32=None, scale=None):
    """e32: measured fp32-vs-float64 error of this output (see the module docstring); scale: max|ref| of the
    WHOLE map when `ref` is a sample of it."""
    got = got.detach().cpu().numpy()
    ref = ref.numpy() if isinstance(ref, torch.Tensor) else ref
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = (float(np.abs(ref).max()) if scale is None else float(scale)) + 1e-12
    err = np.abs(got - ref)
    a = _atol(e32)
    tol = RTOL * np.abs(ref) + a * scale
    assert (err <= tol).all(), f"{name}: max err {err.max():.3e} (scale {scale:.3e}, allowed A {a:.2e}), " \
                               f"{int((err > tol).sum())} / {err.size} outside 1e-3"
    print(f"[parity] {name:>16s}: max|err|/max|ref| = {err.max() / scale:.2e}  (allowed abs term {a:.2e}"
          + (f", fp32-vs-fp64 {e32:.2e})" if e32 is not None else ", floor)"))
    return float(err.max() / scale)


@pytest.mark.parametrize("radar,B,H,W", [(False, 1, 256, 416), (True, 2, 448, 800), (False, 1, 448, 800)],
                         ids=["centernet_256x416", "centerfusion_middle_448x800_bs2",
                              "centernet_448x800_bs1_BASELINE_config1_shape"])
def test_accuracy_anchored_on_float64(dev, radar, B, H, W):
    """The yardstick that does not depend on anybody's fp32 rounding: the oracle evaluated in float64.
    The HIP path must be as close to it as the reference's own fp32 arithmetic (the fp32 oracle) is -
    RMS error within 1.25x or inside 5e-5 of the output's RMS, worst element within 2x (+ a floor): `_gate` above - on
    EVERY output, including the secondary heads (three chained split-bf16 layers behind the frustum map)
    of the configuration bench.py measures (Centerfusion_Middle, 448x800).  On that configuration the exact-fp32 build
    (`conv_f16 = False`, `heads_bf16 = False`: cf_conv2d_fused / cf_dcn_v2_fused everywhere) is held to the same bounds."""
    from centerfusiondetect3d_amd import getModel, centernet_config, centerfusion_middle_config
    sd = cases.tuned_state_dict(radar=radar, seed=0)
    x, pc_dep, calib = cases.model_inputs(B, H, W, seed=5, radar=radar, n_points=(80, 200))
    noise, r32, r64 = _fp32_noise(sd, x, pc_dep, calib, radar)
    builds = [("hip", {})]
    if (radar, B, H, W) == (True, 2, 448, 800):
        # the exact-fp32 build (bench.py --exact-fp32, C2_exact_fp32) at a size where its tiles are the benchmark's: at B = 2 the
        # heads have 44,800 pixels and run the 128x128 plain form of cf_conv2d_fused; same oracle runs, same constants
        builds.append(("exact-fp32", dict(conv_f16=False, heads_bf16=False)))
    for tag, flags in builds:
        m = getModel((centerfusion_middle_config if radar else centernet_config)((H, W)))
        for k, v in flags.items():
            setattr(m, k, v)
        m.load_state_dict(sd)
        m = m.to(dev).eval()
        with torch.no_grad():
            y = m(x.to(dev), pc_dep=pc_dep.to(dev) if radar else None, calib=calib.to(dev))[0]
        if flags:
            launched = {st[0].__name__ for plan in m._all_plans() for st in plan.steps if st and not isinstance(st[0], str)}
            assert "cf_conv2d_fused" in launched and "cf_dcn_v2_fused" in launched and "cf_head_fused" not in launched
        if not radar:
            assert len(m.heads) == 9 and set(r64) <= set(y)           # CenterNet.yaml: 9 heads, one hidden layer each, no radar
        if radar:
            # discrete path first: same painted map as the fp32 oracle, bit for bit
            assert torch.equal(y["pc_hm"].cpu(), r32["pc_hm"]) and int((r32["pc_hm"] != 0).sum()) > 0
        for k, t in r64.items():
            if k == "calib":
                continue
            g, c = y[k].double().cpu(), r32[k].double()
            scale = float(t.abs().max()) + 1e-300
            rms = float(t.pow(2).mean().sqrt()) + 1e-300
            e_gpu, e_cpu = float((g - t).abs().max()) / scale, float((c - t).abs().max()) / scale
            r_gpu, r_cpu = float((g - t).pow(2).mean().sqrt()) / rms, float((c - t).pow(2).mean().sqrt()) / rms
            print(f"[fp64 {tag}] {k:>16s}: max-norm hip {e_gpu:.2e} fp32-oracle {e_cpu:.2e} | rms hip {r_gpu:.2e} fp32-oracle {r_cpu:.2e}")
            _gate(k, r_gpu, r_cpu, e_gpu, e_cpu)
            _assert_maps_close(y[k], r32[k], k, e32=noise[k])
        del m, y


_DRAWS = {}      # weight seed -> (sd, inputs, fp32 oracle, float64 oracle): the two oracle runs serve both head arithmetics


@pytest.mark.parametrize("heads_mx", [True, False], ids=["fp16_fp6_first_layers", "bf16x3"])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_accuracy_gate_holds_on_every_weight_draw(dev, seed, heads_mx):
    """The float64-anchored gate over four weight / input draws (the seeds, inputs and size of tests/tools/eval_mx_gate_gpu.py: the
    bench configuration's shape at one frame), for the default head arithmetic AND for `heads_mx = False` - a gate that is only run
    on the draw it passes is not evidence.  Draw 3 is the one where the neck amplifies least, the fp32
    oracle is right to ~1e-5 of an output's RMS and the RMS ratio reaches 1.4 (bf16x3) / 1.8 (fp16 + FP6) at errors of
    1.6e-5: inside the criterion through its absolute floor, which is what the criterion is for."""
    from centerfusiondetect3d_amd import getModel, centerfusion_middle_config
    from oracle import frustum_ref
    H, W, B = 448, 800, 1
    if seed not in _DRAWS:
        sd = cases.tuned_state_dict(radar=True, seed=seed)
        x, pc_dep, calib = cases.model_inputs(B, H, W, seed=100 + seed, radar=True, n_points=(80, 200))
        noise, r32, r64 = _fp32_noise(sd, x, pc_dep, calib, True)
        _DRAWS[seed] = (sd, x, pc_dep, calib, r32, r64)
    sd, x, pc_dep, calib, r32, r64 = _DRAWS[seed]
    m = getModel(centerfusion_middle_config((H, W)))
    m.heads_mx = heads_mx
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    with torch.no_grad():
        y = m(x.to(dev), pc_dep=pc_dep.to(dev), calib=calib.to(dev))[0]
    assert torch.equal(y["pc_hm"].cpu(), r32["pc_hm"])
    worst = 0.0
    for k, t in r64.items():
        if k in ("calib", "pc_hm", "pc_hm_in", "pc_hm_out"):
            continue
        g, c = y[k].double().cpu(), r32[k].double()
        scale, rms = float(t.abs().max()) + 1e-300, float(t.pow(2).mean().sqrt()) + 1e-300
        r_gpu, r_cpu = float((g - t).pow(2).mean().sqrt()) / rms, float((c - t).pow(2).mean().sqrt()) / rms
        e_gpu, e_cpu = float((g - t).abs().max()) / scale, float((c - t).abs().max()) / scale
        worst = max(worst, r_gpu / (r_cpu + 1e-300))
        print(f"[gate seed {seed} mx={int(heads_mx)}] {k:>14s}: rms hip {r_gpu:.2e} fp32-oracle {r_cpu:.2e} (ratio {r_gpu / r_cpu:.2f}) | "
              f"max hip {e_gpu:.2e} fp32-oracle {e_cpu:.2e}")
        _gate(k, r_gpu, r_cpu, e_gpu, e_cpu)
    print(f"[gate seed {seed} mx={int(heads_mx)}] worst RMS ratio {worst:.2f}")


@pytest.mark.parametrize("tag,radar,B,H,W", [("centerfusion_small", True, 2, 128, 160),
                                             ("centernet_small", False, 1, 96, 128)])
def test_forward_matches_reference_golden(dev, golden_dir, tag, radar, B, H, W):
    g = np.load(os.path.join(golden_dir, f"model_{tag}.npz"))
    m = _model(radar, dev, (H, W))
    x, pc_dep, calib = cases.model_inputs(B, H, W, seed=1, radar=radar)
    pc_d = pc_dep.to(dev) if radar else None
    with torch.no_grad():
        out = m(x.to(dev), pc_dep=pc_d, calib=calib.to(dev))
    assert isinstance(out, list) and len(out) == 1
    y = out[0]
    assert list(y.keys()) == [str(k) for k in g["key_order"]]
    for k, v in y.items():
        if k == "calib":
            assert torch.equal(v.cpu(), calib)
            continue
        assert v.is_cuda and v.dtype == torch.float32
        _assert_maps_close(v, g[f"out_{k}"], k)
    if radar:
        # integer paint geometry: identical pixel set, and the view contract of detectHeads.py:172
        assert np.array_equal((y["pc_hm"] != 0).cpu().numpy(), g["out_pc_hm"] != 0)
        assert int((y["pc_hm"] != 0).sum()) == int(g["n_painted"]) > 0
        assert y["pc_hm_in"].data_ptr() == pc_d.data_ptr()
    # a fresh dict with fresh tensors every call (consumers mutate it, decode.py:120-121)
    with torch.no_grad():
        out2 = m(x.to(dev), pc_dep=pc_d, calib=calib.to(dev))
    assert out2[0] is not y and out2[0]["heatmap"].data_ptr() != y["heatmap"].data_ptr()
    for k in y:
        if k not in ("calib",):
            assert torch.equal(out2[0][k], y[k]), f"{k}: forward is not deterministic"


@pytest.mark.parametrize("flags", [dict(heads_mx=False), dict(pack_mx_fused=False), dict(proj_fuse=False, stem_pool=False),
                                   dict(conv_patch=False), dict(heads_bf16=False), dict(conv_f16=False, heads_bf16=False)],
                         ids=["heads_bf16x3", "separate_pack_pass", "project_and_pool_launches", "slot_kernels_only",
                              "exact_fp32_heads", "exact_fp32_build"])
def test_forward_matches_reference_golden_on_the_switchable_head_paths(dev, golden_dir, flags):
    """(also: `proj_fuse = False`, `stem_pool = False` - the four `project` convolutions and the level-2 max-pool as their own
    launches, bench.py --no-proj-fuse --no-stem-pool - and `conv_patch = False` - every f16x3 convolution on the slot kernel, conv2 + project from its two-source
    slot table - against the same goldens; `heads_bf16 = False`: the exact-fp32 layer-by-layer heads, also what a head with more than
    16 outputs gets; with `conv_f16 = False` the exact-fp32 build of bench.py --exact-fp32.)
    the A/B switches of the heads' first layer keep working at module level: `heads_mx = False` (bf16x3, the round-4
    arithmetic - bench.py --heads-bf16x3) against the reference's golden outputs with the same tolerance, and
    `pack_mx_fused = False` (cf_pack_feat_mx as its own launch instead of the DCN epilogue): same tolerance, and bit-identical to the
    default wherever the producing DCN does not split K"""
    from centerfusiondetect3d_amd import getModel, centerfusion_middle_config
    B, H, W = 2, 128, 160
    g = np.load(os.path.join(golden_dir, "model_centerfusion_small.npz"))
    x, pc_dep, calib = cases.model_inputs(B, H, W, seed=1, radar=True)
    m = getModel(centerfusion_middle_config((H, W)))
    for k, v in flags.items():
        setattr(m, k, v)
    m.load_state_dict(cases.tuned_state_dict(radar=True, seed=0), strict=True)
    m = m.to(dev).eval()
    with torch.no_grad():
        y = m(x.to(dev), pc_dep=pc_dep.to(dev), calib=calib.to(dev))[0]
        ref = _model(True, dev, (H, W))(x.to(dev), pc_dep=pc_dep.to(dev), calib=calib.to(dev))[0]
    assert m._mx_active == (bool(flags.get("heads_mx", True)) and bool(flags.get("heads_bf16", True)))
    launched = {st[0].__name__ for plan in m._all_plans() for st in plan.steps if st and not isinstance(st[0], str)}
    assert ("cf_head_fused" in launched) == bool(flags.get("heads_bf16", True))
    names = {n for plan in m._all_plans() for n in plan.step_index}
    # the heads' mx rows come out of the feature map's DCN epilogue unless that is switched off (round 6 lost this for single-plan
    # forwards for a few commits: an extra launch that every parity test passes - so it is pinned here)
    assert ("feat.pack_mx" in names) == (m._mx_active and not (flags.get("pack_mx_fused", True) and flags.get("conv_f16", True)))
    proj_fused = flags.get("proj_fuse", True) and flags.get("conv_f16", True)      # (the exact-fp32 build fuses nothing)
    assert any(n.endswith(".project") for n in names) == (not proj_fused)
    assert any(n.endswith(".conv2+project") for n in names) == proj_fused
    for k, v in y.items():
        if k == "calib":
            continue
        _assert_maps_close(v, g[f"out_{k}"], k)
    assert np.array_equal((y["pc_hm"] != 0).cpu().numpy(), g["out_pc_hm"] != 0)
    del ref
    if "pack_mx_fused" in flags:
        # (at 32 x 40 the feature map's DCN splits K unless it writes the rows itself, so the two forms differ in rounding
        #  there; on a map above the K-split size they are the same arithmetic: bit-identical)
        H2, W2 = 192, 256
        x2, pc2, cal2 = cases.model_inputs(1, H2, W2, seed=2, radar=True)
        outs = []
        for fused in (True, False):
            m2 = getModel(centerfusion_middle_config((H2, W2)))
            m2.pack_mx_fused = fused
            m2.load_state_dict(cases.tuned_state_dict(radar=True, seed=0), strict=True)
            m2 = m2.to(dev).eval()
            with torch.no_grad():
                outs.append(m2(x2.to(dev), pc_dep=pc2.to(dev), calib=cal2.to(dev))[0])
        for k in outs[0]:
            if k != "calib":
                assert torch.equal(outs[0][k], outs[1][k]), k


def test_decoder_peaks_travel_with_the_heat_map(dev):
    """model.heads_lanes: the forward computes the decoder's NMS + top-k on a side stream and hands it to decode.py through the
    heat map tensor, with a checksum of the bits the peaks were computed from.  The decoded rows must be the ones decode
    computes by itself; the hand-over must lapse when K differs or the tensor is replaced; and ANY in-place change of the map
    between forward and fusionDecode - an ordinary one, or one through `heat.data`, which no version counter sees (VERDICT r5
    item 6) - must be honoured: decode re-sums the map and its top-k launches recompute on the device when the sums differ
    (the reference's fusionDecode always reads the map it is given, model/decode.py:38-57).  `heads_lanes = False` must give
    the same maps."""
    from centerfusiondetect3d_amd import decode_packed, ops
    H, W, B = 128, 160, 3
    m = _model(True, dev, (H, W))
    x, pc_dep, calib = cases.model_inputs(B, H, W, seed=4, radar=True)

    def forward():
        with torch.no_grad():
            return m(x.to(dev), pc_dep=pc_dep.to(dev), calib=calib.to(dev))

    def fresh(o):                                                 # what decode computes from scratch for these maps
        ref = dict(o)
        ref["heatmap"] = o["heatmap"].clone()
        assert getattr(ref["heatmap"], "_cf_peaks", None) is None   # a replaced tensor carries nothing
        return decode_packed([ref], (H // 4, W // 4), K=100)[0]

    out = forward()
    hm = out[0]["heatmap"]
    assert m.heads_lanes and getattr(hm, "_cf_peaks", None) is not None
    K, ptr, s_c, i_c, c_c, sums = hm._cf_peaks
    assert K == 100 and ptr == hm.data_ptr()
    s_r, i_r, c_r = ops.topk_peaks(hm, K, nms=True)
    assert torch.equal(s_c, s_r) and torch.equal(i_c, i_r) and torch.equal(c_c, c_r)
    assert sums.shape == (2 * ops.CHECKSUM_PARTS,) and torch.equal(sums[:ops.CHECKSUM_PARTS], ops.checksum64(hm)) and int(sums[0]) != 0
    det_plain = fresh(out[0])
    det_cached, _ = decode_packed([dict(out[0])], (H // 4, W // 4), K=K)
    assert torch.equal(det_cached, det_plain)
    assert torch.equal(s_c, s_r) and torch.equal(i_c, i_r)        # (unchanged map: the conditional launches left the peaks alone)
    det_k, _ = decode_packed([dict(out[0])], (H // 4, W // 4), K=K // 2)     # another K: computed afresh
    assert torch.equal(det_k, det_plain[:, :K // 2])

    # in-place changes between forward and decode, by four routes; each must decode like a fresh tensor with the same contents
    def new_peak(t):                                              # a peak that was not there: class 3 at (5, 7) of image 1
        t[1, 3, 5, 7] = 0.99

    for name, mutate in (("mul_", lambda t: t.mul_(0.5)),
                         (".data.mul_", lambda t: t.data.mul_(0.5)),
                         (".data new peak", lambda t: new_peak(t.data)),
                         (".data swap", lambda t: t.data.copy_(t.data.flip(0)))):   # same multiset of values: a plain sum is blind to it
        o = forward()[0]
        h = o["heatmap"]
        before = decode_packed([dict(o)], (H // 4, W // 4), K=K)[0].clone()
        v0 = h._version
        mutate(h)
        if name.startswith(".data"):
            assert h._version == v0, name                         # the hole: nothing autograd can see has changed
        got = decode_packed([dict(o)], (H // 4, W // 4), K=K)[0]
        assert torch.equal(got, fresh(o)), name
        assert not torch.equal(got[..., :2], before[..., :2]), name
    with torch.inference_mode():                                  # inference tensors carry the peaks as well (no version is needed)
        out_i = forward()
        assert getattr(out_i[0]["heatmap"], "_cf_peaks", None) is not None
        det_i, _ = decode_packed([dict(out_i[0])], (H // 4, W // 4), K=K)
    assert torch.equal(det_i, det_plain)
    m2 = _model(True, dev, (H, W))
    m2.heads_lanes = False
    m2.invalidate()
    with torch.no_grad():
        out2 = m2(x.to(dev), pc_dep=pc_dep.to(dev), calib=calib.to(dev))
    assert getattr(out2[0]["heatmap"], "_cf_peaks", None) is None
    for k in out2[0]:
        if k not in ("calib", "heatmap"):
            assert torch.equal(out2[0][k], out[0][k]), k


def test_forward_and_decode_fullres_vs_reference_samples(dev, golden_dir):
    from centerfusiondetect3d_amd import fusionDecode
    g = np.load(os.path.join(golden_dir, "model_centerfusion_fullres.npz"))
    m = _model(True, dev, (448, 800))
    x, pc_dep, calib = cases.model_inputs(1, 448, 800, seed=2, radar=True, n_points=(80, 200))
    with torch.no_grad():
        out = m(x.to(dev), pc_dep=pc_dep.to(dev), calib=calib.to(dev))
    y = out[0]
    noise, r32, _ = _fp32_noise(cases.tuned_state_dict(radar=True, seed=0), x, pc_dep, calib, True)
    for k, v in y.items():
        if k == "calib":
            continue
        assert tuple(v.shape[2:]) == (112, 200)
        flat = v.reshape(-1).cpu()
        _assert_maps_close(flat[g[f"idx_{k}"]], g[f"val_{k}"], k, e32=noise[k], scale=float(r32[k].abs().max()))
    assert int((y["pc_hm"] != 0).sum()) == int(g["n_painted"])
    det = fusionDecode(out, outputSize=(112, 200), K=100, norm2d=False)
    assert np.array_equal(det["classIds"].cpu().numpy(), g["det_classIds"])      # index path
    cx = (det["centers"][..., 0].cpu().numpy() * 200).round().astype(int)
    assert np.array_equal(cx, (g["det_centers"][..., 0] * 200).round().astype(int))
    for k, v in det.items():
        _assert_maps_close(v, g[f"det_{k}"], f"det_{k}")


def test_forward_matches_oracle_other_seed_and_ragged_radar(dev):
    """Oracle comparison on inputs the golden files do not hold: a frame with no radar at all,
    a dense one, different weights."""
    from centerfusiondetect3d_amd import getModel, centerfusion_middle_config
    H, W, B = 96, 160, 3
    sd = cases.tuned_state_dict(radar=True, seed=7)
    m = getModel(centerfusion_middle_config((H, W)))
    m.load_state_dict(sd)
    m = m.to(dev)
    x, pc_dep, calib = cases.model_inputs(B, H, W, seed=11, radar=True, n_points=(30, 31))
    pc_dep[1] = 0                                           # frame without radar returns
    with torch.no_grad():
        ref = model_ref.forward(sd, x, pc_dep=pc_dep, calib=calib)[0]
        y = m(x.to(dev), pc_dep=pc_dep.to(dev), calib=calib.to(dev))[0]
    for k in ref:
        if k != "calib":
            _assert_maps_close(y[k], ref[k], k)
    assert float(y["pc_hm"][1].abs().max()) == 0.0
    assert np.array_equal((y["pc_hm"] != 0).cpu().numpy(), (ref["pc_hm"] != 0).numpy())


def test_batch_sharding_is_bit_exact(dev):
    """Multi-GPU acceptance property on one device: a shard of the batch gives
    bit-identical head maps and detections to the same frames inside the full batch."""
    from centerfusiondetect3d_amd import decode_packed
    H, W, B = 128, 160, 4
    m = _model(True, dev, (H, W))
    x, pc_dep, calib = cases.model_inputs(B, H, W, seed=5, radar=True)
    xd, pd, cd = x.to(dev), pc_dep.to(dev), calib.to(dev)
    with torch.no_grad():
        full = m(xd, pc_dep=pd, calib=cd)
        det_full, _ = decode_packed(full, (H // 4, W // 4), 100)
        for lo, hi in ((0, 2), (2, 4), (1, 2)):
            part = m(xd[lo:hi].contiguous(), pc_dep=pd[lo:hi].contiguous(), calib=cd[lo:hi].contiguous())
            # `full` had rotation2 renamed by decode; compare before decoding the shard
            for k, v in part[0].items():
                kk = "rotation" if k == "rotation2" else k
                if k not in ("calib", "rotation"):
                    assert torch.equal(v, full[0][kk][lo:hi]), k
            det, _ = decode_packed(part, (H // 4, W // 4), 100)
            assert torch.equal(det, det_full[lo:hi])


def test_contract_errors(dev):
    from centerfusiondetect3d_amd import getModel, centerfusion_middle_config, _lib
    m = getModel(centerfusion_middle_config((64, 64))).to(dev)
    x = torch.zeros(1, 3, 64, 64, device=dev)
    with pytest.raises(ValueError):
        m(x)                                                 # radar model needs pc_dep / calib
    with pytest.raises(ValueError):
        m(torch.zeros(1, 3, 60, 64, device=dev), pc_dep=torch.zeros(1, 3, 15, 16, device=dev),
          calib=torch.zeros(1, 3, 4, device=dev))
    with pytest.raises(_lib.CfHipError):
        m.cpu()(torch.zeros(1, 3, 64, 64))                   # no CPU fallback
    m.train()
    with pytest.raises(NotImplementedError):
        m(x, pc_dep=torch.zeros(1, 3, 16, 16, device=dev), calib=torch.zeros(1, 3, 4, device=dev))


def test_config_c4_dcn_heavy_offsets(dev):
    """BASELINE config 4: every IDA node is deformable (the default topology) with offsets raised to
    O(8 px) so the bilinear gather leaves the 3x3 neighbourhood and crosses image borders."""
    from centerfusiondetect3d_amd import getModel, centerfusion_middle_config
    H, W, B = 128, 160, 2
    sd = model_ref.make_state_dict(radar=True, seed=3, offset_bias_std=8.0)
    sd["detectHead_0.depth.2.bias"].fill_(-3.0)
    sd["detectHead_0.dimension.2.bias"].copy_(torch.tensor([1.6, 1.9, 4.4]))
    sd["detectHead_0.widthHeight.2.bias"].copy_(torch.tensor([9.0, 7.0]))
    m = getModel(centerfusion_middle_config((H, W)))
    m.load_state_dict(sd)
    m = m.to(dev)
    x, pc_dep, calib = cases.model_inputs(B, H, W, seed=21, radar=True)
    with torch.no_grad():
        ref = model_ref.forward(sd, x, pc_dep=pc_dep, calib=calib)[0]
        y = m(x.to(dev), pc_dep=pc_dep.to(dev), calib=calib.to(dev))[0]
    for k in ref:
        if k != "calib":
            _assert_maps_close(y[k], ref[k], k)
    assert np.array_equal((y["pc_hm"] != 0).cpu().numpy(), (ref["pc_hm"] != 0).numpy())


def test_config_c5_highres_896x1600(dev):
    """BASELINE config 5 (nuScenes full resolution, maps 224x400): one frame against the oracle, and
    at bs=8 the size-independent properties - deterministic, shard == full batch bit for bit."""
    from centerfusiondetect3d_amd import getModel, centerfusion_middle_config, decode_packed
    H, W = 896, 1600
    sd = cases.tuned_state_dict(radar=True, seed=0)
    m = getModel(centerfusion_middle_config((H, W)))
    m.load_state_dict(sd)
    m = m.to(dev)
    x, pc_dep, calib = cases.model_inputs(8, H, W, seed=31, radar=True, n_points=(100, 200))
    xd, pd, cd = x.to(dev), pc_dep.to(dev), calib.to(dev)
    noise, ref, _ = _fp32_noise(sd, x[:1], pc_dep[:1], calib[:1], True)     # fp32 and float64 oracle, one frame
    with torch.no_grad():
        full = m(xd, pc_dep=pd, calib=cd)
        one = m(xd[:1].contiguous(), pc_dep=pd[:1].contiguous(), calib=cd[:1].contiguous())
        again = m(xd, pc_dep=pd, calib=cd)
    for k, v in ref.items():
        if k == "calib":
            continue
        assert tuple(full[0][k].shape[2:]) == (224, 400)
        _assert_maps_close(one[0][k], v, k, e32=noise[k])
        assert torch.equal(one[0][k], full[0][k][:1]), k
        assert torch.equal(again[0][k], full[0][k]), k
    det, _ = decode_packed(full, (224, 400), 100)
    det1, _ = decode_packed(one, (224, 400), 100)
    assert torch.equal(det1, det[:1]) and bool(torch.isfinite(det).all())


def test_config_c2_full_size_properties(dev):
    """BASELINE config 2 at its full size (bs=16, 448x800): shards of the batch reproduce the full
    batch bit for bit (what makes the 8-GPU data-parallel run equal to the single-GPU one), and
    frame order is respected (a permuted batch gives permuted outputs)."""
    from centerfusiondetect3d_amd import decode_packed
    H, W, B = 448, 800, 16
    m = _model(True, dev, (H, W))
    x, pc_dep, calib = cases.model_inputs(B, H, W, seed=41, radar=True, n_points=(50, 200))
    xd, pd, cd = x.to(dev), pc_dep.to(dev), calib.to(dev)
    with torch.no_grad():
        full = m(xd, pc_dep=pd, calib=cd)
        det_full, _ = decode_packed(full, (112, 200), 100)
        perm = torch.arange(B - 1, -1, -1, device=dev)
        rev = m(xd[perm].contiguous(), pc_dep=pd[perm].contiguous(), calib=cd[perm].contiguous())
        det_rev, _ = decode_packed(rev, (112, 200), 100)
        assert torch.equal(det_rev, det_full[perm])
        for lo, hi in ((0, 2), (8, 16)):
            part = m(xd[lo:hi].contiguous(), pc_dep=pd[lo:hi].contiguous(), calib=cd[lo:hi].contiguous())
            det, _ = decode_packed(part, (112, 200), 100)
            assert torch.equal(det, det_full[lo:hi])
        # shards of 1 / 2 / 4 frames take the small-grid tiles (half-height 3x3 tiles, 64-pixel DCN tiles: the tile
        # shape follows the launch size, the K order does not) - every output map bit for bit, not only the decode
        ref_maps = m(xd, pc_dep=pd, calib=cd)
        for lo, hi in ((5, 6), (6, 8), (12, 16)):
            part = m(xd[lo:hi].contiguous(), pc_dep=pd[lo:hi].contiguous(), calib=cd[lo:hi].contiguous())
            for k, v in part[0].items():
                assert torch.equal(v, ref_maps[0][k][lo:hi]), (k, lo, hi)
    assert int((full[0]["pc_hm"] != 0).sum()) > 0
    # ... and frames of the bs=16 batch against the oracle (not only against the HIP path itself); `full` had
    # rotation2 renamed to rotation by the decode above, as the reference's decode does
    sd = cases.tuned_state_dict(radar=True, seed=0)
    for f in (3, 12):
        sl = slice(f, f + 1)
        noise, r32, _ = _fp32_noise(sd, x[sl], pc_dep[sl], calib[sl], True)
        for k, v in r32.items():
            if k in ("calib", "rotation"):
                continue
            kk = "rotation" if k == "rotation2" else k
            _assert_maps_close(full[0][kk][sl], v, f"frame{f}.{k}", e32=noise[k])
        assert torch.equal(full[0]["pc_hm"][sl].cpu(), r32["pc_hm"])


def test_forward_is_reproducible_behind_unrelated_kernels(dev):
    """Glitch stress (tools/stress_model.py, shortened): the forward is deterministic by construction,
    so every repetition must reproduce the first bit for bit - also when an unrelated GEMM or a large
    fill runs in between and changes cache / LDS / timing state.  (This is the test that caught a
    scheduling-dependent 4-pixel glitch in an earlier form of the f16x3 DCN kernel, which plain
    back-to-back repetitions never showed.)"""
    H, W, B = 448, 800, 16
    m = _model(True, dev, (H, W))
    x, pc_dep, calib = cases.model_inputs(B, H, W, seed=43, radar=True, n_points=(50, 200))
    xd, pd, cd = x.to(dev), pc_dep.to(dev), calib.to(dev)
    noise = torch.randn(4096, 4096, device=dev)
    with torch.no_grad():
        ref = {k: v.clone() for k, v in m(xd, pc_dep=pd, calib=cd)[0].items()}
        for i in range(40):
            if i % 2:
                noise = (noise @ noise) * 1e-4
            else:
                torch.empty(64 << 20, device=dev).fill_(float(i))
            y = m(xd, pc_dep=pd, calib=cd)[0]
            for k in ref:
                assert torch.equal(y[k], ref[k]), f"forward {i}: {k} differs from the first forward"


@pytest.mark.parametrize("radar,B", [(True, 2), (False, 1)])
def test_graph_replay_equals_eager(dev, radar, B):
    """model.use_graph: the forward captured once as a HIP graph and replayed - same bits as the eager
    launches, fresh output tensors per call, `pc_hm_in` still a view of the caller's pc_dep, and new
    inputs really flow through the static buffers."""
    H, W = 128, 160
    m = _model(radar, dev, (H, W))
    outs = {}
    for seed in (11, 12):
        x, pc_dep, calib = cases.model_inputs(B, H, W, seed=seed, radar=radar)
        xd, pd, cd = x.to(dev), (pc_dep.to(dev) if radar else None), calib.to(dev)
        with torch.no_grad():
            m.use_graph = False
            eager = m(xd, pc_dep=pd, calib=cd)[0]
            m.use_graph = True
            graph = m(xd, pc_dep=pd, calib=cd)[0]
            again = m(xd, pc_dep=pd, calib=cd)[0]
        assert list(graph.keys()) == list(eager.keys())
        for k in eager:
            if k == "calib":
                assert graph[k].data_ptr() == eager[k].data_ptr() == cd.data_ptr()
                continue
            assert torch.equal(graph[k], eager[k]), (seed, k)
            assert torch.equal(again[k], eager[k]), (seed, k)
            if k != "pc_hm_in":
                assert again[k].data_ptr() != graph[k].data_ptr(), k       # fresh tensors every call
        if radar:
            assert graph["pc_hm_in"].data_ptr() == pd.data_ptr()
            assert graph["pc_hm"].data_ptr() == graph["pc_hm_out"].data_ptr()      # aliases stay aliases
        outs[seed] = eager["heatmap"].clone()
    assert not torch.equal(outs[11], outs[12])
    m.use_graph = False


def test_two_stream_forward_equals_single_stream(dev):
    """model.streams = 2 (the default for batches >= 8): backbone + neck as two sub-batches with their own plans on
    concurrent HIP streams, heads for the whole batch on the caller's stream - bit for bit the single-stream result
    (also on repetition: no buffer is shared between the streams), views and aliases as in the single-stream dict;
    streams = 4 and a camera-only model likewise."""
    from centerfusiondetect3d_amd import decode_packed
    H, W, B = 448, 800, 16
    m = _model(True, dev, (H, W))
    assert m.streams == 2
    x, pc_dep, calib = cases.model_inputs(B, H, W, seed=45, radar=True, n_points=(50, 200))
    xd, pd, cd = x.to(dev), pc_dep.to(dev), calib.to(dev)
    with torch.no_grad():
        m.streams = 1
        one = m(xd, pc_dep=pd, calib=cd)
        det1, _ = decode_packed([dict(one[0])], (112, 200), 100)     # (decode renames rotation2 in the dict it gets)
        m.min_sub_batch = 4                                       # (the default, 6, would not split 16 frames four ways)
        for n_streams in (2, 4):
            m.streams = n_streams
            for rep in range(3):
                two = m(xd, pc_dep=pd, calib=cd)
                assert list(two[0].keys()) == list(one[0].keys())
                for k in one[0]:
                    assert two[0][k].shape == one[0][k].shape, k
                    assert torch.equal(two[0][k], one[0][k]), (n_streams, rep, k)
                det2, _ = decode_packed([dict(two[0])], (112, 200), 100)
                assert torch.equal(det1, det2)
            assert two[0]["pc_hm_in"].data_ptr() == pd.data_ptr()
            assert two[0]["pc_hm"].data_ptr() == two[0]["pc_hm_out"].data_ptr()
        assert any(isinstance(k, tuple) and "trunk" in k for k in m._plans)     # the split path really ran
    mc = _model(False, dev, (256, 416))
    xc = cases.model_inputs(8, 256, 416, seed=46, radar=False)[0].to(dev)
    mc.min_sub_batch = 1                                        # (counted in 448x800-frame equivalents: 4 frames of 256x416 = 1.2)
    with torch.no_grad():
        mc.streams = 1
        a = mc(xc)[0]
        mc.streams = 2
        b = mc(xc)[0]
    assert any("trunk" in k for k in mc._plans)
    for k in a:
        if k != "calib":
            assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("tag,radar,B,H,W", [("centerfusion_small", True, 2, 128, 160),
                                             ("centernet_small", False, 1, 96, 128)])
def test_stage_buffers_match_reference_submodules(dev, golden_dir, tag, radar, B, H, W):
    """The HIP path's intermediate maps (plan.debug, NHWC) against values the REFERENCE's own sub-modules
    produced (`base` levels 1-5, the DLA-up maps, the feature map; level0 never leaves LDS in the fused stem)."""
    g = np.load(os.path.join(golden_dir, f"model_{tag}.npz"))
    m = _model(radar, dev, (H, W))
    x, pc_dep, calib = cases.model_inputs(B, H, W, seed=1, radar=radar)
    with torch.no_grad():
        m(x.to(dev), pc_dep=pc_dep.to(dev) if radar else None, calib=calib.to(dev))
    plan = list(m._plans.values())[-1]
    dbg = dict(plan.debug)
    dbg["feat"] = plan.feat
    checked = 0
    for n in (k[len("stage_val_"):] for k in g.files if k.startswith("stage_val_")):
        if n not in dbg:
            assert n == "y0"
            continue
        t = dbg[n].permute(0, 3, 1, 2).contiguous()
        assert list(t.shape) == g[f"stage_shape_{n}"].tolist(), n
        got = t.reshape(-1)[torch.from_numpy(g[f"stage_idx_{n}"]).to(dev)].cpu().numpy()
        ref = g[f"stage_val_{n}"]
        scale = float(np.abs(ref).max()) + 1e-12
        err = np.abs(got - ref)
        assert (err <= RTOL * np.abs(ref) + ATOL_FLOOR * scale).all(), (n, float(err.max() / scale))
        print(f"[stage] {n:>5s}: max|err|/max|ref| = {err.max() / scale:.2e}")
        checked += 1
    assert checked == 10


def test_one_model_two_streams_two_threads(dev):
    """Re-entrancy (SURVEY §8(b) "re-entrant per stream"): one model driven from two HIP streams, by two host
    threads at once - each stream gets its own plan (own intermediate buffers), so forwards in flight on different
    streams never share memory; results equal the sequential ones bit for bit."""
    import threading
    H, W, B = 128, 160, 2
    m = _model(True, dev, (H, W))
    ins = []
    for seed in (61, 62):
        x, pc_dep, calib = cases.model_inputs(B, H, W, seed=seed, radar=True)
        ins.append((x.to(dev), pc_dep.to(dev), calib.to(dev)))
    with torch.no_grad():
        want = [{k: v.clone() for k, v in m(a, pc_dep=b, calib=c)[0].items()} for a, b, c in ins]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    got = [None, None]
    errs = []

    def work(i):
        try:
            with torch.no_grad(), torch.cuda.stream(streams[i]):
                for _ in range(6):                                   # several forwards in flight per stream
                    got[i] = m(ins[i][0], pc_dep=ins[i][1], calib=ins[i][2])[0]
        except Exception as e:                                        # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    torch.cuda.synchronize()
    assert not errs, errs
    for i in range(2):
        for k, v in want[i].items():
            if k != "calib":
                assert torch.equal(got[i][k], v), (i, k)
    sids = {k[4] for k in m._plans if isinstance(k, tuple) and len(k) == 5}
    assert len(sids) >= 3                                             # default stream + the two side streams


@pytest.mark.parametrize("radar,B,H,W", [(True, 1, 448, 800), (True, 3, 128, 160), (False, 2, 96, 128), (True, 6, 448, 800)])
def test_two_lane_neck_equals_single_stream(dev, radar, B, H, W):
    """model.lanes (small batches): the IDA projections issued on a side stream beside the node chain - bit for bit
    the single-stream forward, also when repeated back to back (cross-lane events, no shared scratch)."""
    m = _model(radar, dev, (H, W))
    x, pc_dep, calib = cases.model_inputs(B, H, W, seed=71, radar=radar)
    xd, pd, cd = x.to(dev), (pc_dep.to(dev) if radar else None), calib.to(dev)
    with torch.no_grad():
        m.lanes = False
        one = m(xd, pc_dep=pd, calib=cd)[0]
        m.invalidate()
        m.lanes = True
        outs = [m(xd, pc_dep=pd, calib=cd)[0] for _ in range(4)]
    plan = list(m._plans.values())[-1]
    assert plan.use_lanes and 1 in plan.lanes
    for y in outs:
        for k in one:
            if k != "calib":
                assert torch.equal(y[k], one[k]), k


@pytest.mark.parametrize("radar,B,H,W", [(True, 1, 32, 32), (True, 5, 32, 96), (False, 2, 64, 32), (True, 1, 448, 128)])
def test_smallest_legal_inputs_and_portrait_shapes(dev, radar, B, H, W):
    """The smallest inputs the module accepts (H, W multiples of 32: level 5 is then a 1 x 1 .. 1 x 3 map, every kernel runs its
    ragged-tile / tiny-grid paths) and a portrait one, against the oracle; the decode of the HIP maps equals the oracle's decode
    of the SAME maps bit for bit (near-ties in the scores may order two arithmetics' own maps differently on maps this small)."""
    from centerfusiondetect3d_amd import fusionDecode
    sd = cases.tuned_state_dict(radar=radar, seed=0)
    m = _model(radar, dev, (H, W))
    x, pc_dep, calib = cases.model_inputs(B, H, W, seed=3, radar=radar, n_points=(2, 6))
    K = min(100, 10 * (H // 4) * (W // 4))
    with torch.no_grad():
        y = m(x.to(dev), pc_dep=pc_dep.to(dev) if radar else None, calib=calib.to(dev))
        ref = model_ref.forward(sd, x, pc_dep=pc_dep if radar else None, calib=calib, radar=radar)
    for k, v in ref[0].items():
        if k != "calib":
            _assert_maps_close(y[0][k], v, k)
    y_cpu = [{k: (v.cpu().clone() if torch.is_tensor(v) else v) for k, v in y[0].items()}]
    det = fusionDecode(y, outputSize=(H // 4, W // 4), K=K)
    det_ref = decode_ref.fusion_decode(y_cpu, (H // 4, W // 4), K)
    for k in ("scores", "classIds", "centers", "bboxes"):
        assert np.array_equal(det[k].cpu().numpy(), det_ref[k].numpy()), k


def test_plan_cache_is_an_lru_and_frees_evicted_buffers(dev):
    """A service that sees varying batch sizes must not keep one plan set (every intermediate buffer of a forward) per
    size for ever: at most `max_plan_sets` (default 4) live, the least recently used set is dropped whole and its memory
    returns to the allocator (VERDICT r2 weak 8 / ADVICE).  Results after re-building an evicted plan are unchanged."""
    H, W = 128, 160
    m = _model(True, dev, (H, W))
    assert m.max_plan_sets == 4
    x, pc_dep, calib = cases.model_inputs(8, H, W, seed=5, radar=True)
    xd, pd, cdv = x.to(dev), pc_dep.to(dev), calib.to(dev)
    mem, first = [], {}
    import gc
    gc.collect()                                   # models of earlier tests: their memory must not be freed under our feet
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    with torch.no_grad():
        for B in (8, 7, 6, 5, 4, 3, 2, 1):                       # descending: later sets are smaller
            out = m(xd[:B], pc_dep=pd[:B], calib=cdv[:B])[0]
            first[B] = out["heatmap"].clone()
            del out
            torch.cuda.synchronize()
            mem.append(torch.cuda.memory_allocated() - base - sum(t.numel() * 4 for t in first.values()))
            assert len(m._plan_sets) <= 4 and len({k[:5] for k in m._plans}) <= 4
        assert {k[0] for k in m._plans} == {1, 2, 3, 4}          # the four most recent batch sizes
        assert mem[-1] < mem[3], mem                             # 4 small sets take less than the 4 large ones did
        assert max(mem) <= 1.05 * mem[3], mem                    # never more than four sets alive
        again = m(xd[:8], pc_dep=pd[:8], calib=cdv[:8])[0]       # evicted -> rebuilt
        assert torch.equal(again["heatmap"], first[8])
        # graphs: the same bound, and a graph owns the plans it was captured with
        m.use_graph = True
        for B in (1, 2, 3, 4, 5, 6):
            g = m(xd[:B], pc_dep=pd[:B], calib=cdv[:B])[0]
            assert torch.equal(g["heatmap"], first[B]), B
            assert len(m._graphs) <= 4
        assert torch.equal(m(xd[:1], pc_dep=pd[:1], calib=cdv[:1])[0]["heatmap"], first[1])   # evicted graph re-captured


def test_no_captured_graph_is_collected_inside_a_capture(dev):
    """Collecting a torch.cuda.CUDAGraph that has become cyclic garbage while ANOTHER stream capture is under way aborts
    the process (its destructor destroys the graph while the runtime is in global capture mode; plain-torch reproducer:
    tools/repro_gc_capture.py graph -> rc 134, tensors / events survive).  That killed one full GPU suite run: the
    models of earlier tests are cyclic garbage, and torch.cuda.graph() no longer collects on entry by default.
    _forward_graph therefore (1) collects BEFORE the capture and (2) holds the collector off until it has ended - both
    checked here from inside the capture: the dead model's graph is already gone, and the collector is disabled."""
    import gc, weakref
    H, W = 96, 128
    x, _, calib = cases.model_inputs(1, H, W, seed=3, radar=False)
    xd, cdv = x.to(dev), calib.to(dev)
    gc.collect()
    was_on = gc.isenabled()
    gc.disable()                                 # nothing is collected behind this test's back
    seen = {}
    try:
        with torch.no_grad():
            a = _model(False, dev, (H, W))
            a.use_graph = True
            ref = a(xd, calib=cdv)[0]["heatmap"].clone()
            dead_graph = weakref.ref(next(iter(a._graphs.values()))[0])
            cyc = [a]
            cyc.append(cyc)                      # the first model is now reachable only through a cycle
            del a, cyc
            assert dead_graph() is not None      # ... and, with the collector off, still pending
            b = _model(False, dev, (H, W))
            b.use_graph = True
            eager = b._forward_eager

            def spy(*args, **kw):
                if torch.cuda.is_current_stream_capturing():
                    seen["graph_alive"] = dead_graph() is not None
                    seen["gc_enabled"] = gc.isenabled()
                return eager(*args, **kw)

            b._forward_eager = spy
            got = b(xd, calib=cdv)[0]["heatmap"]
        assert seen == {"graph_alive": False, "gc_enabled": False}, seen
        assert torch.equal(got, ref)
        assert not gc.isenabled()                # _forward_graph restores the state it found (off, here)
    finally:
        if was_on:
            gc.enable()
        gc.collect()
