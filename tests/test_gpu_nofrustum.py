"""GPU: middle fusion WITHOUT frustum association (MODEL.FRUSTUM = False; base_model.py:67-81, detectHeads.py:165-191) against
the fixture the reference's own forward produced (tests/golden/make_golden_nofrustum.py).

What is exact: the normalisation of the caller's radar map (in place, 1 - x / 60 with a true fp32 division: `pc_hm_in`, `pc_hm`,
`pc_hm_out`, the caller's tensor after one call and after a second call on the same tensor), the primary heads against the
FRUSTUM = True model (same kernels, same inputs), the decode of given maps.  The secondary heads are held to the criterion of
the module goldens (tests/test_gpu_model.py, `_assert_maps_close`, imported - not restated)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.golden import cases
from tests.golden.make_golden_nofrustum import nofrustum_inputs, B, H, W
from tests.test_gpu_model import _assert_maps_close

SECONDARY = ("velocity", "nuscenes_att", "depth2", "rotation2")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "model_centerfusion_nofrustum_small.npz"))


def _model(dev, frustum=False, size=(H, W), **flags):
    from centerfusiondetect3d_amd import getModel, centerfusion_middle_config
    cfg = centerfusion_middle_config(size)
    cfg.MODEL.FRUSTUM = frustum
    m = getModel(cfg)
    for k, v in flags.items():
        setattr(m, k, v)
    m.load_state_dict(cases.tuned_state_dict(radar=True, seed=0), strict=True)
    return m.to(dev).eval()


def _inside(view, t):
    lo = t.data_ptr()
    return lo <= view.data_ptr() < lo + t.numel() * t.element_size()


def test_fixture_inputs_hold_the_corner_values():
    _, pc_dep, _ = nofrustum_inputs()
    d = pc_dep[:, 0]
    assert int((d == 0).sum()) > 0 and int((d != 0).sum()) > 0 and int((d == 60).sum()) >= 2
    assert bool((pc_dep[:, 1][d == 0] != 0).any())           # a FILLED pixel (it carries a velocity) at depth exactly 0


def test_forward_matches_reference_golden_and_mutates_the_callers_map(dev, golden):
    g = golden
    m = _model(dev)
    x, pc_dep, calib = nofrustum_inputs()
    pc = pc_dep.to(dev)
    with torch.no_grad():
        out = m(x.to(dev), pc_dep=pc, calib=calib.to(dev))
    assert isinstance(out, list) and len(out) == 1
    y = out[0]
    assert list(y.keys()) == [str(k) for k in g["key_order"]]
    # the caller's tensor: normalised in place, once; empty pixels are 1.0 now
    assert np.array_equal(pc.cpu().numpy(), g["pc_dep_after"])
    assert np.array_equal(pc[:, 1:].cpu().numpy(), pc_dep[:, 1:].numpy())
    for k in ("pc_hm_in", "pc_hm", "pc_hm_out"):
        assert y[k].shape == g[f"out_{k}"].shape, k
        assert np.array_equal(y[k].cpu().numpy(), g[f"out_{k}"]), k
    assert y["pc_hm_in"].data_ptr() == pc.data_ptr() and _inside(y["pc_hm_in"], pc) and _inside(y["pc_hm"], pc)
    assert torch.equal(y["pc_hm_out"], y["pc_hm"]) and torch.equal(y["pc_hm_in"], pc[:, :1])
    first = {k: v.clone() for k, v in y.items()}
    for k, v in first.items():
        if k == "calib":
            assert torch.equal(v.cpu(), calib)
            continue
        assert v.is_cuda and v.dtype == torch.float32
        _assert_maps_close(v, g[f"out_{k}"], k)
    # launches: the direct pass instead of top-k + association, the head kernels as they were
    launched = [st[0].__name__ for plan in m._all_plans() for st in plan.steps if st and not isinstance(st[0], str)]
    assert launched.count("cf_pc_hm_direct") == 1 and launched.count("cf_head_fused") == 2
    assert not any(n in launched for n in ("cf_topk_frustum", "cf_frustum_assoc"))
    # the same tensor again: the reference normalises it a second time
    with torch.no_grad():
        y2 = m(x.to(dev), pc_dep=pc, calib=calib.to(dev))[0]
    assert np.array_equal(pc.cpu().numpy(), g["pc_dep_after2"])
    assert np.array_equal(y2["pc_hm"].cpu().numpy(), g["out2_pc_hm"])
    for k in ("depth2", "velocity"):
        _assert_maps_close(y2[k], g[f"out2_{k}"], f"second call {k}")
    for k in ("heatmap", "reg", "depth"):
        assert torch.equal(y2[k], first[k]), k


@pytest.mark.parametrize("flags", [dict(), dict(heads_mx=False), dict(heads_bf16=False)],
                         ids=["default", "heads_bf16x3", "exact_fp32_heads"])
def test_primary_heads_are_bit_identical_to_the_frustum_model(dev, golden, flags):
    x, pc_dep, calib = nofrustum_inputs()
    with torch.no_grad():
        a = _model(dev, frustum=True, **flags)(x.to(dev), pc_dep=pc_dep.to(dev), calib=calib.to(dev))[0]
        b = _model(dev, frustum=False, **flags)(x.to(dev), pc_dep=pc_dep.to(dev), calib=calib.to(dev))[0]
    assert list(a.keys()) == list(b.keys())
    for k in a:
        if k in SECONDARY or k in ("calib", "depthMap", "pc_hm", "pc_hm_in", "pc_hm_out"):
            continue
        assert torch.equal(a[k], b[k]), k
    for k in SECONDARY + ("depthMap",):                        # (every head arithmetic against the reference's outputs)
        _assert_maps_close(b[k], golden[f"out_{k}"], k)


def test_decode_of_the_nofrustum_outputs(dev, golden):
    """The decode tests' way (tests/test_gpu_ops.py): the SAME maps - here the reference's no-frustum outputs, from the fixture -
    through fusionDecode on the device, against what the reference's fusionDecode returned for them: every field bit for bit.
    (The model's own maps are decoded too and compared with the CPU oracle's decode of those very maps: on a 32 x 40 map with an
    almost flat random-weight heat map the top-100 scores lie 1e-5 apart, which is the fp32 noise of the network itself, so two
    correct evaluations of the NETWORK need not order them alike; the decode of given maps has no such freedom.)"""
    from centerfusiondetect3d_amd import fusionDecode
    from oracle import decode_ref
    g = golden
    maps = {str(k): torch.from_numpy(g[f"out_{k}"]).to(dev) for k in g["key_order"] if str(k) != "calib"}
    det = fusionDecode([maps], outputSize=(H // 4, W // 4), K=100, norm2d=False)
    ref_keys = {k[4:] for k in g.files if k.startswith("det_")}
    assert set(det.keys()) == ref_keys
    for k in ref_keys:
        assert np.array_equal(det[k].cpu().numpy(), g[f"det_{k}"]), k
    assert "rotation2" not in maps and "rotation" in maps
    m = _model(dev)
    x, pc_dep, calib = nofrustum_inputs()
    with torch.no_grad():
        out = m(x.to(dev), pc_dep=pc_dep.to(dev), calib=calib.to(dev))
        cpu = [{k: (v.cpu().clone() if torch.is_tensor(v) else v) for k, v in out[0].items()}]
        det_hip = fusionDecode(out, outputSize=(H // 4, W // 4), K=100)
        det_cpu = decode_ref.fusion_decode(cpu, (H // 4, W // 4), 100)
    for k in ("classIds", "scores", "centers"):
        assert np.array_equal(det_hip[k].cpu().numpy(), det_cpu[k].numpy()), k


def test_range_guards_leave_the_callers_map_alone(dev):
    m = _model(dev)
    x, pc_dep, calib = nofrustum_inputs()
    xd, pc, cd = x.to(dev), pc_dep.to(dev), calib.to(dev)
    m.check_ranges(xd, pc, cd)
    assert torch.equal(pc.cpu(), pc_dep)
    m.calibrate(xd, pc, cd)
    assert torch.equal(pc.cpu(), pc_dep)
    m.measure_ranges(xd, pc, cd)
    assert torch.equal(pc.cpu(), pc_dep)


def test_graph_and_two_stream_paths_equal_the_plain_path(dev, golden):
    """use_graph: the graph normalises its static copy and channel 0 is copied back - the caller's tensor ends up normalised once
    per call and the three pc_hm outputs are views of it; two trunk streams: the normalisation runs once, for the whole batch,
    on the caller's stream.  Outputs equal the single-stream eager ones bit for bit."""
    x, pc_dep, calib = nofrustum_inputs()
    xd, cd = x.to(dev), calib.to(dev)
    m = _model(dev)
    m.streams = 1
    pc0 = pc_dep.to(dev)
    with torch.no_grad():
        plain = m(xd, pc_dep=pc0, calib=cd)[0]
    after1 = pc0.clone()
    assert np.array_equal(after1.cpu().numpy(), golden["pc_dep_after"])

    def same(y, pc, what):
        assert list(y.keys()) == list(plain.keys())
        assert torch.equal(pc, after1), what
        for k in plain:
            if k != "calib":
                assert torch.equal(y[k], plain[k]), (what, k)
        for k in ("pc_hm_in", "pc_hm", "pc_hm_out"):
            assert _inside(y[k], pc), (what, k)
        assert y["pc_hm_in"].data_ptr() == pc.data_ptr()

    with torch.no_grad():
        m.streams, m.min_sub_batch = 2, 0
        pc = pc_dep.to(dev)
        y = m(xd, pc_dep=pc, calib=cd)[0]
        assert any(isinstance(k, tuple) and "trunk" in k for k in m._plans)     # the split path really ran
        same(y, pc, "two streams")
        for streams in (1, 2):
            m.streams, m.use_graph = streams, True
            for rep in range(2):                                   # capture + replay, then replay alone
                pc = pc_dep.to(dev)
                y = m(xd, pc_dep=pc, calib=cd)[0]
                same(y, pc, f"graph, {streams} stream(s), call {rep}")
            y2 = m(xd, pc_dep=pc, calib=cd)[0]                     # the same tensor again: twice normalised, as in eager
            assert np.array_equal(pc.cpu().numpy(), golden["pc_dep_after2"])
            assert np.array_equal(y2["pc_hm"].cpu().numpy(), golden["out2_pc_hm"])
        m.use_graph = False


def test_direct_pass_on_unaligned_and_odd_maps(dev):
    """cf_pc_hm_direct on its own: odd map sizes and a 4-byte-aligned pointer take the one-pixel path; both write the same
    channels-last copies as the frustum kernel's layout (fp32 NHWC4 and split-bf16 hi / lo)."""
    from centerfusiondetect3d_amd import _lib
    lib = _lib.load()
    rs = np.random.RandomState(3)
    for (Bq, h, w, off) in ((2, 32, 40, 0), (1, 7, 9, 0), (3, 5, 4, 1), (1, 28, 50, 3)):
        src = torch.from_numpy(rs.uniform(0, 60, (Bq, 3, h, w)).astype(np.float32))
        src[:, 0][torch.from_numpy(rs.uniform(size=(Bq, h, w)) < 0.5)] = 0.0
        store = torch.zeros(src.numel() + 8, device=dev)
        pc = store[off:off + src.numel()].view(Bq, 3, h, w)
        pc.copy_(src)
        hm4 = torch.full((Bq, h, w, 4), 7.0, device=dev)
        hm8 = torch.full((Bq, h, w, 2, 8), 7.0, device=dev, dtype=torch.bfloat16)
        _lib.check(lib.cf_pc_hm_direct(pc.data_ptr(), Bq, h, w, 60.0, hm4.data_ptr(), hm8.data_ptr(), _lib.stream_ptr()))
        want = src.clone()
        want[:, :1] /= 60.0
        want[:, :1] = 1 - want[:, :1]
        assert torch.equal(pc.cpu(), want)
        assert float(store[:off].abs().sum()) == 0 and float(store[off + src.numel():].abs().sum()) == 0
        nhwc = want.permute(0, 2, 3, 1)
        assert torch.equal(hm4[..., :3].cpu(), nhwc) and float(hm4[..., 3].abs().sum()) == 0
        hi = nhwc.bfloat16()
        lo = (nhwc - hi.float()).bfloat16()
        got = hm8.cpu()
        assert torch.equal(got[..., 0, :3], hi) and torch.equal(got[..., 1, :3], lo)
        assert float(got[..., 3:].float().abs().sum()) == 0
