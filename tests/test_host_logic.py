"""CPU: host-side logic of the product package - weight packing (validated by emulating the
implicit GEMM with the packed weights + slot table in numpy), BN folding, the parameter tree /
state_dict contract, config-derived heads, and the no-fallback rule."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from centerfusiondetect3d_amd import (getModel, centerfusion_middle_config, centernet_config, packing,
                                      getAffineTransform, _lib)
from oracle import model_ref, pillar_ref


def emulate_igemm(pc, srcs, stride):
    """out[m][n] = sum_slots sum_e  src[b, y*stride+dy, x*stride+dx, c_off+e] * W[n][4*slot+e]."""
    B, H, W, _ = srcs[0].shape
    Ho = (H + 2 * pc.pad - pc.kh) // stride + 1
    Wo = (W + 2 * pc.pad - pc.kh) // stride + 1
    out = np.zeros((B, Ho, Wo, pc.n_pad), np.float64)
    w = pc.weight.numpy().astype(np.float64)
    ys, xs = np.arange(Ho) * stride, np.arange(Wo) * stride
    for j, (src, dy, dx, c_off) in enumerate(pc.slots.numpy().tolist()):
        if c_off < 0:
            assert not w[:, 4 * j:4 * j + 4].any()
            continue
        t = srcs[src]
        yy, xx = ys + dy, xs + dx
        oky, okx = (yy >= 0) & (yy < H), (xx >= 0) & (xx < W)
        patch = np.zeros((B, Ho, Wo, 4))
        sub = t[:, yy[oky]][:, :, xx[okx]][..., c_off:c_off + 4]
        patch[np.ix_(range(B), np.nonzero(oky)[0], np.nonzero(okx)[0], range(sub.shape[-1]))] = sub
        out += patch @ w[:, 4 * j:4 * j + 4].T
    return out[..., :pc.n] + pc.bias.numpy()[:pc.n]


@pytest.mark.parametrize("ci_list,strides,k,stride", [([16], [16], 3, 2), ([3], [4], 7, 1),
                                                      ([64, 3], [64, 4], 3, 1), ([32, 64, 32], [32, 64, 32], 1, 1)])
def test_pack_conv_slot_table_is_a_convolution(ci_list, strides, k, stride):
    g = torch.Generator().manual_seed(0)
    B, H, W, co = 2, 9, 11, 10
    xs = [torch.randn(B, c, H, W, generator=g) for c in ci_list]
    w = torch.randn(co, sum(ci_list), k, k, generator=g)
    b = torch.randn(co, generator=g)
    ref = F.conv2d(torch.cat(xs, 1), w, b, stride, k // 2).permute(0, 2, 3, 1).numpy()
    pc = packing.pack_conv(w, b, [packing.Source(c, s) for c, s in zip(ci_list, strides)], stride=stride)
    assert pc.k_pad % 32 == 0 and pc.n_pad % 32 == 0 and pc.slots.shape == (pc.k_pad // 4, 4)
    sl = pc.slots.view(-1, 8, 4)
    assert bool((sl[:, :, 0] == sl[:, :1, 0]).all()), "a 32-wide K chunk must stay inside one source"
    srcs = []
    for x, s in zip(xs, strides):
        t = np.full((B, H, W, s), 7.0)          # padding lanes hold junk: weights there must be 0
        t[..., :x.shape[1]] = x.permute(0, 2, 3, 1).numpy()
        srcs.append(t)
    np.testing.assert_allclose(emulate_igemm(pc, srcs, stride), ref, rtol=1e-5, atol=1e-5)


def test_pack_conv_f16_with_projection_is_conv_plus_1x1():
    """packing.pack_conv_f16(proj=...): the slot table + the fragment-packed fp16 hi/lo weights, emulated in numpy, give
    conv3x3(t) + conv1x1(pooled) + both biases (what the reference computes as bn2(conv2(.)) + project(bottom):
    dla.py:96-107, 56-62); the projection's slots (source 1, tap (0, 0)) follow the slice-major 3x3 part."""
    g = torch.Generator().manual_seed(5)
    C_, Cp, B, H, W = 64, 32, 1, 5, 6
    w2, b2 = torch.randn(C_, C_, 3, 3, generator=g) * 0.05, torch.randn(C_, generator=g)
    wp, bp = torch.randn(C_, Cp, 1, 1, generator=g) * 0.3, torch.randn(C_, generator=g)
    pc = packing.pack_conv_f16(w2, b2, [packing.Source(C_, C_)], proj=(wp, bp, packing.Source(Cp, Cp)))
    assert pc.patch and pc.proj_k == Cp and pc.k_pad == 9 * C_ + Cp and pc.real_cin == (C_, Cp)
    slots = pc.slots.numpy()
    assert (slots[:9 * C_ // 8, 0] == 0).all() and (slots[9 * C_ // 8:, 0] == 1).all() and (slots[9 * C_ // 8:, 1:3] == 0).all()
    # fragments [rt][ks][plane][lane = 32 h + i][8] -> dense (N, K): W[32 rt + i][16 ks + 8 h + j]
    f = pc.weight.float().numpy().astype(np.float64)
    dense = (f[:, :, 0] + f[:, :, 1]).reshape(pc.n_pad // 32, pc.k_pad // 16, 2, 32, 8).transpose(0, 3, 1, 2, 4).reshape(pc.n_pad, pc.k_pad)
    dense *= pc.out_scale * 16.0                                    # 2^-s
    t, pooled = torch.randn(B, H, W, C_, generator=g).numpy(), torch.randn(B, H, W, Cp, generator=g).numpy()
    srcs = [t, pooled]
    out = np.zeros((B, H, W, pc.n_pad))
    for j, (src, dy, dx, c_off) in enumerate(slots.tolist()):
        x = np.zeros((B, H, W, 8))
        ys, xs = np.arange(H) + dy, np.arange(W) + dx
        oky, okx = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
        x[np.ix_(np.arange(B), np.nonzero(oky)[0], np.nonzero(okx)[0])] = srcs[src][:, ys[oky]][:, :, xs[okx]][..., c_off:c_off + 8]
        out += x @ dense[:, 8 * j:8 * j + 8].T
    out += pc.bias.numpy()
    ref = (F.conv2d(torch.from_numpy(t).permute(0, 3, 1, 2).double(), w2.double(), b2.double(), 1, 1)
           + F.conv2d(torch.from_numpy(pooled).permute(0, 3, 1, 2).double(), wp.double(), bp.double())).permute(0, 2, 3, 1).numpy()
    assert np.abs(out[..., :C_] - ref).max() < 2e-6 * np.abs(ref).max()


def test_fold_bn_and_pack_dcn():
    g = torch.Generator().manual_seed(1)
    w, b = torch.randn(8, 32, 3, 3, generator=g), torch.randn(8, generator=g)
    bn = (torch.rand(8) + 0.5, torch.randn(8), torch.randn(8), torch.rand(8) + 0.5)
    x = torch.randn(1, 32, 6, 6, generator=g)
    ref = F.batch_norm(F.conv2d(x, w, b, 1, 1), bn[2], bn[3], bn[0], bn[1], False, 0.0, 1e-5)
    wf, bf = packing.fold_bn(w, b, bn)
    torch.testing.assert_close(F.conv2d(x, wf, bf, 1, 1), ref, rtol=1e-4, atol=1e-5)
    pd = packing.pack_dcn(wf, bf)
    assert pd.weight.shape == (32, 9 * 32) and pd.n == 8
    assert torch.equal(pd.weight[:8].view(8, 9, 32)[:, 4], wf[:, :, 1, 1])     # k = tap*C + c
    assert not pd.weight[8:].any()


@pytest.mark.parametrize("radar", [True, False])
def test_state_dict_contract(radar):
    m = getModel((centerfusion_middle_config if radar else centernet_config)())
    ref = model_ref.make_state_dict(radar=radar)
    sd = m.state_dict()
    assert set(sd) == set(ref)
    assert all(sd[k].shape == ref[k].shape and sd[k].dtype == ref[k].dtype for k in sd)
    n_params = sum(v.numel() for k, v in sd.items() if "running" not in k and "num_batches" not in k)
    assert abs(n_params / 1e6 - (21.36 if radar else 20.51)) < 0.01
    # reference init facts the detector relies on
    assert float(sd["detectHead_0.heatmap.2.bias"][0]) == pytest.approx(-4.6)
    assert not sd["ida_up.proj_1.conv_offset_mask.weight"].any()
    up = sd["ida_up.up_2.weight"]
    assert up.shape == (64, 1, 8, 8) and torch.equal(up[0], up[63])
    m._packed, m._plans = object(), {"x": 1}
    m.load_state_dict(ref, strict=True)
    assert m._packed is None and not m._plans          # weights changed -> re-pack lazily


def test_config_heads_match_reference_derivation():
    c = centerfusion_middle_config()
    assert list(c.heads.keys()) == ["heatmap", "reg", "widthHeight", "depth", "rotation", "dimension",
                                    "amodal_offset", "nuscenes_att", "velocity", "depth2", "rotation2"]
    assert c.head_conv["velocity"] == [256, 256, 256] and c.head_conv["reg"] == [256]
    n = centernet_config()
    assert "depth2" not in n.heads and all(v == [256] for v in n.head_conv.values())
    assert c.MODEL.OUTPUT_SIZE == (112, 200)


def test_no_cpu_fallback_and_scope_guards():
    m = getModel(centerfusion_middle_config((64, 64)))
    with pytest.raises(_lib.CfHipError):
        m(torch.zeros(1, 3, 64, 64), pc_dep=torch.zeros(1, 3, 16, 16), calib=torch.zeros(1, 3, 4))
    cfg = centerfusion_middle_config()
    cfg.MODEL.DLA.NODE = "Conv"
    with pytest.raises(NotImplementedError):
        getModel(cfg)
    cfg = centerfusion_middle_config()
    cfg.MODEL.FUSION_STRATEGY = "early"
    with pytest.raises(NotImplementedError):
        getModel(cfg)


def test_affine_transform_matches_oracle():
    for (w, h), out in (((1600, 900), (200, 112)), ((1600, 900), (800, 448)), ((1280, 720), (400, 224))):
        a = getAffineTransform((w / 2, h / 2), float(max(w, h)), 0, out)
        b = pillar_ref.affine_transform_matrix((w / 2, h / 2), float(max(w, h)), out)
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-12)


# ------------------------------------------------------------------- legacy checkpoint names
def _legacy_fixture():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "legacy_keys.npz"))


@pytest.mark.parametrize("tag,cfg", [("centerfusion", centerfusion_middle_config), ("centernet", centernet_config)])
def test_legacy_names_follow_the_reference_mapping(tag, cfg):
    """tests/golden/legacy_keys.npz holds, for every key of our state_dict, the names the REFERENCE's
    toggleWeightName gives it (model/model.py:169-250; v1 = hm./dep_sec./actf/conv.conv_offset_mask, v2 = bare
    head names): our mapper agrees in both directions."""
    from centerfusiondetect3d_amd import checkpoint as ck
    g = _legacy_fixture()
    new, old, old2 = (list(g[f"{tag}_{s}"]) for s in ("new", "old", "oldv2"))
    m = getModel(cfg((64, 64)))
    assert list(m.state_dict().keys()) == new
    assert sum(a != b for a, b in zip(new, old)) > 150
    for k, a, b in zip(new, old, old2):
        assert ck.to_new_name(a) == k and ck.to_new_name(b) == k and ck.to_new_name(k) == k
        assert ck.to_new_name("module." + a) == k
        assert ck.to_old_name(k, 1) == a and ck.to_old_name(k, 2) == b


def test_legacy_keyed_checkpoint_loads(tmp_path):
    """A DataParallel-prefixed, legacy-keyed checkpoint with one wrong-shaped and one unknown entry loads through
    elastic_load_state_dict / loadModel with the reference's semantics (rename, skip shape mismatch, drop unknown)."""
    from centerfusiondetect3d_amd import checkpoint as ck
    g = _legacy_fixture()
    new, old = list(g["centerfusion_new"]), list(g["centerfusion_old"])
    cfg = centerfusion_middle_config((64, 64))
    gen = torch.Generator().manual_seed(3)
    m0 = getModel(cfg)
    src = {k: (torch.randn(v.shape, generator=gen) if v.is_floating_point() else v.clone())
           for k, v in m0.state_dict().items()}
    legacy = {"module." + o: src[k] for k, o in zip(new, old)}
    assert "module.hm.0.weight" in legacy and "module.dla_up.ida_0.proj_1.conv.conv_offset_mask.weight" in legacy
    legacy["module.hm.2.bias"] = torch.zeros(3)                         # wrong shape: the model keeps its own
    legacy["module.some.unknown.key"] = torch.zeros(1)
    m, rep = ck.elastic_load_state_dict(getModel(cfg), legacy)
    assert rep["dropped"] == ["module.some.unknown.key"] and rep["skipped_shape"] == ["module.hm.2.bias"]
    assert not rep["missing"]
    for k, v in m.state_dict().items():
        if k == "detectHead_0.heatmap.2.bias":
            assert float(v[0]) == pytest.approx(-4.6)                       # untouched initial bias (detectHeads.py:93)
        else:
            assert torch.equal(v, src[k]), k
    # loadModel from a file, as Detector.__init__ does (detector.py:29-31)
    path = tmp_path / "ckpt.pth"
    del legacy["module.hm.2.bias"], legacy["module.some.unknown.key"]
    torch.save({"epoch": 7, "state_dict": legacy}, path)
    cfg.MODEL.LOAD_DIR = str(path)
    ckpt, m2, start = ck.loadModel(getModel(cfg), cfg)
    assert ckpt["epoch"] == 7 and start == 1
    for k, v in m2.state_dict().items():
        if k != "detectHead_0.heatmap.2.bias":
            assert torch.equal(v, src[k]), k


def test_detector_constructor_is_the_references(tmp_path):
    """detector.py:21: `Detector(config, show=False, pause=False)`; our extensions (`model=`, `device=`, `range_policy=`) are keyword
    only, so a positional `show` can never be taken for a module.  A `MODEL.LOAD_DIR` that names no file raises (the
    reference's `torch.load` would, detector.py:30-31) - before anything touches the GPU, and never silently running
    random-init weights; `show=True` (visualisation, out of scope) raises rather than being ignored."""
    import inspect
    from centerfusiondetect3d_amd import Detector
    ps = list(inspect.signature(Detector.__init__).parameters.values())
    assert [(p.name, p.default) for p in ps[:4]] == [("self", inspect.Parameter.empty),
                                                      ("config", inspect.Parameter.empty), ("show", False), ("pause", False)]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in ps[4:]) and {p.name for p in ps[4:]} == {"model", "device", "range_policy", "range_check_every"}
    cfg = centerfusion_middle_config((64, 64))
    cfg.MODEL.LOAD_DIR = str(tmp_path / "no_such_checkpoint.pth")
    with pytest.raises(FileNotFoundError):
        Detector(cfg)
    cfg.MODEL.LOAD_DIR = ""
    with pytest.raises(NotImplementedError):
        Detector(cfg, True)
    with pytest.raises(TypeError):
        Detector(cfg, getModel(cfg))                                   # the round-3 signature's positional model


def test_reference_loader_accepts_our_module():
    """The reference's own elasticLoadStateDict, given OUR module and a DataParallel checkpoint under the legacy names,
    loaded every entry into the key of the same name and shape (tests/golden/legacy_keys.npz records, per key, the shape
    it saw and the checkpoint entry it loaded there; make_golden_legacy.py).  Our module still has those keys and
    shapes, and our loader puts every entry where the reference's did."""
    from centerfusiondetect3d_amd import checkpoint as ck
    g = _legacy_fixture()
    for tag, cfg in (("centerfusion", centerfusion_middle_config), ("centernet", centernet_config)):
        new, old = list(g[f"{tag}_new"]), list(g[f"{tag}_old"])
        shapes, loaded_from = list(g[f"{tag}_shapes"]), list(g[f"{tag}_refload_from"])
        assert len(shapes) == len(loaded_from) == len(new)
        assert loaded_from == ["module." + o for o in old]              # the reference kept none of the module's own tensors
        own = getModel(cfg((64, 64))).state_dict()
        assert list(own) == new and [",".join(map(str, v.shape)) for v in own.values()] == shapes
        gen = torch.Generator().manual_seed(4)
        ckpt = {"module." + o: (torch.randn(own[k].shape, generator=gen) if own[k].is_floating_point()
                                else torch.full_like(own[k], 1000 + i)) for i, (k, o) in enumerate(zip(new, old))}
        m, rep = ck.elastic_load_state_dict(getModel(cfg((64, 64))), ckpt)
        assert not rep["dropped"] and not rep["skipped_shape"] and not rep["missing"]
        for (k, v), src in zip(m.state_dict().items(), loaded_from):
            assert torch.equal(v, ckpt[src]), (tag, k, src)


def test_no_exec_masked_prefetch_in_pinned_loops():
    """the scheduling-pinned MFMA loops hold no exec-masked operand load (tools/check_isa.py
    compiles the kernels to gfx950 assembly - no GPU needed - and scans them)."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "check_isa.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    assert "conv3x3_f16x3_kernel" in r.stdout and "head_patch16_kernel" in r.stdout


def test_design_md_is_a_document_and_quotes_the_collected_test_counts():
    """no table cell over 400 characters, no unfilled placeholder, and the two test counts of section 6 are
    what pytest collects (tools/check_design.py --fix-counts writes them)."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "check_design.py"), "--counts"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:]


def test_deform_conv2d_has_torchvisions_signature():
    """The operator-level drop-in binds exactly as torchvision.ops.deform_conv2d does (names, order, defaults), so the
    reference's keyword call (model/networks/dla.py:461-470) and positional calls both land; without a GPU it raises
    CfHipError - there is no CPU path behind it."""
    import inspect
    import pytest
    import torch
    from centerfusiondetect3d_amd import ops, _lib
    sig = inspect.signature(ops.deform_conv2d)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [
        ("input", inspect.Parameter.empty), ("offset", inspect.Parameter.empty), ("weight", inspect.Parameter.empty),
        ("bias", None), ("stride", (1, 1)), ("padding", (0, 0)), ("dilation", (1, 1)), ("mask", None)]
    x, off, w = torch.zeros(1, 32, 4, 4), torch.zeros(1, 18, 4, 4), torch.zeros(8, 32, 3, 3)
    with pytest.raises(_lib.CfHipError):
        ops.deform_conv2d(input=x, offset=off, weight=w, bias=None, stride=(1, 1), padding=(1, 1), dilation=(1, 1),
                          mask=torch.ones(1, 9, 4, 4))


def test_integration_md_snippets_parse_and_import_real_names():
    """Every ```python block of INTEGRATION.md is valid Python, every name it imports from this package exists, and
    every keyword it passes to decode_post_packed / run_pipelined / deform_conv2d is a real parameter (the round-2
    document carried a stale struct and a stale call)."""
    import ast, importlib, inspect, os, re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    blocks = re.findall(r"```python\n(.*?)```", text, re.S)
    assert len(blocks) >= 6
    import centerfusiondetect3d_amd as pkg
    for src in blocks:
        tree = ast.parse(src)
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom) and node.module and node.module.startswith("centerfusiondetect3d_amd"):
                mod = importlib.import_module(node.module)
                for alias in node.names:
                    assert hasattr(mod, alias.name), f"INTEGRATION.md imports {alias.name} from {node.module}"
            if isinstance(node, ast.Call):
                name = node.func.attr if isinstance(node.func, ast.Attribute) else getattr(node.func, "id", None)
                target = {"decode_post_packed": pkg.decode_post_packed, "run_pipelined": pkg.Detector.run_pipelined,
                          "radar_to_pc_dep": pkg.radar_to_pc_dep}.get(name)
                if target is not None:
                    params = inspect.signature(target).parameters
                    for kw in node.keywords:
                        assert kw.arg in params, f"INTEGRATION.md passes {kw.arg}= to {name}"
                    assert len(node.args) <= len([p for p in params if p != "self"]), name


def test_range_guard_host_logic():
    """The host side of the dynamic-range guard without a GPU: the pre-scale rule, the calibration
    state and what voids it, and the argument blocks carrying in_scale / out_scale as the C ABI documents them."""
    import math
    from centerfusiondetect3d_amd import ops, _lib
    # the rule: 16 while max |x| * 16 leaves a factor 4 to 65504, else the largest power of two with max |x| * s <= 65504 / 8
    assert ops.in_scale_for(0.0) == ops.in_scale_for(1.0) == ops.in_scale_for(1023.0) == 16.0
    for a in (1024.0, 2047.0, 4094.0, 5000.0, 65504.0, 1e6, 2.3e7, 3e30):
        s = ops.in_scale_for(a)
        assert s < 16.0 and math.frexp(s)[0] == 0.5                      # a power of two
        assert a * s <= 65504.0 / 8.0 < a * s * 2.0                      # the largest one inside the headroom
    assert ops.in_scale_for(5000.0, headroom=2.0) == 4.0
    for bad in (float("nan"), float("inf")):
        with pytest.raises(_lib.CfHipError, match="not finite"):
            ops.in_scale_for(bad)
    # argument blocks: in_scale = 0 (= 16) by default, out_scale follows a calibrated in_scale
    w, b = torch.randn(64, 64, 3, 3) * 0.05, torch.zeros(64)
    pc = packing.pack_conv_f16(w, b, [packing.Source(64, 64)])
    x = torch.zeros(1, 8, 8, 64)
    a0 = ops.conv_args(pc, [x], [64], 1, 8, 8, x, 64)
    a1 = ops.conv_args(pc, [x], [64], 1, 8, 8, x, 64, in_scale=0.5)
    assert a0.in_scale == 0.0 and a0.out_scale == pytest.approx(pc.out_scale)
    assert a1.in_scale == 0.5 and a1.out_scale == pytest.approx(pc.out_scale * 32.0)
    # calibration state of the module: set / get, scales, and load_state_dict voids it
    m = getModel(centerfusion_middle_config((64, 64)))
    assert m.calibration() is None and m._range_checked is False and m._scale("base.level2.tree1.conv1") is None
    m.set_calibration({"base.level2.tree1.conv1": 10.0, "base.level5.tree1.conv2": 40000.0, "base.level5.project": 9.0,
                       "heads.primary.0": 3000.0})
    assert m._range_checked and m.calibration()["base.level5.tree1.conv2"] == 40000.0
    assert m._scale("base.level2.tree1.conv1") == 16.0 and m._scale("base.level5.tree1.conv2") == 0.125
    assert m._scale("base.level3.tree1.conv1") is None                  # not measured: the default
    m.load_state_dict(m.state_dict())
    assert m.calibration() is None and m._range_checked is False
    with pytest.raises(_lib.CfHipError):
        m.measure_ranges(torch.zeros(1, 3, 64, 64))                     # device tensors only: no CPU path
