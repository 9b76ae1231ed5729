"""Early radar fusion, everything that needs no GPU: the parameter tree against the reference's, the configurations that must
still raise, the radar stem packing, the plan's step list (plans are built on the CPU device: buffers are never touched while
building), and the CPU composition the GPU tests compare against (tests/early_ref.py) held to the reference-generated fixture
under the criteria of tests/test_oracle_golden.py (imported)."""
import os

import numpy as np
import pytest
import torch

from tests import early_ref
from tests.golden.make_golden_early import early_inputs, early_state_dict, FIXTURE, B, H, W
from tests.test_oracle_golden import _close


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, FIXTURE))


def _cfg(size=(H, W)):
    from centerfusiondetect3d_amd import centerfusion_early_config
    return centerfusion_early_config(size)


def test_state_dict_keys_and_shapes_equal_the_references(golden):
    from centerfusiondetect3d_amd import getModel
    sd = getModel(_cfg()).state_dict()
    assert len(sd) == 418
    # (as a mapping: the reference registers its heads before the backbone, this module the other way round - load_state_dict
    #  does not read the order)
    ref = dict(zip((str(k) for k in golden["sd_keys"]), (str(s) for s in golden["sd_shapes"])))
    assert len(ref) == 418 and {k: ",".join(str(int(n)) for n in v.shape) for k, v in sd.items()} == ref
    assert tuple(sd["base.base_layer.0.weight"].shape) == (16, 6, 7, 7)
    assert tuple(sd["detectHead_0.velocity.0.weight"].shape) == (256, 64, 3, 3)
    assert not any("depth2" in k or "rotation2" in k for k in sd)
    m = getModel(_cfg())
    m.load_state_dict(early_state_dict(0), strict=True)


def test_every_other_combination_still_raises():
    from centerfusiondetect3d_amd import DLASeg, getModel, centerfusion_middle_config, centernet_config
    with pytest.raises(NotImplementedError):
        DLASeg(34, 6, centerfusion_middle_config((H, W)))          # six channels without early
    with pytest.raises(NotImplementedError):
        DLASeg(34, 6, centernet_config((H, W)))
    with pytest.raises(NotImplementedError):
        DLASeg(34, 3, _cfg())                                      # early needs the six
    c = _cfg()
    c.DATASET.ONE_HOT_PC = True
    with pytest.raises(NotImplementedError):
        getModel(c)
    with pytest.raises(NotImplementedError):
        DLASeg(34, 6, c)
    c = _cfg()
    c.DATASET.RADAR_PC = False                                     # "early" without radar is the camera-only model: three channels
    with pytest.raises(NotImplementedError):
        DLASeg(34, 6, c)
    c = _cfg()
    c.MODEL.FUSION_STRATEGY = "late"
    with pytest.raises(NotImplementedError):
        getModel(c)


def test_pc_dep_none_raises_before_any_launch():
    from centerfusiondetect3d_amd import getModel
    m = getModel(_cfg())

    class NotATensor:                       # (a stand-in that passes the device checks: the ValueError must come before any device work)
        is_cuda, shape, device = True, (B, 3, H, W), torch.device("cpu")

        def dim(self):
            return 4

        def float(self):
            return self

        def contiguous(self):
            return self

    with pytest.raises(ValueError):
        m(NotATensor(), pc_dep=None, calib=None)
    assert m._packed is None and not m._plans


def test_radar_stem_packing_unpacks_to_the_folded_scaled_weights():
    from centerfusiondetect3d_amd import packing
    g = torch.Generator().manual_seed(3)
    w = torch.randn(16, 6, 7, 7, generator=g) * 0.1
    bn = tuple(torch.rand(16, generator=g) + 0.5 for _ in range(4))
    wf, bf = packing.fold_bn(w, None, bn)
    rest = (torch.randn(16, 16, 3, 3, generator=g), torch.zeros(16), torch.randn(32, 16, 3, 3, generator=g), torch.zeros(32))
    ps = packing.pack_stem_early(wf, bf, *rest)
    s = 1.0 / (ps.scale_base * 16.0)                                # 2^s: ONE scale for all six channels
    assert s == 2.0 ** round(np.log2(s)) and 8192 <= float(wf.abs().max()) * s < 16384
    for frag, part in ((ps.w_base, wf[:, :3]), (ps.w_base_radar, wf[:, 3:])):
        assert tuple(frag.shape) == (13, 2, 64, 8) and frag.dtype == torch.float16
        hi, lo = packing.unpack_stem_base(frag)
        want = (part.double() * s).float()
        assert torch.equal(hi, want.half().float()) and torch.equal(lo, (want - want.half().float()).half().float())
        assert torch.equal(frag[:, 0, :, 0:4], frag[:, 0, :, 4:8]) and float(frag[:, 1, :, 4:8].abs().sum()) == 0   # {hi, hi} / {lo, 0}
        assert float(frag[:, :, :, 3].abs().sum()) == 0 and float(frag[12, :, 16:].abs().sum()) == 0                  # channel 3, taps 49-51
    # zero radar weights: the image part is pack_stem's, byte for byte
    w0 = wf.clone()
    w0[:, 3:] = 0
    p0, p3 = packing.pack_stem_early(w0, bf, *rest), packing.pack_stem(wf[:, :3], bf, *rest)
    assert torch.equal(p0.w_base, p3.w_base) and p0.scale_base == p3.scale_base and float(p0.w_base_radar.abs().sum()) == 0


def _steps(model, part="all", Bq=B):
    from centerfusiondetect3d_amd.plan import _Plan, feat_operand
    dev = torch.device("cpu")
    model._prepare(dev)
    kw = {}
    if part != "all":
        spec = feat_operand(model)
        feat = torch.empty(Bq, H // 4, W // 4, 64)
        kw = dict(feat=feat, feat_in=torch.empty((Bq, H // 4, W // 4, *spec[0]), dtype=spec[1]) if spec else (feat if part == "heads" else None))
    p = _Plan(model, Bq, H, W, dev, part=part, **kw)
    names = {v: k for k, v in p.step_index.items()}
    return p, [names.get(i, st if st is None or isinstance(st[0], str) else st[0].__name__) for i, st in enumerate(p.steps)]


@pytest.mark.parametrize("flags", [dict(), dict(heads_mx=False), dict(lanes=False, heads_lanes=False)], ids=["default", "bf16x3", "no_lanes"])
def test_plan_has_the_direct_pass_before_the_stem_and_two_head_launches(flags):
    from centerfusiondetect3d_amd import getModel
    m = getModel(_cfg())
    for k, v in flags.items():
        setattr(m, k, v)
    p, names = _steps(m)
    assert names.index("pc_hm_direct") == 0 and names.index("base.stem") == 1 and names.count("pc_hm_direct") == 1
    assert p.direct_step == 0 and p.in_step == 1 and type(p.stem).__name__ == "StemEarlyArgs"
    assert names.count("tails.primary") == 1 and names.count("tails.chained") == 1 and "tails.secondary" not in names
    assert names.index("tails.primary") < names.index("tails.chained")
    assert p.primary == ["heatmap", "reg", "widthHeight", "depth", "rotation", "dimension", "amodal_offset"]
    assert p.chained == ["nuscenes_att", "velocity"] and not p.radar and not p.frustum
    assert p.topk_step is None and p.frustum_step is None
    assert ("feat.split_bf16" in names) == bool(flags.get("heads_mx", True))
    fused = [st for st in p.steps if st and not isinstance(st[0], str) and st[0].__name__ == "cf_head_fused"]
    assert len(fused) == 2
    chained = fused[1][1]._obj
    assert chained.n_src == 1 and chained.mx == 0 and chained.tail.n_hidden == 2 and chained.tail.n_heads == 2
    assert fused[0][1]._obj.mx == int(flags.get("heads_mx", True)) and fused[0][1]._obj.tail.n_hidden == 0
    # the split forward: trunks without the pass (it runs once, in front of the forks), the heads plan without any radar step
    pt, nt = _steps(m, "trunk")
    assert nt[0] == "base.stem" and "pc_hm_direct" not in nt and pt.direct_step is None
    ph, nh = _steps(m, "heads", 2 * B)
    assert "pc_hm_direct" not in nh and nh.count("tails.chained") == 1


# step lists of the two existing model kinds at 128 x 160, B = 2, default knobs: (number of steps, SHA-256 of the "\n"-joined names);
# taken from the parent commit with this file's `_steps` (the dump method of docs/history.md, "the forward plan leaves model.py")
PARENT_STEPS = {"middle": (103, "b594b1d222ce9632ab1622ff1696775caeb320718febb79be7afe05b5b8ee523"), "centernet": (101, "ec905784e06321229b43c43b02449c1869a2e0a44b6ec8e026e3a3868fb3a354")}


@pytest.mark.parametrize("kind", ["middle", "centernet"])
def test_existing_models_step_lists_are_the_parents(kind):
    import hashlib
    from centerfusiondetect3d_amd import getModel, centerfusion_middle_config, centernet_config
    m = getModel((centerfusion_middle_config if kind == "middle" else centernet_config)((H, W)))
    p, names = _steps(m)
    assert p.direct_step is None and not p.chained and not p.early
    text = "\n".join(str(n) for n in names)
    assert (len(names), hashlib.sha256(text.encode()).hexdigest()) == PARENT_STEPS[kind]


def test_cpu_composition_matches_the_reference_fixture(golden):
    """fp32, the criteria of tests/test_oracle_golden.py (`_close`, its defaults for the outputs and its stage form for the feature
    map); the caller's map bit for bit after one and after two calls; key order."""
    g = golden
    sd = early_state_dict(0)
    x, pc_dep, calib = early_inputs()
    pc = pc_dep.clone()
    with torch.no_grad():
        out, feat = early_ref.forward(sd, x, pc, calib, want_feat=True)
    y = out[0]
    assert list(y.keys()) == [str(k) for k in g["key_order"]]
    assert np.array_equal(pc.numpy(), g["pc_dep_after"]) and np.array_equal(pc[:, 1:].numpy(), pc_dep[:, 1:].numpy())
    for k, v in y.items():
        if k != "calib":
            _close(v, g[f"out_{k}"])
    flat = feat.reshape(-1)
    assert list(feat.shape) == g["stage_shape_feat"].tolist()
    _close(flat[g["stage_idx_feat"]], g["stage_val_feat"], rtol=1e-4, atol=1e-5 * float(flat.abs().max()))
    with torch.no_grad():
        y2 = early_ref.forward(sd, x, pc, calib)[0]
    assert np.array_equal(pc.numpy(), g["pc_dep_after2"])
    for k in ("heatmap", "velocity"):
        _close(y2[k], g[f"out2_{k}"])


def test_checkpoint_load_model_takes_a_418_key_file(tmp_path):
    """checkpoint.loadModel on an early checkpoint: current names as they are, legacy head names through the mapping where they exist."""
    from centerfusiondetect3d_amd import getModel
    from centerfusiondetect3d_amd.checkpoint import loadModel, to_old_name
    sd = early_state_dict(0)
    for legacy in (False, True):
        cfg = _cfg()
        cfg.MODEL.LOAD_DIR = str(tmp_path / f"early_{int(legacy)}.pth")
        torch.save({"epoch": 3, "state_dict": {(to_old_name(k) if legacy else k): v for k, v in sd.items()}}, cfg.MODEL.LOAD_DIR)
        m = getModel(cfg)
        _, m, start = loadModel(m, cfg)
        got = m.state_dict()
        assert start == 1 and len(got) == 418 and all(torch.equal(got[k], v) for k, v in sd.items())
