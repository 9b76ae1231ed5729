"""GPU: `build_targets` (cf_targets_build, three launches) against tests/golden/targets_cases.npz - what the reference's own
initReturn / transformBbox / addInstance and its no-frustum branch produced for the cases of tests/targets_cases.py.

Tolerances.  Integer and flag tensors, the set of non-zero heat pixels, the painted set of pc_hm and its values, and every float
that involves no exp / sin / cos / atan2 are compared for EQUALITY.  The rest - heat values, target.rotation, target.bboxes3d - may
differ by one fp32 ulp: a faithfully rounded float64 exp / sin / cos, rounded to fp32, is at most one ulp from the correctly
rounded value.  The ulp is the fp32 spacing at the larger of the two magnitudes.  The number of elements that differ at all is
printed per case."""
import os

import numpy as np
import pytest
import torch

from tests import targets_cases as tc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP_KEYS = ("heatmap0", "target.rotation", "target.bboxes3d")
LOSS_GATE = 5e-6                     # the criterion's own gate (tests/test_gpu_loss.py)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "targets_cases.npz")))


def build(case, dev, ann=None, pc_dep=None):
    from centerfusiondetect3d_amd import build_targets, pack_annotations
    cfg = tc.config_for(case)
    if ann is None:
        ann = pack_annotations(case["anns"], class_ids=case["class_ids"], max_objs=case["max_objs"], config=cfg)
    if pc_dep is None and case["radar"]:
        pc_dep = torch.from_numpy(case["pc_dep"]).to(dev)
    batch = build_targets(ann, torch.from_numpy(case["trans"]), torch.from_numpy(case["calib"]), cfg, pc_dep=pc_dep,
                          scale_factor=torch.from_numpy(case["scale"]), num_classes=tc.NUM_CLASSES, device=dev)
    return cfg, ann, pc_dep, batch


def flat(batch):
    out = {k: v for k, v in batch.items() if torch.is_tensor(v)}
    out.update({"target." + k: v for k, v in batch["target"].items()})
    return out


def ulps(got, ref):
    """|got - ref| in units of the fp32 spacing at max(|got|, |ref|)"""
    big = np.maximum(np.abs(got), np.abs(ref)).astype(np.float32)
    return np.abs(got.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.maximum(big, np.float32(1e-30))).astype(np.float64)


@pytest.mark.parametrize("name", tc.NAMES)
def test_against_the_reference_fixture(dev, golden, name):
    case = tc.build(name)
    _, _, pc_dep, batch = build(case, dev)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in flat(batch).items()}
    want = {k.split("/out_")[1]: v for k, v in golden.items() if k.startswith(name + "/out_")}
    assert set(got) == set(want) | {"calib"} | ({"pc_dep"} if case["radar"] else set())
    assert np.array_equal(got["calib"], case["calib"])
    if case["radar"]:
        assert batch["pc_dep"].data_ptr() == pc_dep.data_ptr() and np.array_equal(got["pc_dep"], case["pc_dep"])
    differing = {}
    for k, ref in want.items():
        g = got[k]
        assert g.dtype == ref.dtype and g.shape == ref.shape, (k, g.dtype, g.shape)
        differing[k] = int((g != ref).sum())
        if k in ULP_KEYS:
            assert np.array_equal(g != 0, ref != 0), f"{name} {k}: the non-zero sets differ"
            worst = float(ulps(g, ref).max()) if g.size else 0.0
            assert worst <= 1.0, f"{name} {k}: {worst} ulp"
        else:
            assert np.array_equal(g, ref), f"{name} {k}: {differing[k]} elements differ"
    print(f"{name}: elements that differ at all: " + ", ".join(f"{k} {n}/{want[k].size}" for k, n in differing.items() if k in ULP_KEYS))
    if name == "frustum_order":                                         # the case reaches what it is named for
        assert int((want["pc_hm"][0, 0] != 0).sum()) > 0


def test_two_calls_give_the_same_bits_and_touch_no_input(dev):
    for name in ("full", "nofrustum"):
        case = tc.build(name)
        _, ann, pc_dep, a = build(case, dev)
        tables = [t.clone() for t in (ann.table, ann.itable, ann.counts)]
        _, _, _, b = build(case, dev, ann=ann, pc_dep=pc_dep)
        torch.cuda.synchronize()
        fa, fb = flat(a), flat(b)
        for k in fa:
            assert torch.equal(fa[k].view(torch.uint8), fb[k].view(torch.uint8)), (name, k)
        assert torch.equal(pc_dep.cpu(), torch.from_numpy(case["pc_dep"]))                   # the caller's radar map
        for t, kept in zip((ann.table, ann.itable, ann.counts), tables):
            assert torch.equal(t, kept)
        assert a["pc_hm"].data_ptr() != pc_dep.data_ptr()


def test_captured_in_a_graph_and_replayed_on_new_tables(dev, golden):
    """frustum_order -> basic's first image (same shapes): a host sync inside build_targets would fail the capture, a decision
    taken on the host would replay the first case's"""
    from centerfusiondetect3d_amd import build_targets, pack_annotations
    first, second = tc.build("frustum_order"), tc.build("basic")
    cfg = tc.config_for(first)
    pack = lambda anns: pack_annotations(anns, config=cfg).to(dev)
    ann = pack(first["anns"])
    trans, calib = torch.from_numpy(first["trans"]).to(dev), torch.from_numpy(first["calib"]).to(dev)
    pc_dep, scale = torch.from_numpy(first["pc_dep"]).to(dev), torch.from_numpy(first["scale"]).to(dev)
    call = lambda: build_targets(ann, trans, calib, cfg, pc_dep=pc_dep, scale_factor=scale)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        call()                                                          # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        batch = call()
    graph.replay()
    torch.cuda.synchronize()
    eager = call()
    for k, v in flat(eager).items():
        assert torch.equal(v, flat(batch)[k]), k
    ann.copy_(pack(second["anns"][:1]))
    trans.copy_(torch.from_numpy(second["trans"][:1]))
    pc_dep.copy_(torch.from_numpy(second["pc_dep"][:1]))
    graph.replay()
    torch.cuda.synchronize()
    eager = call()
    torch.cuda.synchronize()
    for k, v in flat(eager).items():
        assert torch.equal(v, flat(batch)[k]), k
    ref = golden["basic/out_pc_hm"][:1]
    assert np.array_equal(batch["pc_hm"].cpu().numpy(), ref) and (ref != 0).any()
    assert np.array_equal(batch["mask"].cpu().numpy(), golden["basic/out_mask"][:1])


def _random_outputs(cfg, B, h, w, dev, seed):
    g = torch.Generator().manual_seed(seed)
    out = {}
    for head, c in cfg.heads.items():
        v = torch.randn(B, c, h, w, generator=g)
        if head == "heatmap":
            v = torch.sigmoid(v).clamp(1e-4, 1 - 1e-4)
        if head in ("depth", "depth2"):
            v = 1.0 / (torch.sigmoid(v) + 1e-6) - 1.0
        out[head] = v.to(dev)
    return [out]


def test_loss_on_our_batch_equals_the_loss_on_the_reference_batch(dev, golden):
    """the criterion on random head maps (28 x 50, B = 2): the batch built here against the batch the reference built (the fixture)"""
    from centerfusiondetect3d_amd import GenericLoss
    case = tc.build("basic")
    cfg, _, _, ours = build(case, dev)
    theirs = {"target": {}}
    for k, v in golden.items():
        if k.startswith("basic/out_"):
            key = k.split("/out_")[1]
            (theirs["target"] if key.startswith("target.") else theirs)[key.replace("target.", "")] = torch.from_numpy(v).to(dev)
    outputs = _random_outputs(cfg, 2, 28, 50, dev, seed=5)
    crit = GenericLoss(cfg, tc.NUM_CLASSES).train()
    with torch.no_grad():
        t_ours, l_ours = crit(outputs, ours)
        t_ref, l_ref = crit(outputs, theirs)
    assert bool(torch.isfinite(t_ours)) and float(t_ref) != 0.0
    for k in l_ref:
        a, b = float(l_ours[k]), float(l_ref[k])
        print(f"loss {k}: ours {a!r}, on the reference's batch {b!r}")
        assert abs(a - b) <= LOSS_GATE * max(abs(b), 1e-30), (k, a, b)


def test_end_to_end_training_step_from_annotations(dev):
    """annotations -> build_targets -> DLASeg.train() forward with batch['pc_hm'] -> GenericLoss -> backward, on the 64 x 64
    middle-fusion frozen-backbone model of tests/test_gpu_model_train.py and the radar map of cases.model_inputs"""
    from centerfusiondetect3d_amd import GenericLoss, build_targets, config as cfgmod, getModel, pack_annotations
    from tests.golden import cases
    torch.manual_seed(11)
    cfg = cfgmod.centerfusion_middle_config((64, 64))
    cfg.MODEL.FREEZE_BACKBONE = True
    cfgmod.update_loss_weights(cfg)
    m = getModel(cfg).to(dev)
    x, pc_dep, calib = cases.model_inputs(2, 64, 64, seed=3, radar=True)
    x, pc_dep, calib = x.to(dev), pc_dep.to(dev), calib.to(dev)
    rs = np.random.RandomState(21)
    T = tc.matrix(16, src_w=256.0)
    anns = [tc._random_image(rs, T, 16, 16, n) for n in (5, 3)]
    for image in anns:                                                  # depths the radar map of model_inputs holds (8..40 m)
        for a in image:
            a["depth"] = float(rs.uniform(10.0, 38.0))
    ann = pack_annotations(anns, max_objs=16, config=cfg)
    trans = torch.from_numpy(np.stack([T, T]))
    batch = build_targets(ann, trans, calib, cfg, pc_dep=pc_dep, device=dev)
    assert tuple(batch["pc_hm"].shape) == (2, 3, 16, 16) and batch["pc_dep"].data_ptr() == pc_dep.data_ptr()
    m.train()
    y = m(x, pc_hm=batch["pc_hm"], pc_dep=pc_dep, calib=calib)
    assert torch.equal(y[0]["pc_hm"], batch["pc_hm"][:, :1])
    crit = GenericLoss(cfg, int(cfg.DATASET.NUM_CLASSES)).train()
    total, _ = crit(y, batch)
    total.backward()
    assert bool(torch.isfinite(total))
    grads = [p.grad for n, p in m.named_parameters() if n.startswith("detectHead_0.")]
    assert grads and all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    assert any(float(g.abs().max()) > 0 for g in grads)
    drawn = batch["mask"] > 0
    assert int(drawn.sum()) > 0 and torch.equal(batch["layerMask"][:, 0], drawn)
