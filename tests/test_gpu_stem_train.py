"""GPU, module level: `DLASeg` training its stem too (`unfreeze_stem`), so that every parameter of the model learns - B = 2, middle
fusion (MODEL.FRUSTUM = False) and early fusion, set up as tests/test_gpu_base_train.py.

`forward_stem_train` against the hand composition of three `ops.stem_conv_bn_relu` calls (NCHW) on copies of the same parameters:
the map, the running statistics and all nine parameter gradients bit for bit - nothing in the operator uses atomics and the
layout launches in between move bits.  Against the float64 graph of tests/stem_train_ref.py on the same weights the level-1 map
and the nine gradients lie within the larger of 1e-5 and twice the fp32 CPU graph's error.  Then a full training step."""
import pytest
import torch

from tests import loss_ref
from tests import stem_train_ref as T
from tests.golden import cases

pytestmark = pytest.mark.gpu

KINDS = ["middle_nofrustum", "early"]
GATE = 1e-5
STEM_PREFIXES = ("base.base_layer.", "base.level0.", "base.level1.")
SEED_HINT = {"middle_nofrustum": 1, "early": 0}        # tests/stem_train_ref.stem_input: the draw that keeps KINK on these weights


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _config(kind, freeze=True):
    from centerfusiondetect3d_amd import config as cfg
    make = {"middle_nofrustum": cfg.centerfusion_middle_config, "early": cfg.centerfusion_early_config}[kind]
    c = make((64, 96))
    if kind == "middle_nofrustum":
        c.MODEL.FRUSTUM = False
    c.MODEL.FREEZE_BACKBONE = freeze
    return cfg.update_loss_weights(c)


def _setup(kind, dev):
    """model (the neck's offset convolutions drawn, not zero), inputs, the radar map"""
    from centerfusiondetect3d_amd import getModel
    torch.manual_seed(11)
    cfg = _config(kind)
    m = getModel(cfg)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.startswith(("dla_up.", "ida_up.")) and ".conv_offset_mask." in name:
                p.copy_(torch.randn(p.shape, generator=g) * (0.02 if name.endswith("weight") else 0.3))
    m = m.to(dev)
    x, pc_dep, calib = cases.model_inputs(2, 64, 96, seed=3, radar=True)
    x, pc_dep, calib = x.to(dev), pc_dep.to(dev), calib.to(dev)
    pc_hm = pc_dep.clone()
    pc_hm[:, :1] = 1.0 - pc_hm[:, :1] / float(cfg.DATASET.MAX_PC_DIST)
    return cfg, m, x, dict(pc_hm=pc_hm, pc_dep=pc_dep, calib=calib)


def _stem_names(m):
    return [n for n, _ in m.named_parameters() if n.startswith(STEM_PREFIXES)]


def _loss(cfg, y, dev):
    from centerfusiondetect3d_amd import GenericLoss
    crit = GenericLoss(cfg, int(cfg.DATASET.NUM_CLASSES)).train()
    batch = loss_ref.batch_for([y], M=16, seed=77)
    batch = {k: ({kk: vv.to(dev) for kk, vv in v.items()} if isinstance(v, dict) else v.to(dev)) for k, v in batch.items()}
    return crit([y], batch)[0]


def _hand_stem(m, x, pc):
    """base_layer, level0, level1 through ops.stem_conv_bn_relu (NCHW) on copies of m's parameters ->
    (the level-1 map, {name: leaf}, {name: running statistic})"""
    from centerfusiondetect3d_amd import ops
    leaves = {n: p.detach().clone().requires_grad_(True) for n, p in m.named_parameters() if n.startswith(STEM_PREFIXES)}
    stats = {n: b.detach().clone() for n, b in m.named_buffers() if n.startswith(STEM_PREFIXES) and "running" in n}
    t = x
    for i, (p, stride) in enumerate(T.STEM):
        t = ops.stem_conv_bn_relu(t, leaves[p + ".0.weight"], leaves[p + ".1.weight"], leaves[p + ".1.bias"], stats[p + ".1.running_mean"],
                                  stats[p + ".1.running_var"], stride=stride, training=True, radar=pc if i == 0 else None)
    return t, leaves, stats


@pytest.mark.parametrize("kind", KINDS)
def test_forward_stem_train_is_the_hand_composition_of_three_operators(dev, kind):
    cfg, m, x, kw = _setup(kind, dev)
    pc = kw["pc_hm"] if kind == "early" else None
    m.unfreeze_stem().train()
    assert len(_stem_names(m)) == 9 and all(m.get_parameter(n).requires_grad for n in _stem_names(m))
    want, leaves, stats = _hand_stem(m, x, pc)
    y1 = m.forward_stem_train(x, pc)
    assert tuple(y1.shape) == (2, 32, 32, 48) and y1.requires_grad and bool(torch.isfinite(y1).all()) and float(y1.detach().max()) > 0
    assert torch.equal(y1, want)
    for n, s in stats.items():
        assert torch.equal(m.get_buffer(n), s), n
        assert not torch.equal(s, torch.zeros_like(s)) and not torch.equal(s, torch.ones_like(s)), n       # (they moved)
    assert all(int(b) == 1 for n, b in m.named_buffers() if n.startswith(STEM_PREFIXES) and n.endswith("num_batches_tracked"))
    assert m._stale
    R = torch.randn(y1.shape, generator=torch.Generator().manual_seed(9)).to(dev)
    (y1 * R).sum().backward()
    (want * R).sum().backward()
    for n in _stem_names(m):
        a, b = m.get_parameter(n).grad, leaves[n].grad
        assert a is not None and bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0, n
        assert torch.equal(a, b), (n, float((a - b).abs().max()), float(b.abs().max()))
    assert all(p.grad is None for n, p in m.named_parameters() if not n.startswith(STEM_PREFIXES))
    assert x.grad is None and kw["pc_hm"].grad is None
    # eval mode: the running statistics, no update, still differentiable
    m.eval()
    before = {n: b.detach().clone() for n, b in m.named_buffers() if n.startswith(STEM_PREFIXES)}
    y2 = m.forward_stem_train(x, pc)
    assert y2.requires_grad and torch.equal(y2, m.forward_stem_train(x, pc))
    assert all(torch.equal(m.get_buffer(n), b) for n, b in before.items())


@pytest.mark.parametrize("kind", KINDS)
def test_stem_against_the_float64_graph_on_the_same_weights(dev, kind):
    from centerfusiondetect3d_amd import getModel
    torch.manual_seed(11)
    m = getModel(_config(kind)).to(dev)
    sd ={k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    x, pc, R, seed = T.stem_input(sd, kind == "early", hint=SEED_HINT[kind])
    print(f"{kind}: seed {seed} (hint {SEED_HINT[kind]})")
    (g64, m64), (g32, _) = T.stem_graph(sd, x, pc, R, torch.float64), T.stem_graph(sd, x, pc, R, torch.float32)
    assert m64 >= T.KINK
    gate = {}
    for n in g64:
        e = T.relerr(g32[n], g64[n])
        gate[n] = max(GATE, 2 * e)
        print(f"{kind} {n}: fp32 CPU error {e:.2e}, gate {gate[n]:.2e}")
    m.unfreeze_stem().train()
    y1 = m.forward_stem_train(x.to(dev), None if pc is None else pc.to(dev))
    (y1 * R.to(dev)).sum().backward()
    got = {"level1": y1.detach()}
    got.update({n: m.get_parameter(n).grad for n in _stem_names(m)})
    assert set(got) == set(g64) and len(got) == 10
    errs = {n: T.relerr(got[n].cpu(), g64[n]) for n in g64}
    for n, e in errs.items():
        print(f"{kind} {n}: {e:.2e} (gate {gate[n]:.2e})")
    for n, e in errs.items():
        assert e <= gate[n], (kind, n, e, gate[n])


@pytest.mark.parametrize("kind", KINDS)
def test_training_step_moves_every_parameter_and_the_eval_forward_follows(dev, kind):
    from centerfusiondetect3d_amd import getModel
    cfg, m, x, kw = _setup(kind, dev)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    m.unfreeze_stem().train()
    kw["pc_hm"].requires_grad_(True)
    y = m(x, **kw)[0]
    for h in cfg.heads:
        assert bool(torch.isfinite(y[h]).all()), h
    m.zero_grad()
    _loss(cfg, y, dev).backward()
    for name, p in m.named_parameters():
        assert p.requires_grad and p.grad is not None and bool(torch.isfinite(p.grad).all()), name
        assert float(p.grad.abs().max()) > 0, name
    if kind == "early":
        g = m.get_parameter("base.base_layer.0.weight").grad
        assert tuple(g.shape) == (16, 6, 7, 7) and float(g[:, 3:6].abs().max()) > 0 and float(g[:, :3].abs().max()) > 0
    assert kw["pc_hm"].grad is None and x.grad is None
    for n, b in m.named_buffers():
        if n.endswith("num_batches_tracked"):
            assert int(b) == 1, n
    params = list(m.parameters())
    gmax = max(float(p.grad.abs().max()) for p in params)
    torch.optim.SGD(params, lr=0.05 / gmax).step()
    for name, p in m.named_parameters():
        assert not torch.equal(p, before[name]), name
    m.eval()
    with torch.no_grad():
        y2 = m(x, pc_dep=kw["pc_dep"].clone(), calib=kw["calib"])[0]
    fresh = getModel(cfg).to(dev)
    fresh.load_state_dict(m.state_dict())
    with torch.no_grad():
        y3 = fresh(x, pc_dep=kw["pc_dep"].clone(), calib=kw["calib"])[0]
    for h in cfg.heads:
        assert torch.equal(y2[h], y3[h]), h


def test_the_stem_training_forward_is_the_composition_of_its_four_parts(dev):
    cfg, m, x, kw = _setup("middle_nofrustum", dev)
    m.unfreeze_stem().train()
    stats = {n: b.detach().clone() for n, b in m.named_buffers()}
    y = m(x, **kw)[0]
    m.load_state_dict({**m.state_dict(), **stats})           # the running statistics as they were: the second forward starts alike
    ref = m.train().forward_heads(m.forward_neck(m.forward_levels(m.forward_stem_train(x))), **kw)[0]
    for h in cfg.heads:
        assert torch.equal(y[h], ref[h]), h


@pytest.mark.parametrize("kind", KINDS)
def test_unfreeze_stem_false_restores_the_unfreeze_base_forward_and_the_frozen_stem(dev, kind):
    cfg, m, x, kw = _setup(kind, dev)
    pc = kw["pc_hm"] if kind == "early" else None
    m.train().unfreeze_base()
    stats = {n: b.detach().clone() for n, b in m.named_buffers()}
    y_base = m(x, **kw)[0]
    s1 = m.forward_stem(x, pc)
    m.load_state_dict({**m.state_dict(), **stats})
    m.train().unfreeze_stem().unfreeze_stem(False)
    assert not m._stem_train and not m._base_train and not m._neck_train
    assert not any(p.requires_grad for n, p in m.named_parameters() if not n.startswith("detectHead_0."))
    m.unfreeze_base()
    assert not any(p.requires_grad for n, p in m.named_parameters() if n.startswith(STEM_PREFIXES))
    y2 = m(x, **kw)[0]
    for h in cfg.heads:
        assert torch.equal(y2[h], y_base[h]), h
    # without the call, forward_stem is the no-grad tensor it was and the stem's counters stay where they were
    s2 = m.forward_stem(x, pc)
    assert s2.grad_fn is None and not s2.requires_grad and torch.equal(s1, s2) and torch.equal(s2, m.forward_stem(x, pc))
    assert all(int(b) == 0 for n, b in m.named_buffers() if n.startswith(STEM_PREFIXES) and n.endswith("num_batches_tracked"))
    # unfreeze_base(False) behind unfreeze_stem() freezes the stem as well
    m.unfreeze_stem().unfreeze_base(False)
    assert not m._stem_train and not any(p.requires_grad for n, p in m.named_parameters() if n.startswith("base."))


def test_unfreeze_stem_needs_the_frozen_backbone_mode_and_training_refuses_a_graph(dev):
    from centerfusiondetect3d_amd import config as cfgm, getModel
    c = cfgm.centernet_config((64, 96))
    c.MODEL.FREEZE_BACKBONE = False
    m = getModel(cfgm.update_loss_weights(c)).to(dev)
    with pytest.raises(NotImplementedError, match="FREEZE_BACKBONE"):
        m.unfreeze_stem()
    m.train()
    with pytest.raises(NotImplementedError, match="frozen-backbone") as e:
        m(torch.zeros(2, 3, 64, 96, device=dev))
    assert "unfreeze_stem()" in str(e.value)
    c = cfgm.centernet_config((64, 96))
    c.MODEL.FREEZE_BACKBONE = True
    m = getModel(cfgm.update_loss_weights(c)).to(dev).unfreeze_stem().train()
    m.use_graph = True
    with pytest.raises(NotImplementedError, match="use_graph"):
        m(torch.zeros(2, 3, 64, 96, device=dev))
    with pytest.raises(NotImplementedError, match="use_graph"):
        m.forward_stem_train(torch.zeros(2, 3, 64, 96, device=dev))
