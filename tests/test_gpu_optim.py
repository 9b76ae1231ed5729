"""GPU: FusedAdamW / FusedSGD (csrc/cf_optim.hip) against torch's own optimizers on the CPU in float64, given the same parameters
and gradients.

Gate, per tensor and per state (p, exp_avg, exp_avg_sq / momentum_buffer): max |x - x64| <= 2 * e_ref + 2^-23 * max |x64|, where
e_ref is the error of `torch.optim.*(foreach=False)` in fp32 on the CPU against that float64 run, measured here - twice the fp32
reference's own error is this project's standing rule (tests/test_gpu_stem_train.py), the one-ulp floor covers a tensor where torch
happens to round exactly.

Shapes, with C = ops.OPTIM_CHUNK: numel 1, 3, 4, 5, C-1, C, C+1, 2C+7 (16-byte path, its tail, one and several workgroups per
tensor), a 4-D tensor, a parameter that starts one element into its storage and one whose gradient alone does (the 4-byte path, on
more than one chunk), and 700 tensors of one to nine elements.  Gradients span 1e-6 .. 10 with every seventh element exactly 0;
five steps with fresh gradients each, the first step being special in both optimizers."""
import copy
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

STEPS = 5
HYPER = {"adamw": dict(lr=2.5e-4, weight_decay=5e-4), "sgd": dict(lr=1e-2, momentum=0.9, weight_decay=5e-4)}
STATES = {"adamw": ("exp_avg", "exp_avg_sq"), "sgd": ("momentum_buffer",)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _fused(kind):
    from centerfusiondetect3d_amd import FusedAdamW, FusedSGD
    return {"adamw": FusedAdamW, "sgd": FusedSGD}[kind]


def _torch(kind):
    return {"adamw": torch.optim.AdamW, "sgd": torch.optim.SGD}[kind]


def grad_like(shape, gen):
    """magnitudes 1e-6 .. 10 (log-uniform), random signs, every seventh element exactly 0"""
    n = 1
    for s in shape:
        n *= s
    g = 10.0 ** (torch.rand(n, generator=gen) * 7.0 - 6.0)
    g = g * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1)
    g[::7] = 0.0
    return g.float().reshape(shape)


@functools.lru_cache(maxsize=None)
def shape_set():
    """-> (shapes, layouts): layouts[i] in 'plain' / 'pview' (the parameter is a view one element into its storage) /
    'gview' (its gradient is)"""
    from centerfusiondetect3d_amd import ops
    C = ops.OPTIM_CHUNK
    shapes = [(1,), (3,), (4,), (5,), (C - 1,), (C,), (C + 1,), (2 * C + 7,), (3, 5, 7, 2), (C + 5,), (2 * C + 3,)]
    layouts = ["plain"] * 9 + ["pview", "gview"]
    gen = torch.Generator().manual_seed(70)
    for n in torch.randint(1, 10, (700,), generator=gen).tolist():
        shapes.append((n,))
        layouts.append("plain")
    return tuple(shapes), tuple(layouts)


@functools.lru_cache(maxsize=None)
def problem(seed=0, steps=STEPS):
    """-> (initial parameters, gradients per step): CPU fp32, shared between the tests - do not write to them"""
    shapes, _ = shape_set()
    gen = torch.Generator().manual_seed(100 + seed)
    inits = [torch.randn(s, generator=gen) * 0.5 for s in shapes]
    grads = [[grad_like(s, gen) for s in shapes] for _ in range(steps)]
    return inits, grads


def cpu_run(kind, inits, grads, dtype, hyper=None, groups=None, lr_lambda=None, start=None):
    """torch's single-tensor optimizer on the CPU in `dtype` -> (parameters, states).  grads[s][i] None: no gradient that step.
    groups: list of (indices, overrides).  start: (state_dict, first step) to continue from."""
    ps = [torch.nn.Parameter(t.detach().clone().to(dtype)) for t in inits]
    hyper = dict(HYPER[kind], **(hyper or {}))
    spec = ps if groups is None else [dict(params=[ps[i] for i in idx], **over) for idx, over in groups]
    opt = _torch(kind)(spec, foreach=False, **hyper)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda) if lr_lambda else None
    for step in grads:
        for p, g in zip(ps, step):
            p.grad = None if g is None else g.detach().clone().to(dtype)
        opt.step()
        if sched:
            sched.step()
    return [p.detach() for p in ps], [dict(opt.state.get(p, {})) for p in ps]


def dev_params(inits, layouts, dev):
    ps = []
    for t, lay in zip(inits, layouts):
        if lay == "pview":
            store = torch.zeros(t.numel() + 1, device=dev)
            store[1:].copy_(t.reshape(-1))
            p = torch.nn.Parameter(store[1:].view(t.shape))
            assert p.data_ptr() % 16 == 4 and p.is_contiguous()
        else:
            p = torch.nn.Parameter(t.to(dev))
            assert p.data_ptr() % 16 == 0
        ps.append(p)
    return ps


def set_grads(ps, layouts, step, dev):
    """fresh gradients: written in place where the parameter has one (the storage stays), assigned otherwise"""
    for p, lay, g in zip(ps, layouts, step):
        if g is None:
            continue
        if p.grad is not None:
            p.grad.copy_(g.to(dev))
        elif lay == "gview":
            store = torch.zeros(g.numel() + 1, device=dev)
            store[1:].copy_(g.reshape(-1))
            p.grad = store[1:].view(g.shape)
            assert p.grad.data_ptr() % 16 == 4 and p.data_ptr() % 16 == 0
        else:
            p.grad = g.to(dev)


def check_gate(kind, got_p, got_states, ref64, ref32, what=""):
    """every tensor and state within 2 * e_ref + one ulp of the float64 run; -> the worst err / bound"""
    (p64, s64), (p32, s32) = ref64, ref32
    worst = 0.0
    for i in range(len(p64)):
        rows = [("p", got_p[i], p64[i], p32[i])]
        for name in STATES[kind]:
            if s64[i].get(name) is None:
                assert got_states[i].get(name) is None, (what, i, name)
                continue
            assert got_states[i].get(name) is not None, (what, i, name)
            rows.append((name, got_states[i][name], s64[i][name], s32[i][name]))
        for name, got, r64, r32 in rows:
            assert got.dtype == torch.float32 and tuple(got.shape) == tuple(r64.shape), (what, i, name)
            e_ref = float((r32.double() - r64).abs().max())
            bound = 2 * e_ref + 2.0 ** -23 * float(r64.abs().max())
            err = float((got.detach().double().cpu() - r64).abs().max())
            assert err <= bound, (what, kind, i, tuple(r64.shape), name, err, bound, e_ref)
            if bound > 0:
                worst = max(worst, err / bound)
    return worst


def fused_states(opt, ps):
    return [dict(opt.state.get(p, {})) for p in ps]


@functools.lru_cache(maxsize=None)
def reference(kind):
    inits, grads = problem()
    return cpu_run(kind, inits, grads, torch.float64), cpu_run(kind, inits, grads, torch.float32)


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_five_steps_on_every_shape_against_float64(dev, kind):
    from centerfusiondetect3d_amd import ops
    inits, grads = problem()
    shapes, layouts = shape_set()
    ref64, ref32 = reference(kind)
    ps = dev_params(inits, layouts, dev)
    opt = _fused(kind)(ps, **HYPER[kind])
    hy = HYPER[kind]
    for s, step in enumerate(grads):
        set_grads(ps, layouts, step, dev)
        before = [p.detach().clone() for p in ps[:12]] if s == 0 else None
        opt.step()
        if s == 0 and kind == "sgd":
            # zero gradient, no buffer yet: plain decay, bit for bit - g' = fl(wd * p), p = fl(p - lr * g') with lr and wd as fp32
            # (formed in float64, where the product of two fp32 values is exact)
            lr32, wd32 = float(torch.tensor(hy["lr"]).float()), float(torch.tensor(hy["weight_decay"]).float())
            for p, b, g in zip(ps[:12], before, step):
                z = (g == 0).to(dev)
                gp = (b.double() * wd32).float()
                want = (b.double() - lr32 * gp.double()).float()
                assert torch.equal(p.detach()[z], want[z]) and int(z.sum()) >= 1
    worst = check_gate(kind, ps, fused_states(opt, ps), ref64, ref32, "five steps")
    print(f"{kind}: worst error / gate over {len(ps)} tensors = {worst:.3f}")
    if kind == "adamw":
        # the elements whose gradient was 0 in every step kept zero moments: five plain decays p *= 1 - lr * wd, bit for bit
        decay = float(torch.tensor(1.0 - hy["lr"] * hy["weight_decay"], dtype=torch.float64).float())
        for i in list(range(11)) + [40, 400]:
            z = torch.ones(shapes[i], dtype=torch.bool)
            for step in grads:
                z &= step[i] == 0
            want = inits[i].clone()
            for _ in range(STEPS):
                want = want * decay
            st = opt.state[ps[i]]
            assert int(z.sum()) >= 1 and torch.equal(ps[i].detach().cpu()[z], want[z]), i
            assert float(st["exp_avg"].cpu()[z].abs().max()) == 0 and float(st["exp_avg_sq"].cpu()[z].abs().max()) == 0
    # a discriminating reference: the gate separates the first step's special cases (one more step moves p by far more)
    assert ops.OPTIM_CHUNK % 4 == 0 and any(n[0] > 2 * ops.OPTIM_CHUNK for n in shapes)


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_a_parameter_without_gradient_is_skipped_and_joins_late_with_its_own_step_count(dev, kind):
    """b has no gradient in steps 1-2: untouched, no state.  From step 3 on it is updated like a parameter an optimizer saw first
    at that step - bit for bit a second fused optimizer that did, and within the gate of torch's float64 run (whose per-parameter
    step count starts at 1 then).  a and c continue as if b were not there.  The tables are rebuilt when b joins."""
    from centerfusiondetect3d_amd import ops
    C = ops.OPTIM_CHUNK
    gen = torch.Generator().manual_seed(5)
    shapes = [(C + 9,), (2 * C + 2,), (33,)]
    inits = [torch.randn(s, generator=gen) for s in shapes]
    grads = [[grad_like(s, gen) for s in shapes] for _ in range(STEPS)]
    for s in range(2):
        grads[s][1] = None
    lay = ["plain"] * 3
    ps = dev_params(inits, lay, dev)
    opt = _fused(kind)(ps, **HYPER[kind])
    for s, step in enumerate(grads):
        set_grads(ps, lay, step, dev)
        opt.step()
        if s < 2:
            assert ps[1].grad is None and torch.equal(ps[1].detach().cpu(), inits[1]) and ps[1] not in opt.state
            assert ps[1]._version == 0 and set(opt.state_dict()["state"]) == {0, 2}
    sd = opt.state_dict()["state"]
    if kind == "adamw":
        assert [float(sd[i]["step"]) for i in range(3)] == [5.0, 3.0, 5.0]
    # bit for bit: b alone for three steps, a and c alone for five
    alone = dev_params([inits[1]], ["plain"], dev)
    o2 = _fused(kind)(alone, **HYPER[kind])
    for step in grads[2:]:
        set_grads(alone, ["plain"], [step[1]], dev)
        o2.step()
    assert torch.equal(alone[0], ps[1])
    rest = dev_params([inits[0], inits[2]], ["plain"] * 2, dev)
    o3 = _fused(kind)(rest, **HYPER[kind])
    for step in grads:
        set_grads(rest, ["plain"] * 2, [step[0], step[2]], dev)
        o3.step()
    assert torch.equal(rest[0], ps[0]) and torch.equal(rest[1], ps[2])
    # and torch's own bookkeeping agrees
    check_gate(kind, ps, fused_states(opt, ps), cpu_run(kind, inits, grads, torch.float64), cpu_run(kind, inits, grads, torch.float32),
               "late parameter")


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_two_groups_and_a_scheduled_learning_rate(dev, kind):
    gen = torch.Generator().manual_seed(6)
    shapes = [(1000,), (7, 9), (4099,), (2,)]
    inits = [torch.randn(s, generator=gen) for s in shapes]
    grads = [[grad_like(s, gen) for s in shapes] for _ in range(STEPS)]
    groups = [([0, 1], {}), ([2, 3], dict(lr=HYPER[kind]["lr"] * 3, weight_decay=1e-2))]
    lam = lambda e: 1.0 / (1.0 + e)
    lay = ["plain"] * 4
    ps = dev_params(inits, lay, dev)
    opt = _fused(kind)([dict(params=[ps[i] for i in idx], **over) for idx, over in groups], **HYPER[kind])
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lam)
    lrs = []
    for step in grads:
        set_grads(ps, lay, step, dev)
        opt.step()
        sched.step()
        lrs.append([g["lr"] for g in opt.param_groups])
    assert lrs[0][1] == pytest.approx(3 * lrs[0][0]) and lrs[-1][0] == pytest.approx(HYPER[kind]["lr"] / 6)
    run = lambda dt: cpu_run(kind, inits, grads, dt, groups=groups, lr_lambda=lam)
    check_gate(kind, ps, fused_states(opt, ps), run(torch.float64), run(torch.float32), "groups + LambdaLR")
    # the groups did differ: the same run with one group misses the gate on the second group's tensors
    one = cpu_run(kind, inits, grads, torch.float64, lr_lambda=lam)
    assert float((one[0][2] - ps[2].detach().double().cpu()).abs().max()) > 100 * 2.0 ** -23 * float(one[0][2].abs().max())


def test_step_bumps_the_version_counters(dev):
    from centerfusiondetect3d_amd import FusedAdamW, ops
    S, P, D = (1, 1), (1, 1), (1, 1)
    rnd = lambda *s, seed: torch.randn(*s, generator=torch.Generator().manual_seed(seed))
    x, off = rnd(1, 32, 9, 11, seed=1).to(dev), rnd(1, 18, 9, 11, seed=2).to(dev)
    w = torch.nn.Parameter((rnd(32, 32, 3, 3, seed=3) * 0.1).to(dev))
    opt = FusedAdamW([w], lr=1e-2)
    prev = ops.set_dcn_pack_verify(False)      # the version counter alone must tell: no checksum of the live bits
    try:
        ops.clear_dcn_pack_cache()
        with torch.no_grad():
            a = ops.deform_conv2d(x, off, w, None, S, P, D, None)
        v0 = w._version
        w.grad = rnd(32, 32, 3, 3, seed=4).to(dev)
        opt.step()
        assert w._version > v0
        with torch.no_grad():
            b = ops.deform_conv2d(x, off, w, None, S, P, D, None)
            ops.clear_dcn_pack_cache()
            fresh = ops.deform_conv2d(x, off, w.detach().clone(), None, S, P, D, None)
        assert torch.equal(b, fresh) and not torch.equal(a, b)
    finally:
        ops.set_dcn_pack_verify(prev)
    # a step between a forward that saved w and its backward: autograd notices
    xr = x.clone().requires_grad_(True)
    y = (xr[0, :, :3, :3] * w[0]).sum()
    opt.step()
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.backward()


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
@pytest.mark.parametrize("direction", ["to_torch", "from_torch"])
def test_state_dict_moves_between_this_optimizer_and_torchs(dev, kind, direction):
    """three steps on one side, its state_dict() into the other side's optimizer on cloned parameters, two more steps on both with
    equal gradients: both ends within the gate of the float64 run of all five steps"""
    inits, grads = problem()
    inits, grads = inits[:14], [g[:14] for g in grads]
    lay = ["plain"] * 14
    ref64, ref32 = cpu_run(kind, inits, grads, torch.float64), cpu_run(kind, inits, grads, torch.float32)
    ps = dev_params(inits, lay, dev)
    make_here = lambda params: _fused(kind)(params, **HYPER[kind])
    make_torch = lambda params: _torch(kind)(params, foreach=False, **HYPER[kind])
    first, second = (make_here, make_torch) if direction == "to_torch" else (make_torch, make_here)
    o1 = first(ps)
    for step in grads[:3]:
        set_grads(ps, lay, step, dev)
        o1.step()
    # (a copy, as a checkpoint file would be: state_dict() hands out the live tensors and torch's load_state_dict keeps a tensor
    # that already has the parameter's dtype and device, so without it both optimizers would update one set of moments)
    sd = copy.deepcopy(o1.state_dict())
    names = set(STATES[kind]) | ({"step"} if kind == "adamw" else set())
    assert set(sd["state"]) == set(range(14)) and all(set(v) == names for v in sd["state"].values())
    if kind == "adamw":
        assert all(float(v["step"]) == 3.0 for v in sd["state"].values())
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    o2 = second(qs)
    o2.load_state_dict(sd)
    for step in grads[3:]:
        set_grads(ps, lay, step, dev)
        set_grads(qs, lay, step, dev)
        o1.step()
        o2.step()
    check_gate(kind, ps, [dict(o1.state[p]) for p in ps], ref64, ref32, f"{direction}: the side that kept going")
    check_gate(kind, qs, [dict(o2.state[q]) for q in qs], ref64, ref32, f"{direction}: the side that loaded")
    if kind == "adamw":
        assert all(float(v["step"]) == 5.0 for v in o2.state_dict()["state"].values())


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_steady_state_step_neither_syncs_nor_allocates(dev, kind):
    inits, grads = problem()
    shapes, layouts = shape_set()
    inits, layouts = inits[:40], layouts[:40]
    on_dev = [[g.to(dev) for g in step[:40]] for step in grads]
    ps = dev_params(inits, layouts, dev)
    opt = _fused(kind)(ps, **HYPER[kind])
    for s in range(2):
        set_grads(ps, layouts, grads[s][:40], dev)
        opt.step()
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for s in range(2, STEPS):
            for p, g in zip(ps, on_dev[s]):
                p.grad.copy_(g)                                   # in place, device to device: the storage stays
            n0 = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
            opt.step()
            assert torch.cuda.memory_stats(dev)["allocation.all.allocated"] == n0, s
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    ref64 = cpu_run(kind, inits, [g[:40] for g in grads], torch.float64)
    ref32 = cpu_run(kind, inits, [g[:40] for g in grads], torch.float32)
    check_gate(kind, ps, fused_states(opt, ps), ref64, ref32, "steady state")
    # zero_grad() keeps the storage (set_to_none=False is this class's default), so the next step is a steady-state one too
    ptrs = [p.grad.data_ptr() for p in ps]
    opt.zero_grad()
    assert [p.grad.data_ptr() for p in ps] == ptrs and all(float(p.grad.abs().max()) == 0 for p in ps[:3])
