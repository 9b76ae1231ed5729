"""GPU: the neck's training operators (ops.deform_conv_block, ops.upsample_dw_add) and the kernels under them
(csrc/cf_neck_bwd.hip) against float64 autograd on the CPU (tests/neck_train_ref.py).

Criterion per tensor: max|got - ref64| / max|ref64|.  Single-operator gates are tests/dcn_backward_ref.case_gate's: 5e-6 where
the fp32 CPU graph's own error on that case and tensor is below 2.5e-6, otherwise twice that error, the case unusable above
1.25e-5; the fp32 error and the gate are computed on the CPU and printed before the operator runs.  The conditioning case of
batch norm (input mean 100, std 0.1) has its own rule - twice the fp32 CPU error, no ceiling: fp32 CPU itself is at about
1.7e-5 (y) and 5.8e-5 (ggamma) there, a single-pass variance would miss by about 6e-2.  The block and the IDA stage are held to
1e-5 (the IDA stage: the larger of 1e-5 and twice the fp32 CPU graph's error); the block's DCN bias gradient, zero in exact
arithmetic under batch statistics, to the gate times max|ref g(bn_bias)|."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import neck_train_ref as T
from tests.dcn_backward_ref import case_gate, relerr


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def nhwc(t, dev, pad_to=None):
    t = t.float().permute(0, 2, 3, 1).contiguous()
    if pad_to is not None and t.shape[-1] < pad_to:
        t = torch.cat((t, torch.zeros(*t.shape[:3], pad_to - t.shape[-1])), dim=-1).contiguous()
    return t.to(dev)


def nchw(t):
    return t.detach().cpu().permute(0, 3, 1, 2)


def gates(tag, g32, g64, names):
    out = {}
    for n in names:
        e = relerr(g32[n], g64[n])
        out[n] = case_gate(e)
        print(f"{tag} {n}: fp32 CPU error {e:.2e}, gate {out[n]:.2e}")
    return out


def hold(tag, got, ref, gate):
    for n, g in gate.items():
        e = relerr(got[n].detach().cpu(), ref[n])
        print(f"{tag} {n}: {e:.2e} (gate {g:.2e})")
    for n, g in gate.items():
        assert relerr(got[n].detach().cpu(), ref[n]) <= g, (tag, n)


# ---- offset convolution backward (cf_conv3x3_bwd_weight / cf_conv3x3_bwd_data) ----
@pytest.mark.parametrize("i", range(len(T.CONV_CASES)))
def test_offset_conv_backward_with_the_mask_derivative_folded_in(dev, i):
    from centerfusiondetect3d_amd import ops
    inp = T.conv_inputs(i)
    (g64, act64), (g32, _) = T.conv_graph(inp, torch.float64), T.conv_graph(inp, torch.float32)
    gate = gates(str(T.CONV_CASES[i]), g32, g64, ("gx", "gw", "gbias"))
    x, cw, cb, G = inp
    xn, om, gom = nhwc(x, dev), nhwc(act64, dev, 32), nhwc(G, dev, 32)
    gom[..., 27:] = float("nan")                 # (channels 27..31 are ignored, whatever they hold)
    gw, gb = ops.run_conv3x3_bwd_weight(gom, om, xn)
    gx = ops.run_conv3x3_bwd_data(gom, om, cw.to(dev), torch.zeros_like(xn))
    hold(str(T.CONV_CASES[i]), {"gx": nchw(gx), "gw": gw, "gbias": gb}, g64, gate)
    gw2, gb2 = ops.run_conv3x3_bwd_weight(gom, om, xn)
    assert torch.equal(gw, gw2) and torch.equal(gb, gb2)
    base = torch.full_like(xn, 3.0)              # the data kernel ADDS into what the DCN left in gx
    assert relerr(nchw(ops.run_conv3x3_bwd_data(gom, om, cw.to(dev), base.clone()) - base), g64["gx"]) <= 2 * gate["gx"] + 1e-6
    only_b = ops.run_conv3x3_bwd_weight(gom, om, xn, want_gw=False)
    assert only_b[0] is None and torch.equal(only_b[1], gb)


# ---- batch norm + ReLU ----
def bn_run(dev, inp, training=True):
    from centerfusiondetect3d_amd import ops
    x, gamma, beta, rm, rv, R = inp
    xn, g, b = nhwc(x, dev), gamma.to(dev), beta.to(dev)
    rmd, rvd = rm.to(dev).clone(), rv.to(dev).clone()
    y, mean, invstd = ops.run_bn_relu_forward(xn, g, b, rmd, rvd, training, T.MOMENTUM, T.EPS)
    gz, gg, gb = ops.run_bn_relu_backward(nhwc(R, dev), xn, g, b, mean, invstd, training)
    return {"y": nchw(y), "gx": nchw(gz), "ggamma": gg, "gbeta": gb, "running_mean": rmd, "running_var": rvd}


BN_NAMES = ("y", "gx", "ggamma", "gbeta", "running_mean", "running_var")


@pytest.mark.parametrize("i", range(len(T.BN_CASES)))
def test_bn_relu_forward_backward_and_running_statistics(dev, i):
    inp = T.bn_inputs(i)
    (g64, _), (g32, _) = T.bn_graph(inp, torch.float64), T.bn_graph(inp, torch.float32)
    gate = gates(str(T.BN_CASES[i]), g32, g64, BN_NAMES)
    got = bn_run(dev, inp)
    hold(str(T.BN_CASES[i]), got, g64, gate)
    again = bn_run(dev, inp)
    assert all(torch.equal(got[n], again[n]) for n in BN_NAMES)


def test_bn_relu_with_the_running_statistics(dev):
    inp = T.bn_inputs(1, training=False)
    (g64, m), (g32, _) = T.bn_graph(inp, torch.float64, False), T.bn_graph(inp, torch.float32, False)
    assert m >= T.KINK
    gate = gates("eval", g32, g64, ("y", "gx", "ggamma", "gbeta"))
    got = bn_run(dev, inp, training=False)
    hold("eval", got, g64, gate)
    assert torch.equal(got["running_mean"].cpu(), inp[3]) and torch.equal(got["running_var"].cpu(), inp[4])


def test_bn_conditioning_case(dev):
    inp = T.bn_inputs(0, cond=True)
    (g64, _), (g32, _) = T.bn_graph(inp, torch.float64), T.bn_graph(inp, torch.float32)
    gate = {}
    for n in ("y", "gx", "ggamma", "gbeta"):
        e = relerr(g32[n], g64[n])
        gate[n] = 2 * e                          # this case's own rule: twice the fp32 CPU error measured here, no ceiling
        print(f"conditioning {n}: fp32 CPU error {e:.2e}, gate {gate[n]:.2e}")
    hold("conditioning", bn_run(dev, inp), g64, gate)


def test_bn_with_one_value_per_channel_raises(dev):
    from centerfusiondetect3d_amd import ops
    p = [t.to(dev) for t in T.block_params(32, 32, 0)]
    with pytest.raises(ValueError):
        ops.deform_conv_block(torch.zeros(1, 32, 1, 1, device=dev), *p)
    y = ops.deform_conv_block(torch.zeros(1, 32, 1, 1, device=dev), *p, training=False)
    assert tuple(y.shape) == (1, 32, 1, 1)


# ---- upsample ----
@pytest.mark.parametrize("i", range(len(T.UP_CASES)))
def test_upsample_dw_add_forward_and_backward(dev, i):
    from centerfusiondetect3d_amd import ops
    inp, f = T.up_inputs(i), T.UP_CASES[i][4]
    g64, g32 = T.up_graph(inp, f, torch.float64), T.up_graph(inp, f, torch.float32)
    gate = gates(str(T.UP_CASES[i]), g32, g64, ("out", "gx", "gw"))
    x, w, skip, R = [t.to(dev).requires_grad_(k < 3) for k, t in enumerate(inp)]
    out = ops.upsample_dw_add(x, w, f, skip)
    (out * R).sum().backward()
    hold(str(T.UP_CASES[i]), {"out": out, "gx": x.grad, "gw": w.grad}, g64, gate)
    assert torch.equal(skip.grad, R)             # the skip's gradient is gout, bit for bit
    first = w.grad.clone()
    w.grad = None
    (ops.upsample_dw_add(x, w, f, skip) * R).sum().backward()
    assert torch.equal(first, w.grad)


# ---- the block ----
def block_run(dev, inp, need=(True,) * 7, training=True, in_scales=None):
    from centerfusiondetect3d_amd import ops
    x, params, R = inp
    leaves = [t.to(dev).clone().requires_grad_(nd) for t, nd in zip((x, *params[:6]), need)]
    rm, rv = params[6].to(dev).clone(), params[7].to(dev).clone()
    y = ops.deform_conv_block(leaves[0], *leaves[1:], rm, rv, training=training, momentum=T.MOMENTUM, eps=T.EPS, in_scales=in_scales)
    if any(need):
        (y * R.to(dev)).sum().backward()
    res = {"y": y.detach(), "running_mean": rm, "running_var": rv}
    res.update({n: t.grad for n, t in zip(T.BLOCK_NAMES, leaves)})
    return res, y


@pytest.mark.parametrize("i", range(len(T.BLOCK_CASES)))
def test_block_output_and_all_seven_gradients(dev, i):
    inp = T.block_inputs(i)
    g64, margin = T.block_graph(inp, torch.float64)
    assert margin >= T.KINK
    got, _ = block_run(dev, inp)
    names = ("y",) + tuple(n for n in T.BLOCK_NAMES if n != "b") + ("running_mean", "running_var")
    hold(str(T.BLOCK_CASES[i]), got, g64, {n: T.BLOCK_GATE for n in names})
    zero = float(got["b"].abs().max()) / float(g64["bn_b"].abs().max())
    print(f"{T.BLOCK_CASES[i]} max|g_bias| / max|ref g(bn_bias)|: {zero:.2e}")
    assert zero <= T.BLOCK_GATE


def test_ida_stage(dev):
    from centerfusiondetect3d_amd import ops
    inp = T.ida_inputs()
    (g64, margin), (g32, _) = T.ida_graph(inp, torch.float64), T.ida_graph(inp, torch.float32)
    assert margin >= T.KINK
    names = ("y",) + tuple(n for n in T.IDA_NAMES if not n.endswith(".b"))
    gate = {}
    for n in names:
        e = relerr(g32[n], g64[n])
        gate[n] = max(1e-5, 2 * e)
        print(f"IDA stage {n}: fp32 CPU error {e:.2e}, gate {gate[n]:.2e}")
    x, skip, up_w, pp, pn, R = inp
    lx, ls, lu = [t.to(dev).requires_grad_(True) for t in (x, skip, up_w)]
    lpp, lpn = [t.to(dev).requires_grad_(True) for t in pp[:6]], [t.to(dev).requires_grad_(True) for t in pn[:6]]
    p = ops.deform_conv_block(lx, *lpp, pp[6].to(dev), pp[7].to(dev))
    y = ops.deform_conv_block(ops.upsample_dw_add(p, lu, 2, ls), *lpn, pn[6].to(dev), pn[7].to(dev))
    (y * R.to(dev)).sum().backward()
    got = {"y": y}
    got.update({n: t.grad for n, t in zip(T.IDA_NAMES, [lx, ls, lu, *lpp, *lpn])})
    hold("IDA stage", got, g64, gate)


# ---- launch selection ----
RUNS = ("run_bn_relu_backward", "run_dcn_bwd_data", "run_dcn_bwd_weight", "run_conv3x3_bwd_weight", "run_conv3x3_bwd_data",
        "run_upsample_dw_bwd")


def record(monkeypatch):
    from centerfusiondetect3d_amd import ops
    calls = []
    for name in RUNS:
        fn = getattr(ops, name)
        monkeypatch.setattr(ops, name, (lambda fn, name: lambda *a, **k: (calls.append(name), fn(*a, **k))[1])(fn, name))
    return calls


def test_only_the_launches_needs_input_grad_asks_for_run(dev, monkeypatch):
    calls = record(monkeypatch)
    inp = T.block_inputs(0)
    ref, _ = T.block_graph(inp, torch.float64)
    want = {(False, False, False, False, False, True, True): ["run_bn_relu_backward"],
            (False, False, False, True, True, False, False): ["run_bn_relu_backward", "run_dcn_bwd_weight"],
            (False, True, True, False, False, False, False): ["run_bn_relu_backward", "run_dcn_bwd_data", "run_conv3x3_bwd_weight"],
            (True, False, False, False, False, False, False): ["run_bn_relu_backward", "run_dcn_bwd_data", "run_conv3x3_bwd_data"],
            (True,) * 7: ["run_bn_relu_backward", "run_dcn_bwd_data", "run_conv3x3_bwd_weight", "run_conv3x3_bwd_data",
                          "run_dcn_bwd_weight"]}
    for need, expect in want.items():
        calls.clear()
        got, _ = block_run(dev, inp, need)
        assert calls == expect, (need, calls)
        for n, nd in zip(T.BLOCK_NAMES, need):
            assert (got[n] is not None) == nd
            if nd and n != "b":
                assert relerr(got[n].cpu(), ref[n]) <= T.BLOCK_GATE, n


def test_upsample_launches_only_what_is_asked_for(dev, monkeypatch):
    from centerfusiondetect3d_amd import ops
    calls = record(monkeypatch)
    x, w, skip, R = [t.to(dev) for t in T.up_inputs(1)]
    (ops.upsample_dw_add(x, w, 2, skip.requires_grad_(True)) * R).sum().backward()
    assert calls == [] and torch.equal(skip.grad, R)
    (ops.upsample_dw_add(x.requires_grad_(True), w, 2, skip.detach()) * R).sum().backward()
    assert calls == ["run_upsample_dw_bwd"] and x.grad is not None


def test_parameter_gradients_are_bitwise_reproducible(dev):
    inp = T.block_inputs(1)
    a, _ = block_run(dev, inp)
    b, _ = block_run(dev, inp)
    for n in T.BLOCK_NAMES[1:] + ("y", "running_mean", "running_var"):
        assert torch.equal(a[n], b[n]), n


def test_no_grad_path_carries_no_grad_fn_and_double_backward_raises(dev):
    from centerfusiondetect3d_amd import ops
    inp = T.block_inputs(0)
    _, y = block_run(dev, inp, need=(False,) * 7)
    assert y.grad_fn is None and not y.requires_grad
    with torch.no_grad():
        x, params, _ = inp
        p = [t.to(dev).requires_grad_(True) for t in params[:6]]
        y = ops.deform_conv_block(x.to(dev), *p, params[6].to(dev), params[7].to(dev))
    assert y.grad_fn is None
    x, params, R = inp
    lx = x.to(dev).requires_grad_(True)
    p = [t.to(dev).requires_grad_(True) for t in params[:6]]
    y = ops.deform_conv_block(lx, *p, params[6].to(dev), params[7].to(dev))
    (gx,) = torch.autograd.grad((y * R.to(dev)).sum(), lx, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()


def test_in_scales_skip_the_range_check_and_its_host_sync(dev, monkeypatch):
    from centerfusiondetect3d_amd import ops
    inp = T.block_inputs(0)
    with_check, _ = block_run(dev, inp)

    def boom(*a, **k):
        raise AssertionError("absmax must not run when in_scales is given")
    monkeypatch.setattr(ops, "absmax", boom)
    got, _ = block_run(dev, inp, in_scales=(16.0, 16.0))
    assert torch.equal(got["y"], with_check["y"]) and torch.equal(got["w"], with_check["w"])
    prev = ops.set_dcn_range_check(False)
    try:
        off, _ = block_run(dev, inp)
    finally:
        ops.set_dcn_range_check(prev)
    assert torch.equal(off["y"], with_check["y"])


def test_an_optimizer_step_is_seen_by_the_packed_weight_cache(dev):
    from centerfusiondetect3d_amd import ops
    x, params, R = T.block_inputs(0)
    p = [t.to(dev).requires_grad_(True) for t in params[:6]]
    stats = lambda: (params[6].to(dev), params[7].to(dev))
    y0 = ops.deform_conv_block(x.to(dev), *p, *stats())
    with torch.no_grad():
        p[0].mul_(0.5)                          # conv_offset_mask.weight
        p[2].mul_(2.0)                          # the DCN weight
    y1 = ops.deform_conv_block(x.to(dev), *p, *stats())
    fresh = [t.detach().clone().requires_grad_(True) for t in p]
    y2 = ops.deform_conv_block(x.to(dev), *fresh, *stats())
    assert not torch.equal(y0, y1) and torch.equal(y1, y2)
