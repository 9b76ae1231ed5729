"""GPU: the base's training operators (ops.conv_bn_act, ops.max_pool2x2) and the kernels under them (csrc/cf_base_bwd.hip)
against float64 autograd on the CPU (tests/base_train_ref.py).

Criterion per tensor: max|got - ref64| / max|ref64|.  Single-operator gates are tests/dcn_backward_ref.case_gate's: 5e-6 where
the fp32 CPU graph's own error on that case and tensor is below 2.5e-6, otherwise twice that error, the case unusable above
1.25e-5; the fp32 error and the gate are computed on the CPU and printed before the operator runs.  The block is held to 1e-5
(the neck block's gate), or twice the fp32 CPU graph's error where that is larger.  The max-pool gradient equals torch's CPU
autograd on the same fp32 values exactly.  Nothing here uses float atomics: every output is compared bit for bit between two runs."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import base_train_ref as T
from tests.dcn_backward_ref import case_gate, relerr


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def nhwc(t, dev):
    return t.float().permute(0, 2, 3, 1).contiguous().to(dev)


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


# ---- convolution backward (cf_conv_bwd_weight / cf_conv_bwd_data) ----
@pytest.mark.parametrize("i", range(len(T.CONV_CASES)))
def test_conv_backward_weight_and_data(dev, i):
    from centerfusiondetect3d_amd import ops
    B, Ci, Co, H, W, k, s = T.CONV_CASES[i]
    inp = T.conv_inputs(i)
    for mask_odd in ((False, True) if s == 2 else (False,)):
        tag = f"{T.CONV_CASES[i]}{' gz zero on the odd output pixels' if mask_odd else ''}"
        (g64, G), (g32, _) = T.conv_graph(inp, k, s, torch.float64, mask_odd), T.conv_graph(inp, k, s, torch.float32, mask_odd)
        gate = gates(tag, g32, g64, ("gx", "gw"))
        xn, w, gz = nhwc(inp[0], dev), inp[1].to(dev), nhwc(G, dev)
        gw = ops.run_conv_bwd_weight(gz, xn, k, s)
        gx = ops.run_conv_bwd_data(gz, w, H, W, s)
        assert tuple(gw.shape) == (Co, Ci, k, k) and tuple(gx.shape) == (B, H, W, Ci)
        hold(tag, {"gx": nchw(gx), "gw": gw}, g64, gate)
        gw2, gx2 = ops.run_conv_bwd_weight(gz, xn, k, s), ops.run_conv_bwd_data(gz, w, H, W, s)
        assert torch.equal(gw, gw2) and torch.equal(gx, gx2)


# ---- batch norm + [residual] + [ReLU] ----
BN_NAMES = ("y", "gx", "ggamma", "gbeta", "running_mean", "running_var")


def bn_run(dev, inp, residual, relu, training=True):
    from centerfusiondetect3d_amd import ops
    x, gamma, beta, rm, rv, res, R = inp
    xn, g, b = nhwc(x, dev), gamma.to(dev), beta.to(dev)
    rn = nhwc(res, dev) if residual else None
    rmd, rvd = rm.to(dev).clone(), rv.to(dev).clone()
    y, mean, invstd = ops.run_bn_act_forward(xn, g, b, rmd, rvd, training, T.MOMENTUM, T.EPS, rn, relu)
    gz, gr, gg, gb = ops.run_bn_act_backward(nhwc(R, dev), xn, g, b, mean, invstd, training, rn, relu, want_gres=residual)
    out = {"y": nchw(y), "gx": nchw(gz), "ggamma": gg, "gbeta": gb, "running_mean": rmd, "running_var": rvd}
    if residual:
        out["gres"] = nchw(gr)
    return out


@pytest.mark.parametrize("i", range(len(T.BN_CASES)))
@pytest.mark.parametrize("residual,relu", T.BN_MODES)
def test_bn_act_forward_backward_and_running_statistics(dev, i, residual, relu):
    from centerfusiondetect3d_amd import ops
    inp = T.bn_inputs(i, residual, relu)
    (g64, _), (g32, _) = T.bn_graph(inp, torch.float64, residual, relu), T.bn_graph(inp, torch.float32, residual, relu)
    names = BN_NAMES + (("gres",) if residual else ())
    tag = f"{T.BN_CASES[i]} residual={residual} relu={relu}"
    gate = gates(tag, g32, g64, names)
    got = bn_run(dev, inp, residual, relu)
    hold(tag, got, g64, gate)
    again = bn_run(dev, inp, residual, relu)
    assert all(torch.equal(got[n], again[n]) for n in names)
    if not residual and relu:
        # the bits of cf_bn_relu_*: the same kernels
        x, gamma, beta, rm, rv, _, R = inp
        xn, g, b, rmd, rvd = nhwc(x, dev), gamma.to(dev), beta.to(dev), rm.to(dev).clone(), rv.to(dev).clone()
        y, mean, invstd = ops.run_bn_relu_forward(xn, g, b, rmd, rvd, True, T.MOMENTUM, T.EPS)
        gz, gg, gb = ops.run_bn_relu_backward(nhwc(R, dev), xn, g, b, mean, invstd, True)
        old = {"y": nchw(y), "gx": nchw(gz), "ggamma": gg, "gbeta": gb, "running_mean": rmd, "running_var": rvd}
        assert all(torch.equal(got[n], old[n]) for n in BN_NAMES)


@pytest.mark.parametrize("residual,relu", T.BN_MODES)
def test_bn_act_in_eval_mode_leaves_the_running_statistics_untouched(dev, residual, relu):
    inp = T.bn_inputs(1, residual, relu, training=False)
    (g64, m), (g32, _) = T.bn_graph(inp, torch.float64, residual, relu, False), T.bn_graph(inp, torch.float32, residual, relu, False)
    assert m >= T.KINK
    names = ("y", "gx", "ggamma", "gbeta") + (("gres",) if residual else ())
    gate = gates(f"eval residual={residual} relu={relu}", g32, g64, names)
    got = bn_run(dev, inp, residual, relu, training=False)
    hold("eval", got, g64, gate)
    assert torch.equal(got["running_mean"].cpu(), inp[3]) and torch.equal(got["running_var"].cpu(), inp[4])


def test_bn_act_computes_only_what_is_wanted(dev):
    from centerfusiondetect3d_amd import ops
    x, gamma, beta, rm, rv, res, R = T.bn_inputs(0, True, True)
    xn, g, b, rn, Rn = nhwc(x, dev), gamma.to(dev), beta.to(dev), nhwc(res, dev), nhwc(R, dev)
    y, mean, invstd = ops.run_bn_act_forward(xn, g, b, None, None, True, T.MOMENTUM, T.EPS, rn, True)
    full = ops.run_bn_act_backward(Rn, xn, g, b, mean, invstd, True, rn, True)
    for keep in range(4):
        want = [j == keep for j in range(4)]
        part = ops.run_bn_act_backward(Rn, xn, g, b, mean, invstd, True, rn, True, *want)
        assert all((t is None) != w for t, w in zip(part, want)) and torch.equal(part[keep], full[keep])
    assert torch.equal(full[1], torch.where(y > 0, Rn, torch.zeros_like(Rn)))            # gres = gy under the ReLU mask


# ---- max-pool ----
@pytest.mark.parametrize("i", range(len(T.POOL_CASES)))
def test_max_pool_gradient_goes_to_the_first_maximum_as_aten_sends_it(dev, i):
    from centerfusiondetect3d_amd import ops
    x, R = T.pool_input(i)
    out_ref, gx_ref = T.pool_graph(x, R)
    xd = x.to(dev).requires_grad_(True)
    out = ops.max_pool2x2(xd)
    (out * R.to(dev)).sum().backward()
    assert torch.equal(out.detach().cpu(), out_ref) and torch.equal(xd.grad.cpu(), gx_ref)
    gx = ops.run_maxpool2x2_bwd(nhwc(R, dev), nhwc(x, dev))
    assert torch.equal(nchw(gx), gx_ref)
    assert torch.equal(ops.maxpool2x2(nhwc(x, dev)), nhwc(out_ref, dev))                  # (the plain launch is untouched)


def test_max_pool_of_an_odd_map_writes_zeros_behind_the_last_window(dev):
    from centerfusiondetect3d_amd import ops
    x = torch.relu(T.rnd(1, 32, 5, 7, seed=3))
    R = T.rnd(1, 32, 2, 3, seed=4)
    _, gx_ref = T.pool_graph(x, R)
    assert torch.equal(nchw(ops.run_maxpool2x2_bwd(nhwc(R, dev), nhwc(x, dev))), gx_ref)


# ---- the block ----
@pytest.mark.parametrize("kind", sorted(T.BLOCK_CASES))
def test_conv_bn_act_block_forward_backward_and_running_statistics(dev, kind):
    from centerfusiondetect3d_amd import ops
    B, cins, Co, H, W, k, s, has_res, relu = T.BLOCK_CASES[kind]
    inp = T.block_inputs(kind)
    (g64, _), (g32, _) = T.block_graph(kind, inp, torch.float64), T.block_graph(kind, inp, torch.float32)
    gate = {}
    for n in g64:
        e = relerr(g32[n], g64[n])
        gate[n] = max(T.BLOCK_GATE, 2 * e)
        print(f"{kind} {n}: fp32 CPU error {e:.2e}, gate {gate[n]:.2e}")
    xs, params, res, R = inp

    def run():
        lxs = [t.to(dev).requires_grad_(True) for t in xs]
        w, g, b = [t.to(dev).requires_grad_(True) for t in params[:3]]
        rm, rv = params[3].to(dev).clone(), params[4].to(dev).clone()
        lr = res.to(dev).requires_grad_(True) if has_res else None
        x = torch.cat(lxs, dim=1) if len(lxs) > 1 else lxs[0]
        y = ops.conv_bn_act(x, w, g, b, rm, rv, stride=s, residual=lr, relu=relu)
        (y * R.to(dev)).sum().backward()
        out = {"y": y.detach(), "w": w.grad, "bn_w": g.grad, "bn_b": b.grad, "running_mean": rm, "running_var": rv}
        out.update({f"x{j}": t.grad for j, t in enumerate(lxs)})
        if has_res:
            out["res"] = lr.grad
        return out
    got = run()
    hold(kind, got, g64, gate)
    again = run()
    assert all(torch.equal(got[n], again[n]) for n in got), kind


def test_conv_bn_act_computes_only_the_requested_gradients(dev):
    from centerfusiondetect3d_amd import ops
    xs, params, res, R = T.block_inputs("conv2_residual")
    names = ("x", "w", "bn_w", "bn_b", "res")
    for keep in range(5):
        leaves = [t.to(dev).requires_grad_(j == keep) for j, t in enumerate((xs[0], *params[:3], res))]
        y = ops.conv_bn_act(leaves[0], leaves[1], leaves[2], leaves[3], params[3].to(dev).clone(), params[4].to(dev).clone(),
                            residual=leaves[4])
        (y * R.to(dev)).sum().backward()
        assert [t.grad is not None for t in leaves] == [j == keep for j in range(5)], names[keep]
        assert bool(torch.isfinite(leaves[keep].grad).all()) and float(leaves[keep].grad.abs().max()) > 0


def test_conv_bn_act_argument_errors(dev):
    from centerfusiondetect3d_amd import ops
    p = [t.to(dev) for t in T.block_params(32, 32, 3, 0)]
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        ops.conv_bn_act(torch.zeros(1, 32, 1, 1, device=dev), *p)
    y = ops.conv_bn_act(torch.zeros(1, 32, 1, 1, device=dev), *p, training=False)
    assert tuple(y.shape) == (1, 32, 1, 1)
    with pytest.raises(NotImplementedError):
        ops.conv_bn_act(torch.zeros(1, 32, 4, 4, device=dev, dtype=torch.float64), *p)
    with pytest.raises(NotImplementedError):
        ops.conv_bn_act(torch.zeros(1, 48, 4, 4, device=dev), *[t.to(dev) for t in T.block_params(48, 32, 3, 0)])
    with pytest.raises(NotImplementedError):
        ops.conv_bn_act(torch.zeros(1, 32, 4, 4, device=dev), *[t.to(dev) for t in T.block_params(32, 32, 1, 0)], stride=2)
    with pytest.raises(Exception, match="not finite"):
        ops.conv_bn_act(torch.full((1, 32, 4, 4), float("nan"), device=dev), *p)          # the range rule of deform_conv2d
    y = ops.conv_bn_act(torch.full((1, 32, 4, 4), 1e4, device=dev), *p, training=False)   # beyond the default pre-scale's range
    assert bool(torch.isfinite(y).all())
    ops.conv_bn_act(torch.zeros(1, 32, 4, 4, device=dev), *p, in_scale=16.0)               # (in_scale: no check)
