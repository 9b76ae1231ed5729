"""GPU: the stem's training operator (ops.stem_conv_bn_relu) and the kernels under it (csrc/cf_stem_train.hip) against float64
autograd on the CPU (tests/stem_train_ref.py).

Criterion per tensor: max|got - ref64| / max|ref64|.  The convolution kernels - forward z, gw, gx - are held to the project's rule
for cf_conv_bwd_*: the larger of 5e-6 and twice the fp32 CPU graph's own error on that case and tensor, computed on the CPU and
printed before the kernel runs.  The block is held to 1e-5 (the base block's gate) or twice the fp32 CPU graph's error where that
is larger.  Nothing here uses float atomics: every output is compared bit for bit between two runs."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import stem_train_ref as T
from tests.stem_train_ref import relerr


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def nhwc(t, dev):
    return t.float().permute(0, 2, 3, 1).contiguous().to(dev)


def nchw(t):
    return t.detach().cpu().permute(0, 3, 1, 2)


def gates(tag, g32, g64, names, floor):
    out = {}
    for n in names:
        e = relerr(g32[n], g64[n])
        out[n] = max(floor, 2 * e)
        print(f"{tag} {n}: fp32 CPU error {e:.2e}, gate {out[n]:.2e}")
    return out


def hold(tag, got, ref, gate):
    for n, g in gate.items():
        e = relerr(got[n].detach().cpu(), ref[n])
        print(f"{tag} {n}: {e:.2e} (gate {g:.2e})")
    for n, g in gate.items():
        assert relerr(got[n].detach().cpu(), ref[n]) <= g, (tag, n)


# ---- the convolution: cf_stem_conv_forward / cf_stem_conv_bwd_weight / cf_stem_conv_bwd_data ----
@pytest.mark.parametrize("i", range(len(T.CONV_CASES)))
def test_conv_forward_weight_and_data_gradient(dev, i):
    from centerfusiondetect3d_amd import ops
    B, Ci, Co, H, W, k, s = T.CONV_CASES[i]
    assert T.conv_geometry(B, Ci, Co, H, W, k, s) == T.CONV_GEOMETRY[i]           # the branch this case is there for binds
    inp = T.conv_inputs(i)
    x, radar, w, _ = inp
    ho, wo = T.out_hw(H, W, k, s)
    names = ("z", "gw") + (("gx",) if k == 3 else ())
    for mask_odd in (False, True):
        tag = f"{T.CONV_CASES[i]}{' gz zero on the odd output pixels' if mask_odd else ''}"
        (g64, G), (g32, _) = T.conv_all(inp, k, s, torch.float64, mask_odd), T.conv_all(inp, k, s, torch.float32, mask_odd)
        gate = gates(tag, g32, g64, names, T.CONV_GATE)
        xd = (x.to(dev) if k == 7 else nhwc(x, dev))
        rd = None if radar is None else radar.to(dev)
        wd, gz = w.to(dev), nhwc(G, dev)

        def run():
            out = {"z": ops.run_stem_conv_forward(xd, wd, s, rd), "gw": ops.run_stem_conv_bwd_weight(gz, xd, k, Ci, s, rd)}
            if k == 3:
                out["gx"] = ops.run_stem_conv_bwd_data(gz, wd, H, W, s)
            return out
        got = run()
        assert tuple(got["z"].shape) == (B, ho, wo, Co) and tuple(got["gw"].shape) == (Co, Ci, k, k)
        assert k == 7 or tuple(got["gx"].shape) == (B, H, W, Ci)
        hold(tag, {n: (t if n == "gw" else nchw(t)) for n, t in got.items()}, g64, gate)
        again = run()
        assert all(torch.equal(got[n], again[n]) for n in got)
        if radar is not None:
            # the radar map sampled in the kernel against the materialised six-channel input: the same sums in the same order
            x6 = T.full_input(x, radar).to(dev)
            assert torch.equal(got["z"], ops.run_stem_conv_forward(x6, wd, s, None))
            assert torch.equal(got["gw"], ops.run_stem_conv_bwd_weight(gz, x6, k, Ci, s, None))


# ---- the block ----
def block_run(dev, kind, inp, training=True, stats=None):
    from centerfusiondetect3d_amd import ops
    _, _, _, _, _, k, s = T.BLOCK_CASES[kind]
    x, radar, params, R = inp
    lx = x.to(dev).requires_grad_(k == 3)
    w, g, b = [t.to(dev).requires_grad_(True) for t in params[:3]]
    rm, rv = params[3].to(dev).clone(), params[4].to(dev).clone()
    y = ops.stem_conv_bn_relu(lx, w, g, b, rm, rv, stride=s, training=training, momentum=T.MOMENTUM, eps=T.EPS,
                              radar=None if radar is None else radar.to(dev))
    (y * R.to(dev)).sum().backward()
    out = {"y": y.detach(), "w": w.grad, "bn_w": g.grad, "bn_b": b.grad, "running_mean": rm, "running_var": rv}
    if k == 3:
        out["x"] = lx.grad
    return out


@pytest.mark.parametrize("kind", sorted(T.BLOCK_CASES))
def test_block_forward_backward_and_running_statistics(dev, kind):
    inp = T.block_inputs(kind)
    (g64, m64), (g32, _) = T.block_graph(kind, inp, torch.float64), T.block_graph(kind, inp, torch.float32)
    assert m64 >= T.KINK
    gate = gates(kind, g32, g64, list(g64), T.BLOCK_GATE)
    got = block_run(dev, kind, inp)
    assert set(got) == set(g64)
    hold(kind, got, g64, gate)
    again = block_run(dev, kind, inp)
    assert all(torch.equal(got[n], again[n]) for n in got), kind


@pytest.mark.parametrize("kind", sorted(T.BLOCK_CASES))
def test_block_in_eval_mode_is_the_running_statistics_affine(dev, kind):
    from centerfusiondetect3d_amd import ops
    _, _, _, _, _, k, s = T.BLOCK_CASES[kind]
    inp = T.block_inputs(kind, False)
    x, radar, params, R = inp
    (g64, m64), (g32, _) = T.block_graph(kind, inp, torch.float64, False), T.block_graph(kind, inp, torch.float32, False)
    assert m64 >= T.KINK
    names = [n for n in g64 if not n.startswith("running")]
    gate = gates(f"eval {kind}", g32, g64, names, T.BLOCK_GATE)
    got = block_run(dev, kind, inp, training=False)
    hold(f"eval {kind}", got, g64, gate)
    assert torch.equal(got["running_mean"].cpu(), params[3]) and torch.equal(got["running_var"].cpu(), params[4])
    # bit for bit the affine of the running statistics (cf_bn_act_train_forward, training = 0) on the kernel's own pre-BN map
    xd = x.to(dev) if k == 7 else nhwc(x, dev)
    w, g, b, rm, rv = [t.to(dev) for t in params]
    z = ops.run_stem_conv_forward(xd, w, s, None if radar is None else radar.to(dev))
    y, _, _ = ops.run_bn_act_forward(z, g, b, rm, rv, False, T.MOMENTUM, T.EPS, None, True)
    assert torch.equal(got["y"], ops.nhwc_to_nchw(y))


def test_block_computes_only_the_requested_gradients(dev):
    from centerfusiondetect3d_amd import ops
    x, _, params, R = T.block_inputs("level1")
    for keep in range(4):
        leaves = [t.to(dev).requires_grad_(j == keep) for j, t in enumerate((x, *params[:3]))]
        y = ops.stem_conv_bn_relu(*leaves, params[3].to(dev).clone(), params[4].to(dev).clone(), stride=2)
        (y * R.to(dev)).sum().backward()
        assert [t.grad is not None for t in leaves] == [j == keep for j in range(4)], keep
        assert bool(torch.isfinite(leaves[keep].grad).all()) and float(leaves[keep].grad.abs().max()) > 0


def test_nhwc_twin_is_the_operator_without_the_layout_launches(dev):
    from centerfusiondetect3d_amd import ops
    x, _, params, R = T.block_inputs("level0")
    p = [t.to(dev) for t in params]
    a = ops.stem_conv_bn_relu(x.to(dev), p[0], p[1], p[2], p[3].clone(), p[4].clone())
    b = ops.stem_conv_bn_relu_nhwc(nhwc(x, dev), p[0], p[1], p[2], p[3].clone(), p[4].clone())
    assert tuple(b.shape) == (x.shape[0], x.shape[2], x.shape[3], 16) and torch.equal(a, ops.nhwc_to_nchw(b))


def test_argument_errors(dev):
    from centerfusiondetect3d_amd import _lib, ops
    p7 = [t.to(dev) for t in T.block_params(3, 16, 7, 0)]
    p6 = [t.to(dev) for t in T.block_params(6, 16, 7, 0)]
    p3 = [t.to(dev) for t in T.block_params(16, 16, 3, 0)]
    x3, x16 = torch.zeros(1, 3, 8, 8, device=dev), torch.zeros(1, 16, 8, 8, device=dev)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        ops.stem_conv_bn_relu(torch.zeros(1, 3, 1, 1, device=dev), *p7)
    y = ops.stem_conv_bn_relu(torch.zeros(1, 3, 1, 1, device=dev), *p7, training=False)
    assert tuple(y.shape) == (1, 16, 1, 1)
    with pytest.raises(NotImplementedError, match="input gradient"):
        ops.stem_conv_bn_relu(x3.clone().requires_grad_(True), *p7)
    with pytest.raises(NotImplementedError, match="input gradient"):
        ops.stem_conv_bn_relu(x3, *p6, radar=torch.zeros(1, 3, 2, 2, device=dev, requires_grad=True))
    with pytest.raises(NotImplementedError):
        ops.stem_conv_bn_relu(x3.double(), *p7)
    with pytest.raises(NotImplementedError):
        ops.stem_conv_bn_relu(x16, *[t.to(dev) for t in T.block_params(16, 24, 3, 0)])
    with pytest.raises(NotImplementedError):
        ops.stem_conv_bn_relu(x16, *[t.to(dev) for t in T.block_params(16, 16, 5, 0)])
    with pytest.raises(NotImplementedError):
        ops.stem_conv_bn_relu(x3, *p7, stride=2)
    with pytest.raises(NotImplementedError):
        ops.stem_conv_bn_relu(torch.zeros(1, 32, 8, 8, device=dev), *[t.to(dev) for t in T.block_params(32, 32, 3, 0)])
    with pytest.raises(_lib.CfHipError):
        ops.stem_conv_bn_relu(x3.cpu(), *p7)
    y = ops.stem_conv_bn_relu(torch.full((1, 16, 8, 8), 1e30, device=dev), *p3, training=False)    # exact fp32: no range to guard
    assert tuple(y.shape) == (1, 16, 8, 8)
