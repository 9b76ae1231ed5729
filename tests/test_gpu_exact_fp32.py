"""GPU: the exact-fp32 kernels of csrc/cf_gemm.hip (`cf_conv2d_fused`, `cf_dcn_v2_fused`) against float64 on every tile form
the dispatch can launch, in both `precise` modes - the arithmetic every other kernel of the package is judged by.

Criterion everywhere: max|got - ref64| / max|ref64|.  Convolution gate, per case: twice the larger of two fp32 yardsticks
evaluated on the CPU on the case's own inputs - torch's fp32 `F.conv2d` and the kernel's summation scheme restated
(tests/exact_fp32_ref.py); the kernel's order (two products per MFMA step, K in slot order) is a third fp32 order beside them.
A precise gate may not come out above 1.5e-6 (the split-fp16 convolution's gate), none above 4e-6: the inputs are held to that.
DCN gate: the backward tests' rule, 5e-6 while the fp32 oracle's own error stays below 2.5e-6 on every case.  Every output
buffer is NaN-filled before the launch, and what the launch may not write must still be NaN afterwards.
tests/test_exact_fp32_cpu.py proves from the library that these tables reach every reachable form."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import dcn_ref
from tests import exact_fp32_ref as R

S, P, D = (1, 1), (1, 1), (1, 1)
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X box"
    from centerfusiondetect3d_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ convolution
_CONV = {}     # case name -> inputs, packed weights, float64 reference and the gate: computed once, shared, never changed


def _conv_case(name):
    if name not in _CONV:
        from centerfusiondetect3d_amd import packing
        c = R.CONV_CASES[name]
        base = dict(c, act=R.ACT_NONE) if c["act"] in (R.ACT_SIGMOID_CLAMP, R.ACT_RAW_AND_SIGDEPTH) else c
        x, w, b, r = R.conv_inputs(c)
        srcs, tensors = R.conv_sources(c, x)
        pc = packing.pack_conv(w, b, [packing.Source(*s) for s in srcs], stride=c["stride"])
        ref64 = R.conv_ref(x, w, b, r, c["stride"], base["act"])                      # (acts 2 / 3: the raw map)
        t32 = R.conv_ref(x, w, b, r, c["stride"], base["act"], torch.float32)
        m32 = R.nchw(R.summation_model(pc, tensors, c["B"], c["H"], c["W"], c["precise"],
                                       None if r is None else R.nhwc(r), base["act"]))
        gate, e_t, e_m = R.conv_gate(ref64, t32, m32)
        assert gate <= (R.GATE_CEILING_PRECISE if c["precise"] else R.GATE_CEILING), (name, gate)   # a condition on the inputs
        _CONV[name] = dict(c=c, pc=pc, tensors=tensors, r=r, ref64=ref64, gate=gate, e_t=e_t, e_m=e_m)
    return _CONV[name]


def _run_conv(dev, k, frames=None):
    """One cf_conv2d_fused launch of a case (its first `frames` frames) into NaN-filled buffers -> (out, out2) on the CPU, NCHW.
    NHWC rows are 4 floats wider than N (the `_hconv` form: N = 256 at column 64 of 384), the surplus must stay NaN."""
    from centerfusiondetect3d_amd import ops, _lib
    c = k["c"]
    B = c["B"] if frames is None else frames
    H, W, N = c["H"], c["W"], c["Co"]
    Ho, Wo = R.out_hw(H, W, c["k"], c["stride"])
    assert R.tile_form(_lib.load(), B * Ho * Wo, N, R.n_pad_of(N), c["layout"], c["act"], c["precise"], False) == \
        (c["form"] if frames is None else (R.KIND_TILE, 64, 64))
    pc = k["pc"].to(dev)
    srcs = [t[:B].contiguous().to(dev) for t in k["tensors"]]
    res = None if k["r"] is None else R.nhwc(k["r"][:B]).to(dev)
    out2 = None
    if c["layout"] == R.NCHW:
        out = torch.full((B, N, Ho, Wo), NAN, device=dev)
        if c["act"] == R.ACT_RAW_AND_SIGDEPTH:
            out2 = torch.full((B, N, Ho, Wo), NAN, device=dev)
        a = ops.conv_args(pc, srcs, [t.shape[-1] for t in srcs], B, H, W, out, 0, c["act"], None, 0, R.NCHW, out2, 0, c["precise"])
        ops.run_conv(a)
        return out.cpu(), None if out2 is None else out2.cpu()
    width, col = (384, 64) if c["hconv"] else (N + 4, 0)
    buf = torch.full((B, Ho, Wo, width), NAN, device=dev)
    a = ops.conv_args(pc, srcs, [t.shape[-1] for t in srcs], B, H, W, buf, width, c["act"], res, N if res is not None else 0,
                      R.NHWC, None, col, c["precise"])
    ops.run_conv(a)
    buf = buf.cpu()
    outside = torch.cat([buf[..., :col], buf[..., col + N:]], dim=3)
    assert outside.numel() > 0 and bool(torch.isnan(outside).all()), "the launch wrote outside its N columns"
    return R.nchw(buf[..., col:col + N]), None


@pytest.mark.parametrize("name", list(R.CONV_CASES))
def test_conv_against_float64_on_every_tile_form(dev, name):
    k = _conv_case(name)
    c, ref = k["c"], k["ref64"]
    out, out2 = _run_conv(dev, k)
    assert out.shape == ref.shape and not bool(torch.isnan(out).any())
    if c["act"] == R.ACT_SIGMOID_CLAMP:
        exp = torch.clamp(torch.sigmoid(ref), 1e-4, 1 - 1e-4).float()
        print(f"[exact fp32] {name}: form {c['form']}, sigmoid-clamp max|err| {float((out - exp).abs().max()):.2e}")
        torch.testing.assert_close(out, exp, rtol=1e-5, atol=1e-6)
        return
    err = R.relerr(out, ref)
    print(f"[exact fp32] {name}: form {c['form']} precise {int(c['precise'])} | torch fp32 {k['e_t']:.2e} summation model "
          f"{k['e_m']:.2e} gate {k['gate']:.2e} | kernel {err:.2e}")
    assert err <= k["gate"], (name, err, k["gate"])
    if c["act"] == R.ACT_RAW_AND_SIGDEPTH:
        assert not bool(torch.isnan(out2).any())
        torch.testing.assert_close(out2, (1.0 / (torch.sigmoid(ref) + 1e-6) - 1.0).float(), rtol=1e-4, atol=1e-4)


# ------------------------------------------------------------------------------------------------ DCN
_DCN = {}


def _dcn_cases():
    """inputs, float64 reference and the fp32 oracle's own error of all four cases (the gate is a statement about all of them)"""
    if not _DCN:
        from centerfusiondetect3d_amd import packing
        for name, case in R.DCN_CASES.items():
            x, off, ml, w, b = R.dcn_inputs(case)
            ref64 = F.relu(R.dcn_ref_out(x, off, ml, w, b))
            e32 = R.relerr(F.relu(R.dcn_ref_out(x, off, ml, w, b, torch.float32)), ref64)
            _DCN[name] = dict(case=case, x=R.nhwc(x), off=off, ml=ml, pd=packing.pack_dcn(w, b), ref64=ref64, e32=e32)
        gate = R.dcn_gate([k["e32"] for k in _DCN.values()])
        print("[exact fp32] DCN fp32-oracle error per case: " + ", ".join(f"{n} {k['e32']:.2e}" for n, k in _DCN.items())
              + f" -> gate {gate:.1e}")
        for k in _DCN.values():
            k["gate"] = gate
    return _DCN


def _run_dcn(dev, pd, x, om, precise, act=R.ACT_RELU, mask_activated=False, form=None):
    """One cf_dcn_v2_fused launch into a NaN-filled buffer whose rows are 4 floats wider than N -> NCHW on the CPU"""
    from centerfusiondetect3d_amd import ops, _lib
    B, H, W, _ = x.shape
    if form is not None:
        assert R.tile_form(_lib.load(), B * H * W, pd.n, pd.n_pad, R.NHWC, act, precise, True) == form
    pd = pd.to(dev)
    buf = torch.full((B, H, W, pd.n + 4), NAN, device=dev)
    a = ops.dcn_args(pd, x.to(dev), om.to(dev), om.shape[-1], B, H, W, buf, pd.n + 4, act, precise)
    a.mask_activated = int(mask_activated)
    assert a.out_scale == 0.0                       # (run_dcn picks the exact kernel by it)
    ops.run_dcn(a)
    buf = buf.cpu()
    assert bool(torch.isnan(buf[..., pd.n:]).all()), "the launch wrote outside its N columns"
    out = R.nchw(buf[..., :pd.n])
    assert not bool(torch.isnan(out).any())
    return out


@pytest.mark.parametrize("precise", [True, False], ids=["precise", "plain"])
@pytest.mark.parametrize("name", list(R.DCN_CASES))
def test_dcn_against_float64_on_every_tile_form(dev, name, precise):
    k = _dcn_cases()[name]
    out = _run_dcn(dev, k["pd"], k["x"], R.offmask32(k["off"], k["ml"]), precise, form=k["case"][6])
    err = R.relerr(out, k["ref64"])
    print(f"[exact fp32] dcn {name}: form {k['case'][6]} precise {int(precise)} | fp32 oracle {k['e32']:.2e} gate {k['gate']:.1e} "
          f"| kernel {err:.2e}")
    assert err <= k["gate"], (name, precise, err)
    if name == R.DCN_MASK_ACTIVATED_CASE:           # the same layer with the sigmoid applied by the caller
        out = _run_dcn(dev, k["pd"], k["x"], R.offmask32(k["off"], torch.sigmoid(k["ml"])), precise, mask_activated=True)
        err = R.relerr(out, k["ref64"])
        print(f"[exact fp32] dcn {name}: mask_activated = 1, precise {int(precise)} | kernel {err:.2e}")
        assert err <= k["gate"], (name, precise, err)


# ------------------------------------------------------------------------------------------------ shard == full
@pytest.mark.parametrize("name", R.SHARD_CONV_CASES)
def test_conv_tile_form_never_changes_a_bit(dev, name):
    """Per output the K order is the chunk order whatever the tile: frames run alone (a 64x64 launch, asserted in _run_conv)
    give the bits of the full launch (128x128 plain, 64x128 precise) - shard == full across a tile threshold."""
    k = _conv_case(name)
    full, _ = _run_conv(dev, k)
    for frames in (1, 2):
        part, _ = _run_conv(dev, k, frames=frames)
        assert torch.equal(part, full[:frames]), (name, frames, float((part - full[:frames]).abs().max()))


@pytest.mark.parametrize("precise", [True, False], ids=["precise", "plain"])
def test_dcn_tile_form_never_changes_a_bit(dev, precise):
    k = _dcn_cases()[R.SHARD_DCN_CASE]
    om = R.offmask32(k["off"], k["ml"])
    full = _run_dcn(dev, k["pd"], k["x"], om, precise, form=k["case"][6])
    for frames in (1, 2):
        part = _run_dcn(dev, k["pd"], k["x"][:frames].contiguous(), om[:frames].contiguous(), precise, form=(R.KIND_TILE, 64, 64))
        assert torch.equal(part, full[:frames]), (frames, float((part - full[:frames]).abs().max()))


# ------------------------------------------------------------------------------------------------ known answers
# the eight cases of tests/test_oracle_dcn.py through cf_dcn_v2_fused (Cin padded to the kernel's 32), with the tolerances
# of tests/test_gpu_deform_conv2d.py, which runs them through the f16x3 kernel
def _op(dev, precise, x, off, w, b, mask):
    from centerfusiondetect3d_amd import packing
    Bn, _, H, W = x.shape
    pd = packing.pack_dcn(w, torch.zeros(w.shape[0]) if b is None else b)
    om = R.offmask32(off, torch.ones(Bn, 9, H, W) if mask is None else mask)
    return _run_dcn(dev, pd, R.nhwc(x), om, precise, act=R.ACT_NONE, mask_activated=True)


@pytest.fixture(params=[True, False], ids=["precise", "plain"])
def op(request, dev):
    return lambda *a: _op(dev, request.param, *a)


def test_kat_zero_offset_unit_mask_is_conv2d(op):
    x, w, b = R.rnd(2, 32, 13, 17), R.rnd(6, 32, 3, 3, seed=1, scale=1 / 17), R.rnd(6, seed=2)
    got = op(x, torch.zeros(2, 18, 13, 17), w, b, torch.ones(2, 9, 13, 17))
    torch.testing.assert_close(got, F.conv2d(x, w, b, 1, 1), rtol=1e-5, atol=1e-5)


def test_kat_mask_none_is_unmodulated(op):
    x, w = R.rnd(1, 32, 8, 9), R.rnd(5, 32, 3, 3, seed=1, scale=1 / 17)
    off = R.rnd(1, 18, 8, 9, seed=2)
    torch.testing.assert_close(op(x, off, w, None, None), op(x, off, w, None, torch.ones(1, 9, 8, 9)), rtol=0, atol=0)
    torch.testing.assert_close(op(x, off, w, None, None), dcn_ref.deform_conv2d(x, off, w, None, S, P, D, None),
                               rtol=1e-5, atol=1e-5)


def test_kat_integer_offset_is_shifted_conv(op):
    x, w = R.rnd(1, 32, 12, 15), R.rnd(3, 32, 3, 3, seed=1, scale=1 / 17)
    dy, dx = 2, -3
    off = torch.zeros(1, 18, 12, 15)
    off[:, 0::2] = dy
    off[:, 1::2] = dx
    Pd = 5
    full = F.conv2d(F.pad(x, (Pd, Pd, Pd, Pd)), w)
    exp = full[:, :, Pd - 1 + dy:Pd - 1 + dy + 12, Pd - 1 + dx:Pd - 1 + dx + 15]
    torch.testing.assert_close(op(x, off, w, None, None), exp, rtol=1e-5, atol=1e-5)


def test_kat_offset_channel_order_dy_then_dx_per_tap(op):
    x, w = R.rnd(1, 32, 9, 9), torch.zeros(1, 32, 3, 3)
    w[0, :, 1, 2] = 1.0
    off = torch.zeros(1, 18, 9, 9)
    off[:, 2 * 5] = 1.0                              # tap k = 5 (i=1, j=2) one row down
    exp = torch.zeros(1, 1, 9, 9)
    exp[:, 0, :8, :8] = x[:, :, 1:, 1:].sum(1)
    torch.testing.assert_close(op(x, off, w, None, None), exp, rtol=1e-5, atol=1e-5)


def test_kat_mask_is_linear_per_tap(op):
    x, w = R.rnd(1, 32, 8, 8), R.rnd(2, 32, 3, 3, seed=1, scale=1 / 17)
    off = R.rnd(1, 18, 8, 8, seed=2)
    g = torch.Generator().manual_seed(3)
    m1, m2 = torch.rand(1, 9, 8, 8, generator=g), torch.rand(1, 9, 8, 8, generator=g)
    f = lambda m: op(x, off, w, None, m)
    torch.testing.assert_close(f(m1 + 2 * m2), f(m1) + 2 * f(m2), rtol=1e-4, atol=1e-5)


def test_kat_all_out_of_range_gives_bias(op):
    x, w, b = R.rnd(1, 32, 6, 6), R.rnd(4, 32, 3, 3, seed=1), R.rnd(4, seed=2)
    got = op(x, torch.full((1, 18, 6, 6), 100.0), w, b, torch.ones(1, 9, 6, 6))
    torch.testing.assert_close(got, b.view(1, 4, 1, 1).expand(1, 4, 6, 6).contiguous(), rtol=0, atol=1e-6)


def test_kat_half_pixel_is_mean_of_integer_neighbours(op):
    x, w = R.rnd(1, 32, 10, 10), R.rnd(2, 32, 3, 3, seed=1, scale=1 / 17)

    def run(dx):
        off = torch.zeros(1, 18, 10, 10)
        off[:, 1::2] = dx
        return op(x, off, w, None, None)
    torch.testing.assert_close(run(0.5), 0.5 * (run(0.0) + run(1.0)), rtol=1e-5, atol=1e-5)


def test_kat_border_rule_minus_one_exclusive(op):
    x = torch.ones(1, 32, 4, 4)
    w = torch.zeros(1, 32, 3, 3)
    w[0, 0, 1, 1] = 1.0
    off = torch.zeros(1, 18, 4, 4)
    off[:, 8] = -0.25
    out = op(x, off, w, None, None)
    assert torch.allclose(out[0, 0, 0], torch.full((4,), 0.75)) and torch.allclose(out[0, 0, 1:], torch.ones(3, 4))
    off[:, 8] = -1.0
    out = op(x, off, w, None, None)
    assert torch.all(out[0, 0, 0] == 0) and torch.all(out[0, 0, 1:] == 1)
