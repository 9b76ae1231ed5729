"""GPU: autograd through `centerfusiondetect3d_amd.ops.deform_conv2d` (cf_dcn_v2_bwd_data / cf_dcn_v2_bwd_weight) against
autograd through the CPU oracle `oracle/dcn_ref.deform_conv2d` in float64 (torchvision's convention: floor held constant, the
right-hand derivative at integer positions).  Loss = (out * R).sum() with a fixed random R, so grad_output is dense.

Criterion per gradient (gx, goffset, gmask, gw, gbias): max|got - ref64| / max|ref64|.

Offsets are CONSTRUCTED: the offset gradient jumps at integer sampling positions, and fp32 and float64 can land on different
sides of an integer, so after drawing the offsets every sampling coordinate whose fractional part is within 1e-3 of an integer
is moved (in float64) to exactly 1e-3 away; the offsets are then rounded to fp32 (the operator's input type; |h| < 64, so the
rounding moves a coordinate by < 4e-6) and the test asserts on the CPU, on the very coordinates fp32 and float64 arithmetic
produce from them, that none is closer than 1e-3 - 1e-5 to an integer.  No case is excluded.

The gates.  The project's forward gate is 5e-6.  The same backward through the oracle in fp32 on the CPU, against float64
(tools/dcn_backward_oracle_error.py; docs/experiments/dcn_backward.md), measured per case:

    case (B,Cin,Cout,H,W,scale)      gx        goffset   gw        gbias     gmask
    (1,32,27,5,7,1)                  2.7e-07   2.0e-07   3.6e-07   6.6e-08   3.0e-07
    (2,64,64,9,13,2)                 5.0e-07   4.2e-07   6.4e-07   1.1e-07   7.5e-07
    (2,32,64,17,21,8)                8.2e-07   1.0e-06   7.4e-07   6.4e-08   1.4e-06
    (1,128,32,8,40,3)                1.4e-06   1.6e-06   1.1e-06   9.6e-08   1.8e-06
    (2,64,64,9,13,2) mask=None       5.2e-07   5.3e-07   5.3e-07   8.2e-08   -
    (1,160,192,6,9,2)                3.1e-07   3.7e-07   3.4e-07   1.2e-07   4.0e-07
    worst                            1.4e-06   1.6e-06   1.1e-06   1.2e-07   1.8e-06

Every gradient's fp32-oracle error is below 2.5e-6 on every one of these six cases, so their gate is 5e-6 (the rule: 5e-6 where
the fp32 oracle meets 2.5e-6 everywhere, otherwise twice its worst error - twice because the kernel's summation order, atomics
and the K split, is another fp32 order than the CPU's, and nothing more).

The cases after them (NEW_CASES of tests/dcn_backward_ref.py) are there for the branches csrc/cf_dcn_bwd.hip picks from the
problem size - the slab cap of the weight gradient, the reduce kernel over many slabs, four chunks per wave of the data kernel,
its dynamic LDS at the 32768-byte floor, above 64 KB and at the most N = 1024 takes; tests/test_dcn_backward_cpu.py asserts the
geometry each one reaches.  The same rule holds for them per case and per gradient, from the fp32 oracle run on the CPU at test
time (`case_gates`; both numbers are printed before the operator runs): 5e-6 while the fp32 oracle's own error on that case and
gradient is below 2.5e-6, otherwise twice that error; above 1.25e-5 the case fails as unusable.  Measured by the same tool:

    case (B,Cin,Cout,H,W,scale)      gx        goffset   gw        gbias     gmask
    (1,512,256,7,9,2)                4.5e-07   2.3e-07   4.3e-07   1.4e-07   4.1e-07
    (1,512,256,35,53,2)              1.8e-06   1.9e-06   1.7e-06   1.5e-07   2.6e-06
    (1,512,256,61,89,2)              3.6e-06   4.5e-06   2.9e-06   1.3e-07   5.0e-06
    (1,64,64,116,250,2)              8.1e-06   8.9e-06   6.7e-06   1.6e-07   9.0e-06
    (1,256,128,6,11,3)               4.9e-07   5.3e-07   3.6e-07   8.1e-08   7.6e-07
    (2,128,128,5,9,2) mask=None      3.6e-07   3.6e-07   3.5e-07   8.6e-08   -
    (1,256,64,9,7,30)                1.9e-07   2.2e-07   2.0e-07   6.3e-08   2.4e-07
    (1,64,320,5,6,2)                 4.5e-07   4.0e-07   3.3e-07   7.5e-08   4.6e-07
    (1,32,1024,3,5,2)                4.3e-07   3.8e-07   1.9e-07   1.7e-07   3.3e-07

On the three large maps the fp32 oracle is above 2.5e-6 for a known reason: a sampling coordinate near 250 carries an fp32
rounding of about 1.5e-5 in its fractional part, and the kernel commits the same rounding.  So their gates are up to 1.8e-5
(gx / goffset / gw / gmask of the 116 x 250 map: 1.6e-5 / 1.8e-5 / 1.3e-5 / 1.8e-5); gbias is 5e-6 everywhere.  The fp32 sums
depend on the CPU's thread count in the last digit, so a gate computed at test time can differ from this table by a few per cent.

The call-sequence test (cases, helpers and the graph itself: tests/dcn_backward_ref.py) runs torch's own GPU convolution, batch
norm and their backward around the operator.  The same graph on the oracle in fp32 on the CPU, against float64:

    DeformConv sequence (1,32,32,12,16)   com_w     com_b     w         b         x
                                      5.5e-07   1.4e-07   6.3e-07   1.3e-07   5.9e-07

By the rule above the operator's share of that graph is held to 5e-6; torch's GPU convolution and batch norm, forward and
backward, are two more fp32 stages whose summation order is neither the oracle's nor ours, and get as much again: the bound
on every gradient of the sequence is 1e-5 of max|ref|."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import dcn_ref
from tests.dcn_backward_ref import (CASES, NAMES, NEW_CASES, S, P, D, SEQ_NAMES, SEQ_SHAPE, case_gate, integer_distance, make_case,
                                    oracle_grads, relerr, rnd, sequence_grads)

GATE = {"gx": 5e-6, "goffset": 5e-6, "gmask": 5e-6, "gw": 5e-6, "gbias": 5e-6}
SEQ_GATE = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def op_grads(dev, x, off, w, b, mask, R, need=(True,) * 5):
    """the same gradients through the operator on the device (None where `need` is False), and the output"""
    from centerfusiondetect3d_amd import ops
    leaves = [None if t is None else t.detach().to(dev).requires_grad_(n) for t, n in zip((x, off, w, b, mask), need)]
    out = ops.deform_conv2d(leaves[0], leaves[1], leaves[2], leaves[3], S, P, D, leaves[4])
    (out * R.to(dev)).sum().backward()
    return {n: (None if t is None or t.grad is None else t.grad.cpu()) for n, t in zip(NAMES, leaves)}, out


@functools.lru_cache(maxsize=None)
def reference(i):
    """float64 oracle gradients of case i: computed once, shared, never written to"""
    return oracle_grads(*make_case(i))


@functools.lru_cache(maxsize=None)
def case_gates(i):
    """the gates of case i.  The first six: GATE.  One of NEW_CASES: per gradient, from the fp32 oracle's own error against float64
    on that case, computed here on the CPU and printed (tests/dcn_backward_ref.case_gate); nothing of the kernel enters it"""
    if i not in NEW_CASES:
        return dict(GATE)
    g32, ref = oracle_grads(*make_case(i), dtype=torch.float32), reference(i)
    e32 = {n: relerr(g32[n], ref[n]) for n in NAMES if ref[n] is not None}
    print(f"[deform_conv2d backward] {CASES[i]}: fp32 oracle " + "  ".join(f"{n} {e:.2e}" for n, e in e32.items()))
    gates = {n: case_gate(e) for n, e in e32.items()}
    print(f"[deform_conv2d backward] {CASES[i]}: gate        " + "  ".join(f"{n} {g:.2e}" for n, g in gates.items()))
    return gates


def check(tag, got, ref, names, gates=GATE):
    errs = {n: relerr(got[n], ref[n]) for n in names}
    print(f"[deform_conv2d backward] {tag}: " + "  ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    for n, e in errs.items():
        assert got[n].shape == ref[n].shape and got[n].dtype == torch.float32
        assert e <= gates[n], (tag, n, e, gates[n])


@pytest.mark.parametrize("i", range(len(CASES)))
def test_backward_matches_the_float64_oracle(dev, i):
    x, off, w, b, mask, R = make_case(i)
    ref = reference(i)
    gates = case_gates(i)                                         # (before the operator runs: printed whatever happens next)
    got, _ = op_grads(dev, x, off, w, b, mask, R)
    if mask is None:
        assert got["gmask"] is None and ref["gmask"] is None
    check(str(CASES[i]), got, ref, [n for n in NAMES if ref[n] is not None], gates)


# ---- known answers ----
def test_zero_offset_unit_mask_is_conv2d_backward(dev):
    B, Ci, Co, H, W = 2, 32, 6, 13, 17
    x, w, b, R = rnd(B, Ci, H, W), rnd(Co, Ci, 3, 3, seed=1, scale=1 / 17), rnd(Co, seed=2), rnd(B, Co, H, W, seed=3)
    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, w, b))
    (F.conv2d(xd, wd, bd, 1, 1) * R.double()).sum().backward()
    got, _ = op_grads(dev, x, torch.zeros(B, 18, H, W), w, b, torch.ones(B, 9, H, W), R)
    check("zero offset", got, {"gx": xd.grad, "gw": wd.grad, "gbias": bd.grad}, ("gx", "gw", "gbias"))


def test_integer_offset_on_one_tap_is_the_shifted_conv_backward(dev):
    B, Ci, Co, H, W, tap, dy, dx = 1, 32, 5, 12, 15, 4, 1, -2
    x, w, b, R = rnd(B, Ci, H, W), rnd(Co, Ci, 3, 3, seed=1, scale=1 / 17), rnd(Co, seed=2), rnd(B, Co, H, W, seed=3)
    off = torch.zeros(B, 18, H, W)
    off[:, 2 * tap], off[:, 2 * tap + 1] = float(dy), float(dx)
    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, w, b))
    keep = torch.ones(1, 1, 3, 3, dtype=torch.float64)
    keep[0, 0, tap // 3, tap % 3] = 0.0
    Pd = 4
    xp = F.pad(xd, (Pd, Pd, Pd, Pd))
    y0, x0 = Pd - 1 + tap // 3 + dy, Pd - 1 + tap % 3 + dx
    shifted = xp[:, :, y0:y0 + H, x0:x0 + W]                      # what tap `tap` samples at every output pixel
    out = F.conv2d(xd, wd * keep, bd, 1, 1) + torch.einsum("oc,bchw->bohw", wd[:, :, tap // 3, tap % 3], shifted)
    (out * R.double()).sum().backward()
    mask = torch.ones(B, 9, H, W)
    got, _ = op_grads(dev, x, off, w, b, mask, R)
    check("integer offset", got, {"gx": xd.grad, "gw": wd.grad, "gbias": bd.grad}, ("gx", "gw", "gbias"))
    ref = oracle_grads(x, off, w, b, mask, R)                     # floor held constant: the right-hand derivative
    check("integer offset", got, ref, ("goffset", "gmask"))


def test_all_samples_out_of_range(dev):
    B, Ci, Co, H, W = 1, 32, 4, 6, 6
    x, w, b, R = rnd(B, Ci, H, W), rnd(Co, Ci, 3, 3, seed=1), rnd(Co, seed=2), rnd(B, Co, H, W, seed=3)
    got, _ = op_grads(dev, x, torch.full((B, 18, H, W), 100.0), w, b, torch.ones(B, 9, H, W), R)
    for n in ("gx", "gw", "goffset", "gmask"):
        assert torch.count_nonzero(got[n]) == 0, n
    check("all out of range", got, {"gbias": R.double().sum((0, 2, 3))}, ("gbias",))


def test_mask_gradient_does_not_depend_on_the_mask(dev):
    x, off, w, b, mask, R = make_case(1)
    other = torch.rand(mask.shape, generator=torch.Generator().manual_seed(5)) * 3.0
    g1, _ = op_grads(dev, x, off, w, b, mask, R)
    g2, _ = op_grads(dev, x, off, w, b, other, R)
    check("mask linearity", g2, {"gmask": g1["gmask"]}, ("gmask",))
    assert relerr(g2["goffset"], g1["goffset"]) > 1e-2            # (the offset gradient does depend on it)


# ---- what is launched ----
def test_only_the_kernels_needs_input_grad_asks_for_are_launched(dev, monkeypatch):
    from centerfusiondetect3d_amd import ops
    calls = []
    data, weight = ops.run_dcn_bwd_data, ops.run_dcn_bwd_weight
    monkeypatch.setattr(ops, "run_dcn_bwd_data", lambda a: (calls.append("data"), data(a))[1])
    monkeypatch.setattr(ops, "run_dcn_bwd_weight", lambda a: (calls.append("weight"), weight(a))[1])
    x, off, w, b, mask, R = make_case(0)
    ref = reference(0)
    got, _ = op_grads(dev, x, off, w, b, mask, R, need=(False, False, True, False, False))
    assert calls == ["weight"]
    assert [n for n in NAMES if got[n] is not None] == ["gw"]
    check("weight only", got, ref, ("gw",))
    del calls[:]
    got, _ = op_grads(dev, x, off, w, b, mask, R, need=(True, False, False, False, False))
    assert calls == ["data"]
    assert [n for n in NAMES if got[n] is not None] == ["gx"]
    check("input only", got, ref, ("gx",))
    del calls[:]
    got, _ = op_grads(dev, x, off, w, b, mask, R, need=(False, True, False, True, True))
    assert calls == ["data", "weight"]
    assert [n for n in NAMES if got[n] is not None] == ["goffset", "gbias", "gmask"]
    check("offset, bias, mask", got, ref, ("goffset", "gbias", "gmask"))


def test_weight_and_bias_gradients_are_bitwise_reproducible(dev):
    for i in (2, CASES.index((1, 512, 256, 35, 53, 2.0, True))):  # three slabs; seven capped ones, the last short
        x, off, w, b, mask, R = make_case(i)
        g1, _ = op_grads(dev, x, off, w, b, mask, R)
        g2, _ = op_grads(dev, x, off, w, b, mask, R)
        assert torch.equal(g1["gw"], g2["gw"]) and torch.equal(g1["gbias"], g2["gbias"]), CASES[i]
        check(f"second call {CASES[i]}", g2, reference(i), ("gx",), case_gates(i))   # (float atomics: compared under the gate only)


def test_the_reference_deformconv_call_sequence_trains(dev):
    """DeformConv.forward as the reference spells it (dla.py:456-472), now with a loss behind it: the gradient reaches
    conv_offset_mask's weight and bias, the DCN's weight and bias and the input, and equals the same graph's on the oracle in
    float64.  The graph has two kinks the comparison must stay clear of (checked on the CPU, on the float64 graph): a sampling
    coordinate on an integer and a ReLU input at zero."""
    from centerfusiondetect3d_amd.ops import deform_conv2d
    H, W = SEQ_SHAPE[3:]
    got, _, _ = sequence_grads(deform_conv2d, dev, torch.float32)
    assert got[4] is not None and got[0] is not None, "no gradient reaches the input / conv_offset_mask"
    ref, offset, z = sequence_grads(dcn_ref.deform_conv2d, "cpu", torch.float64)
    assert float(integer_distance(offset[0:1], H, W, torch.float64)) > 1e-5 and float(z.abs().min()) > 1e-5
    errs = {n: relerr(gg.cpu(), rr) for n, gg, rr in zip(SEQ_NAMES, got, ref)}
    print("[deform_conv2d backward] DeformConv sequence: " + "  ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    for n, e in errs.items():
        assert e <= SEQ_GATE, (n, e)


def test_no_grad_path_is_untouched(dev):
    from centerfusiondetect3d_amd import ops
    x, off, w, b, mask, _ = (None if t is None else t.to(dev) for t in make_case(1))
    a = ops.deform_conv2d(x, off, w, b, S, P, D, mask)
    assert a.grad_fn is None and not a.requires_grad
    assert torch.equal(a, ops.deform_conv2d(x, off, w, b, S, P, D, mask))
    wp = torch.nn.Parameter(w)
    with torch.no_grad():
        c = ops.deform_conv2d(x, off, wp, b, S, P, D, mask)
    assert c.grad_fn is None and not c.requires_grad and torch.equal(a, c)


def test_double_backward_raises(dev):
    from centerfusiondetect3d_amd import ops
    x, off, w, b, mask, R = (None if t is None else t.to(dev) for t in make_case(0))
    x.requires_grad_(True)
    out = ops.deform_conv2d(x, off, w, b, S, P, D, mask)
    assert out.grad_fn is not None
    (gx,) = torch.autograd.grad((out * out).sum(), x, create_graph=True)     # (grad_output = 2 out: it requires grad)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gx.sum().backward()
