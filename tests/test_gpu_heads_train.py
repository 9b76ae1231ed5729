"""GPU: `ops.head_stack` (cf_head_train_forward / cf_head_backward) against the reference-structured head as a torch
nn.Sequential on the CPU in float64 (tests/heads_train_ref.py: cases, constructions, geometry).

Gate, per quantity (the raw map, the activated map, every layer's weight and bias gradient): max|got - ref64| / max|ref64| is
held by the project's rule (`heads_train_ref.case_gate`): 5e-6 where the fp32 CPU oracle's own error on that case and quantity is
below 2.5e-6, otherwise twice that error; a case whose oracle error exceeds 1.25e-5 is unusable.  Nothing of the kernel enters a
gate.  The oracle errors (tools/heads_train_oracle_error.py, CPU; the worst quantity of each case, and which it is):

    dy_5x7_c1           1.9e-07 (y)       dy_3x5_c1           3.0e-07 (y)       dy_one_tile_c2      2.4e-07 (y)
    dy_17x33_sec_c3     1.0e-06 (gw0)     dy_17x33_sparse_c8  1.9e-07 (y)       dy_zero_c10         3.6e-07 (y)
    lin_tile32_c16      3.7e-07 (y)       lin_tile33_c10      1.2e-06 (gw3)     lin_slab257_c2      1.1e-06 (gb0)
    lin_two_chunks_c2   2.2e-06 (gb1)     lin_heatmap_c3      1.3e-06 (gw0)     lin_depth_c1        5.7e-07 (y)

so every gate is 5e-6 (the test computes them again from the oracle, on the CPU).  The all-zero case is held to exact zeros."""
import pytest
import torch

from tests import heads_train_ref as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def run_hip(case, dev):
    """the case through ops.head_stack -> a result dict shaped like heads_train_ref.run_reference's"""
    from centerfusiondetect3d_amd import ops
    ws = [w.float().to(dev).requires_grad_(True) for w in case["weights"]]
    bs = [b.float().to(dev).requires_grad_(True) for b in case["biases"]]
    x = case["x"].float().to(dev)
    x2 = None if case["x2"] is None else case["x2"].float().to(dev)
    r = ops.head_stack(x, ws, bs, final=case["final"], x2=x2, chunk_px=case["chunk_px"])
    out, y = r if case["final"] is not None else (r, r)
    out.backward(case["dy"].float().to(dev))
    torch.cuda.synchronize()
    return dict(y=y.detach().cpu(), out=out.detach().cpu(), gw=[w.grad.cpu() for w in ws], gb=[b.grad.cpu() for b in bs])


@pytest.mark.parametrize("name", list(T.CASES))
def test_head_stack_against_float64(dev, name):
    case = T.build(name)
    r64, _ = T.reference(name)
    oracle = T.oracle_errors(name)
    got = run_hip(case, dev)
    failures = []
    for (label, ref), (_, val) in zip(T.quantities(r64), T.quantities(got)):
        assert val.shape == ref.shape and val.dtype == torch.float32
        assert torch.isfinite(val).all(), label
        e, gate = T.rel_err(val, ref), T.case_gate(oracle[label])
        print(f"[head_stack] {name:20s} {label:4s}: error {e:.2e}   fp32 oracle {oracle[label]:.2e}   gate {gate:.1e}")
        if float(ref.abs().max()) == 0.0:
            if not bool((val == 0).all()):
                failures.append((label, "not exactly zero"))
        elif not e <= gate:
            failures.append((label, e, gate))
    assert not failures, failures


def test_relu_mask_is_the_forwards_on_exact_zeros(dev):
    """dyadic case: hidden pre-activations that are exactly 0 exist (the CPU test counts them); a kernel that took ReLU'(0) = 1
    would miss the first layer's gradients by far more than the gate - pinned here against a float64 run that does so"""
    name = "dy_17x33_sec_c3"
    case, (r64, _) = T.build(name), T.reference(name)
    got = run_hip(case, dev)
    # float64 with ReLU'(0) = 1: relu(z) replaced by z * (z >= 0)
    x = torch.cat([case["x"], case["x2"]], 1)
    ws = [w.clone().requires_grad_(True) for w in case["weights"]]
    bs = [b.clone().requires_grad_(True) for b in case["biases"]]
    cur = x
    for l, (w, b) in enumerate(zip(ws, bs)):
        cur = T._conv(cur, w, b)
        if l + 1 < len(ws):
            cur = cur * (cur >= 0).double()
    cur.backward(case["dy"])
    wrong = T.rel_err(ws[0].grad, r64["gw"][0])
    assert wrong > 1e-4, "the case cannot tell the two conventions apart"
    assert T.rel_err(got["gw"][0], r64["gw"][0]) <= 5e-6


def test_forward_is_reproducible_and_no_grad_has_no_graph(dev):
    from centerfusiondetect3d_amd import ops
    case = T.build("dy_17x33_sec_c3")
    ws = [w.float().to(dev).requires_grad_(True) for w in case["weights"]]
    bs = [b.float().to(dev).requires_grad_(True) for b in case["biases"]]
    x, x2 = case["x"].float().to(dev), case["x2"].float().to(dev)
    a = ops.head_stack(x, ws, bs, x2=x2)
    b = ops.head_stack(x, ws, bs, x2=x2, chunk_px=576)           # another chunking, same bits
    assert a.grad_fn is not None and torch.equal(a, b)
    with torch.no_grad():
        c = ops.head_stack(x, ws, bs, x2=x2)
    assert c.grad_fn is None and torch.equal(a, c)
    with pytest.raises(NotImplementedError, match="frozen trunk"):
        ops.head_stack(x.clone().requires_grad_(True), ws, bs, x2=x2)
    # the second source is the concatenation, never materialised
    d = ops.head_stack(torch.cat([x, x2], 1), ws, bs)
    assert torch.equal(a, d)
