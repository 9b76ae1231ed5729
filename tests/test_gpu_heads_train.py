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
    dy_1x40_c2          1.8e-07 (y)       dy_40x1_sec_c2      5.1e-07 (y)       dy_1x1_c3           2.3e-07 (y)
    dy_nh1_c4           1.0e-06 (gw0)     dy_cx72_sec_c3      2.9e-07 (y)       dy_cx8_c2           3.0e-07 (y)
    lin_cin512_c2       8.3e-07 (y)       lin_8img_dense_c3   1.6e-06 (gb1)     lin_8img_5chunks_c2 1.3e-06 (gw0)
    lin_8img_1500_c2    5.9e-07 (gb0)     lin_8img_heat_c10   2.0e-06 (gb0)     lin_1img_nh1_c16    8.8e-07 (gw0)
    rep234_gridcaps     9.8e-07 (gw1)     rep64_default_chunk 1.7e-06 (gb2)

so every gate is 5e-6 (the test computes them again from the oracle, on the CPU).  The all-zero case is held to exact zeros.

The replicated cases (heads_train_ref.REPLICATED) reach the sizes a direct reference cannot: R copies of a base batch.  Every
replica's raw map is held to the base's float64 map and is bit-identical to replica 0's and to the operator's map of the base
alone; the gradients are held to the float64 run of just the images that carry a dY, gated by the fp32 run of that same batch.
The strided test reads the first case's sources through row strides above the channel counts, through a stride that is no
multiple of 4 and from a pointer that is not 16-byte aligned, the padding filled with NaN: an over-read shows even where it is
multiplied by zero.

What stays untested: the grid-stride loop of `head_gemm_kernel` in the BACKWARD (a list above 131,072 positions in one chunk; the
forward's is reached by rep234_gridcaps), and dense gradients above 4,488 positions: at 35,904 dense positions the fp32 CPU
oracle's own error on gb1 / gb2 is 1.2e-5 / 1.7e-5, beyond what the rule accepts as a reference, so no gate can be stated."""
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


@pytest.mark.parametrize("name", list(T.REPLICATED))
def test_replicated_batch_against_float64(dev, name):
    from centerfusiondetect3d_amd import ops
    rep = T.rep_build(name)
    base, R = rep["base"], rep["R"]
    r64_base, _ = T.reference(T.REPLICATED[name][0])
    r64, _ = T.rep_reference(name)
    oracle = T.rep_oracle_errors(name)
    ws = [w.float().to(dev).requires_grad_(True) for w in base["weights"]]
    bs = [b.float().to(dev).requires_grad_(True) for b in base["biases"]]
    x, x2 = (None if t is None else t.to(dev) for t in T.rep_sources(name))
    y = ops.head_stack(x, ws, bs, x2=x2, chunk_px=rep["chunk_px"])
    y.backward(rep["dy_full"].to(dev))
    with torch.no_grad():
        alone = ops.head_stack(base["x"].float().to(dev), ws, bs, x2=None if x2 is None else base["x2"].float().to(dev))
    torch.cuda.synchronize()
    got = y.detach().view(R, *alone.shape)
    same_as_first, same_as_alone = bool((got == got[:1]).all()), bool((got == alone[None]).all())
    failures = []
    assert torch.isfinite(got).all()
    # every replica's map against the base's float64 map (the worst replica: max |got - ref| over all / max |ref|)
    e, gate = T.rel_err(got.cpu(), r64_base["y"][None]), T.case_gate(oracle["y"])
    print(f"[head_stack] {name:20s} y   : error {e:.2e}   fp32 oracle {oracle['y']:.2e}   gate {gate:.1e}")
    if not e <= gate:
        failures.append(("y", e, gate))
    res = dict(gw=[w.grad.cpu() for w in ws], gb=[b.grad.cpu() for b in bs])
    del x, x2, y, got
    torch.cuda.empty_cache()
    for (label, ref), (_, val) in zip(T.quantities(r64)[2:], T.quantities(dict(y=None, out=None, **res))[2:]):
        assert val.shape == ref.shape and val.dtype == torch.float32
        assert torch.isfinite(val).all(), label
        e, gate = T.rel_err(val, ref), T.case_gate(oracle[label])
        print(f"[head_stack] {name:20s} {label:4s}: error {e:.2e}   fp32 oracle {oracle[label]:.2e}   gate {gate:.1e}")
        if not e <= gate:
            failures.append((label, e, gate))
    assert not failures, failures
    assert same_as_first, "a replica's map differs from replica 0's in some bit"
    assert same_as_alone, "a replica's map differs in some bit from the operator's map of the base alone"


def _padded(t_nhwc, stride, dev):
    """the (B,h,w,C) tensor as the leading channels of a contiguous (B,h,w,stride) one whose other channels are NaN"""
    out = torch.full((*t_nhwc.shape[:3], stride), float("nan"), device=dev)
    out[..., :t_nhwc.shape[3]] = t_nhwc
    return out


@pytest.mark.parametrize("variant", ["s80_nhwc4", "s66", "misaligned"])
def test_strided_and_misaligned_sources(dev, variant):
    """dy_17x33_sec_c3 through ops.head_stack_nhwc: rows wider than the channels read (NaN behind them), a row stride that is no
    multiple of 4 and a source that is not 16-byte aligned (both: no vector loads) - same float64 reference, same gates, and the
    forward's bits are the packed call's (the case is dyadic: every summation order gives the exact hidden maps)"""
    from centerfusiondetect3d_amd import ops
    name = "dy_17x33_sec_c3"
    case, (r64, _), oracle = T.build(name), T.reference(name), T.oracle_errors(name)
    xp = case["x"].float().to(dev).permute(0, 2, 3, 1).contiguous()
    x2p = case["x2"].float().to(dev).permute(0, 2, 3, 1).contiguous()
    c_x, c_x2 = xp.shape[3], x2p.shape[3]
    if variant == "s80_nhwc4":
        xn, x2n = _padded(xp, 80, dev), _padded(x2p, 4, dev)
        assert torch.isnan(xn[..., c_x:]).all() and torch.isnan(x2n[..., c_x2:]).all()
    elif variant == "s66":
        xn, x2n = _padded(xp, 66, dev), x2p
        assert xn.shape[3] % 4 and torch.isnan(xn[..., c_x:]).all()
    else:
        store = torch.empty(xp.numel() + 1, device=dev)
        xn, x2n = store[1:].view(xp.shape), x2p
        xn.copy_(xp)
        assert store.data_ptr() % 16 == 0 and xn.data_ptr() % 16 == 4 and xn.is_contiguous() and torch.equal(xn, xp)
    ws = [w.float().to(dev).requires_grad_(True) for w in case["weights"]]
    bs = [b.float().to(dev).requires_grad_(True) for b in case["biases"]]
    with torch.no_grad():
        packed = ops.head_stack_nhwc(xp, c_x, x2p, c_x2, ws, bs)
    y = ops.head_stack_nhwc(xn, c_x, x2n, c_x2, ws, bs)
    y.backward(case["dy"].float().to(dev))
    torch.cuda.synchronize()
    got = dict(y=y.detach().cpu(), out=y.detach().cpu(), gw=[w.grad.cpu() for w in ws], gb=[b.grad.cpu() for b in bs])
    failures = []
    for (label, ref), (_, val) in zip(T.quantities(r64), T.quantities(got)):
        assert val.shape == ref.shape and val.dtype == torch.float32
        e, gate = T.rel_err(val, ref), T.case_gate(oracle[label])
        print(f"[head_stack] {variant:20s} {label:4s}: error {e:.2e}   fp32 oracle {oracle[label]:.2e}   gate {gate:.1e}")
        if not bool(torch.isfinite(val).all()):
            failures.append((label, "not finite"))
        elif not e <= gate:
            failures.append((label, e, gate))
    assert not failures, failures
    assert torch.equal(y.detach(), packed), "the forward's bits differ from the packed call's"


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
