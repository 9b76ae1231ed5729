"""Shared reference of the head input-gradient tests (tests/test_heads_dgrad_cpu.py, tests/test_gpu_heads_input_grad.py): the
gradient of the cases of tests/heads_train_ref.py with respect to their sources - gx for `x`, gx2 for the second source `x2` -
from the reference-structured head on the CPU, in float64 as the reference and in fp32 as the oracle whose own error sets the
gate (`heads_train_ref.case_gate`: 5e-6 where that error is below 2.5e-6, twice the error above, unusable above 1.25e-5).
Nothing of the kernel enters a gate.  The constructions of heads_train_ref keep the ReLU masks of fp32 and float64 identical, so
the two runs differentiate the same piecewise-linear function."""
import functools

import torch

from tests.heads_train_ref import CASES, REPLICATED, build, _conv, final_act, rel_err, case_gate, rep_build, rep_sources  # noqa: F401


def run_reference(case, dtype):
    """-> dict(y, out, gx, gx2 | None, gw, gb) of the head on the CPU in `dtype`: conv3x3 -> ReLU -> [conv1x1 -> ReLU]* ->
    conv1x1 -> the case's final activation, the case's dy arriving at the activated map"""
    c_x = case["x"].shape[1]
    def leaf(t):                     # (a copy: the case's own tensors are shared and stay as they are)
        return t.detach().to(dtype).clone().requires_grad_(True)

    x = leaf(case["x"] if case["x2"] is None else torch.cat([case["x"], case["x2"]], 1))
    ws, bs = [leaf(w) for w in case["weights"]], [leaf(b) for b in case["biases"]]
    cur = x
    for l, (w, b) in enumerate(zip(ws, bs)):
        cur = _conv(cur, w, b)
        if l + 1 < len(ws):
            cur = torch.relu(cur)
    out = final_act(cur, case["final"])
    out.backward(case["dy"].to(dtype))
    g = x.grad
    return dict(y=cur.detach(), out=out.detach(), gx=g[:, :c_x].contiguous(), gx2=None if case["x2"] is None else g[:, c_x:].contiguous(),
                gw=[w.grad for w in ws], gb=[b.grad for b in bs])


@functools.lru_cache(maxsize=None)
def reference(name):
    """(float64 result, fp32 result) of case `name`, computed once"""
    case = build(name)
    return run_reference(case, torch.float64), run_reference(case, torch.float32)


@functools.lru_cache(maxsize=None)
def rep_reference(name):
    """(float64 result, fp32 result) of the batch of just the images of a replicated case that carry a dY: a head is per-image, so
    their gx is the replicated batch's at those images, and every other image's gx is exactly zero"""
    small = rep_build(name)["small"]
    return run_reference(small, torch.float64), run_reference(small, torch.float32)


def _errors(r64, r32):
    e = {"gx": rel_err(r32["gx"], r64["gx"])}
    if r64["gx2"] is not None:
        e["gx2"] = rel_err(r32["gx2"], r64["gx2"])
    return e


def oracle_errors(name):
    """{"gx": e, "gx2": e (cases with a second source)}: the fp32 CPU oracle's own error against float64"""
    return _errors(*reference(name))


def rep_oracle_errors(name):
    return _errors(*rep_reference(name))


def gates(errors):
    """{label: gate} by the project's rule; raises where the oracle is unusable"""
    return {k: case_gate(v) for k, v in errors.items()}
