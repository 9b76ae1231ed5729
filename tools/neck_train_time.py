"""Time of the neck's training step (forward_neck + backward to every dla_up / ida_up parameter and the four level maps' consumer)
at bs 16, 3 x 448 x 800, against the composition a user could run before: the reference's module order from F.conv2d,
ops.deform_conv2d, F.batch_norm and F.conv_transpose2d (NCHW, torch's own convolution / batch-norm kernels around the operator).
HIP events, median of 20 steps after 5 warm ones; then one more step with an event pair around every launch wrapper for the split.

    python tools/neck_train_time.py [--batch 16] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from centerfusiondetect3d_amd import config as cfgm, getModel, ops  # noqa: E402

WRAPPED = ("run_conv_f16", "run_offmask_activate", "run_dcn", "run_bn_relu_forward", "upsample_dw", "run_bn_relu_backward", "run_dcn_bwd_data",
           "run_dcn_bwd_weight", "run_conv3x3_bwd_weight", "run_conv3x3_bwd_data", "run_upsample_dw_bwd")


def timed(fn, warm=5, steps=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def torch_neck(m, levels):
    """the reference's neck in its module order on torch's kernels + ops.deform_conv2d, batch statistics (momentum 0: the
    model's running statistics stay as they are)"""
    g, b = m.get_parameter, m.get_buffer

    def block(p, x):
        om = F.conv2d(x, g(p + ".conv_offset_mask.weight"), g(p + ".conv_offset_mask.bias"), padding=1)
        o1, o2, mask = torch.chunk(om, 3, dim=1)
        y = ops.deform_conv2d(x, torch.cat((o1, o2), dim=1), g(p + ".weight"), g(p + ".bias"), padding=(1, 1), mask=torch.sigmoid(mask))
        return F.relu(F.batch_norm(y, b(p + ".activation.0.running_mean").clone(), b(p + ".activation.0.running_var").clone(),
                                   g(p + ".activation.0.weight"), g(p + ".activation.0.bias"), True, 0.1, 1e-5))

    def ida(p, layers, startp, endp):
        for i in range(startp + 1, endp):
            j = i - startp
            w = g(f"{p}.up_{j}.weight")
            f = w.shape[-1] // 2
            up = F.conv_transpose2d(block(f"{p}.proj_{j}", layers[i]), w, stride=f, padding=f // 2, groups=w.shape[0])
            layers[i] = block(f"{p}.node_{j}", up + layers[i - 1])

    layers = list(levels)
    out = [layers[-1]]
    for i in range(3):
        ida(f"dla_up.ida_{i}", layers, len(layers) - i - 2, len(layers))
        out.insert(0, layers[-1])
    y = out[:3]
    ida("ida_up", y, 0, 3)
    return y[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    c = cfgm.centernet_config((448, 800))
    c.MODEL.FREEZE_BACKBONE = True
    m = getModel(cfgm.update_loss_weights(c))
    with torch.no_grad():
        for name, p in m.named_parameters():
            if ".conv_offset_mask." in name:
                p.normal_(0.0, 0.02 if name.endswith("weight") else 0.3)
    m = m.to(dev)
    x = torch.randn(a.batch, 3, 448, 800, device=dev)
    m.calibrate(x)                                   # per-layer pre-scales: no range check (host sync) per block
    m.unfreeze_neck().train()
    levels = m.forward_base(x)
    R = torch.randn(a.batch, 64, 112, 200, device=dev)

    def zero():
        for p in m.parameters():
            p.grad = None

    def hip_step():
        zero()
        m.forward_neck(levels).backward(R)

    def torch_step():
        zero()
        torch_neck(m, levels).backward(R)

    res = {"batch": a.batch, "hip_ms": timed(hip_step), "hip_forward_ms": timed(lambda: m.forward_neck(levels))}
    prev = ops.set_dcn_range_check(False)            # (the comparison pays no host sync either)
    res["torch_ms"] = timed(torch_step)
    res["torch_forward_ms"] = timed(lambda: torch_neck(m, levels))
    ops.set_dcn_range_check(prev)

    spans, orig = [], {n: getattr(ops, n) for n in WRAPPED}

    def wrap(name, fn):
        def inner(*args, **kw):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            r = fn(*args, **kw)
            e.record()
            spans.append((name, s, e))
            return r
        return inner
    for n, fn in orig.items():
        setattr(ops, n, wrap(n, fn))
    hip_step()
    torch.cuda.synchronize()
    for n, fn in orig.items():
        setattr(ops, n, fn)
    split = {}
    for n, s, e in spans:
        split[n] = split.get(n, 0.0) + s.elapsed_time(e)
    res["hip_split_ms"] = {k: round(v, 3) for k, v in split.items()}
    res["hip_split_calls"] = {k: sum(1 for n, _, _ in spans if n == k) for k in split}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
