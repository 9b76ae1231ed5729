"""Time of the base's training step from level 2 upward (forward_levels + backward to every base.level[2-5] parameter) at bs 16,
3 x 448 x 800, against the same graph from F.conv2d / F.batch_norm / F.max_pool2d in torch's NHWC memory format (channels_last)
on the same parameters, same machine, same run.  HIP events, median of 20 steps after 5 warm ones; then one more step with an event
pair around every launch wrapper for the split, and the two convolution backward kernels alone on level 4's 256 -> 256 layer
against the fp32 MFMA peak.  The host re-pack of the forward weights after an optimizer step is not in these figures (the weights
do not change between the steps timed here), as in tools/neck_train_time.py.

    python tools/base_train_time.py [--batch 16] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from centerfusiondetect3d_amd import config as cfgm, getModel, ops  # noqa: E402

WRAPPED = ("run_conv_f16", "run_bn_act_forward", "maxpool2x2", "run_bn_act_backward", "run_conv_bwd_weight", "run_conv_bwd_data",
           "run_maxpool2x2_bwd")
LEVELS = ((2, 1, False), (3, 2, True), (4, 2, True), (5, 1, True))
FP32_MFMA_PEAK = 157e12           # FLOP/s of the fp32-input MFMA on one MI355X (the vector fp32 rate)


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


def torch_levels(m, x):
    """DLA.forward's levels 2-5 on torch's kernels, channels_last, batch statistics (copies of the running statistics: the
    model's stay as they are)"""
    g, b = m.get_parameter, m.get_buffer
    names = {n for n, _ in m.named_parameters()}

    def cba(conv, bn, t, stride=1, residual=None, relu=True):
        w = g(conv + ".weight")
        z = F.conv2d(t, w, None, stride=stride, padding=(w.shape[-1] - 1) // 2)
        z = F.batch_norm(z, b(bn + ".running_mean").clone(), b(bn + ".running_var").clone(), g(bn + ".weight"), g(bn + ".bias"), True,
                         0.1, 1e-5)
        if residual is not None:
            z = z + residual
        return F.relu(z) if relu else z

    def block(p, t, stride, residual):
        o = cba(p + ".conv1", p + ".bn1", t, stride=stride)
        return cba(p + ".conv2", p + ".bn2", o, residual=t if residual is None else residual)

    def tree(p, levels, t, stride, level_root, children=None):
        children = [] if children is None else children
        bottom = F.max_pool2d(t, stride, stride) if stride > 1 else t
        residual = cba(p + ".project.0", p + ".project.1", bottom, relu=False) if (p + ".project.0.weight") in names else bottom
        if level_root:
            children.append(bottom)
        if levels > 1:
            x1 = tree(p + ".tree1", levels - 1, t, stride, False)
            children.append(x1)
            return tree(p + ".tree2", levels - 1, x1, 1, False, children)
        x1 = block(p + ".tree1", t, stride, residual)
        x2 = block(p + ".tree2", x1, 1, None)
        return cba(p + ".root.conv", p + ".root.bn", torch.cat([x2, x1, *children], 1))

    out = []
    for lvl, levels, root in LEVELS:
        x = tree(f"base.level{lvl}", levels, x, 2, root)
        out.append(x)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    c = cfgm.centernet_config((448, 800))
    c.MODEL.FREEZE_BACKBONE = True
    m = getModel(cfgm.update_loss_weights(c)).to(dev)
    x = torch.randn(a.batch, 3, 448, 800, device=dev)
    m.calibrate(x)                                   # per-layer pre-scales: no range check (host sync) per block
    m.unfreeze_base().train()
    y1 = m.forward_stem(x)
    y1_cl = y1.contiguous(memory_format=torch.channels_last)
    Rs = [torch.randn(a.batch, ch, 224 >> (j + 1), 400 >> (j + 1), device=dev) for j, ch in enumerate((64, 128, 256, 512))]
    Rs_cl = [r.contiguous(memory_format=torch.channels_last) for r in Rs]

    def zero():
        for p in m.parameters():
            p.grad = None

    def hip_step():
        zero()
        torch.autograd.backward(m.forward_levels(y1), Rs)

    def torch_step():
        zero()
        torch.autograd.backward(torch_levels(m, y1_cl), Rs_cl)

    res = {"batch": a.batch, "hip_ms": timed(hip_step), "hip_forward_ms": timed(lambda: m.forward_levels(y1)),
           "torch_ms": timed(torch_step), "torch_forward_ms": timed(lambda: torch_levels(m, y1_cl))}

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

    # level 4's 256 -> 256 3x3 layer alone: the two backward kernels against the fp32 MFMA peak
    B, H, W, C = a.batch, 28, 50, 256
    xn, gz = torch.randn(B, H, W, C, device=dev), torch.randn(B, H, W, C, device=dev)
    w = torch.randn(C, C, 3, 3, device=dev) / 48.0
    flops = 2.0 * B * H * W * 9 * C * C
    for name, fn in (("cf_conv_bwd_weight", lambda: ops.run_conv_bwd_weight(gz, xn, 3, 1)),
                     ("cf_conv_bwd_data", lambda: ops.run_conv_bwd_data(gz, w, H, W, 1))):
        ms = timed(fn)[0]
        res[name + "_256_ms"] = round(ms, 4)
        res[name + "_256_peak_fraction"] = round(flops / (ms * 1e-3) / FP32_MFMA_PEAK, 4)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
