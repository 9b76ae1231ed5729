"""Time of the stem's training step (forward_stem_train + backward to every base.base_layer / level0 / level1 parameter) at bs 16,
3 x 448 x 800, against the same three blocks from F.conv2d / F.batch_norm in torch's NHWC memory format (channels_last) on the same
parameters, same machine, same run.  HIP events, median of 20 steps after 5 warm ones with min and max; forward + backward and
forward alone; then one more step with an event pair around every launch wrapper for the split, and the peak memory autograd
holds between the forward and the backward (the saved maps are about 0.37 GB each at this size).

    python tools/stem_train_time.py [--batch 16] [--early] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from centerfusiondetect3d_amd import config as cfgm, getModel, ops  # noqa: E402

WRAPPED = ("run_stem_conv_forward", "run_bn_act_forward", "run_bn_act_backward", "run_stem_conv_bwd_weight", "run_stem_conv_bwd_data",
           "nhwc_to_nchw", "nchw_to_nhwc")
STEM = (("base.base_layer", 1), ("base.level0", 1), ("base.level1", 2))


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
    return round(statistics.median(ms), 3), round(min(ms), 3), round(max(ms), 3)


def torch_stem(m, x):
    """base_layer, level0, level1 on torch's kernels, channels_last, batch statistics (copies of the running statistics: the
    model's stay as they are); x: the three- or six-channel image"""
    g, b = m.get_parameter, m.get_buffer
    t = x
    for p, stride in STEM:
        w = g(p + ".0.weight")
        z = F.conv2d(t, w, None, stride=stride, padding=(w.shape[-1] - 1) // 2)
        t = F.relu(F.batch_norm(z, b(p + ".1.running_mean").clone(), b(p + ".1.running_var").clone(), g(p + ".1.weight"),
                                g(p + ".1.bias"), True, 0.1, 1e-5))
    return t


def held(fn):
    """bytes allocated while fn()'s result - and the graph autograd saved for it - is alive, over what was allocated before"""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    y = fn()
    torch.cuda.synchronize()
    n = torch.cuda.memory_allocated() - base
    del y
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--early", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    c = (cfgm.centerfusion_early_config if a.early else cfgm.centernet_config)((448, 800))
    c.MODEL.FREEZE_BACKBONE = True
    m = getModel(cfgm.update_loss_weights(c)).to(dev)
    x = torch.randn(a.batch, 3, 448, 800, device=dev)
    pc = torch.rand(a.batch, 3, 112, 200, device=dev) if a.early else None
    m.unfreeze_stem().train()
    x_cl = x if pc is None else torch.cat([x, F.interpolate(pc, size=x.shape[-2:], mode="nearest")], dim=1)
    x_cl = x_cl.contiguous(memory_format=torch.channels_last)
    R = torch.randn(a.batch, 32, 224, 400, device=dev)
    R_cl = R.contiguous(memory_format=torch.channels_last)

    def zero():
        for p in m.parameters():
            p.grad = None

    def hip_step():
        zero()
        m.forward_stem_train(x, pc).backward(R)

    def torch_step():
        zero()
        torch_stem(m, x_cl).backward(R_cl)

    res = {"batch": a.batch, "early": bool(a.early), "hip_ms": timed(hip_step), "hip_forward_ms": timed(lambda: m.forward_stem_train(x, pc)),
           "torch_ms": timed(torch_step), "torch_forward_ms": timed(lambda: torch_stem(m, x_cl))}
    res["hip_held_gb"] = round(held(lambda: m.forward_stem_train(x, pc)) / 1e9, 3)
    res["torch_held_gb"] = round(held(lambda: torch_stem(m, x_cl)) / 1e9, 3)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    hip_step()
    torch.cuda.synchronize()
    res["hip_step_peak_gb"] = round((torch.cuda.max_memory_allocated() - base) / 1e9, 3)
    zero()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    torch_step()
    torch.cuda.synchronize()
    res["torch_step_peak_gb"] = round((torch.cuda.max_memory_allocated() - base) / 1e9, 3)

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
    res["hip_launches_ms"] = [(n, round(s.elapsed_time(e), 3)) for n, s, e in spans]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
