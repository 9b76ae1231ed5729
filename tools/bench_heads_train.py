"""Dev tool (GPU box): time forward + backward of the eleven middle-fusion detection heads on a frozen trunk's feature map at the
workload's size - B = 16, 448 x 800 input (112 x 200 maps), 64 feature channels + 3 radar channels for the secondary heads - for
five arms on one device, alternating step by step after a warm-up:
  hip_loss   ops.head_stack_nhwc (cf_head_train_forward / cf_head_backward) with a GenericLoss-shaped output gradient: non-zero at
             128 object centres per image for ten heads, dense for the heat map
  hip_dense  the same with every head's output gradient dense
  torch      the same heads as nn.Sequential of torch convolutions (NCHW, the concatenated 67-channel input for the secondary
             heads) with the loss-shaped gradient (dense torch autograd does the same work for any gradient)
  hip_loss_dx  hip_loss with the feature map requiring grad and input_grad=True (cf_head_backward_dx): the eleven heads' NHWC
             gradients of the map are summed by autograd
  torch_dx   torch with the same map requiring grad (the secondary heads' 67-channel input concatenated inside the step)
Each timed step is: grads to None, every head's forward, one torch.autograd.backward over all heads, between two HIP events.
    python tools/bench_heads_train.py [--steps 20] [--warmup 3] [--batch 16] [--out FILE] [--arms a,b] [--heads h1,h2]
--arms / --heads restrict the run (a profiler's trace of one arm on one head: the share of a kernel in its step).
Prints median / min / max per arm in milliseconds, the workspace bytes of the largest head's backward, and one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SECONDARY = ("velocity", "nuscenes_att", "depth2", "rotation2")


def main():
    import torch
    from torch import nn
    from centerfusiondetect3d_amd import _lib, ops, centerfusion_middle_config
    argv = sys.argv[1:]
    opt = lambda k, d: type(d)(argv[argv.index(k) + 1]) if k in argv else d
    steps, warmup, B, path = opt("--steps", 20), opt("--warmup", 3), opt("--batch", 16), opt("--out", "")
    only_arms, only_heads = opt("--arms", ""), opt("--heads", "")
    assert torch.cuda.is_available(), "bench_heads_train.py measures on the GPU only"
    dev = torch.device("cuda:0")
    h, w, M = 112, 200, 128
    cfg = centerfusion_middle_config((4 * h, 4 * w))
    g = torch.Generator().manual_seed(5)
    feat = torch.randn(B, h, w, 64, generator=g).to(dev)             # NHWC, as the trunk leaves it
    pc = torch.rand(B, h, w, 3, generator=g).to(dev)
    feat_nchw = feat.permute(0, 3, 1, 2).contiguous()
    cat_nchw = torch.cat([feat, pc], -1).permute(0, 3, 1, 2).contiguous()

    heads, seqs, dy_loss, dy_dense = {}, {}, {}, {}
    centres = torch.stack([torch.randperm(h * w, generator=g)[:M] for _ in range(B)])          # (B, M) pixel indices
    for name, cout in cfg.heads.items():
        if only_heads and name not in only_heads.split(","):
            continue
        widths = list(cfg.head_conv[name])
        cin = 67 if name in SECONDARY else 64
        layers, chans = [], [cin] + widths + [cout]
        for l in range(len(chans) - 1):
            layers.append(nn.Conv2d(chans[l], chans[l + 1], 3 if l == 0 else 1, padding=1 if l == 0 else 0))
            if l + 2 < len(chans):
                layers.append(nn.ReLU(inplace=True))
        seq = nn.Sequential(*layers).to(dev)
        seqs[name] = seq
        convs = [m for m in seq if isinstance(m, nn.Conv2d)]
        heads[name] = ([c.weight.detach().clone().requires_grad_(True) for c in convs],
                       [c.bias.detach().clone().requires_grad_(True) for c in convs])
        dense = torch.randn(B, cout, h, w, generator=g)
        keep = torch.zeros(B, h * w)
        keep.scatter_(1, centres, 1.0)
        dy_dense[name] = dense.to(dev)
        dy_loss[name] = (dense if name == "heatmap" else dense * keep.view(B, 1, h, w)).to(dev)

    feat_g = feat.clone().requires_grad_(True)                       # the arms with a gradient of the map
    feat_nchw_g = feat_nchw.clone().requires_grad_(True)
    pc_nchw = pc.permute(0, 3, 1, 2).contiguous()

    def hip(dys, dx=False):
        def step():
            for ws, bs in heads.values():
                for p in ws + bs:
                    p.grad = None
            feat_g.grad = None
            ys = [ops.head_stack_nhwc(feat_g if dx else feat, 64, pc if n in SECONDARY else None, 3 if n in SECONDARY else 0, ws, bs,
                                      input_grad=dx)
                  for n, (ws, bs) in heads.items()]
            torch.autograd.backward(ys, [dys[n] for n in heads])
        return step

    def torch_arm(dx=False):
        def step():
            for s in seqs.values():
                for p in s.parameters():
                    p.grad = None
            feat_nchw_g.grad = None
            if dx:
                cat = torch.cat([feat_nchw_g, pc_nchw], 1) if any(n in SECONDARY for n in heads) else None
                ys = [seqs[n](cat if n in SECONDARY else feat_nchw_g) for n in heads]
            else:
                ys = [seqs[n](cat_nchw if n in SECONDARY else feat_nchw) for n in heads]
            torch.autograd.backward(ys, [dy_loss[n] for n in heads])
        return step

    arms = {"hip_loss": hip(dy_loss), "hip_dense": hip(dy_dense), "torch": torch_arm(),
            "hip_loss_dx": hip(dy_loss, True), "torch_dx": torch_arm(True)}

    # the arms compute the same thing (faster and different is not faster): first-layer weight gradients, loss-shaped dY
    arms["hip_loss"]()
    arms["torch"]()
    torch.cuda.synchronize()
    # (a guard against a gross mismatch only: the HIP arm is held to float64 by tests/test_gpu_heads_train.py; torch's device
    #  convolutions are whatever MIOpen picks, and on random inputs a hidden unit within rounding of zero may take the other side
    #  of the ReLU in the two arms, which moves one weight-gradient column by ~1 / sqrt(active pixels))
    worst = 0.0
    for n, (ws, _) in heads.items():
        ref = [m for m in seqs[n] if isinstance(m, nn.Conv2d)][0].weight.grad
        d = float((ws[0].grad - ref).abs().max() / ref.abs().max())
        print(f"  {n:14s} first-layer weight gradient, hip_loss vs torch: {d:.2e} of max", flush=True)
        worst = max(worst, d)
    assert worst < 5e-2, "the two arms do not compute the same thing"
    # ... and so do the two arms with a gradient of the map (the same guard, on that gradient)
    arms["hip_loss_dx"]()
    arms["torch_dx"]()
    torch.cuda.synchronize()
    ref = feat_nchw_g.grad
    d = float((feat_g.grad.permute(0, 3, 1, 2) - ref).abs().max() / ref.abs().max())
    print(f"  gradient of the feature map, hip_loss_dx vs torch_dx: {d:.2e} of max", flush=True)
    assert d < 5e-2, "the two arms with a gradient of the map do not compute the same thing"
    if only_arms:
        arms = {k: v for k, v in arms.items() if k in only_arms.split(",")}

    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in arms}
    for _ in range(steps):
        for name, fn in arms.items():             # alternating: the arms see the same machine state
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    lib = _lib.load()
    res = {"B": B, "h": h, "w": w, "centres_per_image": M, "steps": steps, "device": torch.cuda.get_device_name(0),
           "workspace_bytes_backward_secondary": int(lib.cf_head_bwd_workspace_bytes(B, h, w, 67, 2, 0)),
           "workspace_bytes_backward_primary": int(lib.cf_head_bwd_workspace_bytes(B, h, w, 64, 0, 0)),
           "workspace_bytes_forward_secondary": int(lib.cf_head_train_workspace_bytes(B, h, w, 67, 2, 0)),
           "workspace_bytes_backward_dx_secondary": int(lib.cf_head_bwd_dx_workspace_bytes(B, h, w, 67, 2, 0)),
           "workspace_bytes_backward_dx_primary": int(lib.cf_head_bwd_dx_workspace_bytes(B, h, w, 64, 0, 0))}
    for name, t in times.items():
        t = sorted(t)
        res[name] = {"median_ms": t[len(t) // 2], "min_ms": t[0], "max_ms": t[-1]}
        print(f"{name:10s} heads forward + backward: median {res[name]['median_ms']:9.2f} ms  min {res[name]['min_ms']:9.2f} ms  "
              f"max {res[name]['max_ms']:9.2f} ms  ({steps} steps)")
    ratio = lambda a, b: res[a]["median_ms"] / res[b]["median_ms"] if a in res and b in res else None
    res["torch_over_hip_loss"] = ratio("torch", "hip_loss")
    res["hip_dense_over_hip_loss"] = ratio("hip_dense", "hip_loss")
    res["torch_dx_over_hip_loss_dx"] = ratio("torch_dx", "hip_loss_dx")
    res["hip_loss_dx_over_hip_loss"] = ratio("hip_loss_dx", "hip_loss")
    line = json.dumps(res)
    print(line)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
