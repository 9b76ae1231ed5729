"""Dev tool (GPU box): time forward + backward of the criterion at the workload's size - B = 16, 10 classes, 112 x 200 maps,
M = 128 object slots, the middle-fusion heads - for two arms on one device, alternating call by call after a warm-up:
  hip    centerfusiondetect3d_amd.GenericLoss (cf_loss_forward / cf_loss_backward)
  torch  tests/loss_ref.generic_loss on the device in fp32: the criterion as plain torch ops (gathers on the NCHW maps and
         torch.where for the zero-count branches, so it has neither the reference's NHWC copies nor its host syncs - the
         reference's own module can only be slower than this arm)
Each timed call is zero_grad (set to None) + forward + total.backward(), between two HIP events; the arms' totals are compared
first (faster and different is not faster).
    python tools/bench_loss.py [--calls 100] [--warmup 20] [--batch 16] [--out FILE]
Prints median / p95 / min per arm in microseconds and one JSON line; the bytes a forward has to read (the two heat maps) over
the hip arm's time is printed as an orientation, not as a kernel rate (the time includes the host side of four launches)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_inputs(B, C, h, w, M, dev):
    """seeded maps and batch at the benchmark's size: tests/loss_ref.py's object rows and targets, maps of the middle-fusion heads"""
    import torch
    from tests import loss_ref
    g = torch.Generator().manual_seed(9)
    centers, cls, mask, wh = loss_ref._object_rows(g, B, C, h, w, M, False, False)
    chans = {"reg": 2, "widthHeight": 2, "depth": 1, "rotation": 8, "dimension": 3, "amodal_offset": 2, "nuscenes_att": 8,
             "velocity": 3, "depth2": 1, "rotation2": 8}
    out = {"heatmap": torch.sigmoid(torch.randn(B, C, h, w, generator=g) * 2).clamp(1e-4, 1 - 1e-4)}
    out.update({k: torch.randn(B, ch, h, w, generator=g) for k, ch in chans.items()})
    batch = loss_ref._targets(g, B, M, torch.rand(B, C, h, w, generator=g) ** 4, mask, cls, wh, centers)
    out = {k: v.to(dev).requires_grad_(True) for k, v in out.items()}
    batch = {k: ({kk: vv.to(dev) for kk, vv in v.items()} if isinstance(v, dict) else v.to(dev)) for k, v in batch.items()}
    return [out], batch


def main():
    import torch
    from centerfusiondetect3d_amd import GenericLoss, centerfusion_middle_config, update_loss_weights
    from tests import loss_ref
    argv = sys.argv[1:]
    opt = lambda k, d: type(d)(argv[argv.index(k) + 1]) if k in argv else d
    calls, warmup, B, path = opt("--calls", 100), opt("--warmup", 20), opt("--batch", 16), opt("--out", "")
    assert torch.cuda.is_available(), "bench_loss.py measures on the GPU only"
    dev = torch.device("cuda:0")
    C, h, w, M = 10, 112, 200, 128
    cfg = update_loss_weights(centerfusion_middle_config((4 * h, 4 * w)))
    outputs, batch = make_inputs(B, C, h, w, M, dev)
    crit = GenericLoss(cfg, C).train()

    def clear():
        for v in outputs[0].values():
            v.grad = None

    def hip():
        total, _ = crit(outputs, batch)
        total.backward()
        return total

    def torch_arm():
        total, _ = loss_ref.generic_loss(outputs, batch, cfg, True, torch.float32)
        total.backward()
        return total
    arms = {"hip": hip, "torch": torch_arm}

    totals, grads = {}, {}
    for name, fn in arms.items():
        clear()
        totals[name] = float(fn().detach())
        grads[name] = {k: v.grad.clone() for k, v in outputs[0].items()}
    rel = abs(totals["hip"] - totals["torch"]) / abs(totals["torch"])
    gerr = max(float((grads["hip"][k] - grads["torch"][k]).abs().max() / grads["torch"][k].abs().max()) for k in grads["hip"])
    print(f"totals: hip {totals['hip']:.8g}  torch {totals['torch']:.8g}  rel {rel:.2e}; worst gradient difference {gerr:.2e} of max", flush=True)
    assert rel < 1e-5 and gerr < 1e-5, "the two arms do not compute the same thing"

    spin = torch.randn(4096, 4096, device=dev)
    for _ in range(30):
        spin = (spin @ spin) * 1e-4                # warm the clocks
    for _ in range(warmup):
        for fn in arms.values():
            clear()
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in arms}
    for _ in range(calls):
        for name, fn in arms.items():             # alternating: both arms see the same machine state
            clear()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3)
    res = {"B": B, "C": C, "h": h, "w": w, "M": M, "calls": calls, "device": torch.cuda.get_device_name(0)}
    for name, t in times.items():
        t = sorted(t)
        res[name] = {"median_us": t[len(t) // 2], "p95_us": t[min(len(t) - 1, int(0.95 * len(t)))], "min_us": t[0]}
        print(f"{name:6s} forward + backward: median {res[name]['median_us']:9.1f} us  p95 {res[name]['p95_us']:9.1f} us  "
              f"min {res[name]['min_us']:9.1f} us  ({calls} calls)")
    heat_bytes = 2 * B * C * h * w * 4
    print(f"heat maps read by a forward: {heat_bytes / 1e6:.1f} MB; over the hip arm's whole median call: "
          f"{heat_bytes / res['hip']['median_us'] / 1e6:.3f} TB/s (host side of the launches included)")
    res["speedup_median"] = res["torch"]["median_us"] / res["hip"]["median_us"]
    line = json.dumps(res)
    print(line)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
