"""Early radar fusion, what it costs (no threshold: figures for docs/experiments/early_fusion_ab.txt).  bs = 16 at 448 x 800 on
one MI355X, bench.py's seeded inputs, alternating on one box in one process:

  * the stem launch alone, HIP events around each launch: cf_stem_fused_early / cf_stem_fused / early / ... (--launches each);
  * forward + decode (fusionDecode) per step, HIP events around each step: early / image-only / middle fusion / early / ...

    python tools/bench_early.py [--batch 16] [--launches 30] [--steps 20] [--rounds 3] [--out FILE]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(ms):
    s = sorted(ms)
    return f"min {s[0]:.4f}  p50 {s[len(s) // 2]:.4f}  max {s[-1]:.4f}  (n = {len(s)})"


def _timed(fn, n, warm=5):
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--height", type=int, default=448)
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bench
    from centerfusiondetect3d_amd import (getModel, fusionDecode, ops, packing, centerfusion_early_config,
                                          centerfusion_middle_config, centernet_config)
    dev = torch.device("cuda:0")
    B, H, W = a.batch, a.height, a.width
    images, pc_dep, calib = bench.make_inputs(B, H, W, dev, 0)
    lines = [f"bs {B}, {H} x {W}, {torch.cuda.get_device_name(0)}; ms per launch / per step (HIP events)"]

    torch.manual_seed(0)
    models = {}
    for name, cfg in (("early", centerfusion_early_config), ("image-only", centernet_config), ("middle", centerfusion_middle_config)):
        models[name] = getModel(cfg((H, W))).to(dev).eval()
    # ---- the stem launch alone, on the early model's weights (the three-channel kernel on their image part)
    sd = models["early"].state_dict()
    bn = lambda n: tuple(sd[f"base.{n}.1.{k}"] for k in ("weight", "bias", "running_mean", "running_var"))
    folded = [t for n in ("base_layer", "level0", "level1") for t in packing.fold_bn(sd[f"base.{n}.0.weight"], None, bn(n))]
    pe = packing.pack_stem_early(*folded).to(dev)
    p3 = packing.pack_stem(folded[0][:, :3].contiguous(), *folded[1:]).to(dev)
    out = torch.empty((B, H // 2, W // 2, 32), device=dev)
    pool = torch.empty((B, H // 4, W // 4, 32), device=dev)
    pc_n = pc_dep.clone()
    pc_n[:, :1] = 1 - pc_n[:, :1] / 60.0
    for r in range(a.rounds):
        lines.append(f"stem alone, round {r}: cf_stem_fused_early  {_stats(_timed(lambda: ops.stem_fused_early(pe, images, pc_n, out, pool), a.launches))}")
        lines.append(f"stem alone, round {r}: cf_stem_fused        {_stats(_timed(lambda: ops.stem_fused(p3, images, out, pool), a.launches))}")

    # ---- forward + decode
    def step(name):
        m = models[name]
        kw = {} if name == "image-only" else dict(pc_dep=pc_dep.clone() if name == "early" else pc_dep)
        with torch.no_grad():
            fusionDecode(m(images, calib=calib, **kw), outputSize=(H // 4, W // 4), K=100)

    for r in range(a.rounds):
        for name in models:
            lines.append(f"forward + decode, round {r}: {name:>10s}  {_stats(_timed(lambda: step(name), a.steps))}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
