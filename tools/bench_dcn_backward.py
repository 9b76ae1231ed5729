"""Dev tool (GPU box): time cf_dcn_v2_bwd_data and cf_dcn_v2_bwd_weight on layer shapes with HIP events, back to back after a
warm-up.  Every shape runs in a child process of its own under a time limit.
    python tools/bench_dcn_backward.py [B,C,N,H,W ...] [--mag 2.0] [--limit 120]
Prints per kernel the time, for the data kernel the atomic bytes of gx (M * 9 taps * 4 corners * C * 4 B: every corner counted as
valid) over the time, and the GEMM FLOPs (2 * M * N * 9 C per kernel) over the time."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 64, 64, 112, 200), (16, 64, 64, 112, 200), (1, 256, 256, 28, 50)]


def one(B, C, N, H, W, mag):
    sys.path.insert(0, ROOT)
    import torch
    from centerfusiondetect3d_amd import ops, _lib
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, H, W, C, generator=g).to(dev)
    om = torch.zeros(B, H, W, 32)
    om[..., :18] = torch.randn(B, H, W, 18, generator=g) * mag
    om[..., 18:27] = torch.sigmoid(torch.randn(B, H, W, 9, generator=g))
    om = om.to(dev)
    w = (torch.randn(N, C, 3, 3, generator=g) * (C * 9) ** -0.5).to(dev)
    gout = torch.randn(B, H, W, N, generator=g).to(dev)
    gx, gom = torch.zeros_like(x), torch.empty_like(om)
    gw, gb = torch.empty_like(w), torch.empty(N, device=dev)
    ws = torch.empty(_lib.load().cf_dcn_v2_bwd_workspace_bytes(B, H, W, C, N), device=dev, dtype=torch.uint8)
    a = ops.dcn_bwd_args(gout, x, om, weight=w, gx=gx, gom=gom, gw=gw, gbias=gb, workspace=ws)
    spin = torch.randn(4096, 4096, device=dev)
    for _ in range(30):
        spin = (spin @ spin) * 1e-4            # warm the clocks
    M, flops = B * H * W, 2.0 * B * H * W * N * 9 * C
    res = {}
    for name, run in (("data", ops.run_dcn_bwd_data), ("weight", ops.run_dcn_bwd_weight)):
        best = 1e9
        for rep in range(3):
            for _ in range(3):
                run(a)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                run(a)
            e1.record()
            torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1) * 50)       # us per launch
        res[name] = best
    ab = M * 9 * 4 * C * 4
    print(f"{B}x{C}->{N} {H}x{W} offsets ~{mag} px | data {res['data']:9.1f} us  gx atomics {ab / 1e6:8.1f} MB "
          f"{ab / res['data'] / 1e6:6.3f} TB/s  {flops / res['data'] / 1e6:6.2f} TFLOP/s | weight {res['weight']:9.1f} us  "
          f"{flops / res['weight'] / 1e6:6.2f} TFLOP/s  (workspace {ws.numel() / 1e6:.1f} MB)", flush=True)


def main():
    argv = sys.argv[1:]
    opt = lambda k, d: float(argv[argv.index(k) + 1]) if k in argv else d
    mag, limit = opt("--mag", 2.0), opt("--limit", 120.0)
    if "--one" in argv:
        return one(*(int(v) for v in argv[argv.index("--one") + 1].split(",")), mag)
    skip = {i + 1 for i, a in enumerate(argv) if a in ("--mag", "--limit")}
    shapes = [tuple(int(v) for v in a.split(",")) for i, a in enumerate(argv) if not a.startswith("--") and i not in skip] or SHAPES
    for s in shapes:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", ",".join(str(v) for v in s), "--mag", str(mag)],
                           timeout=limit)
        if r.returncode:                       # a run that failed ends the series: nothing more is started on the device
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
