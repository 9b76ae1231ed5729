"""Uncertainty-weighted decode and the depth-map launch, what they cost (no threshold: figures for docs/history.md).  bs = 16 on
112 x 200 maps, K = 100, on one MI355X, HIP events around each launch, alternating on one box in one process:

  * cf_decode_post / cf_decode_post_unc and cf_decode_gather / cf_decode_gather_unc on the same peaks and maps;
  * cf_depth_maps on three maps (depth, pc_hm_out, and pc_hm_in as the channel-0 view of a (B,3,H,W) tensor).

`--lib PATH` times the two plain decode exports of ANOTHER build of libcfhip.so (the parent commit's) beside this tree's, in the
same process and rounds: the default decode must not move beyond the run-to-run spread.

    python tools/bench_uncertainty.py [--batch 16] [--launches 200] [--rounds 3] [--lib PATH] [--out FILE]"""
import argparse
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(ms):
    s = sorted(ms)
    return f"min {s[0] * 1e3:7.2f}  p50 {s[len(s) // 2] * 1e3:7.2f}  p90 {s[len(s) * 9 // 10] * 1e3:7.2f}  max {s[-1] * 1e3:7.2f} us  (n = {len(s)})"


def _timed(fn, n, warm=10):
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
    ap.add_argument("--height", type=int, default=112)
    ap.add_argument("--width", type=int, default=200)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from centerfusiondetect3d_amd import _lib, ops
    dev = torch.device("cuda:0")
    B, H, W, K = a.batch, a.height, a.width, 100
    g = torch.Generator(device="cpu").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    heat = torch.sigmoid(rnd(B, 10, H, W) * 1.2 - 3.0)
    scores, inds, classes = ops.topk_peaks(heat, K, nms=True)
    maps = {"reg": rnd(B, 2, H, W), "wh": rnd(B, 2, H, W), "depth": rnd(B, 1, H, W).abs() * 20 + 2, "rot": rnd(B, 8, H, W),
            "dim": rnd(B, 3, H, W).abs() + 0.1, "amodal": rnd(B, 2, H, W), "att": rnd(B, 8, H, W), "vel": rnd(B, 3, H, W)}
    unc = rnd(B, 1, H, W) * 0.5 - 0.5
    calib = torch.tensor([[1266.4, 0, 816.3, 0], [0, 1266.4, 491.5, 0], [0, 0, 1, 0]], device=dev).repeat(B, 1, 1).contiguous()
    tinv = torch.tensor([[8.0, 0, 0], [0, 8.0, 0]], device=dev)
    det = torch.empty((B, K, 33), device=dev)
    post = torch.empty((B, K, 54), device=dev)
    args, _keep = ops._decode_args(scores, inds, classes, maps, H, W, (H, W), False, det)
    lib, st = _lib.load(), _lib.stream_ptr()
    arms = {
        "cf_decode_post": lambda: lib.cf_decode_post(C.byref(args), calib.data_ptr(), tinv.data_ptr(), post.data_ptr(), st),
        "cf_decode_post_unc": lambda: lib.cf_decode_post_unc(C.byref(args), unc.data_ptr(), calib.data_ptr(), tinv.data_ptr(),
                                                             post.data_ptr(), st),
        "cf_decode_gather": lambda: lib.cf_decode_gather(C.byref(args), st),
        "cf_decode_gather_unc": lambda: lib.cf_decode_gather_unc(C.byref(args), unc.data_ptr(), st),
    }
    if a.lib:
        other = C.CDLL(os.path.abspath(a.lib))
        for name in ("cf_decode_post", "cf_decode_gather"):
            fn = getattr(other, name)
            fn.restype, fn.argtypes = _lib.SYMBOLS[name]
        arms["cf_decode_post   (--lib)"] = lambda: other.cf_decode_post(C.byref(args), calib.data_ptr(), tinv.data_ptr(),
                                                                        post.data_ptr(), st)
        arms["cf_decode_gather (--lib)"] = lambda: other.cf_decode_gather(C.byref(args), st)
    pc = torch.zeros((B, 3, H, W), device=dev)
    pc[:, 0] = (rnd(B, H, W) > 1.0).float() * rnd(B, H, W).abs()
    dmaps = [rnd(B, 1, H, W), rnd(B, 1, H, W).abs(), pc[:, :1]]
    dm_out = torch.empty((3, B, H, W), device=dev, dtype=torch.uint8)
    arms["cf_depth_maps (3 maps)"] = lambda: ops.depth_maps(dmaps, out=dm_out)
    lines = [f"bs {B}, {H} x {W} maps, K = {K}, {torch.cuda.get_device_name(0)}; microseconds per launch (HIP events around each)"]
    for r in range(a.rounds):
        for name, fn in arms.items():
            rc = fn()
            assert torch.is_tensor(rc) or rc == 0, (name, rc)
            lines.append(f"round {r}: {name:<26s} {_stats(_timed(fn, a.launches))}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
