"""Dev tool (GPU box): time the training inputs at the workload's size - B = 16 frames of 900 x 1600 -> 448 x 800 - in four arms:
  augment colour     centerfusiondetect3d_amd.augment_images (cf_augment_images: the stats and the finish launch) on device-resident
                     frames and parameters drawn by draw_augmentation with the default DATASET settings (shift 0.2, flip 0.5)
  augment plain      the same with colour=False (one launch: warp, / 255, Normalize)
  preprocess         preProcessImages at the same shape: the inference warp, the yardstick
  host               tests/train_inputs_ref.augment_frame per frame on one core (numpy warp + the torch-CPU fp32 chain), host clock
Each device call lies between two HIP events, after a clock warm-up.  The calls rotate over `--sets` copies of the frames and of
the output (default 6: 415 MB of frames, more than the 256 MB Infinity Cache, so that a call finds its source in HBM as a
training step does; `--sets 1` times the cache-resident case).  The arms' results are compared first: faster and different
is not faster.  The bytes are the algorithm's, from the shapes: the source once, the output once, and for `colour` the 4-byte
stash written and read once (frames whose shift leaves part of the output outside the source read less than that).
    python tools/bench_train_inputs.py [--calls 200] [--warmup 30] [--batch 16] [--host-frames 5] [--sets 6] [--out FILE]
Prints median / p95 / min per arm and one JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HS, WS, HD, WD = 900, 1600, 448, 800


def stats(ts):
    ts = sorted(ts)
    return {"median": ts[len(ts) // 2], "p95": ts[int(len(ts) * 0.95)], "min": ts[0], "n": len(ts)}


def main():
    import torch
    from centerfusiondetect3d_amd import augment_images, centerfusion_middle_config, draw_augmentation, preProcessImages
    from centerfusiondetect3d_amd.preprocess import NUSCENES_MEAN, NUSCENES_STD
    from tests import train_inputs_cases as cases
    from tests import train_inputs_ref as ref
    argv = sys.argv[1:]
    opt = lambda k, d: type(d)(argv[argv.index(k) + 1]) if k in argv else d
    calls, warmup, B, path = opt("--calls", 200), opt("--warmup", 30), opt("--batch", 16), opt("--out", "")
    host_frames, sets = opt("--host-frames", 5), opt("--sets", 6)
    assert torch.cuda.is_available(), "bench_train_inputs.py measures on the GPU only"
    dev = torch.device("cuda:0")
    cfg = centerfusion_middle_config((HD, WD))
    frames_h = np.concatenate([cases.frames_for(70 + i, 1, HS, WS) for i in range(B)])
    p_h = draw_augmentation(cfg, B, (HS, WS), np.random.RandomState(7), torch.Generator().manual_seed(7))
    frames, p = torch.from_numpy(frames_h).to(dev), p_h.to(dev)
    out = torch.empty((B, 3, HD, WD), device=dev, dtype=torch.float32)
    ring = [(frames, out)] + [(frames.clone(), torch.empty_like(out)) for _ in range(sets - 1)]
    turn = [0]

    def nxt():
        turn[0] = (turn[0] + 1) % sets
        return ring[turn[0]]

    def arm(fn):
        def call():
            f, o = nxt()
            return fn(f, o)
        return call

    arms = {"augment_colour": arm(lambda f, o: augment_images(f, p, (HD, WD), colour=True, out=o)),
            "augment_plain": arm(lambda f, o: augment_images(f, p, (HD, WD), colour=False, out=o)),
            "preprocess": arm(lambda f, o: preProcessImages(f, (HD, WD), out=o))}
    src, dst, stash = B * HS * WS * 3, B * 3 * HD * WD * 4, B * HD * WD * 4
    nbytes = {"augment_colour": src + dst + 2 * stash, "augment_plain": src + dst, "preprocess": src + dst}

    # ---- the arms compute the same thing
    got_c = arms["augment_colour"]().cpu().numpy()
    got_p = arms["augment_plain"]().cpu().numpy()
    torch.set_num_threads(1)
    host_t, words = [], 0
    for b in range(min(host_frames, B)):
        args = (frames_h[b], p_h.trans_in[b].numpy(), (HD, WD), bool(p_h.flip[b]), p_h.order[b].tolist(), p_h.factor[b].numpy(),
                p_h.lighting[b].numpy(), NUSCENES_MEAN, NUSCENES_STD)
        t0 = time.perf_counter()
        want = ref.augment_frame(*args)
        host_t.append((time.perf_counter() - t0) * 1e6)
        assert np.allclose(got_c[b], want, rtol=0, atol=2e-6), f"frame {b}: the device and the host arm differ"
        words += int((got_c[b].view(np.int32) != want.view(np.int32)).sum())
        assert np.array_equal(got_p[b], ref.augment_frame(*args, colour=False)), f"frame {b}: colour=False differs"
    ident = draw_augmentation(cfg, B, (HS, WS), np.random.RandomState(0), train=False).to(dev)
    a, c = augment_images(frames, ident, (HD, WD), colour=False), preProcessImages(frames, (HD, WD))
    assert float((a - c).abs().max()) < 1e-6
    print(f"B = {B}, {HS}x{WS} -> {HD}x{WD}, {sets} buffer sets: {int(p_h.flip.sum())} frames flipped; colour result equals the host arm on "
          f"{min(host_frames, B)} frames ({words} words differ in the last bits)", flush=True)

    spin = torch.randn(4096, 4096, device=dev)
    for _ in range(30):
        spin = (spin @ spin) * 1e-4                # warm the clocks
    result = {"B": B, "src_hw": [HS, WS], "dst_hw": [HD, WD], "unit": "us", "flipped": int(p_h.flip.sum()), "sets": sets}
    for name, call in arms.items():
        for _ in range(warmup):
            call()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
        for s, e in ev:
            s.record()
            call()
            e.record()
        torch.cuda.synchronize()
        st = stats([s.elapsed_time(e) * 1e3 for s, e in ev])
        st["bytes"], st["GBps_at_median"] = nbytes[name], nbytes[name] / st["median"] * 1e-3
        result[name] = st
        print(f"  {name:15s} median {st['median']:9.1f} us  p95 {st['p95']:9.1f}  min {st['min']:9.1f}  (n = {st['n']})  "
              f"{nbytes[name] / 1e6:7.1f} MB -> {st['GBps_at_median']:7.1f} GB/s", flush=True)
    host = stats(host_t)
    result["host_per_frame"] = host
    result["ratio_colour_to_preprocess"] = result["augment_colour"]["median"] / result["preprocess"]["median"]
    print(f"  host, one frame   median {host['median']:9.1f} us  p95 {host['p95']:9.1f}  min {host['min']:9.1f}  (n = {host['n']}, one core); "
          f"x {B} frames = {host['median'] * B / 1e3:.1f} ms per batch")
    print(f"  augment colour / preprocess = {result['ratio_colour_to_preprocess']:.2f} (median over median)")
    line = json.dumps(result)
    print(line)
    if path:
        with open(path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
