#!/usr/bin/env python3
"""bench.py - CenterFusion forward throughput on MI355X (BASELINE.json metric).

    python bench.py --gpus 1 --steps 20 --warmup 5
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

One step = one pass of the hot path over one batch: images / pc_dep / calib already resident in HBM
-> DLA-34 + DCNv2 neck + primary heads + frustum association + secondary heads (model.forward) ->
NMS/top-k decode + 2D->3D postProcess (one gather launch) -> (N>1) RCCL all-gather of the final
(B,100,54) boxes, issued asynchronously so it overlaps the next step's backbone.  Workload = BASELINE
configs[1]: Centerfusion_Middle, bs=16 per GPU, 3x448x800, <=200-point synthetic radar sweeps,
random-init weights (no network for checkpoints).  Weak scaling: every rank runs its own 16 frames.

Prints ONE JSON line on rank 0: `value` (frames/s), `ms_per_step` (wall time of one timed step; the MAX over
ranks), the step distribution and every rank's diagnostics.  A plain run does nothing else: set up, `--warmup`
steps, `--steps` timed steps, the line.  `--dump-outputs DIR` writes the last timed step's result (the gathered
postProcess rows) to DIR/post.npy; inputs and weights are seeded, so equal arguments give equal inputs.

`--full` adds the rest: `roofline` is the dominant kernel (head_patch_kernel: the 7 primary and the 4 secondary
heads, 3x3 conv + 1x1 chain each in one launch, 58 % of all FLOPs, a third of the step) timed with HIP events on
the launch stream; `roofline_gather` the DCN gather layers, timed in a few steps of their own; on one GPU
`other_configs` (the other BASELINE configurations, default shape only) and `cpu_baseline`, the CPU oracle (a
port, not the reference) timed on this host on a bounded sample (`--no-cpu-baseline` skips both).
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # (this pool's driver only does dmabuf IPC: RCCL needs it; set before HIP starts)

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

METRIC = "frames/sec/GPU CenterFusion forward, 3x448x800 bs=16; 1/2/4/8-GPU scaling"
GFLOP_PER_FRAME = 167.49          # 2 x 83.74 GMAC (conv + DCN + offset conv + convT)
FP32_MFMA_PEAK_TFLOPS = 157.3     # MI355X_MICROARCH.md, v_mfma_f32_32x32x2_f32
BF16_MFMA_PEAK_TFLOPS = 2500.0    # MI355X_MICROARCH.md, dense bf16 (v_mfma_f32_32x32x16_bf16)
# dominant kernel = head_patch_kernel (cf_head_fused): its two launches per step (7 primary heads; 4 secondary heads)
DOMINANT = ["tails.primary", "tails.secondary"]
# the gather-bound kernel: the 64 -> 64 DeformConv nodes at the H/4 x W/4 maps (dla.py:456-472), and the chip-wide rate at which
# rows resident in the XCDs' L2s can be gathered (MI355X_MICROARCH.md 'Indexed rows: gather into LDS': 16.8-18.8 TB/s)
GATHER_LAYERS = ["dla_up.ida_2.node_1", "dla_up.ida_2.node_2", "dla_up.ida_2.node_3", "ida_up.node_1", "ida_up.node_2"]
L2_GATHER_PEAK_GBS = 18000.0
# HBM-side bytes per launch of the dominant kernel from separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE
# passes over this same command (FETCH_SIZE x2 on gfx950 per MI355X_MICROARCH.md §HBM); bench.py cannot
# run the profiler on itself, so the committed measurement is reported.
def _latest(pattern):
    """newest committed round of a profile file (profiles/rN_<pattern>)"""
    import glob
    c = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9]*_" + pattern)),
               key=lambda f: int(os.path.basename(f)[1:].split("_")[0]))
    c = [f for f in c if os.path.basename(f).split("_", 1)[1] == pattern]
    return c[-1] if c else os.path.join(ROOT, "profiles", "r3_" + pattern)


TRAFFIC_FILE = _latest("pmc_hbm_traffic.json")
C5_TRAFFIC_FILE = _latest("c5_pmc_hbm_traffic.json")
LAYER_BYTES_PER_FRAME = 1.54e9    # layer-boundary traffic per 448x800 frame (every conv-like layer reads its
                                  # input once, writes its output once, reads its weights once, fp32)
HBM_PEAK_GBS = 8000.0             # MI355X_MICROARCH.md: HBM3E 8 TB/s spec (6.3 TB/s achievable)


def load_traffic(path):
    """A committed PMC traffic file, or None when it is missing or was measured on other kernel sources than the ones
    this tree builds (`_meta.sources_sha`, tools/pmc_traffic.py): a stale number is not reported."""
    try:
        from centerfusiondetect3d_amd.build import sources_sha
        t = json.load(open(path))
        if t.get("_meta", {}).get("sources_sha") != sources_sha():
            return None
        return t
    except Exception:
        return None


def measured_traffic(prefixes=("head_patch16_kernel<4, false", "head_patch16_kernel<4, true")):
    """Average HBM-side bytes per launch over the dominant kernel's two launches per step (primary heads: no pc_hm
    source, secondary heads: with it; the third template argument is the tile orientation the host picked)."""
    t = load_traffic(TRAFFIC_FILE)
    if t is None:
        return None
    try:
        per = []
        for pre in prefixes:
            ks = [k for k in t if k.startswith(pre)]
            per.append(sum((t[k]["fetch_bytes_per_launch_x2_corrected"] + t[k]["write_bytes_per_launch"]) * t[k]["launches"]
                           for k in ks) / sum(t[k]["launches"] for k in ks))
        return round(sum(per) / len(per))
    except Exception:
        return None


def synthetic_weights(model, seed=0, offset_std=0.01):
    """default init, then BN stats/affine randomised and conv_offset_mask made
    non-zero so the deformable gather really moves (offsets O(1-3 px))."""
    g = torch.Generator().manual_seed(seed)
    sd = model.state_dict()
    for k, v in sd.items():
        prefix, leaf = k.rsplit(".", 1)
        is_bn = (prefix + ".running_mean") in sd
        if is_bn and leaf == "running_mean":
            v.copy_(torch.randn(v.shape, generator=g) * 0.1)
        elif is_bn and leaf == "running_var":
            v.copy_(torch.rand(v.shape, generator=g) + 0.5)
        elif is_bn and leaf == "weight":
            v.copy_(torch.rand(v.shape, generator=g) + 0.5)
        elif is_bn and leaf == "bias":
            v.copy_(torch.randn(v.shape, generator=g) * 0.1)
        elif k.endswith("conv_offset_mask.weight"):
            v.copy_(torch.randn(v.shape, generator=g) * offset_std)
        elif k.endswith("conv_offset_mask.bias"):
            v.copy_(torch.randn(v.shape, generator=g))
    model.load_state_dict(sd)
    return model


def synthetic_radar(rng, n, max_dist=60.0, intr=(1266.4, 816.3, 491.5), img_wh=(1600, 900)):
    """<=n radar returns in camera frame -> (pc_2d (3,M), pc_3d (18,M), calib (3,4)), filtered and
    depth-sorted the way detector.py:262-283 hands them to processPointCloud."""
    f, cx, cy = intr
    z = rng.uniform(1.0, max_dist, n)
    pc = np.zeros((18, n))
    pc[0], pc[1], pc[2] = rng.uniform(-0.6, 0.6, n) * z, rng.uniform(-1.0, 1.0, n), z
    pc[8], pc[9] = rng.normal(0, 5, n), rng.normal(0, 5, n)
    u, v = f * pc[0] / z + cx, f * pc[1] / z + cy
    m = (z > 0) & (u > 1) & (u < img_wh[0] - 1) & (v > 1) & (v < img_wh[1] - 1)
    order = np.argsort(z[m])
    pc_3d = pc[:, m][:, order]
    pc_2d = np.stack([u[m][order], v[m][order], z[m][order]])
    calib = np.array([[f, 0, cx, 0], [0, f, cy, 0], [0, 0, 1.0, 0]])
    return pc_2d, pc_3d, calib


def make_inputs(B, H, W, device, seed):
    from centerfusiondetect3d_amd import getAffineTransform, process_point_cloud_batch
    rng = np.random.default_rng(seed)
    g = torch.Generator(device="cpu").manual_seed(seed)
    images = torch.randn(B, 3, H, W, generator=g).to(device)
    frames = [synthetic_radar(rng, int(rng.integers(50, 201))) for _ in range(B)]
    trans = getAffineTransform((800.0, 450.0), 1600.0, 0, (W // 4, H // 4))
    pc_dep = process_point_cloud_batch([f[0] for f in frames], [f[1] for f in frames],
                                       [f[2] for f in frames], trans, (H // 4, W // 4), device=device)
    calib = torch.tensor(np.stack([f[2] for f in frames]), dtype=torch.float32, device=device)
    return images, pc_dep, calib


def cpu_threads():
    """Threads the CPU leg may use: the cgroup CPU quota if there is one (a 1-GPU box exposes 128
    logical CPUs but grants ~16), else the affinity mask."""
    n = len(os.sched_getaffinity(0))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return min(n, int(os.environ.get("CF_CPU_THREADS", "16")))


def cpu_model_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except Exception:
        pass
    return "unknown"


def cpu_baseline(H, W, batch=16, runs=3, seed=0):
    """CPU oracle (our torch-fp32 restatement, kind 'port') per SURVEY.md §8(d): forward + decode timed on this
    host with all granted cores - C2 (Centerfusion_Middle) at bs=1 and bs=`batch`, C1 (CenterNet) at bs=1; median of
    `runs` after one warm-up for the bs=1 legs, ONE run for the bs=`batch` leg (29 s on 16 cores: three would triple
    the bounded sample).  `value` = the better C2 rate (bs=1 is faster on this host: the oracle's DCN gather and the
    fp32 maps of 16 frames fall out of cache); every leg is listed under `runs`.  ~35 s of CPU work at the defaults."""
    from oracle import model_ref, decode_ref
    rs = np.random.RandomState(seed)
    cores = cpu_threads()
    torch.set_num_threads(cores)
    calib1 = torch.tensor([[1266.4, 0, 816.3, 0], [0, 1266.4, 491.5, 0], [0, 0, 1, 0]])

    def leg(radar, bs, n_runs):
        sd = model_ref.make_state_dict(radar=radar, seed=seed)
        x = torch.from_numpy(rs.standard_normal((bs, 3, H, W)).astype(np.float32))
        pc_dep = None
        if radar:
            pc_dep = torch.zeros(bs, 3, H // 4, W // 4)
            for b in range(bs):
                for d in np.sort(rs.uniform(2, 58, 120)):
                    cx, cy = rs.randint(0, W // 4), rs.randint(2, H // 4)
                    pc_dep[b, 0, max(cy - 12, 0):cy, cx:cx + 2] = float(d)
        calib = calib1.repeat(bs, 1, 1)
        ts = []
        with torch.no_grad():
            model_ref.forward(sd, x[:1], pc_dep=pc_dep[:1] if radar else None, calib=calib[:1], radar=radar)   # warm-up
            for _ in range(n_runs):
                t0 = time.perf_counter()
                y = model_ref.forward(sd, x, pc_dep=pc_dep, calib=calib, radar=radar)
                decode_ref.fusion_decode(y, (H // 4, W // 4), 100)
                ts.append(time.perf_counter() - t0)
        med = float(np.median(ts))
        return {"config": "C2 Centerfusion_Middle" if radar else "C1 CenterNet", "batch": bs, "runs": n_runs,
                "median_s": round(med, 3), "min_s": round(min(ts), 3), "max_s": round(max(ts), 3),
                "frames_per_s": round(bs / med, 4),
                "frames_per_s_min_med_max": [round(bs / max(ts), 4), round(bs / med, 4), round(bs / min(ts), 4)]}

    legs = [leg(True, 1, runs), leg(True, batch, 1), leg(False, 1, runs)]
    total = sum(l["median_s"] * l["runs"] for l in legs)
    best = max(legs[:2], key=lambda l: l["frames_per_s"])
    return {"value": best["frames_per_s"], "unit": "frames/s", "cores": cores, "kind": "port",
            "cpu": cpu_model_name(),
            "spread": {"frames_per_s_min_med_max": best["frames_per_s_min_med_max"], "runs": best["runs"],
                       "note": "this leg moved 2.2-3.3 frames/s between driver boxes of the same CPU model (rounds 2-3): "
                               "context for the GPU figure, not a target"},
            "sample": f"torch-fp32 oracle forward+decode, 3x{H}x{W}: C2 bs=1 x{runs}, C2 bs={batch} x1, C1 bs=1 x{runs} "
                      f"after a 1-frame warm-up each, ~{total:.0f} s of CPU work; value = C2 at bs={best['batch']} "
                      f"(its faster batch size on this host)",
            "runs": legs}


def end_to_end(args, dev, model):
    """`Detector.run`-shaped line (kept apart from the contract line): uint8 1600x900 camera frames and raw radar
    sweeps start in pinned HOST memory; per step they cross PCIe, are warped / normalised, ingested and
    pillar-expanded on the device, go through the model and come out as final 3D boxes (B,100,54)."""
    from centerfusiondetect3d_amd import Detector
    from tests.golden import cases_dataset as cd
    B, H, W = args.batch, args.height, args.width
    rs = np.random.RandomState(5)
    frames = torch.from_numpy(rs.randint(0, 256, (B, 900, 1600, 3)).astype(np.uint8)).pin_memory()
    calib = np.concatenate([cd.NUSC_K, np.zeros((3, 1))], axis=1)
    infos = [dict(calib=calib.tolist(), camera_intrinsic=cd.NUSC_K.tolist(), width=1600, height=900)] * B
    sweeps = [cd._sweep(np.random.RandomState(100 + b), int(rs.randint(50, 201))) for b in range(B)]
    det = Detector(model.config, model=model, device=dev)

    def step():
        return det.run(frames, infos, sweeps, merge=False)["post"]

    with torch.no_grad():
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            post = step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, {"post": post})
        # resident-input floor of the same step (inputs already pre-processed on the device): the pipelined chain cannot
        # beat it
        images, pc_dep, metas, calibs = det.pre_process(frames, infos, sweeps)
        for _ in range(2):
            det.process(images, calibs, pc_dep, metas[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            det.process(images, calibs, pc_dep, metas[0])
        torch.cuda.synchronize()
        dt_r = time.perf_counter() - t0
        # the same batches through Detector.run_pipelined: batch i+1's PCIe copy + pre-processing on a feed stream
        # beside batch i's forward (what the reference's DataLoader workers + pinned memory give it).  The generator
        # yields batch i-1 after batch i's forward and batch i+1's staging are queued, so `warmup + steps + 2` batches
        # are fed and the clock stops after `steps` yields: the timed region then holds exactly `steps` forwards
        # (batches warmup+1 .. warmup+steps) and `steps` stagings (warmup+2 .. warmup+steps+1) - the work it is credited
        batches = ((frames, infos, sweeps) for _ in range(args.warmup + args.steps + 2))
        gen = det.run_pipelined(batches, merge=False)
        for _ in range(args.warmup):
            next(gen)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            post_p = next(gen)["post"]
        torch.cuda.synchronize()
        dt_p = time.perf_counter() - t0
        gen.close()
        torch.cuda.synchronize()
    assert torch.equal(post_p, post)
    assert post.shape == (B, 100, 54) and bool(torch.isfinite(post).all())
    assert dt_p >= 0.97 * dt_r, (dt_p, dt_r)            # (a pipelined chain faster than its own resident-input step is a timing bug)
    pipelined = {"frames_per_s": round(B * args.steps / dt_p, 2), "ms_per_step": round(dt_p / args.steps * 1e3, 3),
                 "resident_ms_per_step": round(dt_r / args.steps * 1e3, 3),
                 "what": "Detector.run_pipelined: PCIe copy + pre-processing of batch i+1 on a feed stream beside batch i's forward"}
    return {"pipelined": pipelined, "metric": "frames/sec/GPU CenterFusion end-to-end: uint8 1600x900 frames + raw radar sweeps in pinned host "
                      "memory -> PCIe -> pre-process + radar ingest + pillar expansion -> forward -> decode + postProcess "
                      "(final 3D boxes on the device)",
            "value": round(B * args.steps / dt, 2), "unit": "frames/s", "n_gpus": 1, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3), "higher_is_better": True,
            "data": "synthetic", "config": {"workload": f"Detector.run chain, bs={B}, 3x{H}x{W} network input",
                                            "pcie_bytes_per_frame": 900 * 1600 * 3}}


def other_configs(dev, steps=12):
    """BASELINE.json's other single-GPU configurations on the same build, a few steps each (rank 0, N=1, default run
    only): C4 (offsets O(8 px)), C5 (3x896x1600, bs=8), one-frame latency.  Parity for each: tests/test_gpu_model.py."""
    from centerfusiondetect3d_amd import getModel, centerfusion_middle_config, decode_post_packed
    from centerfusiondetect3d_amd.postprocess import inverse_affine_device
    out = {}

    def measure(B, H, W, offset_std, exact_fp32=False, steps=steps, warm=6):
        model = getModel(centerfusion_middle_config((H, W)))
        if exact_fp32:
            model.conv_f16 = False
            model.heads_bf16 = False
        model = synthetic_weights(model, seed=0, offset_std=offset_std).to(dev).eval()
        images, pc_dep, calib = make_inputs(B, H, W, dev, seed=2000)
        tinv = inverse_affine_device(np.array([800.0, 450.0], np.float32), 1600.0, (W // 4, H // 4), dev)
        dominant = ["heads.primary.0", "heads.secondary.0"] if exact_fp32 else []
        with torch.no_grad():
            for _ in range(warm):
                decode_post_packed(model(images, pc_dep=pc_dep, calib=calib), calib, tinv, (H // 4, W // 4), 100)
            for name in dominant:
                model.time_launch(name, True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                decode_post_packed(model(images, pc_dep=pc_dep, calib=calib), calib, tinv, (H // 4, W // 4), 100)
            torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / steps * 1e3
        r = {"ms_per_step": round(ms, 3), "frames_per_s": round(B / ms * 1e3, 1), "batch": B, "input": f"3x{H}x{W}"}
        if exact_fp32:
            l_ms, l_fl = [], 0.0
            for name in dominant:
                m_, f_ = model.launch_times(name)
                l_ms += m_
                l_fl += f_ * len(m_)
            avg, fl = float(np.mean(l_ms)), l_fl / len(l_ms)
            ach = fl / (avg * 1e-3) / 1e12
            r["dtype"] = "f32"
            r["model_tflops"] = round(B / ms * GFLOP_PER_FRAME * (H * W) / (448 * 800), 2)
            r["model_frac_of_fp32_mfma_peak"] = round(r["model_tflops"] / FP32_MFMA_PEAK_TFLOPS, 4)
            r["roofline"] = {"bound": "mfma", "achieved": round(ach, 2), "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                             "frac": round(ach / FP32_MFMA_PEAK_TFLOPS, 4), "traffic": None,
                             "kernel": "conv_igemm_kernel (v_mfma_f32_32x32x2_f32; the 3x3 first layers of the 7 primary / "
                                       "4 secondary heads)",
                             "flop_per_launch": fl, "avg_launch_ms": round(avg, 4), "launches_timed": len(l_ms)}
        del model, images, pc_dep, calib
        torch.cuda.empty_cache()
        return r

    out["C4_dcn_offsets_8px"] = measure(16, 448, 800, 0.04)
    c5 = out["C5_highres"] = measure(8, 896, 1600, 0.01)
    # BASELINE config 5 is the "HBM-bound roofline point": the whole step against HBM, algorithmic bytes = the
    # layer-boundary model of SURVEY §8(d) (4 x 1.54 GB per 896x1600 frame); traffic = HBM-side bytes of one step over
    # all kernels from the committed rocprofv3 FETCH_SIZE / WRITE_SIZE passes of this configuration
    gbs = 4 * LAYER_BYTES_PER_FRAME * c5["frames_per_s"] / 1e9
    t5 = load_traffic(C5_TRAFFIC_FILE)
    traffic5 = None if t5 is None else round(t5["_meta"]["hbm_bytes_per_forward_all_kernels"])
    tflops5 = 4 * GFLOP_PER_FRAME * c5["frames_per_s"] / 1e3
    c5["roofline"] = {"bound": "hbm", "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                      "frac": round(gbs / HBM_PEAK_GBS, 4), "traffic": traffic5,
                      "bytes_per_step": 4 * LAYER_BYTES_PER_FRAME * 8,
                      # the HBM-side bytes the counters saw, over this run's step time: what the memory system really did
                      "measured_gbs": None if traffic5 is None else round(traffic5 / c5["ms_per_step"] / 1e6, 1),
                      "measured_frac": None if traffic5 is None else round(traffic5 / c5["ms_per_step"] / 1e6 / HBM_PEAK_GBS, 4),
                      "mfma": {"achieved": round(tflops5, 1), "peak": BF16_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                               "frac": round(tflops5 / BF16_MFMA_PEAK_TFLOPS, 4), "flop_per_step": 4 * GFLOP_PER_FRAME * 8e9},
                      "note": "whole step.  `achieved` = ALGORITHMIC layer-boundary bytes (fp32 activations in/out + weights "
                              "per conv-like layer) / time; the counters (`traffic`, `measured_gbs`) see half of that - "
                              "fusion keeps the rest on chip - so the step is NOT HBM-bound at this size: like C2 it is "
                              "bound by MFMA/VALU issue, and `mfma.frac` (x3 for pipe occupancy: 3 passes per MAC) is the "
                              "figure the counters support.  Kernels at 224x400 maps: profiles/r6_c5_kernel_summary.txt"}
    out["C2_exact_fp32"] = measure(16, 448, 800, 0.01, exact_fp32=True, steps=6, warm=2)
    out["C2_single_frame_latency"] = measure(1, 448, 800, 0.01)
    out["C2_one_nuscenes_sample_bs6"] = measure(6, 448, 800, 0.01)     # the 6 cameras of one sample (detector.py:44-155)
    return out


class StepClock:
    """Per-rank diagnostics of the timed steps, so that an N>1 line explains itself (8 Python launch threads share one
    host; a bad scaling figure must be attributable to host enqueue, to the exchange, or to neither):
      host_enqueue_ms  perf_counter around ONE step's launches - forward, decode + postProcess, all-gather submit -
                       before any wait; the MINIMUM over the timed steps = what the host needs when nothing blocks it.
                       host_enqueue_mean_ms is the mean: once the host runs a queue's depth ahead of the GPU its launches
                       block, so the mean tends to the GPU's step time - host-bound is min ~ mean ~ step_ms;
      gather_wait_ms   time the compute stream spends blocked on the previous step's all-gather (HIP events either side
                       of `work.wait()`, which orders the stream and does not block the host); on CPU (gloo rehearsal) the
                       host time of the blocking wait;
      step_ms          this rank's own wall time per step (the headline uses the MAX over ranks).
      step_ms_p50 / _p95 / _max   the distribution of this rank's timed steps: device time between HIP events recorded behind
                       every step's launches on the compute stream (the headline `value` stays frames / total wall time).
    Rank 0 prints every rank's figures as `ranks: [...]`; the line's own step_ms_p50 / p95 / max are the MAX over ranks."""
    FIELDS = ("step_ms", "host_enqueue_ms", "host_enqueue_mean_ms", "gather_wait_ms", "gather_wait_host_ms",
              "step_ms_p50", "step_ms_p95", "step_ms_max")

    def __init__(self, device):
        self.cuda = device is not None and torch.device(device).type == "cuda"
        self.on, self.enq, self.wait_host, self.wait_ev = False, [], [], []
        self.marks = []          # one stamp per timed step boundary: HIP events on the compute stream (host times on CPU)

    def mark(self):
        """(no-op with `untimed_marks`: --in-flight > 1 spreads the steps over several caller streams, their boundaries are
        not on one stream - the distribution then falls back to the mean)
        a step boundary on the compute stream: start() before the first timed step, then behind every step's launches.
        The distribution of the steps (median, not only a mean) is the differences of consecutive marks -
        device time, so a host that runs a queue ahead does not blur it."""
        if getattr(self, "untimed_marks", False):
            return
        if self.cuda:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.marks.append(e)
        else:
            self.marks.append(time.perf_counter())

    def start(self):
        self.on = True
        self.marks = []
        self.mark()

    def enqueue(self, fn):
        t0 = time.perf_counter()
        r = fn()
        if self.on:
            self.enq.append(time.perf_counter() - t0)
            self.mark()
        return r

    def step_times_ms(self):
        """device time between consecutive step boundaries (call after a device sync)"""
        if self.cuda:
            return [a.elapsed_time(b) for a, b in zip(self.marks[:-1], self.marks[1:])]
        return [1e3 * (b - a) for a, b in zip(self.marks[:-1], self.marks[1:])]

    def wait(self, pending):
        if not self.on:
            return pending.wait()
        ev = None
        if self.cuda and pending.work is not None:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        t0 = time.perf_counter()
        out = pending.wait()
        self.wait_host.append(time.perf_counter() - t0)
        if ev is not None:
            ev[1].record()
            self.wait_ev.append(ev)
        return out

    def row(self, dt, steps):
        """-> [step_ms, host_enqueue_ms (min), host_enqueue_mean_ms, gather_wait_ms, gather_wait_host_ms] of this rank
        (call after a device sync)."""
        wh = 1e3 * float(np.mean(self.wait_host)) if self.wait_host else 0.0
        wd = float(np.mean([a.elapsed_time(b) for a, b in self.wait_ev])) if self.wait_ev else (0.0 if self.cuda else wh)
        st = self.step_times_ms() or [dt / steps * 1e3]
        return [dt / steps * 1e3, 1e3 * float(np.min(self.enq)) if self.enq else 0.0,
                1e3 * float(np.mean(self.enq)) if self.enq else 0.0, wd, wh,
                float(np.percentile(st, 50)), float(np.percentile(st, 95)), float(np.max(st))]

    @staticmethod
    def gather_rows(row, world, device):
        """every rank's row -> list of dicts on every rank (one small all-gather, outside the timed region)."""
        import torch.distributed as dist
        t = torch.tensor(row, dtype=torch.float64, device=device)
        if world > 1:
            out = [torch.zeros_like(t) for _ in range(world)]
            dist.all_gather(out, t)
        else:
            out = [t]
        return [dict(rank=r, **{k: round(float(v), 4) for k, v in zip(StepClock.FIELDS, o.tolist())})
                for r, o in enumerate(out)]


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, arrays):
    """{name: tensor} -> out_dir/<name>.npy (float64 stays float64, everything else float32).  An output that would
    take the files past DUMP_LIMIT_BYTES is cut to a fixed, seeded sample of its leading-axis rows (sorted)."""
    os.makedirs(out_dir, exist_ok=True)
    budget = DUMP_LIMIT_BYTES // max(1, len(arrays))
    for name, t in arrays.items():
        a = t.detach().cpu().numpy()
        a = a.astype(np.float64 if a.dtype == np.float64 else np.float32, copy=False)
        if a.nbytes > budget:
            keep = max(1, budget // max(1, a[:1].nbytes))
            a = a[np.sort(np.random.default_rng(0).choice(a.shape[0], keep, replace=False))]
        np.save(os.path.join(out_dir, name + ".npy"), a)


def free_port():
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def spawn_ranks(n, argv):
    """`python bench.py --gpus N` without a launcher: run the ranks as children of torch.distributed.run (one process
    per GPU, RCCL rendezvous on 127.0.0.1) - the reference gets its ranks from Lightning the same way
    (/root/reference/src/lib/trainer.py:54-70, devices=config.GPUS).  Returns the children's exit code."""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__), *argv]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "4")
    return subprocess.run(cmd, env=env).returncode


def rehearse(args, world, rank, collective, json_fd):
    """`--rehearse-cpu`: the multi-rank CONTROL FLOW of this file without a GPU - launcher, rendezvous, the
    submit / wait pipeline of the overlapped all-gather, the drain inside the timed region, barrier fences, the MAX
    over ranks, one JSON line from rank 0 on the saved descriptor, teardown - over gloo with a stand-in for the forward
    (rows that carry their rank and step).  Measures nothing: the line says `"rehearsal": true, "value": null`.  It
    exists because no multi-GPU node is available to the builder: `tests/test_bench_launcher.py` runs it at N = 2."""
    import torch.distributed as dist
    from centerfusiondetect3d_amd.distributed import DetectionGatherer, assume_equal_shards
    assume_equal_shards(True)
    if collective:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(free_port()))
        dist.init_process_group("gloo", rank=rank, world_size=world)
    B = args.batch
    gatherer = DetectionGatherer(torch.device("cpu"), force_collective=args.force_collective)
    pending, n_done = [], [0]
    clock = StepClock(torch.device("cpu"))

    def launches():
        post = torch.full((B, 100, 54), float(1000 * rank + n_done[0]))
        n_done[0] += 1
        pending.append(gatherer.submit(post))

    def step():
        clock.enqueue(launches)
        return clock.wait(pending.pop(0)) if len(pending) > 1 else None

    def drain():
        last = None
        while pending:
            last = clock.wait(pending.pop(0))
        return last

    for _ in range(args.warmup):
        step()
    drain()
    if world > 1:
        dist.barrier()
    clock.start()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    det = drain()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    assert det.shape == (B * world, 100, 54)
    last = args.warmup + args.steps - 1
    for r in range(world):                     # rank-major, every rank's LAST step
        assert bool((det[r * B:(r + 1) * B] == float(1000 * r + last)).all()), (rank, r)
    t = torch.tensor([dt], dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    ranks = StepClock.gather_rows(clock.row(dt, args.steps), world if collective else 1, torch.device("cpu"))
    if rank == 0:
        os.write(json_fd, (json.dumps({"metric": METRIC, "value": None, "unit": "frames/s", "n_gpus": world,
                                       "steps": args.steps, "warmup": args.warmup, "rehearsal": True, "ranks": ranks,
                                       **{k: max(r[k] for r in ranks) for k in ("step_ms_p50", "step_ms_p95", "step_ms_max")},
                                       "ms_per_step": round(float(t.item()) / args.steps * 1e3, 3), "scaling": "weak",
                                       "config": {"workload": "control-flow rehearsal on CPU (gloo), no forward",
                                                  "global_batch": B * world}}) + "\n").encode())
    if collective:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16, help="frames per GPU")
    ap.add_argument("--height", type=int, default=448)
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--offset-std", type=float, default=0.01,
                    help="std of the synthetic conv_offset_mask weights: 0.01 -> offsets O(1-3 px) (C2); 0.04 -> O(8 px), "
                         "BASELINE config C4 (stresses the bilinear gather)")
    ap.add_argument("--streams", type=int, default=2,
                    help="model.streams: backbone + neck as that many sub-batches on concurrent HIP streams (the other "
                         "sub-batch fills launches that cannot fill the chip alone); the heads - the roofline kernel - "
                         "run for the whole batch on the caller's stream, so their HIP-event durations overlap nothing.  "
                         "1 = everything on one stream")
    ap.add_argument("--min-sub-batch", type=int, default=None,
                    help="model.min_sub_batch (frames a trunk stream must keep; default 6): with --streams 4 --min-sub-batch 4 a "
                         "bs=16 step runs four 4-frame trunks (experiment)")
    ap.add_argument("--exact-fp32", action="store_true",
                    help="every product in exact fp32 (fp32 MFMA kernels with two-level summation; conv_f16 / heads_bf16 "
                         "off) instead of the default split-operand products - the accuracy reference build, 3.5x slower")
    ap.add_argument("--heads-bf16x3", action="store_true",
                    help="A/B: the heads' first layers on bf16x3 (3 MFMA passes per product, the round-4 arithmetic) instead of "
                         "fp16 main term + block-scaled FP6 cross terms (1.5 passes; model.heads_mx)")
    ap.add_argument("--no-proj-fuse", action="store_true",
                    help="A/B: the four `project` convolutions as their own launches + residual tensors (the round-4 plan) "
                         "instead of k-steps of tree1.conv2 (cf_conv3x3_proj_f16x3; model.proj_fuse)")
    ap.add_argument("--no-stem-pool", action="store_true",
                    help="A/B: the level-2 Tree's max-pool as its own launch instead of a second output of the stem (model.stem_pool)")
    ap.add_argument("--no-heads-lanes", action="store_true",
                    help="A/B: the decoder's NMS + top-k behind the forward on the caller's stream instead of beside the secondary heads (model.heads_lanes = False)")
    ap.add_argument("--no-trunk-on-caller", action="store_true",
                    help="A/B: every trunk sub-batch on a side stream (round 5) instead of the last one on the caller's stream (model.trunk_on_caller = False)")
    ap.add_argument("--peaks-behind-primary", action="store_true",
                    help="A/B: the decoder's top-k lane starts behind the primary head launch (round 5) instead of behind the frustum chain")
    ap.add_argument("--no-frustum-fused", action="store_true",
                    help="A/B: cf_topk_peaks + cf_frustum_assoc (three launches) between the head launches instead of cf_topk_frustum (model.frustum_fused = False)")
    ap.add_argument("--root-fuse-children", action="store_true",
                    help="A/B: conv2 + Root in one launch also for the Roots that read the Tree's children (model.root_fuse_children)")
    ap.add_argument("--lanes-max-frames", type=int, default=None,
                    help="A/B: model.lanes_max_frames (default 10; trunk sub-batches of the two-stream forward: at most 4: a forward of up to that many 448x800-frame equivalents issues its IDA "
                         "projections on a side stream beside the node chain)")
    ap.add_argument("--in-flight", type=int, default=1,
                    help="experiment (never the default line): consecutive steps alternate over this many caller streams, so the "
                         "heads of step i may run beside the backbone of step i+1 (one plan set per stream)")
    ap.add_argument("--force-collective", action="store_true",
                    help="initialise the RCCL process group and issue the per-step all-gather also at world size 1 (what a "
                         "rank of an N-GPU run does, on a one-GPU box)")
    ap.add_argument("--rehearse-cpu", action="store_true",
                    help="no GPU, no measurement: run this file's multi-rank control flow over gloo with a stand-in forward "
                         "(tests; the JSON line is marked as a rehearsal)")
    ap.add_argument("--use-graph", action="store_true",
                    help="model.use_graph: replay the forward as ONE captured HIP graph - the host then issues one launch per "
                         "step instead of ~165 (diagnosis of an N > 1 run whose ranks' host_enqueue_ms says the host is the "
                         "bottleneck; on one GPU eager launches are as fast: DESIGN.md section 3)")
    ap.add_argument("--end-to-end", action="store_true",
                    help="print the Detector.run-shaped line instead (uint8 frames + raw radar over PCIe -> final boxes)")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline figure: the dominant kernel's roofline (HIP events on its launches "
                         "inside the timed steps) and the DCN gather roofline (a few steps of its own); on one GPU also the "
                         "other BASELINE configurations (default shape only) and the CPU oracle baseline (unless "
                         "--no-cpu-baseline).  Off: set up, warm up, time --steps steps, print the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned (the gathered postProcess rows, "
                         f"(B x n_gpus, 100, 54)) as DIR/post.npy, float32, at most {DUMP_LIMIT_BYTES >> 20} MB in all")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ and "RANK" not in os.environ:
        # started bare (`python bench.py --gpus N`): become the launcher.  This process has not touched the GPU (and
        # never will - importing torch initialises nothing); the ranks are torch.distributed.run's children, rank 0
        # prints the JSON line on the inherited stdout, and their exit code is ours.
        sys.exit(spawn_ranks(args.gpus, sys.argv[1:]))

    # stdout carries exactly ONE line, the JSON result: everything native code prints on fd 1 meanwhile (RCCL's version
    # banner at communicator creation, for one) goes to stderr instead
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        print(f"bench.py[rank {rank}]: --gpus {args.gpus} but WORLD_SIZE={world}: the launcher and the flag disagree",
              file=sys.stderr)
        sys.exit(2)
    import torch.distributed as dist
    collective = world > 1 or args.force_collective
    if args.rehearse_cpu:
        rehearse(args, world, rank, collective, json_fd)
        return
    n_dev = torch.cuda.device_count()          # (counting devices does not initialise HIP on this image)
    if local_rank >= n_dev:
        print(f"bench.py[rank {rank}]: needs GPU index {local_rank} but this node exposes {n_dev} device(s): "
              f"--gpus {args.gpus} cannot run here", file=sys.stderr)
        sys.exit(3)
    assert torch.cuda.is_available(), "bench.py measures the HIP path: it needs an MI355X"
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    if collective:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(free_port()))
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    from centerfusiondetect3d_amd import getModel, centerfusion_middle_config, decode_post_packed
    from centerfusiondetect3d_amd.distributed import DetectionGatherer, assume_equal_shards
    from centerfusiondetect3d_amd.postprocess import inverse_affine_device
    assume_equal_shards(True)
    B, H, W = args.batch, args.height, args.width
    torch.manual_seed(0)             # the default init of the weights synthetic_weights leaves alone: equal arguments, equal outputs
    model = getModel(centerfusion_middle_config((H, W)))
    if args.exact_fp32:
        model.conv_f16 = False
        model.heads_bf16 = False
    if args.heads_bf16x3:
        model.heads_mx = False
    if args.no_proj_fuse:
        model.proj_fuse = False
    if args.no_stem_pool:
        model.stem_pool = False
    if args.root_fuse_children:
        model.root_fuse_children = True
    if args.no_frustum_fused:
        model.frustum_fused = False
    if args.peaks_behind_primary:
        model.peaks_behind_frustum = False
    if args.no_trunk_on_caller:
        model.trunk_on_caller = False
    if args.lanes_max_frames is not None:
        model.lanes_max_frames = args.lanes_max_frames
    if args.no_heads_lanes:
        model.heads_lanes = False
    model = synthetic_weights(model, seed=0, offset_std=args.offset_std).to(dev).eval()
    model.streams = max(1, args.streams)
    if args.min_sub_batch is not None:
        model.min_sub_batch = args.min_sub_batch
    model.use_graph = bool(args.use_graph)
    if args.end_to_end:
        if rank == 0:
            os.write(json_fd, (json.dumps(end_to_end(args, dev, model)) + "\n").encode())
        return
    images, pc_dep, calib = make_inputs(B, H, W, dev, seed=1000 + rank)
    tinv = inverse_affine_device(np.array([800.0, 450.0], np.float32), 1600.0, (W // 4, H // 4), dev)
    gatherer = DetectionGatherer(dev, force_collective=args.force_collective)
    pending = []
    clock = StepClock(dev)

    flight = [torch.cuda.Stream(dev) for _ in range(args.in_flight)] if args.in_flight > 1 else None
    clock.untimed_marks = flight is not None
    n_step = [0]

    def launches():
        if flight is not None:
            with torch.cuda.stream(flight[n_step[0] % len(flight)]):
                n_step[0] += 1
                out = model(images, pc_dep=pc_dep, calib=calib)
                post = decode_post_packed(out, calib, tinv, (H // 4, W // 4), 100)
                pending.append(gatherer.submit(post))
            return
        out = model(images, pc_dep=pc_dep, calib=calib)
        post = decode_post_packed(out, calib, tinv, (H // 4, W // 4), 100)
        pending.append(gatherer.submit(post))

    def step():
        """forward -> decode + postProcess -> (N>1) async all-gather of the final boxes; the gather of step i is
        waited for after step i+1 has been enqueued, so it runs beside that step's backbone."""
        clock.enqueue(launches)
        if len(pending) > 1:
            return clock.wait(pending.pop(0))
        return None

    def drain():
        last = None
        while pending:
            last = clock.wait(pending.pop(0))
        return last

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # exact-fp32 build: the heads are unfused fp32-MFMA convolutions; its dominant launches are the two first layers.
    # Only --full times them (HIP events on those launches inside the timed steps).
    dominant = (["heads.primary.0", "heads.secondary.0"] if args.exact_fp32 else DOMINANT) if args.full else []
    with torch.no_grad():
        for _ in range(args.warmup):
            step()
        drain()
        for name in dominant:
            model.time_launch(name, True)
        fence()
        clock.start()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        det = drain()                      # every gather of the timed steps completes inside the timed region
        fence()
        dt = time.perf_counter() - t0
        clock.on = False
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"post": det})     # before any later step can reuse a buffer
    if args.use_graph and args.full:
        # a graph replay has no per-launch events: the dominant kernel is timed in three eager steps behind the timed region
        model.use_graph = False
        with torch.no_grad():
            step()
            drain()
            for name in dominant:
                model.time_launch(name, True)
            for _ in range(3):
                step()
            drain()
        torch.cuda.synchronize()
        model.use_graph = True
    launch_ms, launch_flops = [], 0.0
    for name in dominant:
        ms, fl = model.launch_times(name)
        model.time_launch(name, False)
        launch_ms += ms
        launch_flops += fl * len(ms)
    # The kernel furthest below the MFMA roofline, against the roof that does bind it: the 64 -> 64 DCN
    # layers at the 112 x 200 maps (dcn_f16x3_kernel<2,2,1,true,1>) gather 9 taps x 4 corner rows of C x 4 bytes per output
    # pixel through the L2 -> TA path.  Timed with HIP events on their launch streams in a few steps BEHIND the timed region
    # (20 more event pairs per step would sit inside `value` otherwise).
    gather = None
    if args.full and not args.exact_fp32 and not args.use_graph:
        with torch.no_grad():
            for name in GATHER_LAYERS:
                model.time_launch(name, True)
            for _ in range(4):
                step()
            drain()
        g_ms, g_bytes = [], 0.0
        for name in GATHER_LAYERS:
            ms, fl = model.launch_times(name)
            model.time_launch(name, False)
            g_ms += ms
            g_bytes += fl / (2.0 * 64) * 4 * 4 * len(ms)      # FLOPs = 2 * M * N * 9 * C (N = 64) -> M * 9 * C samples x 4 corners x 4 B
        if g_ms:
            gather = (float(np.mean(g_ms)), g_bytes / len(g_ms), len(g_ms))
    assert det.shape == (B * world, 100, 54) and bool(torch.isfinite(det).all())

    t = torch.tensor([dt], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    ranks = StepClock.gather_rows(clock.row(dt, args.steps), world, dev)   # (this rank's own dt, before the MAX)
    dt = float(t.item())

    if rank == 0:
        fps = world * B * args.steps / dt
        result = {
            "metric": METRIC, "value": round(fps, 2), "unit": "frames/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": ("f32" if args.exact_fp32 else
                      "f32 storage + f32 accumulate; products as 3 split-operand MFMA passes (f16x3 backbone/neck, bf16x3 heads)"
                      if not model._mx_active else
                      "f32 storage + f32 accumulate; products as split-operand MFMA passes: f16x3 backbone/neck (3 passes), heads' "
                      "first 3x3 layers fp16 main term + block-scaled FP6 e2m3 cross terms (1.5 passes), heads' 1x1 layers bf16x3"),
            "data": "synthetic",
            "config": {"workload": f"Centerfusion_Middle (DLA-34 + DCNv2 neck + pc_dep frustum fusion, 7+4 heads) "
                                   f"forward + NMS/top-100 decode + 2D->3D postProcess, bs={B}/GPU, 3x{H}x{W}, 50-200 radar pts/frame, "
                                   f"random-init weights",
                       "global_batch": B * world, "parallelism": f"dp{world} (batch shard, async all-gather of the final boxes)"},
            "per_gpu_frames_per_s": round(fps / world, 2),
            **{k: max(r[k] for r in ranks) for k in ("step_ms_p50", "step_ms_p95", "step_ms_max")},
            "ranks": ranks,
            "model_tflops": round(fps * GFLOP_PER_FRAME * (H * W) / (448 * 800) / 1e3, 2),
        }
        if args.full:
            avg_ms = float(np.mean(launch_ms))
            launch_flops = launch_flops / len(launch_ms)          # algorithmic FLOPs of an average launch
            achieved = launch_flops / (avg_ms * 1e-3) / 1e12
            peak = FP32_MFMA_PEAK_TFLOPS if args.exact_fp32 else BF16_MFMA_PEAK_TFLOPS
            result["roofline"] = {"bound": "mfma", "achieved": round(achieved, 2), "peak": peak,
                                 "unit": "TFLOP/s", "frac": round(achieved / peak, 4),
                                 "traffic": None if args.exact_fp32 else measured_traffic(),
                                 "kernel": ("conv_igemm_kernel (fp32 MFMA; the 3x3 first layers of the 7 primary / 4 secondary heads)"
                                            if args.exact_fp32 else
                                            "head_patch16_kernel (cf_head_fused, v_mfma_f32_16x16x32_bf16; 2 launches/step: 7 primary heads, 4 secondary heads)"
                                            if not model._mx_active else
                                            "head_patch16_kernel<MX> (cf_head_fused mx: v_mfma_f32_16x16x32_f16 + v_mfma_scale_f32_16x16x128_f8f6f4 first layer, "
                                            "v_mfma_f32_16x16x32_bf16 tail layers; 2 launches/step: 7 primary heads, 4 secondary heads)"),
                                 "note": ("algorithmic FLOPs (2*MACs) against the fp32 MFMA peak" if args.exact_fp32 else
                                          "algorithmic FLOPs (2*MACs); the kernel issues 3 bf16 MFMA passes per MAC "
                                          "(split operands), so MFMA-pipe utilisation is 3x frac" if not model._mx_active else
                                          "algorithmic FLOPs (2*MACs) against the dense bf16/f16 MFMA peak; a first-layer MAC costs 1 fp16 pass + "
                                          "1/2 pass-equivalent of FP6 cross terms (4x rate), a 1x1-layer MAC 3 bf16 passes"),
                                 "flop_per_launch": launch_flops, "avg_launch_ms": round(avg_ms, 4),
                                 "launches_timed": len(launch_ms)}
        if gather is not None:
            g_avg_ms, g_b, g_n = gather
            gbs = g_b / (g_avg_ms * 1e-3) / 1e9
            result["roofline_gather"] = {
                "bound": "l2-gather", "achieved": round(gbs, 1), "peak": L2_GATHER_PEAK_GBS, "unit": "GB/s",
                "frac": round(gbs / L2_GATHER_PEAK_GBS, 4),
                "kernel": "dcn_f16x3_kernel<2,2,1,true,1> (cf_dcn_v2_f16x3: the five 64 -> 64 DeformConv nodes at the H/4 x W/4 maps, "
                          "one launch per trunk stream and layer)",
                "note": "corner-row bytes the bilinear gather requests per launch (pixels x 9 taps x 4 corners x 64 channels x 4 B, "
                        "36 x the unique input) / average launch duration, against the guide's chip-wide L2-resident row-gather rate "
                        "(16.8-18.8 TB/s, MI355X_MICROARCH.md 'Indexed rows: gather into LDS'); launches of the two trunk streams "
                        "overlap, so a launch's duration includes what runs beside it; its MFMA-roofline frac is ~0.05",
                "traffic": measured_traffic(prefixes=("dcn_f16x3_kernel<2, 2, 1, true, 1>",)),   # HBM-side bytes per launch (all 20 launches of the form)
                "bytes_per_launch": g_b, "avg_launch_ms": round(g_avg_ms, 4), "launches_timed": g_n}
        default_run = (B, H, W) == (16, 448, 800) and not args.exact_fp32 and args.offset_std == 0.01
        if args.full and world == 1:
            if args.no_cpu_baseline:
                result["cpu_baseline"] = None
            else:
                if default_run:
                    del images, pc_dep
                    torch.cuda.empty_cache()
                    result["other_configs"] = other_configs(dev)
                result["cpu_baseline"] = cpu_baseline(H, W, batch=B)
        os.write(json_fd, (json.dumps(result) + "\n").encode())
    if collective:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
