"""Time of the parameter update over the full `DLASeg` parameter set (after `unfreeze_stem()`: every parameter has a gradient) with
random gradients: FusedAdamW / FusedSGD of this package against `torch.optim.AdamW` / `SGD` as the reference constructs them
(torch picks its `foreach` implementation on the device) and against torch's own `fused=True` kernels - six arms on private copies
of the parameters, same machine, same process, interleaved rounds.

Per arm, HIP events around `--inner` consecutive steps, divided by their number, median / min / max over `--rounds` rounds after
warm-up, twice: `device_ms_per_step` with the steps queued behind a 100 ms spin kernel (cf_spin_us), so that the host is ahead
and the device runs them back to back - the time the launches themselves take; and `loop_ms_per_step` without it - the pace of a
loop of nothing but steps, which is the host's where a `step()` call costs more than its kernels.  Then the host time of one
`step()` call (a host clock around calls that are not waited for: the enqueue cost); and the bytes
the update has to move (AdamW: read p, g, m, v, write p, m, v = 28 B per parameter; SGD with momentum: read p, g, buf, write p,
buf = 20 B) over the device time, as a fraction of the 6.29 TB/s copy rate of one MI355X.

    python tools/optim_time.py [--rounds 9] [--inner 20] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from centerfusiondetect3d_amd import FusedAdamW, FusedSGD, _lib, config as cfgm, getModel  # noqa: E402

COPY_RATE = 6.29e12              # B/s, the device-to-device copy rate of one MI355X
ADAMW = dict(lr=2.5e-4, weight_decay=5e-4)
SGD = dict(lr=1e-2, momentum=0.9, weight_decay=5e-4)
ARMS = (("adamw_hip", lambda p: FusedAdamW(p, **ADAMW), 28),
        ("adamw_torch_foreach", lambda p: torch.optim.AdamW(p, **ADAMW), 28),
        ("adamw_torch_fused", lambda p: torch.optim.AdamW(p, fused=True, **ADAMW), 28),
        ("sgd_hip", lambda p: FusedSGD(p, **SGD), 20),
        ("sgd_torch_foreach", lambda p: torch.optim.SGD(p, **SGD), 20),
        ("sgd_torch_fused", lambda p: torch.optim.SGD(p, fused=True, **SGD), 20))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_time.py measures on the device: no GPU found")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    c = cfgm.centerfusion_middle_config((448, 800))
    c.MODEL.FREEZE_BACKBONE = True
    m = getModel(cfgm.update_loss_weights(c)).to(dev).unfreeze_stem()
    shapes = [tuple(p.shape) for p in m.parameters()]
    assert all(p.requires_grad for p in m.parameters())
    numel = sum(p.numel() for p in m.parameters())
    res = {"tensors": len(shapes), "parameters": numel, "rounds": a.rounds, "inner": a.inner}

    arms = []
    for name, make, bytes_per in ARMS:
        ps = [torch.nn.Parameter(p.detach().clone()) for p in m.parameters()]
        for p in ps:
            p.grad = torch.randn_like(p) * 1e-2
        try:
            opt = make(ps)
            for _ in range(3):                               # warm-up: states, tables, code objects
                opt.step()
        except (RuntimeError, ValueError) as e:              # an implementation this torch build does not offer on the device
            res[name] = {"unavailable": str(e).splitlines()[0]}
            continue
        arms.append((name, opt, bytes_per))
    torch.cuda.synchronize()

    lib = _lib.load()
    per_step, loop = {name: [] for name, _, _ in arms}, {name: [] for name, _, _ in arms}
    for _ in range(a.rounds):
        for name, opt, _ in arms:
            for out, spin_us in ((per_step, 100000), (loop, 0)):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                if spin_us:
                    _lib.check(lib.cf_spin_us(spin_us, _lib.stream_ptr()), "cf_spin_us")
                s.record()
                for _ in range(a.inner):
                    opt.step()
                e.record()
                e.synchronize()
                out[name].append(s.elapsed_time(e) / a.inner)
    host = {}
    for name, opt, _ in arms:
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.inner):
            t0 = time.perf_counter()
            opt.step()
            ts.append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()                         # (outside the clock: the next call meets an empty queue)
        host[name] = statistics.median(ts)
    for name, _, bytes_per in arms:
        ms = per_step[name]
        med = statistics.median(ms)
        res[name] = {"device_ms_per_step": [round(med, 4), round(min(ms), 4), round(max(ms), 4)],
                     "loop_ms_per_step": [round(statistics.median(loop[name]), 4), round(min(loop[name]), 4), round(max(loop[name]), 4)],
                     "host_ms_per_call": round(host[name], 4),
                     "bytes": bytes_per * numel, "fraction_of_copy_rate": round(bytes_per * numel / (med * 1e-3) / COPY_RATE, 4)}
    for kind in ("adamw", "sgd"):
        best = min((n for n, _, _ in arms if n.startswith(kind)), key=lambda n: res[n]["device_ms_per_step"][0])
        res[kind + "_fastest"] = best
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
