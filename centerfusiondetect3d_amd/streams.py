"""The process-wide side streams: which HIP streams run beside a caller's stream, chosen once by a probe of spin kernels.
Lock order everywhere: `_CAPTURE_LOCK`, then `_SIDE_LOCK`; nothing here synchronises beside another thread's stream capture."""
import threading

import torch

from . import _lib

_SIDE_STREAMS = {}    # (device, caller stream id) -> probed side streams, LRU of _SIDE_KEYS keys per PROCESS
_SIDE_KEYS = 16
_SIDE_LOCK = threading.Lock()
_CAPTURE_LOCK = threading.RLock()   # held while a stream captures AND while a captured graph is destroyed (see DLASeg._forward_graph)
_PROBE_US = 300       # length of one probe spin; two of them take ~1x this when concurrent, ~2x when serialised
_PROBE_LOG = []       # [(device, sid, n, chosen indices, [(i, j, ms)])]: what the probes measured (tests / DESIGN)


def _concurrent(lib, a, b, us=_PROBE_US):
    """True if a `cf_spin_us` on stream `a` and one on stream `b`, issued back to back, overlap in time.  HIP maps
    streams onto a few hardware queues; two streams that share one run their kernels strictly one after the other
    (model.streams = 2 then measures 10.5 instead of 8.5 ms per bs=16 step).  -> (bool, ms from first start to last end)"""
    e0, e1a, e1b = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    gate = torch.cuda.Event()
    gate.record(a)
    b.wait_event(gate)                       # neither spin starts before both streams have drained to here
    e0.record(a)
    _lib.check(lib.cf_spin_us(us, a.cuda_stream), "cf_spin_us")
    e1a.record(a)
    _lib.check(lib.cf_spin_us(us, b.cuda_stream), "cf_spin_us")
    e1b.record(b)
    e1a.synchronize()
    e1b.synchronize()
    ms = max(e0.elapsed_time(e1a), e0.elapsed_time(e1b))
    return ms < 1.6e-3 * us, ms


def _pick_streams(device, cur, n, pool):
    """Extend `pool` to n streams that run concurrently with each other and with the caller's stream `cur` (the
    two-lane neck issues on `cur` and on pool[0]; the heads, the decode and `Detector.run_pipelined`'s consumer run on
    `cur` beside whatever the last pool stream feeds).  Candidates are taken from torch's stream pool
    one at a time and kept only if a pair of spin kernels says they overlap with everything chosen so far - whatever
    else of the process (RCCL's communicator stream, other models, user streams) already sits on the hardware queues.
    Falls back to plain creation order if no concurrent set turns up within 12 candidates (still correct, only slower)."""
    lib = _lib.load()
    tried, log = [], []
    with _CAPTURE_LOCK:                       # the probe synchronises: never beside another thread's stream capture
        torch.cuda.synchronize(device)
        while len(pool) < n and len(tried) < 12:
            c = torch.cuda.Stream(device)
            tried.append(c)
            ok = True
            for x in [cur] + pool:
                good, ms = _concurrent(lib, x, c)
                log.append((len(tried) - 1, "caller" if x is cur else pool.index(x), round(ms, 3)))
                if not good:
                    ok = False
                    break
            if ok:
                pool.append(c)
    fallback = len(pool) < n
    for c in tried:                           # not enough concurrent ones: take what was created, in order
        if len(pool) >= n:
            break
        if c not in pool:
            pool.append(c)
    _PROBE_LOG.append((str(device), int(cur.cuda_stream), n, fallback, log))
    del _PROBE_LOG[:-32]
    return pool


def _side_streams(device, sid, n):
    """The n side streams that work issued on caller stream `sid` of `device` forks onto.  One set per process and caller
    stream, not per model or plan, chosen ONCE by a probe (`_pick_streams`) instead of by creation order: HIP spreads
    streams over a few hardware queues, whether two side streams share a queue decides whether their kernels overlap
    at all (8.5 vs 10.5 ms per bs=16 step), and under torchrun RCCL has taken streams before the first model exists.
    During a graph capture nothing may synchronise: fresh streams are forked as they come (the replay's placement is
    the graph executor's, not these streams')."""
    key = (str(device), int(sid))
    with _SIDE_LOCK:                              # the common case: the set exists
        pool = _SIDE_STREAMS.get(key)
        if pool is not None and len(pool) >= n:
            _SIDE_STREAMS[key] = _SIDE_STREAMS.pop(key)          # re-inserted last: dict order is the LRU order
            return pool[:n]
    # streams are missing: the probe synchronises the device, which must not happen beside another thread's stream
    # capture - lock order is _CAPTURE_LOCK, then _SIDE_LOCK, everywhere (a capturing thread holds the first already)
    with _CAPTURE_LOCK, _SIDE_LOCK:
        pool = _SIDE_STREAMS.pop(key, [])
        if len(pool) < n:
            if torch.cuda.is_current_stream_capturing():
                while len(pool) < n:
                    pool.append(torch.cuda.Stream(device))
            else:
                pool = _pick_streams(device, torch.cuda.current_stream(device), n, pool)
        _SIDE_STREAMS[key] = pool
        while len(_SIDE_STREAMS) > _SIDE_KEYS:
            _SIDE_STREAMS.pop(next(iter(_SIDE_STREAMS)))
        return pool[:n]
