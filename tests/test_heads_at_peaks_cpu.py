"""CPU: the output dict of an at-peaks forward (pending.PendingOutputs) with a stand-in materialiser - which operations complete
the maps, that it happens once, key order, `dict(y)`, decode's private access and its `rotation2` handling, and the plan's
weak-reference flush."""
import gc
import pickle

import pytest
import torch

from centerfusiondetect3d_amd.pending import PendingOutputs

KEYS = ["heatmap", "reg", "depth", "depthMap", "calib", "pc_hm", "velocity", "rotation2"]


def make():
    """a pending dict whose materialiser fills the (zero) maps with their index + 1 and counts its calls"""
    maps = {k: torch.zeros(2) for k in KEYS}
    calls = []

    def materialise():
        calls.append(1)
        for i, k in enumerate(KEYS):
            maps[k].fill_(i + 1.0)

    return PendingOutputs(maps, materialise), calls, maps


READS = {
    "getitem": lambda y: y["reg"],
    "get": lambda y: y.get("reg"),
    "get_missing": lambda y: y.get("nothing"),
    "pop": lambda y: y.pop("reg"),
    "items": lambda y: list(y.items()),
    "values": lambda y: list(y.values()),
    "iter": lambda y: [k for k in y],
    "dict": lambda y: dict(y),
    "unpack": lambda y: {**y},
    "update_into": lambda y: {}.update(y),
    "copy": lambda y: y.copy(),
    "eq": lambda y: y == {},
    "setdefault": lambda y: y.setdefault("reg", None),
    "heatmap": lambda y: y["heatmap"],                        # whoever holds the heat map may write to it
    "pickle": lambda y: pickle.dumps(y),
    "repr": lambda y: repr(y),                                 # (printing the dict shows the maps)
    "str": lambda y: str(y),
    "or": lambda y: y | {},
    "ror": lambda y: {} | y,
    "ior": lambda y: y.__ior__({}),
}


@pytest.mark.parametrize("name", sorted(READS))
def test_a_read_materialises_once(name):
    y, calls, _ = make()
    assert y.pending and not calls
    READS[name](y)
    assert calls == [1] and not y.pending
    for read in READS.values():                                # nothing runs a second time
        if "reg" in y or read not in (READS["getitem"], READS["pop"]):
            read(y)
    assert calls == [1]


def test_key_queries_and_writes_do_not_materialise():
    y, calls, _ = make()
    assert list(y.keys()) == KEYS and len(y) == len(KEYS) and "reg" in y and "rotation" not in y and bool(y)
    y["extra"] = 1
    del y["extra"]
    assert isinstance(y, dict) and repr(type(y).__mro__[1]) == "<class 'dict'>"
    assert y.peek("reg") is dict.__getitem__(y, "reg") and y.peek("nothing", 7) == 7
    assert not calls and y.pending


def test_values_read_are_the_completed_ones_in_key_order():
    y, _, maps = make()
    d = dict(y)
    assert type(d) is dict and list(d) == KEYS
    assert all(d[k] is maps[k] and float(d[k][0]) == i + 1.0 for i, k in enumerate(KEYS))
    y2, _, _ = make()
    assert [float(v[0]) for v in y2.values()] == [i + 1.0 for i in range(len(KEYS))]
    y3, _, _ = make()
    assert [k for k, _ in y3.items()] == KEYS


def test_decode_access_renames_rotation2_without_materialising():
    y, calls, maps = make()
    y.rename("rotation2", "rotation")
    assert not calls and y.pending
    assert list(y.keys()) == KEYS[:-1] + ["rotation"] and y.peek("rotation") is maps["rotation2"]
    assert float(y["rotation"][0]) == len(KEYS)               # completed by the first public read: the same tensor
    assert calls == [1]


def test_a_failing_materialiser_leaves_the_dict_pending():
    state = {"fail": True, "calls": 0}

    def materialise():
        state["calls"] += 1
        if state["fail"]:
            raise RuntimeError("launch failed")

    y = PendingOutputs({"a": 1}, materialise)
    with pytest.raises(RuntimeError):
        y["a"]
    assert y.pending
    state["fail"] = False
    assert y["a"] == 1 and not y.pending and state["calls"] == 2


class _PlanStandIn:
    """the flush of plan._Plan on its own: `_last` and `flush_pending` are all it touches"""
    from centerfusiondetect3d_amd.plan import _Plan
    flush_pending = _Plan.flush_pending

    def __init__(self):
        self._last = None


def test_weak_reference_flush():
    import weakref
    p = _PlanStandIn()
    p.flush_pending()                                          # nothing yet
    y, calls, _ = make()
    p._last = weakref.ref(y)
    p.flush_pending()                                          # still held and unread, no way to release: completed before the next forward
    assert calls == [1] and not y.pending and p._last is None
    y, calls, _ = make()
    p._last = weakref.ref(y)
    y["reg"]
    p.flush_pending()                                          # already read: nothing more
    assert calls == [1]
    y, calls, _ = make()
    p._last = weakref.ref(y)
    del y
    gc.collect()
    p.flush_pending()                                          # dropped: never computed
    assert calls == [] and p._last is None


def test_release_keeps_the_dict_pending_and_runs_once():
    """with a `release` (the plan's: it copies the buffers the dense launches read) the flush completes nothing"""
    import weakref
    maps, calls, released = {k: torch.zeros(2) for k in KEYS}, [], []
    y = PendingOutputs(maps, lambda: calls.append(1), None, lambda: released.append(1))
    p = _PlanStandIn()
    p._last = weakref.ref(y)
    p.flush_pending()
    assert released == [1] and not calls and y.pending and p._last is None
    y.release()                                                # (once)
    assert released == [1] and not calls and y.pending
    y["reg"]
    assert calls == [1] and released == [1] and not y.pending
    y.release()
    assert calls == [1] and released == [1]
    z = PendingOutputs(maps, lambda: calls.append(2), None, lambda: released.append(2))
    z["reg"]
    z.release()                                                # complete: nothing left to release
    assert released == [1] and calls == [1, 2]
