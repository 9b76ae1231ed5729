"""The optimizer half of the reference's training run (model/modelWithLoss.py:57-203): AdamW and SGD as ONE multi-tensor HIP
launch per parameter group (cf_optim_adamw / cf_optim_sgd of include/cf_hip.h), and `configure_optimizers`, the reference's
optimizer + learning-rate schedule for a config.

`FusedAdamW` / `FusedSGD` are `torch.optim.Optimizer` subclasses with torch's constructor arguments, `param_groups` and
`state_dict()` layout, so torch's LR schedulers drive them and a state saved here loads into `torch.optim.AdamW` /
`torch.optim.SGD` and back.  What differs from torch:

  * the update runs in a kernel torch knows nothing about, so `step()` bumps every updated parameter's version counter itself
    (`torch.autograd.graph.increment_version`): `ops.deform_conv2d` keys its weight packs on it, and autograd's check for a
    saved tensor "modified by an inplace operation" relies on it;
  * `zero_grad()` defaults to `set_to_none=False`: the gradients keep their storage, so the device tables (pointers and sizes)
    built at the first step stay valid and a steady-state `step()` allocates nothing, copies nothing to the device and never
    waits for it.  The tables are rebuilt whenever the set of (parameter, gradient) pointers changes - a parameter that receives
    its first gradient later (the defreeze) joins then, with a step count that starts at 1, as torch's per-parameter count does;
  * the per-parameter `step` of AdamW lives as (the group's count) - (the count when the parameter joined) and becomes torch's
    `step` tensor in `state_dict()`;
  * `amsgrad`, `maximize`, `nesterov`, `dampening != 0`, non-fp32, non-contiguous and sparse tensors are refused, and there is
    no CPU path.
"""
import ctypes as C

import torch

from . import _lib, ops


class _FusedOptimizer(torch.optim.Optimizer):
    """Tables, launch and version bump shared by FusedAdamW and FusedSGD.  Per group: `_t` the optimizer's step count, `_key` the
    (parameter, gradient) pointers the device tables were built for, `_tab` those tables."""

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self._t = [0] * len(self.param_groups)
        self._base = {}                     # parameter -> the group's count before the parameter's first update
        self._drop_tables()

    def _drop_tables(self):
        self._key = [None] * len(self.param_groups)
        self._tab = [None] * len(self.param_groups)

    def add_param_group(self, group):
        super().add_param_group(group)
        if hasattr(self, "_t"):             # (the constructor adds its groups before the counts exist)
            self._t.append(0)
            self._drop_tables()

    def zero_grad(self, set_to_none=False):
        """torch's `zero_grad`, with `set_to_none=False` as the default: gradients that keep their storage keep the tables of
        `step()` valid (see the module text); `set_to_none=True` works too and costs a table rebuild per step."""
        super().zero_grad(set_to_none=set_to_none)

    # ---- subclass hooks
    def _new_state(self, p, group):
        raise NotImplementedError

    def _state_ptrs(self, p, group):
        raise NotImplementedError

    def _launch(self, lib, args, group, stream):
        raise NotImplementedError

    # ---- tables
    def _index_of(self, p):
        i = 0
        for g in self.param_groups:
            for q in g["params"]:
                if q is p:
                    return i
                i += 1
        return -1

    def _validate(self, p, g):
        what = None
        if g.is_sparse or g.layout is not torch.strided:
            what = "a sparse gradient"
        elif p.dtype is not torch.float32 or g.dtype is not torch.float32:
            what = f"dtype {p.dtype} / gradient {g.dtype} (fp32 only)"
        elif not p.is_contiguous() or not g.is_contiguous():
            what = "a non-contiguous parameter or gradient"
        if what is not None:
            raise NotImplementedError(f"{type(self).__name__}: parameter {self._index_of(p)} has {what}")
        if not p.is_cuda or not g.is_cuda:
            raise _lib.CfHipError(f"{type(self).__name__}: parameter {self._index_of(p)} is not on the device (no CPU path)")
        if g.device != p.device or g.numel() != p.numel():
            raise _lib.CfHipError(f"{type(self).__name__}: parameter {self._index_of(p)} and its gradient differ in device or size")

    def _build(self, gi, group, live):
        """device tables for the parameters of `group` that have a gradient -> (tensor table, chunk table, n_tensors, n_chunks)"""
        lib = _lib.load()
        t = self._t[gi]
        recs = (_lib.OptimTensor * len(live))()
        for r, p in zip(recs, live):
            self._validate(p, p.grad)
            if p not in self._base:
                self._base[p] = t
                self._new_state(p, group)
            s1, s2 = self._state_ptrs(p, group)
            r.param, r.grad, r.state1, r.state2 = p.data_ptr(), p.grad.data_ptr(), s1, s2
            r.numel, r.step_base = p.numel(), self._base[p]
        n_chunks = C.c_int64(0)
        _lib.check(lib.cf_optim_plan(recs, len(live), None, 0, C.byref(n_chunks)), "cf_optim_plan")
        n = int(n_chunks.value)
        if n == 0:
            return None
        chunks = (_lib.OptimChunk * n)()
        _lib.check(lib.cf_optim_plan(recs, len(live), chunks, n, C.byref(n_chunks)), "cf_optim_plan")
        dev = live[0].device
        if any(p.device != dev for p in live):
            raise _lib.CfHipError(f"{type(self).__name__}: the parameters of group {gi} live on several devices")
        up = lambda buf: torch.frombuffer(bytearray(bytes(buf)), dtype=torch.uint8).to(dev)
        return up(recs), up(chunks), len(live), n

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        for gi, group in enumerate(self.param_groups):
            live, key = [], []
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise NotImplementedError(f"{type(self).__name__}: parameter {self._index_of(p)} has a sparse gradient")
                live.append(p)
                key.append(p.data_ptr())
                key.append(g.data_ptr())
            if not live:
                continue
            if key != self._key[gi]:
                self._tab[gi] = self._build(gi, group, live)
                self._key[gi] = key
            tab = self._tab[gi]
            self._t[gi] += 1
            if tab is None:                 # (only empty tensors)
                continue
            a = _lib.OptimArgs()
            a.tensors, a.chunks, a.n_tensors, a.n_chunks = tab[0].data_ptr(), tab[1].data_ptr(), tab[2], tab[3]
            a.step = self._t[gi]
            with torch.cuda.device(live[0].device):
                self._launch(lib, a, group, _lib.stream_ptr())
            torch.autograd.graph.increment_version(live)
        return loss

    # ---- state dicts in torch's layout
    def _export_steps(self):
        pass

    def _import_steps(self):
        raise NotImplementedError

    def state_dict(self):
        self._export_steps()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._base = {}
        self._t = [0] * len(self.param_groups)
        self._drop_tables()
        self._import_steps()


class FusedAdamW(_FusedOptimizer):
    """`torch.optim.AdamW` (decoupled weight decay, torch's single-tensor formulas in fp32) as one HIP launch per group."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False):
        if amsgrad:
            raise NotImplementedError("FusedAdamW: amsgrad is not implemented")
        if maximize:
            raise NotImplementedError("FusedAdamW: maximize is not implemented")
        lr = float(lr)
        if lr < 0.0 or eps < 0.0 or weight_decay < 0.0 or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"FusedAdamW: invalid lr={lr}, betas={betas}, eps={eps} or weight_decay={weight_decay}")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False))

    def _new_state(self, p, group):
        st = self.state[p]
        if "exp_avg" not in st:
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)

    def _state_ptrs(self, p, group):
        st = self.state[p]
        for k in ("exp_avg", "exp_avg_sq"):
            s = st[k]
            if s.dtype is not torch.float32 or not s.is_contiguous() or s.device != p.device or s.numel() != p.numel():
                raise NotImplementedError(f"FusedAdamW: parameter {self._index_of(p)} has a {k} that is not fp32, contiguous and "
                                          "of the parameter's size and device")
        return st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()

    def _launch(self, lib, a, group, stream):
        if group.get("amsgrad") or group.get("maximize"):
            raise NotImplementedError("FusedAdamW: amsgrad / maximize are not implemented")
        lr, wd = float(group["lr"]), float(group["weight_decay"])
        a.lr, a.decay = lr, 1.0 - lr * wd
        a.beta1, a.beta2, a.eps = float(group["betas"][0]), float(group["betas"][1]), float(group["eps"])
        _lib.check(lib.cf_optim_adamw(C.byref(a), stream), "cf_optim_adamw")

    def _export_steps(self):
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                if p in self._base:
                    self.state[p]["step"] = torch.tensor(float(self._t[gi] - self._base[p]), dtype=torch.float32)

    def _import_steps(self):
        for gi, group in enumerate(self.param_groups):
            steps = {p: int(float(self.state[p]["step"])) for p in group["params"] if p in self.state and "step" in self.state[p]}
            self._t[gi] = max(steps.values(), default=0)
            for p, s in steps.items():
                self._base[p] = self._t[gi] - s


class FusedSGD(_FusedOptimizer):
    """`torch.optim.SGD` (weight decay added to the gradient, momentum buffer seeded with the first gradient) as one HIP launch
    per group."""

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, *, maximize=False):
        if nesterov:
            raise NotImplementedError("FusedSGD: nesterov is not implemented")
        if dampening != 0:
            raise NotImplementedError("FusedSGD: dampening != 0 is not implemented")
        if maximize:
            raise NotImplementedError("FusedSGD: maximize is not implemented")
        lr = float(lr)
        if lr < 0.0 or momentum < 0.0 or weight_decay < 0.0:
            raise ValueError(f"FusedSGD: invalid lr={lr}, momentum={momentum} or weight_decay={weight_decay}")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=0.0, weight_decay=weight_decay, nesterov=False,
                                      maximize=False))

    def _new_state(self, p, group):
        st = self.state[p]
        if group["momentum"] == 0:
            st.setdefault("momentum_buffer", None)
        elif st.get("momentum_buffer") is None:     # (its first value is written, not read: no need to clear it)
            st["momentum_buffer"] = torch.empty_like(p, memory_format=torch.preserve_format)

    def _state_ptrs(self, p, group):
        s = self.state[p].get("momentum_buffer")
        if group["momentum"] == 0:
            return None, None
        if s is None or s.dtype is not torch.float32 or not s.is_contiguous() or s.device != p.device or s.numel() != p.numel():
            raise NotImplementedError(f"FusedSGD: parameter {self._index_of(p)} has a momentum_buffer that is not fp32, contiguous "
                                      "and of the parameter's size and device")
        return s.data_ptr(), None

    def _launch(self, lib, a, group, stream):
        if group.get("nesterov") or group.get("dampening") or group.get("maximize"):
            raise NotImplementedError("FusedSGD: nesterov / dampening / maximize are not implemented")
        a.lr, a.wd, a.momentum = float(group["lr"]), float(group["weight_decay"]), float(group["momentum"])
        _lib.check(lib.cf_optim_sgd(C.byref(a), stream), "cf_optim_sgd")

    def _import_steps(self):
        # torch keeps no count for SGD: a parameter with a buffer has made its first step, the others make it when they join
        for gi, group in enumerate(self.param_groups):
            self._t[gi] = 1
            for p in group["params"]:
                if p in self.state and self.state[p].get("momentum_buffer") is not None:
                    self._base[p] = 0


# ------------------------------------------------------------------------------------------------------- the reference's recipe
TRAIN_DEFAULTS = dict(OPTIMIZER="adam", LR=2.5e-4, LR_STEP=(50,), WARM_EPOCHS=5, EPOCHS=60, LR_SCHEDULER="StepLR", RESUME=False)
MODEL_DEFAULTS = dict(DEFREEZE=-1)
WEIGHT_DECAY = 5e-4
SGD_MOMENTUM = 0.9
FALLBACK_LR = {"adam": 1e-3, "sgd": 1e-2}          # where TRAIN.LR is 0 / None


def _setting(config, section, key):
    node = getattr(config, section, None)
    default = (TRAIN_DEFAULTS if section == "TRAIN" else MODEL_DEFAULTS)[key]
    if node is None:
        return default
    if isinstance(node, dict):
        return node.get(key, default)
    return getattr(node, key, default)


def _step_lr_schedule(optimizer, lr_steps, warm, defreeze, start_epoch):
    """`StepLR` of the reference: x0.1 at every TRAIN.LR_STEP, behind a warm-up of `warm` epochs that doubles the LR each epoch
    up to the start LR - at the start of the run and again behind the defreeze.  Epochs are counted from `start_epoch`, the
    warm-up shifts the drops by its length: all of it as the reference does it, its resume behaviour included."""
    from torch.optim.lr_scheduler import LambdaLR, MultiStepLR, SequentialLR

    def warm_up():
        return LambdaLR(optimizer, lr_lambda=lambda e: 0.5 ** (warm - e))

    def drops(at):
        return MultiStepLR(optimizer, milestones=at, gamma=0.1)

    phases, switch_at = [], []
    if warm:
        phases.append(warm_up())
        switch_at.append(warm)
    if defreeze > start_epoch:                              # a frozen phase comes first
        phases.append(drops([s - start_epoch - warm for s in lr_steps if s < defreeze]))
        switch_at.append(defreeze - start_epoch)
        if warm:
            phases.append(warm_up())
            switch_at.append(defreeze + warm - start_epoch)
    phases.append(drops([s - warm - max(defreeze, start_epoch) for s in lr_steps if s >= defreeze]))
    return SequentialLR(optimizer, phases, milestones=switch_at)


def _cyclic_schedule(optimizer, lr, lr_steps, defreeze, epochs):
    """`CLR` of the reference: a triangular cycle between LR / 15 and LR (five epochs up) until the defreeze, a halving one behind
    it, and from every TRAIN.LR_STEP behind the defreeze on a constant factor 0.1^k."""
    from torch.optim.lr_scheduler import ConstantLR, CyclicLR, SequentialLR

    def cycle(mode):
        return CyclicLR(optimizer, base_lr=lr / 15, max_lr=lr, step_size_up=5, cycle_momentum=False, mode=mode)

    phases, switch_at = [cycle("triangular"), cycle("triangular2")], [defreeze]
    power = 0
    for i, s in enumerate(lr_steps):
        if s <= defreeze:
            continue
        power += 1
        until = lr_steps[i + 1] if i + 1 < len(lr_steps) else epochs
        phases.append(ConstantLR(optimizer, factor=0.1 ** power, last_epoch=-1, total_iters=until - s + 2))
        switch_at.append(s)
    return SequentialLR(optimizer, phases, milestones=switch_at)


def configure_optimizers(model, config, start_epoch=1, fused=True):
    """The reference's optimizer and LR schedule for `config` (model/modelWithLoss.py:57-203) -> (optimizer, scheduler); step the
    scheduler once per epoch.  Reads TRAIN.OPTIMIZER ('adam' -> AdamW, 'sgd' -> SGD with momentum 0.9; weight decay 5e-4 both),
    TRAIN.LR (x0.1 for every TRAIN.LR_STEP a resumed run has passed), TRAIN.LR_SCHEDULER ('StepLR' / 'CLR'), TRAIN.WARM_EPOCHS,
    TRAIN.EPOCHS and MODEL.DEFREEZE, with the reference's defaults (TRAIN_DEFAULTS, MODEL_DEFAULTS) where the config lacks a key.
    Every parameter of the model is handed over, frozen ones included, as the reference does: they join when they receive a
    gradient.  fused=False builds the same on torch.optim."""
    kind = _setting(config, "TRAIN", "OPTIMIZER")
    lr = _setting(config, "TRAIN", "LR")
    lr_steps = tuple(_setting(config, "TRAIN", "LR_STEP"))
    sched = _setting(config, "TRAIN", "LR_SCHEDULER")
    defreeze = _setting(config, "MODEL", "DEFREEZE")
    if kind not in FALLBACK_LR:
        raise ValueError(f"TRAIN.OPTIMIZER = {kind!r}: 'adam' or 'sgd'")
    if sched not in ("StepLR", "CLR"):
        raise ValueError(f"TRAIN.LR_SCHEDULER = {sched!r}: 'StepLR' or 'CLR'")
    start_lr = lr if lr else FALLBACK_LR[kind]
    for s in lr_steps:
        if start_epoch >= s:
            start_lr *= 0.1
    params = model.parameters()
    if kind == "adam":
        optimizer = (FusedAdamW if fused else torch.optim.AdamW)(params, start_lr, weight_decay=WEIGHT_DECAY)
    else:
        optimizer = (FusedSGD if fused else torch.optim.SGD)(params, start_lr, momentum=SGD_MOMENTUM, weight_decay=WEIGHT_DECAY)
    if sched == "CLR":
        scheduler = _cyclic_schedule(optimizer, lr, lr_steps, defreeze, _setting(config, "TRAIN", "EPOCHS"))
    else:
        scheduler = _step_lr_schedule(optimizer, lr_steps, _setting(config, "TRAIN", "WARM_EPOCHS"), defreeze, start_epoch)
    return optimizer, scheduler


OPTIM_CHUNK = ops.OPTIM_CHUNK
