"""CPU: the optimizer half of the training run without a device - `configure_optimizers` against the schedules recorded from
the reference's own function (tests/golden/lr_schedules.npz, make_golden_schedule.py), the refusals of FusedAdamW / FusedSGD,
the argument validation of the C entry points, and the saveModel / loadModel round trip."""
import ctypes as C
import json
import os
import warnings

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = np.load(os.path.join(HERE, "golden", "lr_schedules.npz"))
NAMES = [str(n) for n in FIX["names"]]
# the seven configurations the schedule is pinned on must all be there (an eighth, the SGD twin of the CLR case, may be)
REQUIRED = ["adam_step", "sgd_step_nowarm", "adam_step_defreeze", "adam_step_resume30", "adam_step_resume55", "adam_clr_defreeze",
            "adam_clr"]


def _case_config(case):
    from centerfusiondetect3d_amd import config as cfgm
    c = cfgm.centerfusion_middle_config((64, 96))
    c.TRAIN.OPTIMIZER, c.TRAIN.LR_SCHEDULER, c.TRAIN.LR = case["optimizer"], case["scheduler"], case["lr"]
    c.TRAIN.LR_STEP, c.TRAIN.WARM_EPOCHS, c.TRAIN.EPOCHS = tuple(case["lr_step"]), case["warm_epochs"], case["epochs"]
    c.MODEL.DEFREEZE = case["defreeze"]
    return c


def test_the_fixture_holds_the_pinned_cases():
    assert NAMES[:7] == REQUIRED
    want = {"adam_step": ("adam", "StepLR", [50], 5, -1, 60, 1), "sgd_step_nowarm": ("sgd", "StepLR", [50], 0, -1, 60, 1),
            "adam_step_defreeze": ("adam", "StepLR", [10, 50], 5, 20, 60, 1), "adam_step_resume30": ("adam", "StepLR", [50], 5, -1, 60, 30),
            "adam_step_resume55": ("adam", "StepLR", [50], 5, -1, 60, 55),
            "adam_clr_defreeze": ("adam", "CLR", [90, 170, 210], 5, 100, 230, 1), "adam_clr": ("adam", "CLR", [50], 5, -1, 60, 1)}
    for n, w in want.items():
        c = json.loads(str(FIX[f"{n}.case"]))
        assert (c["optimizer"], c["scheduler"], c["lr_step"], c["warm_epochs"], c["defreeze"], c["epochs"], c["start_epoch"]) == w
        assert c["lr"] == 2.5e-4 and len(FIX[f"{n}.lrs"]) == c["epochs"] + 1


@pytest.mark.parametrize("name", NAMES)
def test_configure_optimizers_gives_the_references_schedule(name):
    from centerfusiondetect3d_amd import configure_optimizers
    case = json.loads(str(FIX[f"{name}.case"]))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                    # (scheduler.step() before optimizer.step(): nothing trains here)
        opt, sched = configure_optimizers(torch.nn.Linear(1, 1), _case_config(case), start_epoch=case["start_epoch"], fused=False)
        assert type(opt).__name__ == str(FIX[f"{name}.optimizer"])
        assert type(opt) is {"AdamW": torch.optim.AdamW, "SGD": torch.optim.SGD}[type(opt).__name__]
        assert opt.defaults["lr"] == float(FIX[f"{name}.lr"]) and opt.defaults["weight_decay"] == float(FIX[f"{name}.weight_decay"])
        if type(opt) is torch.optim.SGD:
            assert opt.defaults["momentum"] == float(FIX[f"{name}.momentum"]) == 0.9
            assert not opt.defaults["nesterov"] and opt.defaults["dampening"] == 0
        assert len(opt.param_groups) == 1 and len(opt.param_groups[0]["params"]) == 2
        lrs = [opt.param_groups[0]["lr"]]
        for _ in range(case["epochs"]):
            sched.step()
            lrs.append(opt.param_groups[0]["lr"])
    want = FIX[f"{name}.lrs"]
    got = np.asarray(lrs, np.float64)
    assert got.shape == want.shape
    rel = np.abs(got - want) / np.abs(want)
    assert float(rel.max()) <= 1e-12, (name, int(rel.argmax()), got[rel.argmax()], want[rel.argmax()])


def test_configure_optimizers_defaults_and_the_fused_classes():
    """a config without the keys gets the reference's defaults (case adam_step); fused=True builds this package's classes with the
    same hyper-parameters on the same scheduler composition - constructing them needs no device"""
    from centerfusiondetect3d_amd import CfgNode, FusedAdamW, FusedSGD, configure_optimizers
    from centerfusiondetect3d_amd import config as cfgm
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        opt, sched = configure_optimizers(torch.nn.Linear(1, 1), CfgNode(TRAIN=CfgNode(UNCERTAINTY_LOSS=False), MODEL=CfgNode()),
                                          fused=False)
        lrs = [opt.param_groups[0]["lr"]]
        for _ in range(60):
            sched.step()
            lrs.append(opt.param_groups[0]["lr"])
        assert np.allclose(lrs, FIX["adam_step.lrs"], rtol=1e-12, atol=0)
        c = cfgm.centerfusion_middle_config((64, 96))
        assert (c.TRAIN.OPTIMIZER, c.TRAIN.LR, c.TRAIN.LR_STEP, c.TRAIN.WARM_EPOCHS, c.TRAIN.EPOCHS, c.TRAIN.LR_SCHEDULER,
                c.TRAIN.RESUME, c.MODEL.DEFREEZE) == ("adam", 2.5e-4, (50,), 5, 60, "StepLR", False, -1)
        opt, sched = configure_optimizers(torch.nn.Linear(3, 2), c)
        assert type(opt) is FusedAdamW and isinstance(opt, torch.optim.Optimizer)
        g = opt.param_groups[0]
        assert (g["betas"], g["eps"], g["weight_decay"]) == ((0.9, 0.999), 1e-8, 5e-4) and g["lr"] == FIX["adam_step.lrs"][0]
        sched.step()
        assert g["lr"] == FIX["adam_step.lrs"][1]
        c.TRAIN.OPTIMIZER = "sgd"
        opt, _ = configure_optimizers(torch.nn.Linear(3, 2), c)
        assert type(opt) is FusedSGD and opt.param_groups[0]["momentum"] == 0.9 and opt.param_groups[0]["weight_decay"] == 5e-4
        c.TRAIN.OPTIMIZER = "rmsprop"
        with pytest.raises(ValueError, match="OPTIMIZER"):
            configure_optimizers(torch.nn.Linear(3, 2), c)
        c.TRAIN.OPTIMIZER, c.TRAIN.LR_SCHEDULER = "adam", "cosine"
        with pytest.raises(ValueError, match="LR_SCHEDULER"):
            configure_optimizers(torch.nn.Linear(3, 2), c)


def test_constructor_defaults_are_torchs_and_the_unsupported_options_raise():
    from centerfusiondetect3d_amd import FusedAdamW, FusedSGD
    p = [torch.nn.Parameter(torch.zeros(3))]
    a, ta = FusedAdamW(p), torch.optim.AdamW(p)
    for k in ("lr", "betas", "eps", "weight_decay", "amsgrad", "maximize"):
        assert a.defaults[k] == ta.defaults[k], k
    s, ts = FusedSGD(p), torch.optim.SGD(p)
    for k in ("lr", "momentum", "dampening", "weight_decay", "nesterov", "maximize"):
        assert s.defaults[k] == ts.defaults[k], k
    with pytest.raises(NotImplementedError, match="amsgrad"):
        FusedAdamW(p, amsgrad=True)
    with pytest.raises(NotImplementedError, match="maximize"):
        FusedAdamW(p, maximize=True)
    with pytest.raises(NotImplementedError, match="nesterov"):
        FusedSGD(p, momentum=0.9, nesterov=True)
    with pytest.raises(NotImplementedError, match="dampening"):
        FusedSGD(p, momentum=0.9, dampening=0.1)
    with pytest.raises(NotImplementedError, match="maximize"):
        FusedSGD(p, maximize=True)
    with pytest.raises(ValueError):
        FusedAdamW(p, lr=-1.0)
    # the state dict of an optimizer that has not stepped is torch's
    assert a.state_dict()["state"] == {} and a.state_dict()["param_groups"][0]["params"] == [0]


@pytest.mark.parametrize("cls", ["FusedAdamW", "FusedSGD"])
def test_step_refuses_what_the_kernel_does_not_take_and_names_the_parameter(cls):
    """non-fp32, non-contiguous and sparse tensors raise NotImplementedError with the parameter's index, CPU parameters CfHipError;
    a parameter without a gradient is skipped (an optimizer none of whose parameters has one does nothing, on any device)"""
    import centerfusiondetect3d_amd as cf
    from centerfusiondetect3d_amd._lib import CfHipError
    make = getattr(cf, cls)
    ok = torch.nn.Parameter(torch.zeros(4))
    opt = make([ok, torch.nn.Parameter(torch.zeros(4))], lr=0.1)
    opt.step()                                             # no gradient anywhere: nothing to do
    assert opt.state_dict()["state"] == {}

    def stepping(p, grad):
        p.grad = grad
        return make([ok, p], lr=0.1)

    half = torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))
    with pytest.raises(NotImplementedError, match=r"parameter 1 .*fp32"):
        stepping(half, torch.zeros(4, dtype=torch.float64)).step()
    strided = torch.nn.Parameter(torch.zeros(4, 4).t())
    assert not strided.is_contiguous()
    with pytest.raises(NotImplementedError, match=r"parameter 1 .*non-contiguous"):
        stepping(strided, torch.zeros(4, 4).t()).step()
    gstr = torch.nn.Parameter(torch.zeros(4, 4))
    with pytest.raises(NotImplementedError, match=r"parameter 1 .*non-contiguous"):
        stepping(gstr, torch.zeros(4, 4).t()).step()
    sp = torch.nn.Parameter(torch.zeros(4, 4))
    with pytest.raises(NotImplementedError, match=r"parameter 1 .*sparse"):
        stepping(sp, torch.zeros(4, 4).to_sparse()).step()
    cpu = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(CfHipError, match=r"parameter 1 .*no CPU path"):
        stepping(cpu, torch.zeros(4)).step()
    assert torch.equal(cpu, torch.zeros(4)) and cpu._version == 0


def test_zero_grad_keeps_the_gradient_storage_by_default():
    from centerfusiondetect3d_amd import FusedAdamW
    p = torch.nn.Parameter(torch.ones(5))
    p.grad = torch.full((5,), 2.0)
    ptr = p.grad.data_ptr()
    opt = FusedAdamW([p])
    opt.zero_grad()
    assert p.grad is not None and p.grad.data_ptr() == ptr and float(p.grad.abs().max()) == 0
    opt.zero_grad(set_to_none=True)
    assert p.grad is None


def test_c_entry_points_validate_without_a_gpu():
    from centerfusiondetect3d_amd import _lib, ops
    lib = _lib.load()
    assert lib.cf_optim_chunk_elems() == _lib.CF_OPTIM_CHUNK == ops.OPTIM_CHUNK and ops.OPTIM_CHUNK % 4 == 0
    for fn, name in ((lib.cf_optim_adamw, b"cf_optim_adamw"), (lib.cf_optim_sgd, b"cf_optim_sgd")):
        assert fn(None, None) == -22 and name in lib.cf_last_error() and b"null args" in lib.cf_last_error()
        a = _lib.OptimArgs()
        a.n_tensors, a.n_chunks, a.step = 1, 1, 1
        assert fn(C.byref(a), None) == -22 and b"null table" in lib.cf_last_error()
        a.tensors, a.chunks = 4096, 8192                  # (never dereferenced: the next checks refuse first)
        a.n_tensors = 0
        assert fn(C.byref(a), None) == -22 and b"n_tensors=0" in lib.cf_last_error()
        a.n_tensors, a.n_chunks = 1, -3
        assert fn(C.byref(a), None) == -22 and b"n_chunks=-3" in lib.cf_last_error()
        a.n_chunks, a.step = 1, 0
        assert fn(C.byref(a), None) == -22 and b"step=0" in lib.cf_last_error()
    # the planner (host side): refusals, then the chunk list of a small table
    n = C.c_int64(-1)
    recs = (_lib.OptimTensor * 4)()
    assert lib.cf_optim_plan(None, 4, None, 0, C.byref(n)) == -22 and b"null table" in lib.cf_last_error()
    assert lib.cf_optim_plan(recs, 4, None, 0, None) == -22
    assert lib.cf_optim_plan(recs, 0, None, 0, C.byref(n)) == -22 and b"n=0" in lib.cf_last_error()
    ch = ops.OPTIM_CHUNK
    for r, numel in zip(recs, (1, 0, 2 * ch + 7, ch)):
        r.numel = numel
    recs[2].numel = -1
    assert lib.cf_optim_plan(recs, 4, None, 0, C.byref(n)) == -22 and b"tensor 2 has numel=-1" in lib.cf_last_error()
    recs[2].numel = 2 * ch + 7
    assert lib.cf_optim_plan(recs, 4, None, 0, C.byref(n)) == 0 and n.value == 5
    chunks = (_lib.OptimChunk * 5)()
    assert lib.cf_optim_plan(recs, 4, chunks, 4, C.byref(n)) == -22 and b"capacity=4" in lib.cf_last_error()
    assert lib.cf_optim_plan(recs, 4, chunks, 5, C.byref(n)) == 0
    assert [(c.tensor, c.offset) for c in chunks] == [(0, 0), (2, 0), (2, ch), (2, 2 * ch), (3, 0)]


def test_optim_struct_layouts_match_c(tmp_path):
    import subprocess
    from centerfusiondetect3d_amd import _lib
    root = os.path.dirname(HERE)
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cf_hip.h"\nint main(){'
                    'printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(cf_optim_tensor), offsetof(cf_optim_tensor, numel),'
                    'offsetof(cf_optim_tensor, step_base), sizeof(cf_optim_chunk), offsetof(cf_optim_chunk, tensor),'
                    'sizeof(cf_optim_args), offsetof(cf_optim_args, lr), offsetof(cf_optim_args, decay),'
                    'offsetof(cf_optim_args, step), CF_OPTIM_CHUNK);return 0;}')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_lib.OptimTensor), _lib.OptimTensor.numel.offset, _lib.OptimTensor.step_base.offset,
                   C.sizeof(_lib.OptimChunk), _lib.OptimChunk.tensor.offset, C.sizeof(_lib.OptimArgs), _lib.OptimArgs.lr.offset,
                   _lib.OptimArgs.decay.offset, _lib.OptimArgs.step.offset, _lib.CF_OPTIM_CHUNK]


class _Small(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 4, 3)
        self.bn = torch.nn.BatchNorm2d(4)


def test_save_model_load_model_round_trip(tmp_path):
    from centerfusiondetect3d_amd import CfgNode, loadModel, saveModel
    torch.manual_seed(3)
    m = _Small()
    with torch.no_grad():
        m.bn.running_mean.copy_(torch.randn(4))
    path = str(tmp_path / "model_7.pth")
    log = {"note": "kept"}
    saveModel(log, m, 7, path)
    assert set(log) == {"note", "state_dict", "epoch"} and log["epoch"] == 7
    raw = torch.load(path, map_location="cpu")
    assert set(raw) == {"note", "state_dict", "epoch"} and raw["note"] == "kept" and raw["epoch"] == 7
    assert list(raw["state_dict"]) == list(m.state_dict())
    cfg = CfgNode(MODEL=CfgNode(LOAD_DIR=path), TRAIN=CfgNode(RESUME=True))
    ckpt, m2, start = loadModel(_Small(), cfg)
    assert start == 8 and ckpt["epoch"] == 7
    for k, v in m.state_dict().items():
        assert torch.equal(m2.state_dict()[k], v), k
    cfg.TRAIN.RESUME = False
    assert loadModel(_Small(), cfg)[2] == 1
    # behind a DataParallel wrapper the keys are the module's own
    saveModel({}, torch.nn.DataParallel(m), 2, path)
    assert list(torch.load(path, map_location="cpu")["state_dict"]) == list(m.state_dict())
