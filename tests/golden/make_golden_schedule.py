"""DEV-ONLY: the learning-rate schedules of the reference's own `ModelWithLoss.configure_optimizers` (model/modelWithLoss.py),
recorded epoch by epoch.  Import recipe: make_golden.py (imported, not copied), plus `lightning.LightningModule = torch.nn.Module`
and an inert `utils.logger`; the function is called unbound on a namespace that carries what it reads (config, model, lr,
start_epoch).  Nothing of the reference is committed: the fixture holds names and numbers.

Per case `<name>`: `<name>.case` (optimizer, scheduler, LR_STEP, WARM_EPOCHS, DEFREEZE, EPOCHS, start_epoch as a JSON string),
`<name>.optimizer` (class name), `<name>.lr` and `<name>.weight_decay` (the optimizer's defaults), `<name>.momentum` (SGD, else NaN)
and `<name>.lrs`: the LR of group 0 before the first epoch, then after every `scheduler.step()` up to EPOCHS (float64, EPOCHS + 1
values).  Only configurations the reference runs are recorded; one that raises stops the script.

    python tests/golden/make_golden_schedule.py
"""
import json
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

FIXTURE = "lr_schedules.npz"
LR = 2.5e-4
# (name, TRAIN.OPTIMIZER, TRAIN.LR_SCHEDULER, TRAIN.LR_STEP, TRAIN.WARM_EPOCHS, MODEL.DEFREEZE, TRAIN.EPOCHS, start_epoch)
CASES = [
    ("adam_step", "adam", "StepLR", (50,), 5, -1, 60, 1),
    ("sgd_step_nowarm", "sgd", "StepLR", (50,), 0, -1, 60, 1),
    ("adam_step_defreeze", "adam", "StepLR", (10, 50), 5, 20, 60, 1),
    ("adam_step_resume30", "adam", "StepLR", (50,), 5, -1, 60, 30),
    ("adam_step_resume55", "adam", "StepLR", (50,), 5, -1, 60, 55),
    ("adam_clr_defreeze", "adam", "CLR", (90, 170, 210), 5, 100, 230, 1),
    ("adam_clr", "adam", "CLR", (50,), 5, -1, 60, 1),
]
OPTIONAL = [("sgd_clr_defreeze", "sgd", "CLR", (90, 170, 210), 5, 100, 230, 1)]      # kept only if the reference runs it


def case_config(opt, sched, lr_step, warm, defreeze, epochs):
    from types import SimpleNamespace as NS
    return NS(TRAIN=NS(OPTIMIZER=opt, LR=LR, LR_STEP=tuple(lr_step), WARM_EPOCHS=warm, EPOCHS=epochs, LR_SCHEDULER=sched),
              MODEL=NS(DEFREEZE=defreeze))


def run_reference(ModelWithLoss, case):
    _, opt, sched, lr_step, warm, defreeze, epochs, start = case
    cfg = case_config(opt, sched, lr_step, warm, defreeze, epochs)
    me = types.SimpleNamespace(config=cfg, model=torch.nn.Linear(1, 1), lr=cfg.TRAIN.LR, start_epoch=start)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                 # (scheduler.step() before optimizer.step(): no training happens here)
        out = ModelWithLoss.configure_optimizers(me)
        optimizer, scheduler = out["optimizer"], out["lr_scheduler"]["scheduler"]
        lrs = [optimizer.param_groups[0]["lr"]]
        for _ in range(epochs):
            scheduler.step()
            lrs.append(optimizer.param_groups[0]["lr"])
    d = optimizer.defaults
    return dict(optimizer=type(optimizer).__name__, lr=float(d["lr"]), weight_decay=float(d["weight_decay"]),
                momentum=float(d.get("momentum", float("nan"))), lrs=np.asarray([float(v) for v in lrs], np.float64))


def main():
    from tests.golden import make_golden as mg
    mg._install_inert_modules()
    sys.modules["lightning"].LightningModule = torch.nn.Module
    sys.path[:0] = [mg.REF, os.path.join(mg.REF, "lib")]
    import utils                                        # noqa: F401  (the reference's package; its logger needs wandb)
    logger = types.ModuleType("utils.logger")
    logger.WandbLogger = type("WandbLogger", (), {})
    sys.modules["utils.logger"] = logger
    try:
        import tqdm                                     # noqa: F401
    except ImportError:
        sys.modules["tqdm"] = types.SimpleNamespace(tqdm=object)
    from model.modelWithLoss import ModelWithLoss

    arrays, names = {}, []
    for case in CASES + OPTIONAL:
        try:
            rec = run_reference(ModelWithLoss, case)
        except Exception as e:                          # noqa: BLE001
            if case in OPTIONAL:
                print(f"  {case[0]:22s} the reference does not run it ({type(e).__name__}: {e}): not recorded")
                continue
            raise
        name = case[0]
        names.append(name)
        arrays[f"{name}.case"] = np.array(json.dumps(dict(optimizer=case[1], scheduler=case[2], lr_step=list(case[3]), warm_epochs=case[4],
                                                          defreeze=case[5], epochs=case[6], start_epoch=case[7], lr=LR)))
        arrays[f"{name}.optimizer"] = np.array(rec["optimizer"])
        for k in ("lr", "weight_decay", "momentum"):
            arrays[f"{name}.{k}"] = np.array(rec[k], np.float64)
        arrays[f"{name}.lrs"] = rec["lrs"]
        lrs = rec["lrs"]
        print(f"  {name:22s} {rec['optimizer']:6s} lr {rec['lr']:.3e} wd {rec['weight_decay']:g}  "
              f"lrs[0..6] {' '.join(f'{v:.3e}' for v in lrs[:7])} ... last {lrs[-1]:.3e}  ({len(lrs)} values)")
        assert len(lrs) == case[6] + 1 and np.isfinite(lrs).all() and (lrs > 0).all()
    arrays["names"] = np.array(names)
    mg.save(FIXTURE, **arrays)


if __name__ == "__main__":
    main()
