"""One training step of the reference's run (model/modelWithLoss.py: `training_step`, `configure_optimizers`,
`on_train_epoch_start`) on this package's own parts, from the batch to the updated weights:

    ts = TrainStep(model, config, num_classes)
    for epoch in range(ts.start_epoch, config.TRAIN.EPOCHS + 1):
        ts.epoch_start(epoch)                  # the defreeze
        for batch in loader:                   # image, pc_hm, pc_dep, calib + the targets of build_targets
            loss, stats = ts.step(batch)
        ts.epoch_end(epoch)                    # the LR schedule

`step` issues zero_grad, the model's training forward, `GenericLoss`, backward and the fused optimizer launch on the current
stream and never waits for the device: `loss` and `stats` are device scalars.  `epoch_start` applies the reference's defreeze
rule (modelWithLoss.py:275-283) - with MODEL.FREEZE_BACKBONE, MODEL.DEFREEZE != -1 and epoch > DEFREEZE every parameter starts
to learn - through `model.unfreeze_stem()`, this model's form of "every requires_grad True"; the optimizer holds all parameters
from the start (as the reference's does) and the late ones join it with a step count of their own.
"""
import torch

from .loss import GenericLoss
from .optim import _setting, configure_optimizers


class TrainStep:
    def __init__(self, model, config, num_classes, start_epoch=1, fused=True):
        self.model = model
        self.config = config
        self.start_epoch = int(start_epoch)
        self.criterion = GenericLoss(config, num_classes).train()
        self.optimizer, self.scheduler = configure_optimizers(model, config, start_epoch=self.start_epoch, fused=fused)
        self.defreeze = int(_setting(config, "MODEL", "DEFREEZE"))
        self.defrozen = self.defreeze == -1

    def epoch_start(self, epoch):
        """on_train_epoch_start: past MODEL.DEFREEZE a frozen-backbone model learns with every parameter, once. -> whether this
        call did the defreeze"""
        model_cfg = getattr(self.config, "MODEL", None)
        if not self.defrozen and bool(getattr(model_cfg, "FREEZE_BACKBONE", False)) and epoch > self.defreeze:
            self.model.unfreeze_stem()
            self.defrozen = True
            return True
        return False

    def step(self, batch):
        """-> (loss, stats): the criterion's total (detached) and its per-head values, all on the device"""
        self.model.train()
        self.optimizer.zero_grad()
        outputs = self.model(batch["image"], pc_hm=batch.get("pc_hm"), pc_dep=batch.get("pc_dep"), calib=batch.get("calib"))
        loss, stats = self.criterion(outputs, batch)
        loss.backward()
        self.optimizer.step()
        return loss.detach(), stats

    def epoch_end(self, epoch):
        """Lightning steps the reference's scheduler once per epoch. -> the LR of the next epoch (group 0)"""
        self.scheduler.step()
        return self.optimizer.param_groups[0]["lr"]
