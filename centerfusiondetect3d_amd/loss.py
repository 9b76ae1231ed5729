"""The reference's criterion, `GenericLoss` (model/genericLoss.py + model/losses.py), on the device: two launches
forward, two backward, no host sync (ops.generic_loss, csrc/cf_loss.hip).

    crit = GenericLoss(config, num_classes)            # the reference's constructor
    total, losses = crit(outputs, batch)               # outputs: [ {head: (B,C,h,w)} ], batch: the reference's dict
    total.backward()

What differs from the reference, on purpose:
  * `losses[...]` are detached 0-d views into one device vector (the reference only ever logs `.mean().item()` of them);
    `total` alone carries the grad_fn.
  * An object centre outside the map is clamped to the nearest valid pixel index (the reference raises in its gather).
  * Device fp32 maps only; bbox2d / bbox3d / lidar_depth / radar_depth weights above 0, DATASET.DECOUPLE_REP and more than
    one output layer raise NotImplementedError.
"""
import torch

from . import _lib, ops
from .config import update_loss_weights

_L1_HEADS = ("reg", "widthHeight", "dimension", "amodal_offset", "velocity")
_UNUSED_WEIGHTS = ("bbox2d", "bbox3d", "lidar_depth", "radar_depth")


def _get(node, name, default=None):
    try:
        return node[name] if isinstance(node, dict) else getattr(node, name)
    except (KeyError, AttributeError):
        return default


class GenericLoss(torch.nn.Module):
    def __init__(self, config, num_classes):
        super().__init__()
        if _get(config, "weights") is None:
            update_loss_weights(config)
        self.config = config
        self.num_classes = num_classes
        weights = config.weights
        for name in _UNUSED_WEIGHTS:
            if float(_get(weights, name, 0.0) or 0.0) > 0:
                raise NotImplementedError(f"GenericLoss on the HIP path: weights.{name} > 0 is not implemented")
        lw = _get(config, "LOSS_WEIGHTS")
        for name in ("LIDAR_DEPTH", "RADAR_DEPTH"):
            if lw is not None and float(_get(lw, name, 0.0) or 0.0) > 0:
                raise NotImplementedError(f"GenericLoss on the HIP path: LOSS_WEIGHTS.{name} > 0 is not implemented")
        if _get(config.DATASET, "DECOUPLE_REP", False):
            raise NotImplementedError("GenericLoss on the HIP path: DATASET.DECOUPLE_REP is not implemented")

    def forward(self, outputs, batch):
        if len(outputs) != 1:
            raise NotImplementedError("GenericLoss on the HIP path: one output layer only")
        output = outputs[0]
        weights = self.config.weights
        heat = output["heatmap"]
        if not torch.is_tensor(heat) or heat.dim() != 4:
            raise _lib.CfHipError("GenericLoss: outputs[0]['heatmap'] must be a (B,C,h,w) tensor")
        out_h, out_w = (int(v) for v in self.config.MODEL.OUTPUT_SIZE)
        if tuple(heat.shape[-2:]) != (out_h, out_w):
            raise NotImplementedError(f"GenericLoss on the HIP path: the maps must be MODEL.OUTPUT_SIZE = {(out_h, out_w)}, "
                                      f"got {tuple(heat.shape[-2:])} (a scaled output layer)")
        if not any(f"depth{i if i > 1 else ''}" in output for i in range(1, 6)):
            raise ValueError("No depth head found in output")

        # the head table, in the order the reference adds its terms to the total (genericLoss.py:110-261)
        unc = output["uncertainty"] if self.training and "uncertainty" in output else None
        table, names = [], []
        for name in ("depth", "depth2"):
            if name in output:
                table.append((ops.LOSS_L1 if unc is None else ops.LOSS_L1_UNC, output[name], batch["depth"], None, weights["depth"]))
                names.append(name)
        for name in _L1_HEADS:
            if name in output:
                table.append((ops.LOSS_L1, output[name], batch[name], None, weights[name]))
                names.append(name)
        for name in ("rotation", "rotation2"):
            if name in output:
                table.append((ops.LOSS_BINROT, output[name], batch["rotres"], batch["rotbin"], weights[name]))
                names.append(name)
        if "nuscenes_att" in output:
            table.append((ops.LOSS_BCE, output["nuscenes_att"], batch["nuscenes_att"], batch["nuscenes_att_mask"],
                          weights["nuscenes_att"]))
            names.append("nuscenes_att")

        total, vec, layer_mask = ops.generic_loss(heat, batch["heatmap0"], batch["target"]["heatCenters"], batch["widthHeight"],
                                                  batch["mask"], batch["classIds"], table, heat_weight=weights["heatmap"],
                                                  out_area=out_h * out_w, uncertainty=unc)
        batch["layerMask"] = layer_mask[:, None]                   # (B, 1, M) bool, as build_targets leaves it
        slot = {"heatmap": 0, "total": len(names) + 1}
        slot.update({name: 1 + i for i, name in enumerate(names)})
        zero = len(names) + 2                                       # heads the config names but the output lacks, `uncertainty`
        keys = list(self.config.heads) + ["total"] + [n for n in ("depth", "depth2") if n in output and n not in self.config.heads]
        losses = {k: vec[slot.get(k, zero)] for k in keys}
        return total, losses
