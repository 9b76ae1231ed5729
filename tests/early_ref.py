"""CPU forward of the EARLY radar fusion model for the tests, composed from oracle.model_ref's building blocks (which work on any
input width): base_model.py:69-79 (in-place normalisation of the caller's map), fusionModules.py:18-35 (nearest upsample + concat),
then img2feats and the nine image-only heads (detectHeads.py:32-132).  Held to the reference-generated fixture by
tests/test_early_cpu.py."""
import torch
import torch.nn.functional as F

from oracle import model_ref

HEADS = ["heatmap", "reg", "widthHeight", "depth", "rotation", "dimension", "amodal_offset", "nuscenes_att", "velocity"]
N_LAYERS = {h: (3 if h in ("nuscenes_att", "velocity") else 1) for h in HEADS}      # hidden layers in front of the output layer


def normalise_(pc_dep, max_pc_dist=60.0):
    """base_model.py:77-78, on the caller's tensor."""
    pc_dep[:, :1] /= max_pc_dist
    pc_dep[:, :1] = 1 - pc_dep[:, :1]
    return pc_dep


def combine(x, pc_hm):
    """ConcateCombiner: channels 0-2 the image, 3-5 the radar map at the image size."""
    return torch.cat([x, F.interpolate(pc_hm.to(x.dtype), size=x.shape[-2:], mode="nearest")], dim=1)


def stem(sd, x6):
    """base_layer + level0 + level1 of dla34_base (dla.py:250-262) on the six-channel image -> the level1 map."""
    t = x6
    for name, stride, pad in (("base_layer", 1, 3), ("level0", 1, 1), ("level1", 2, 1)):
        t = F.relu(model_ref._bn(sd, f"base.{name}.1", F.conv2d(t, sd[f"base.{name}.0.weight"], None, stride, pad)))
    return t


def forward(sd, x, pc_dep, calib=None, max_pc_dist=60.0, normalise=True, hp="detectHead_0", want_feat=False):
    """model(x, pc_dep=, calib=) of the early model in eval mode -> [dict].  normalise=False: pc_dep already is the normalised map
    (a float64 evaluation shares the fp32 run's map)."""
    pc_hm = normalise_(pc_dep, max_pc_dist) if normalise else pc_dep
    feat = model_ref.img2feats(sd, combine(x, pc_hm))
    y = {h: model_ref._head(sd, f"{hp}.{h}", feat, N_LAYERS[h]) for h in HEADS}
    y["heatmap"] = torch.clamp(torch.sigmoid(y["heatmap"]), min=1e-4, max=1 - 1e-4)
    y["depthMap"] = y["depth"]
    y["depth"] = model_ref.sigmoid_depth(y["depth"])
    y["calib"] = calib
    return ([y], feat) if want_feat else [y]
