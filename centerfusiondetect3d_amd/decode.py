"""Drop-in for the reference's model/decode.py:10-174 (`fusionDecode`) on the HIP path.

NMS + top-k run in one kernel over the NCHW heat map (cf_topk_peaks with nms=1) and the ten
per-head gathers + box arithmetic in a second one (cf_decode_gather; with an `uncertainty` head in the outputs
cf_decode_gather_unc, which also weights the scores: decode.py:80-85) that reads the K peak pixels
straight from the NCHW maps - the reference's ten full-map permute().contiguous() copies
(model/utils.py:69-71) do not exist here.  Order among equal scores: (class asc, pixel asc).
"""
import torch

from . import ops
from .pending import PendingOutputs

# column layout of the (B,K,33) detection tensor (== SURVEY.md §8(e) all-gather payload)
DET_FIELDS = [("scores", 1), ("classIds", 1), ("centers", 2), ("bboxes", 4), ("rotation", 8),
              ("dimension", 3), ("amodal_offset", 2), ("nuscenes_att", 8), ("velocity", 3),
              ("depth", 1)]
DET_WIDTH = sum(n for _, n in DET_FIELDS)


def _peaks_and_maps(outputs, K):
    assert isinstance(outputs, list), "output must be a list of dictionaries"
    if len(outputs) != 1:
        raise NotImplementedError("the DLA-34 model yields one output layer; multi-layer decode is not on the path")
    out = outputs[0]
    if "heatmap" not in out:
        return None
    # A forward with model.heads_at_peaks hands out a PendingOutputs: every map but the heat map holds values at that forward's
    # peaks only until someone reads it.  The decoder needs nothing else - provided it decodes exactly those peaks: the same K,
    # and the heat map tensor the forward attached them to (nobody else can hold that tensor: reading it materialises).  It then
    # reads through `peek`; in every other case the maps are materialised first.
    get = out.get
    if isinstance(out, PendingOutputs):
        heat = out.peek("heatmap")
        cached = getattr(heat, "_cf_peaks", None)
        if out.pending and not (cached is not None and cached[0] == K and cached[1] == heat.data_ptr() and heat.is_contiguous()
                                and not torch.cuda.is_current_stream_capturing()):
            out.materialise()
        get = out.peek
    heat = get("heatmap")
    _, _, H, W = heat.shape
    # The forward may have computed exactly these peaks already, beside its own launches (plan._Plan.run: the heat map tensor
    # carries them with a checksum of the bits they were computed from).  They are used only for the very tensor object, and
    # only while its contents still have that checksum: the map is summed again here and the guard launch that follows
    # compares the two sets of partial sums ON THE DEVICE - equal: it returns at once and the carried peaks stand; different (an
    # in-place write, also one through `heat.data`, which bumps no version counter): it recomputes them into the same buffers.
    # The reference's fusionDecode always reads the map it is given (model/decode.py:38-57); so does this, in two short launches
    # instead of the three of the NMS + top-k.
    cached = getattr(heat, "_cf_peaks", None)
    if cached is not None and cached[0] == K and cached[1] == heat.data_ptr() and heat.is_contiguous() \
            and not torch.cuda.is_current_stream_capturing():
        pk_s, pk_i, pk_c, sums = cached[2:]
        ops.checksum64(heat, out=sums[ops.CHECKSUM_PARTS:])
        scores, inds, classes = ops.topk_peaks(heat, K, nms=True, out=(pk_s, pk_i, pk_c), only_if_changed=sums)
    else:
        scores, inds, classes = ops.topk_peaks(heat, K, nms=True)
    depth = get("depth2", get("depth"))
    if "rotation2" in out:
        if isinstance(out, PendingOutputs):
            out.rename("rotation2", "rotation")
        else:
            out["rotation"] = out.pop("rotation2")
    maps = {"reg": get("reg"), "wh": get("widthHeight"), "depth": depth,
            "rot": get("rotation"), "dim": get("dimension"),
            "amodal": get("amodal_offset"), "att": get("nuscenes_att"),
            "vel": get("velocity")}
    present = ["scores", "classIds", "centers"]
    for name, key in (("bboxes", "wh"), ("rotation", "rot"), ("dimension", "dim"),
                      ("amodal_offset", "amodal"), ("nuscenes_att", "att"), ("velocity", "vel"),
                      ("depth", "depth")):
        if maps[key] is not None:
            present.append(name)
    # `uncertainty` (TRAIN.UNCERTAINTY_LOSS): the gather launch multiplies the score it WRITES by exp(-exp(u)) at the peak
    # (model/decode.py:80-85).  `scores` may be the buffer the forward attached to the heat map, shared by every later decode
    # of that tensor, so it is only ever read: a second decode weights the same raw scores again.
    return scores, inds, classes, maps, H, W, present, get("uncertainty")


def decode_packed(outputs, outputSize=(112, 200), K=100, norm2d=False):
    """-> (det (B,K,33) f32, present-field names).  Same side effect on `outputs` as the reference:
    `rotation2` is renamed to `rotation` in the caller's dict (decode.py:120-121)."""
    r = _peaks_and_maps(outputs, K)
    if r is None:
        return None, []
    scores, inds, classes, maps, H, W, present, unc = r
    det = ops.decode_gather(scores, inds, classes, maps, H, W, outputSize, norm2d, uncertainty=unc)
    return det, present


def decode_post_packed(outputs, calibs, trans_inv, outputSize=(112, 200), K=100, norm2d=False, want_det=False):
    """fusionDecode + postProcess in one gather launch (cf_decode_post) -> post (B,K,54) [, det (B,K,33)]:
    the rows `postprocess.unpack_post` names - what Detector.post_process / the evaluation loop hand on
    (detector.py:343-349, model/progressBar.py:95-110) and what the multi-GPU all-gather ships.
    trans_inv: (2,3) f32 device tensor from postprocess.inverse_affine.  Needs the full 3D head set."""
    r = _peaks_and_maps(outputs, K)
    if r is None:
        raise ValueError("decode_post_packed: outputs hold no heatmap")
    scores, inds, classes, maps, H, W, present, unc = r
    if any(v is None for v in maps.values()):
        raise NotImplementedError("decode_post_packed needs the full 3D detection head set")
    B = scores.shape[0]
    return ops.decode_post(scores, inds, classes, maps, H, W, outputSize,
                           calibs.reshape(B, 3, 4).float().contiguous(), trans_inv, norm2d, want_det, uncertainty=unc)


def unpack_detections(det, present=None):
    """(B,K,33) -> dict of tensors shaped like the reference's return value."""
    ret, col = {}, 0
    for name, n in DET_FIELDS:
        if present is None or name in present:
            v = det[..., col:col + n]
            ret[name] = v[..., 0] if name in ("scores", "classIds") else v
        col += n
    return ret


def fusionDecode(outputs, outputSize=(112, 200), K=100, norm2d=False):
    det, present = decode_packed(outputs, outputSize, K, norm2d)
    if det is None:
        return {}
    return unpack_detections(det, present)
