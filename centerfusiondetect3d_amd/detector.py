"""`Detector`: the reference's inference driver (src/lib/detector.py:21-113, 189-349, 397-470) on the HIP
path, end to end on the device:

    uint8 camera frames + raw radar sweeps
      -> preProcessImages        (cf_preprocess_images:   detector.py:206-234)
      -> radar_to_pc_dep         (cf_radar_ingest + cf_pillar_expand | cf_radar_roi_expand, by DATASET.PC_ROI_METHOD:  detector.py:257-292)
      -> model(images, pc_dep=, calib=)                   (detector.py:423)
      -> fusionDecode + postProcess in one gather launch  (cf_decode_post: detector.py:343-349, 397-426)
      -> merge_outputs                                    (detector.py:428-470)

Only the raw bytes (frames, sweeps, calibration) cross PCIe; nothing is warped, projected, sorted,
decoded or unprojected on the host.  Visualisation, file loading by path (cv2.imread) and the debug
windows of the reference are outside the hot path."""
import os

import numpy as np
import torch

from . import _lib, ops
from .decode import decode_post_packed
from .checkpoint import loadModel
from .model import getModel
from .pointcloud import getAffineTransform, radar_to_pc_dep
from .postprocess import inverse_affine, unpack_post
from .preprocess import NUSCENES_MEAN, NUSCENES_STD, preProcessImages

FOCAL_LENGTH = 1200          # datasets/nuscenes.py:34 (used when an image has no calibration)


class Detector(object):
    def __init__(self, config, show=False, pause=False, *, model=None, device=None, range_policy="raise", range_check_every=0):
        """detector.py:21-42: `Detector(config, show=False, pause=False)` builds the model with `getModel(config)`
        and, when `config.MODEL.LOAD_DIR` is set (the reference's radar configs set it,
        configs/Centerfusion_Middle.yaml:43), loads that checkpoint with `loadModel` before `.to(device).eval()`.
        A checkpoint that cannot be read raises, as `torch.load` does in the reference: nothing here falls back to
        random weights.  `model=` / `device=` (keyword only, extensions) hand over an already-built module or pick the
        card.  Visualisation is outside the hot path: `show=True` raises instead of being ignored.

        `range_policy` (keyword only, extension): the split-fp16 kernels clamp activations beyond 65504 / pre-scale (4094 at
        the default pre-scale 16) where the reference's fp32 convolutions accept any magnitude (dla.py:124-159), so the FIRST
        batch after the weights were loaded goes through the model's range guard: "raise" (default) = `model.check_ranges` -
        a `CfHipError` naming the layers if any input reaches half that limit, never a silently clamped map; "calibrate" =
        `model.calibrate` on that batch (per-layer power-of-two pre-scales; results unchanged bit for bit where no layer
        needs one); "off" = no check.  `range_check_every = N > 0` (with a policy other than "off"): every N-th batch the buffers
        that batch's forward left in HBM are re-tested as well (`model.check_resident_ranges()`: one reduction per buffer and a
        device -> host copy, ~2 ms at bs=16, no second forward; raises like the first-batch guard) - for a service whose inputs
        may drift away from the batch it was checked or calibrated on."""
        if range_policy not in ("raise", "calibrate", "off"):
            raise ValueError("range_policy must be 'raise', 'calibrate' or 'off'")
        self.range_policy = range_policy
        self.range_check_every = max(0, int(range_check_every))
        self._batches = 0
        if not isinstance(show, bool) or not isinstance(pause, bool):
            raise TypeError("Detector(config, show=False, pause=False, *, model=None, device=None): "
                            "show / pause are booleans; pass a pre-built module as model=")
        if show:
            raise NotImplementedError("Detector(show=True): the reference's debug windows (detector.py:115-187) are "
                                      "outside the HIP hot path")
        if model is None and config.MODEL.LOAD_DIR != "" and not os.path.isfile(config.MODEL.LOAD_DIR):
            raise FileNotFoundError(f"config.MODEL.LOAD_DIR = {config.MODEL.LOAD_DIR!r}: no such checkpoint "
                                    "(detector.py:30-31 loads it; it is never replaced by random weights)")
        if not torch.cuda.is_available():
            raise _lib.CfHipError("Detector runs on the GPU: the HIP path has no CPU fallback")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.config = config
        if model is None:
            model = getModel(config)
            if config.MODEL.LOAD_DIR != "":
                _, model, _ = loadModel(model, config)
        self.model = model.to(self.device).eval()
        self.mean, self.std = NUSCENES_MEAN, NUSCENES_STD
        self.pause = pause
        self.show = show
        self.visualization = show
        self._tinv = {}

    # ------------------------------------------------------------------------------ pre_process
    def pre_process(self, imageOrigins, img_infos, radar_pcs):
        """-> images (B,3,inH,inW), pc_deps (B,3,outH,outW) or None, metas, calibs (B,3,4); all on the device."""
        frames = imageOrigins if isinstance(imageOrigins, (list, tuple)) else [f for f in imageOrigins]
        height, width = int(frames[0].shape[0]), int(frames[0].shape[1])
        inH, inW = self.config.MODEL.INPUT_SIZE
        outH, outW = self.config.MODEL.OUTPUT_SIZE
        center = np.array([width / 2.0, height / 2.0], dtype=np.float32)
        scale = max(height, width) * 1.0
        transMatInput = getAffineTransform(center, scale, 0, [inW, inH])
        transMatOutput = getAffineTransform(center, scale, 0, [outW, outH])
        images = preProcessImages(imageOrigins, (inH, inW), self.mean, self.std, transMat=transMatInput,
                                  device=self.device)
        calibs, metas = [], []
        for info in img_infos:
            if info is not None and "calib" in info:
                calib = np.array(info["calib"], dtype=np.float32)
            else:
                calib = np.array([[FOCAL_LENGTH, 0, center[0], 0], [0, FOCAL_LENGTH, center[1], 0], [0, 0, 1, 0]],
                                 dtype=np.float32)
            calibs.append(calib)
            metas.append({"calib": calib, "center": center, "scale": scale, "height": height, "width": width,
                          "outputHeight": outH, "outputWidth": outW, "inputHeight": inH, "inputWidth": inW,
                          "transMatInput": transMatInput, "transMatOutput": transMatOutput})
        pc_deps = None
        if self.config.DATASET.RADAR_PC and radar_pcs is not None:
            K3 = np.stack([np.asarray(i["camera_intrinsic"], np.float64).reshape(3, 3) for i in img_infos])
            wh = {(int(i["width"]), int(i["height"])) for i in img_infos}
            if len(wh) != 1:
                raise ValueError("all frames of a batch must share one image size")
            pc_deps = radar_to_pc_dep(radar_pcs, K3, wh.pop(), np.stack([np.asarray(i["calib"], np.float64)
                                                                          for i in img_infos]),
                                      transMatOutput, (outH, outW), max_dist=float(self.config.DATASET.MAX_PC_DIST),
                                      z_offset=float(self.config.DATASET.PC_Z_OFFSET),
                                      pillar_dims=tuple(self.config.DATASET.PILLAR_DIMS), device=self.device,
                                      roi_method=getattr(self.config.DATASET, "PC_ROI_METHOD", "pillars"))
        calibs = torch.from_numpy(np.stack(calibs, axis=0)).to(self.device)
        return images, pc_deps, metas, calibs

    # ---------------------------------------------------------------------------------- process
    @torch.no_grad()
    def process(self, images, calibs, pc_dep=None, meta=None, mark=None):
        """forward + decode + postProcess -> (outputs, post (B,K,54)).  `mark(name)`: stage-boundary callback (`run` with
        `stage_times`)."""
        if self.range_policy != "off" and getattr(self.model, "_range_checked", True) is False:
            # first batch on these weights: the range guard (one slow exact-fp32 forward; sets model._range_checked)
            (self.model.calibrate if self.range_policy == "calibrate" else self.model.check_ranges)(images, pc_dep, calibs)
        outputs = self.model(images, pc_dep=pc_dep, calib=calibs)
        self._batches += 1
        if self.range_policy != "off" and self.range_check_every and self._batches % self.range_check_every == 0:
            self.model.check_resident_ranges()
        if mark is not None:
            mark("net")
        outH, outW = self.config.MODEL.OUTPUT_SIZE
        key = (float(meta["center"][0]), float(meta["center"][1]), float(meta["scale"]), outH, outW)
        tinv = self._tinv.get(key)
        if tinv is None:
            tinv = self._tinv[key] = torch.from_numpy(
                inverse_affine(meta["center"], meta["scale"], (outW, outH))).to(self.device)
        post = decode_post_packed(outputs, calibs, tinv, outputSize=(outH, outW), K=int(self.config.MODEL.K),
                                  norm2d=bool(self.config.MODEL.NORM_2D))
        return outputs, post

    @staticmethod
    def merge_outputs(detects):
        """detector.py:428-470 on host copies of the post-processed fields."""
        keep = (detects["scores"] > -1) & torch.all(detects["dimension"] > 0, dim=2)
        B = detects["scores"].shape[0]
        boxes = [[] for _ in range(B)]
        for b in range(B):
            for j in torch.nonzero(keep[b]).flatten().tolist():
                boxes[b].append({"class": detects["classIds"][b, j], "score": detects["scores"][b, j],
                                 "dimension": detects["dimension"][b, j], "location": detects["locations"][b, j],
                                 "yaw": detects["yaws"][b, j], "bboxes": detects["bboxes"][b, j],
                                 "bboxes3d": detects["bboxes3d"][b, j],
                                 "nuscenes_att": detects["nuscenes_att"][b, j],
                                 "velocity": detects["velocity"][b, j]})
        return boxes

    # -------------------------------------------------------------------------------------- run
    @staticmethod
    def _as_batch(imgInput, img_info, radar_pc):
        if isinstance(imgInput, np.ndarray) and imgInput.ndim == 3:
            imgInput = [imgInput]
        if not isinstance(img_info, (list, tuple)):
            img_info = [img_info]
            radar_pc = [radar_pc] if radar_pc is not None else None
        return imgInput, img_info, radar_pc

    # ------------------------------------------------------------------------------- depth maps
    def _depth_maps_device(self, outputs):
        """-> (keys, (len(keys),B,H,W) uint8 device tensor): one launch (cf_depth_maps), nothing copied yet."""
        if len(outputs) != 1:
            raise NotImplementedError("the DLA-34 model yields one output layer; multi-layer depth maps are not on the path")
        out = outputs[0]
        keys = ["depth"] + [k for k in ("pc_hm_out", "pc_hm_in", "pc_hm_mid") if k in out]
        maps = [out["depthMap"] if "depthMap" in out else out["depth2"] if "depth2" in out else out["depth"]]
        maps += [out[k] for k in keys[1:]]
        outH, outW = self.config.MODEL.OUTPUT_SIZE
        for k, t in zip(keys, maps):
            if t.dim() != 4 or t.shape[1] != 1 or tuple(t.shape[2:]) != (outH, outW):
                raise ValueError(f"depth_maps: {k} has shape {tuple(t.shape)}, expected (B, 1, {outH}, {outW}) - the "
                                 "reference's interpolate to MODEL.OUTPUT_SIZE is the identity on this path")
        return keys, ops.depth_maps(maps)

    def depth_maps(self, outputs):
        """The `depthmaps` of the reference's `Detector.post_process` (detector.py:351-393): {"depth" (from `depthMap`, else
        `depth2`, else `depth`), "pc_hm_out", "pc_hm_in" when the model has them} -> (B,H,W) uint8 HOST arrays, each image
        scaled to its own min .. max.  Min / max, normalisation and the cast run on the device in one launch; only the
        uint8 maps (a quarter of one fp32 map's bytes each) cross PCIe.  Row 0 and column 0 of image 0 - only image 0 -
        count as 0, as in the reference; an image whose map is flat (no radar return: an all-zero `pc_hm_in`) is 0 / 0
        there and all zeros here."""
        with torch.cuda.device(self.device):
            keys, dm = self._depth_maps_device(outputs)
        return self._fetch_depth_maps(keys, dm)

    @staticmethod
    def _fetch_depth_maps(keys, dm):
        host = dm.cpu().numpy()
        return {k: host[i] for i, k in enumerate(keys)}

    def _finish(self, outputs, post, metas, img_infos, merge, dm=None):
        ret = {"outputs": outputs, "post": post, "metas": metas, "img_infos": img_infos}
        if dm is not None:
            ret["depthmaps"] = self._fetch_depth_maps(*dm)
        if merge:
            detects = {k: v.cpu() for k, v in unpack_post(post).items()}
            ret["detects"] = detects
            ret["predictBoxes"] = self.merge_outputs(detects)
        return ret

    def run_pipelined(self, batches, merge=True, depthmaps=False):
        """Generator over `batches` of (imgInput, img_info, radar_pc) - the arguments of `run` - yielding, in order and
        bit for bit, what `run` returns for each.  Software pipeline of depth two:
          * batch i+1's frames cross PCIe and are warped / ingested / pillar-expanded (`pre_process`) on a FEED stream
            while batch i goes through the model on the caller's stream - the host -> device copy (4.3 MB per
            1600x900 frame, 1.4 ms per 16 frames) leaves the critical path;
          * the results of batch i-1 are fetched (`.cpu()`, `merge_outputs`) after batch i's launches are queued, so the
            device never waits for the host.
        `depthmaps=True`: as in `run`; the launch is queued behind batch i's decode and the uint8 maps are fetched with the
        detections of that batch, one batch later.
        The reference gets the same overlap from its DataLoader workers + pinned memory (trainer.py, dataset/); frames
        should sit in pinned host memory for the copy to be asynchronous.  An extension: not in the reference's API."""
        from .streams import _side_streams
        it = iter(batches)

        def feed_stream(main):
            # one stream past the model's own side streams, probed (streams._pick_streams) to run beside them AND beside
            # `main`, where the heads and the decode are
            n = max(int(getattr(self.model, "streams", 2)), 2) + 1
            return _side_streams(self.device, main.cuda_stream, n)[n - 1]

        def stage(batch, feed):
            imgInput, img_info, radar_pc = self._as_batch(*batch)
            with torch.cuda.stream(feed):                           # (reads host memory only: no wait on `main`)
                pre = self.pre_process(imgInput, img_info, radar_pc)
                ev = torch.cuda.Event()
                ev.record(feed)
            return pre + (img_info,), ev

        # The device context and the caller's stream are re-read on every resumption and never held across a `yield`:
        # between two next() calls the caller's own device / stream context is untouched.
        batch = next(it, None)
        if batch is None:
            return
        with torch.cuda.device(self.device):
            staged = stage(batch, feed_stream(torch.cuda.current_stream(self.device)))
        pending = None
        while staged is not None:
            with torch.cuda.device(self.device):
                main = torch.cuda.current_stream(self.device)
                (images, pc_dep, metas, calibs, infos), ev = staged
                main.wait_event(ev)
                for t in (images, pc_dep, calibs):
                    if t is not None:
                        t.record_stream(main)                       # allocated on the feed stream, consumed on `main`
                outputs, post = self.process(images, calibs, pc_dep, metas[0])       # batch i: queued on `main`
                dm = self._depth_maps_device(outputs) if depthmaps else None
                batch = next(it, None)
                staged = stage(batch, feed_stream(main)) if batch is not None else None   # batch i+1: beside it
                done, pending = pending, (outputs, post, metas, infos, merge, dm)
                if done is not None:
                    done = self._finish(*done)                                       # batch i-1: host side
            if done is not None:
                yield done
        with torch.cuda.device(self.device):
            last = self._finish(*pending)
        yield last

    def run(self, imgInput, img_info=None, radar_pc=None, merge=True, stage_times=False, depthmaps=False):
        """imgInput: (H,W,3) uint8 ndarray, a list of them, or a (B,H,W,3) uint8 tensor; img_info: dict or list of
        dicts (`calib`, and for radar `camera_intrinsic`, `width`, `height`); radar_pc: (R,N) array or list.
        -> {"outputs", "post" (B,K,54) device, "metas", "img_infos" (the batch's own, as a list), "detects" (dict of host
        tensors), "predictBoxes"}.

        `depthmaps=True` adds `ret["depthmaps"]`, the second value of the reference's `post_process` that its `run` hands
        on (detector.py:107-112, 351-393): see `depth_maps`.  Without it the dict has exactly the keys above.

        `stage_times=True` adds the reference's per-stage seconds under the reference's keys (its `@return_time` tracing
        hook, utils/utils.py:52-66 on detector.py:44-470; `ret["load"] ... ret["display"]`, detector.py:140-155) plus
        "tot".  The reference brackets every stage with two device synchronisations; here the device stages are
        bracketed by HIP events on the caller's stream and read back once at the end, so timing a run does not
        serialise host and device: "preprocess" (frame copy + warp + radar ingest + pillars), "net" (forward),
        "decode" (the fused decode + postProcess launch), "postprocess" 0.0 (inside "decode"; with `depthmaps` the depth-map
        launch), "merge" (host: fetch + box lists), "load" / "display" 0.0 (no file loading, no visualisation on this path)."""
        imgInput, img_info, radar_pc = self._as_batch(imgInput, img_info, radar_pc)
        marks, mark = [], None
        with torch.cuda.device(self.device):
            if stage_times:
                stream = torch.cuda.current_stream(self.device)

                def mark(name):
                    ev = torch.cuda.Event(enable_timing=True)
                    ev.record(stream)
                    marks.append((name, ev))

                import time
                t_host = time.perf_counter()
                mark("start")
            images, pc_dep, metas, calibs = self.pre_process(imgInput, img_info, radar_pc)
            if stage_times:
                mark("preprocess")
            outputs, post = self.process(images, calibs, pc_dep, metas[0], mark)
            if stage_times:
                mark("decode")
            dm = self._depth_maps_device(outputs) if depthmaps else None
            if stage_times and depthmaps:
                mark("postprocess")
        if not stage_times:
            return self._finish(outputs, post, metas, img_info, merge, dm)
        marks[-1][1].synchronize()
        t_merge = time.perf_counter()
        ret = self._finish(outputs, post, metas, img_info, merge, dm)
        t_end = time.perf_counter()
        ret.update({"load": 0.0, "postprocess": 0.0, "display": 0.0, "merge": t_end - t_merge, "tot": t_end - t_host})
        for (_, e0), (name, e1) in zip(marks[:-1], marks[1:]):
            ret[name] = e0.elapsed_time(e1) * 1e-3
        return ret
