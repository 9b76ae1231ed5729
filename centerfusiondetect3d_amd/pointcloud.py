"""Drop-ins for the radar steps of the hot path, HIP-backed.

  getPcFrustumHeatmap(output, pc_dep, calib, config)  <- utils/pointcloud.py:331-394
  process_point_cloud_batch(...)                       <- dataset/generic_dataset.py:738-828 (all three PC_ROI_METHODs)
  getAffineTransform(center, scale, rotation, out_wh)  <- utils/image.py:21-83 (host, 3-point solve)
"""
import numpy as np
import torch

from . import ops


def getPcFrustumHeatmap(output, pc_dep, calib, config):
    """Same arguments / result as the reference: (B,3,H,W) map, zero where nothing was painted."""
    K = int(config.MODEL.K)
    B = pc_dep.shape[0]
    return ops.topk_frustum(output["heatmap"], output["depth"], output["widthHeight"], output["dimension"],
                            output["rotation"], calib.reshape(B, 3, 4).float(), pc_dep, K,
                            float(config.DATASET.MAX_PC_DIST))


def getAffineTransform(center, scale, rotateFactor, outputSize):
    """Source-image -> output-map affine (utils/image.py:43-83): rotation 0 is the inference path (detector.py:206-221), a
    rotation in degrees (`getDirection`, image.py:21-40) and a two-element scale (of which, as upstream, only the first element
    enters) are the training augmentation's."""
    if isinstance(scale, (np.ndarray, list, tuple)):
        src_w = scale[0]
    else:
        src_w = np.float32(scale)
    dst_w, dst_h = outputSize
    center = np.asarray(center, np.float32)
    src = np.zeros((3, 2), np.float32)
    dst = np.zeros((3, 2), np.float32)
    src[0] = center
    if rotateFactor != 0:
        rad = np.pi * rotateFactor / 180.0
        sin, cos, py = np.sin(rad), np.cos(rad), src_w * -0.5
        direction = np.array([0 * cos - py * sin, 0 * sin + py * cos], np.float32)
    else:
        direction = np.array([0, src_w * -0.5], np.float32)
    src[1] = center + direction
    dst[0] = np.array([dst_w * 0.5, dst_h * 0.5], np.float32)
    dst[1] = dst[0] + np.array([0, dst_w * -0.5], np.float32)
    for p in (src, dst):
        d = p[0] - p[1]
        p[2] = p[1] + np.array([-d[1], d[0]], np.float32)
    A = np.concatenate([src.astype(np.float64), np.ones((3, 1))], axis=1)
    return np.linalg.solve(A, dst.astype(np.float64)).T.copy()


def _expand(pc_2d, pc_3d, counts, calibs, trans, out_hw, pillar_dims, roi_method):
    if roi_method == "pillars":
        return ops.pillar_expand(pc_2d, pc_3d, counts, calibs, trans, out_hw, pillar_dims)
    return ops.radar_roi_expand(pc_2d, pc_3d, counts, calibs, trans, out_hw, roi_method)


def process_point_cloud_batch(pc_2d_list, pc_3d_list, calibs, trans_out, out_hw, pillar_dims=(1.5, 0.2, 0.2),
                              device="cuda", max_points=1024, roi_method="pillars"):
    """Batched processPointCloud (DATASET.PC_ROI_METHOD = `roi_method`: "pillars", "points" or "heatmap"): per-frame
    (3,N) / (R,N) float64 arrays (already <= MAX_PC_DIST-filtered, image-projected and depth-sorted ascending, as
    detector.py:262-283 leaves them) -> pc_dep (B,3,H,W) float32 on `device`."""
    ops.roi_method_id(roi_method)
    B = len(pc_2d_list)
    n_rows = max(10, max(p.shape[0] for p in pc_3d_list))
    max_n = max(1, max(p.shape[1] for p in pc_2d_list))
    if max_n > max_points:
        raise ValueError(f"{max_n} radar points in a frame exceeds the kernel limit {max_points}")
    p2 = np.zeros((B, 3, max_n)); p3 = np.zeros((B, n_rows, max_n)); cnt = np.zeros(B, np.int32)
    for b, (a, c) in enumerate(zip(pc_2d_list, pc_3d_list)):
        n = a.shape[1]
        p2[b, :, :n], p3[b, :c.shape[0], :n], cnt[b] = a[:3], c, n
    calibs = np.asarray(calibs, np.float64).reshape(B, 3, 4)
    trans = np.broadcast_to(np.asarray(trans_out, np.float64), (B, 2, 3)).copy()
    t = lambda a: torch.from_numpy(np.array(a, copy=True, order="C")).to(device)        # (a private, writable copy: torch refuses read-only arrays with a warning)
    return _expand(t(p2), t(p3), t(cnt), t(calibs), t(trans), out_hw, pillar_dims, roi_method)


def radar_to_pc_dep(radar_pcs, intrinsics, img_wh, calibs, trans_out, out_hw, max_dist=60.0, z_offset=0.0,
                    pillar_dims=(1.5, 0.2, 0.2), descending=False, device="cuda", max_points=1024, roi_method="pillars",
                    flip=None):
    """Whole radar side of `Detector.pre_process` on the device (detector.py:257-292): raw per-frame
    sweeps (R x N float64 arrays as unpickled from annotations/radar_pc/<sensor>/<token>.bin, rows
    0..2 = x, y, z in the camera frame) -> depth gate, z offset, image projection + border gate, depth
    sort (cf_radar_ingest) -> pillar expansion (cf_pillar_expand) -> pc_dep (B,3,H,W) fp32.  Only the raw
    points cross PCIe; nothing is filtered, projected or sorted on the host.
    roi_method = DATASET.PC_ROI_METHOD (generic_dataset.py:774-826): "pillars", or "points" / "heatmap" (cf_radar_roi_expand);
    anything else raises ValueError before the device is touched.  The sort is the detector's for every method (ascending:
    detector.py:280-283 does not look at PC_REVERSE, which only the dataset loader reads).
    flip: None, or a per-frame mask (B) of frames whose image is mirrored (the training loader's isFlipped, nuscenes.py:201-205):
    after the sort and before the expansion their points get u = img_w - 1 - u and rows 0 and 8 of pc_3d (x and the x velocity)
    negated, in the ingest's float64, on the device and without a host synchronisation.  `trans_out` may be (2,3) or (B,2,3)."""
    ops.roi_method_id(roi_method)
    B = len(radar_pcs)
    arrs = [np.asarray(p, np.float64) for p in radar_pcs]
    n_rows = max(10, max(a.shape[0] for a in arrs))
    max_n = max(1, max(a.shape[1] for a in arrs))
    if max_n > max_points:
        raise ValueError(f"{max_n} radar points in a frame exceeds the kernel limit {max_points}")
    pc = np.zeros((B, n_rows, max_n)); cnt = np.zeros(B, np.int32)
    for b, a in enumerate(arrs):
        pc[b, :a.shape[0], :a.shape[1]], cnt[b] = a, a.shape[1]
    K = np.ascontiguousarray(np.broadcast_to(np.asarray(intrinsics, np.float64).reshape(-1, 3, 3), (B, 3, 3)))
    t = lambda a: torch.from_numpy(np.array(a, copy=True, order="C")).to(device)        # (a private, writable copy: torch refuses read-only arrays with a warning)
    pc_2d, pc_3d, counts = ops.radar_ingest(t(pc), t(cnt), t(K), img_wh, max_dist, z_offset, descending)
    if flip is not None:
        flip = torch.as_tensor(flip)
        if tuple(flip.shape) != (B,):
            raise ValueError(f"radar_to_pc_dep: flip must have shape ({B},), got {tuple(flip.shape)}")
        live = torch.arange(max_n, device=pc_2d.device)[None, :] < counts[:, None]          # (the padding stays zero)
        m = (flip.to(pc_2d.device, non_blocking=True) != 0)[:, None] & live
        pc_2d[:, 0] = torch.where(m, (int(img_wh[0]) - 1) - pc_2d[:, 0], pc_2d[:, 0])
        for r in (0, 8):
            pc_3d[:, r] = torch.where(m, pc_3d[:, r] * -1, pc_3d[:, r])
    calibs = np.asarray(calibs, np.float64).reshape(B, 3, 4)
    if torch.is_tensor(trans_out):                                      # (AugmentParams.trans_out, possibly on the device already)
        trans = trans_out.to(pc_2d.device, torch.float64, non_blocking=True).expand(B, 2, 3).contiguous()
    else:
        trans = t(np.broadcast_to(np.asarray(trans_out, np.float64), (B, 2, 3)))
    return _expand(pc_2d, pc_3d, counts, t(calibs), trans, out_hw, pillar_dims, roi_method)
