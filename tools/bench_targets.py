"""Dev tool (GPU box): time the training-target builder at the workload's size - B = 16, 10 classes, 112 x 200 maps, 128 object
slots, 40 and 128 annotations per image, about 300 radar pixels per image, radar + frustum association - in two arms:
  hip    centerfusiondetect3d_amd.build_targets on device-resident tables (cf_targets_build: three launches), each call between
         two HIP events; `pack_annotations` (host, dicts -> tables) and the upload of the tables are timed separately
  host   the per-object host loop this replaces, restated in numpy below in the reference's call sequence (one image after the
         other: box transform, Gaussian radius, Gaussian window with np.maximum, rotation bins, 3D corners, distance threshold,
         radar ROI search, rectangle paint), timed with the host clock - no reference import
The arms' results are compared first (mask, heat map, pc_hm): faster and different is not faster.
    python tools/bench_targets.py [--calls 200] [--warmup 30] [--batch 16] [--out FILE]
Prints median / p95 / min per arm and object count and one JSON line."""
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, C, M = 112, 200, 10, 128


def make_case(B, n_obj, seed):
    from tests import targets_cases as tc
    rs = np.random.RandomState(seed)
    T = tc.matrix(W)
    anns, pcs = [], []
    for _ in range(B):
        pc = np.zeros((3, H, W), np.float32)
        image = []
        for i in range(n_obj):
            bw, bh = rs.uniform(1.5, 30.0), rs.uniform(1.5, 24.0)
            x1, y1 = rs.uniform(-3.0, W - 4.0), rs.uniform(-3.0, H - 4.0)
            box = (x1, y1, x1 + bw, y1 + bh)
            depth = 5.0 + 9.0 * (i % 6) + rs.uniform(0.0, 1.0)
            image.append(tc.make_ann(rs, T, box, rs.randint(1, C + 1), depth))
        for _ in range(300):                                            # radar returns near the annotated depths
            a = image[rs.randint(n_obj)]
            s, tx, ty = T[0, 0], T[0, 2], T[1, 2]
            x = int(np.clip(a["bbox"][0] * s + tx + rs.uniform(0, a["bbox"][2] * s), 0, W - 1))
            y = int(np.clip(a["bbox"][1] * s + ty + rs.uniform(0, a["bbox"][3] * s), 0, H - 1))
            tc.put_radar(pc, x, y, a["depth"] + rs.uniform(-0.5, 0.5), rs.normal(0, 4), rs.normal(0, 4))
        anns.append(image)
        pcs.append(pc)
    return anns, np.stack([T] * B), tc.calib_for(B, W), np.stack(pcs)


# ---- the host loop, restated (generic_dataset.py:206-228, 441-687 with image.py / pointcloud.py behind it) ------------------------
def _affine(pts, T):
    p = np.ones((pts.shape[0], 3), np.float32)
    p[:, :2] = pts
    return np.dot(T, p.T).T[:, :2]


def _radius(h, w, ov=0.7):
    b1, c1 = h + w, w * h * (1 - ov) / (1 + ov)
    r1 = (b1 + np.sqrt(b1 ** 2 - 4 * c1)) / 2
    b2, c2 = 2 * (h + w), (1 - ov) * w * h
    r2 = (b2 + np.sqrt(b2 ** 2 - 16 * c2)) / 2
    a3, b3, c3 = 4 * ov, -2 * ov * (h + w), (ov - 1) * w * h
    r3 = (b3 + np.sqrt(b3 ** 2 - 4 * a3 * c3)) / 2
    return min(r1, r2, r3)


def _draw(heat, center, r):
    d = 2 * r + 1
    y, x = np.ogrid[-r:r + 1, -r:r + 1]
    g = np.exp(-(x * x + y * y) / (2 * (d / 6) * (d / 6)))
    g[g < np.finfo(g.dtype).eps * g.max()] = 0
    cx, cy = int(center[0]), int(center[1])
    hh, ww = heat.shape
    l, rt, t, b = min(cx, r), min(ww - cx, r + 1), min(cy, r), min(hh - cy, r + 1)
    np.maximum(heat[cy - t:cy + b, cx - l:cx + rt], g[r - t:r + b, r - l:r + rt], out=heat[cy - t:cy + b, cx - l:cx + rt])


def _corners(dim, yaw):
    c, s = np.cos(yaw), np.sin(yaw)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float32)
    hh, ww, ll = dim
    xs = np.array([1, 1, -1, -1, 1, 1, -1, -1], np.float32) * np.float32(0.5 * ll)
    ys = np.array([0, 0, 0, 0, -1, -1, -1, -1], np.float32) * np.float32(hh)
    zs = np.array([1, -1, -1, 1, 1, -1, -1, 1], np.float32) * np.float32(0.5 * ww)
    return (R @ np.stack([xs, ys, zs])).T


def host_image(anns, T, calib, pc_dep, max_dist=60.0):
    item = {"heatmap0": np.zeros((C, H, W), np.float32), "classIds": np.zeros(M, np.int64), "mask": np.zeros(M, np.float32),
            "truncMask": np.zeros(M, np.float32), "widthHeight": np.zeros((M, 2), np.float32), "reg": np.zeros((M, 2), np.float32),
            "amodal_offset": np.zeros((M, 2), np.float32), "dimension": np.zeros((M, 3), np.float32),
            "depth": np.zeros((M, 1), np.float32), "rotbin": np.zeros((M, 2), np.int64), "rotres": np.zeros((M, 2), np.float32),
            "nuscenes_att": np.zeros((M, 8), np.float32), "nuscenes_att_mask": np.zeros((M, 8), np.float32),
            "velocity": np.zeros((M, 3), np.float32), "pc_hm": np.zeros((3, H, W), np.float32)}
    tg = {"bboxes": np.zeros((M, 4), np.float32), "centers": np.zeros((M, 2), np.float32), "heatCenters": np.zeros((M, 2), np.float32),
          "bboxes3d": np.zeros((M, 8, 3), np.float32), "rotation": np.zeros((M, 8), np.float32)}
    groups = {0: [0, 1], 1: [0, 1], 2: [2, 3, 4], 3: [2, 3, 4], 4: [2, 3, 4], 5: [5, 6, 7], 6: [5, 6, 7], 7: [5, 6, 7]}
    for i, ann in enumerate(anns[:M]):
        cid = ann["category_id"]
        if cid > C or cid <= -999:
            continue
        x, y, bw, bh = ann["bbox"]
        box = np.array([x, y, x + bw, y + bh], np.float32)
        rect = np.array([[box[0], box[1]], [box[0], box[3]], [box[2], box[3]], [box[2], box[1]]])
        rect[:] = _affine(rect, T)
        box = np.array([rect[:, 0].min(), rect[:, 1].min(), rect[:, 0].max(), rect[:, 1].max()])
        box[[0, 2]] = np.clip(box[[0, 2]], 0, W - 1)
        box[[1, 3]] = np.clip(box[[1, 3]], 0, H - 1)
        hgt, wid = box[3] - box[1], box[2] - box[0]
        if hgt <= 0 or wid <= 0:
            continue
        center = np.array([(box[0] + box[2]) / 2, (box[1] + box[3]) / 2], np.float32)
        item["classIds"][i], item["mask"][i], item["truncMask"][i] = cid - 1, 1, ann["truncated"]
        amodal = _affine(np.array(ann["amodal_center"]).reshape(1, -1), T)
        heat_c = center * np.array([1.0, 1.0])
        _draw(item["heatmap0"][cid - 1], heat_c, max(0, int(_radius(math.ceil(hgt), math.ceil(wid)))))
        tg["bboxes"][i], tg["centers"][i], tg["heatCenters"][i] = box, center, heat_c
        item["reg"][i] = center - heat_c
        item["amodal_offset"][i] = amodal - heat_c
        item["widthHeight"][i] = (wid, hgt)
        if ann["attributes"] > 0:
            att = int(ann["attributes"] - 1)
            item["nuscenes_att"][i][att] = 1
            item["nuscenes_att_mask"][i][groups[att]] = 1
        if min(ann["velocity_cam"]) > -1000:
            item["velocity"][i] = np.array(ann["velocity_cam"], np.float32)[:3]
        alpha = ann["alpha"]
        rot = [0, 0, 0, 1, 0, 0, 0, 1]
        if alpha < np.pi / 6.0 or alpha > 5 * np.pi / 6.0:
            r = alpha - (-0.5 * np.pi)
            item["rotbin"][i, 0], item["rotres"][i, 0] = 1, r
            rot[1], rot[2], rot[3] = 1, np.sin(r), np.cos(r)
        if alpha > -np.pi / 6.0 or alpha < -5 * np.pi / 6.0:
            r = alpha - (0.5 * np.pi)
            item["rotbin"][i, 1], item["rotres"][i, 1] = 1, r
            rot[5], rot[6], rot[7] = 1, np.sin(r), np.cos(r)
        tg["rotation"][i] = rot
        item["depth"][i] = ann["depth"] * 1.0
        item["dimension"][i] = ann["dimension"]
        tg["bboxes3d"][i] = _corners(ann["dimension"], ann["yaw"]) + np.array(ann["location"])
        # ground-truth frustum association
        yaw = alpha + np.arctan2(center[0] - calib[0, 2], calib[0, 0])
        yaw = yaw - 2 * np.pi if yaw > np.pi else yaw + 2 * np.pi if yaw < -np.pi else yaw
        z = _corners(ann["dimension"], yaw)[:, 2]
        thr = z.max() - z.min() / 2.0
        bi = [int(np.floor(box[0])), int(np.floor(box[1])), int(np.ceil(box[2])), int(np.ceil(box[3]))]
        roi = pc_dep[:, bi[1]:bi[3] + 1, bi[0]:bi[2] + 1]
        nz = np.nonzero(roi[0])
        if len(nz[0]) > 0:
            d = roi[0][nz]
            ok = (d < ann["depth"] + thr) & (d > max(0, ann["depth"] - thr))
            if ok.any():
                k = np.argmin(d[ok])
                dist, vx, vz = d[ok][k] / np.float32(max_dist), roi[1][nz][ok][k], roi[2][nz][ok][k]
                wi, hi = np.float32(0.3) * wid, np.float32(0.3) * hgt
                w0, w1 = int(center[0] - wi / 2), int(center[0] + wi / 2)
                h0, h1 = int(center[1] - hi / 2), int(center[1] + hi / 2)
                item["pc_hm"][0, h0:h1 + 1, w0:w1 + 2] = dist
                item["pc_hm"][1, h0:h1 + 1, w0:w1 + 2] = vx
                item["pc_hm"][2, h0:h1 + 1, w0:w1 + 2] = vz
    item["target"] = tg
    return item


def stats(ts):
    ts = sorted(ts)
    return {"median": ts[len(ts) // 2], "p95": ts[int(len(ts) * 0.95)], "min": ts[0], "n": len(ts)}


def main():
    import torch
    from centerfusiondetect3d_amd import build_targets, centerfusion_middle_config, pack_annotations
    argv = sys.argv[1:]
    opt = lambda k, d: type(d)(argv[argv.index(k) + 1]) if k in argv else d
    calls, warmup, B, path = opt("--calls", 200), opt("--warmup", 30), opt("--batch", 16), opt("--out", "")
    assert torch.cuda.is_available(), "bench_targets.py measures on the GPU only"
    dev = torch.device("cuda:0")
    cfg = centerfusion_middle_config((4 * H, 4 * W))
    result = {"B": B, "h": H, "w": W, "max_objs": M, "radar_px": 300, "unit": "us"}
    spin = torch.randn(4096, 4096, device=dev)
    for _ in range(30):
        spin = (spin @ spin) * 1e-4                # warm the clocks
    for n_obj in (40, 128):
        anns, trans, calib, pc = make_case(B, n_obj, seed=n_obj)
        t0 = time.perf_counter()
        ann = pack_annotations(anns, config=cfg)
        t_pack = (time.perf_counter() - t0) * 1e6
        trans_d, calib_d, pc_d = torch.from_numpy(trans).to(dev), torch.from_numpy(calib).to(dev), torch.from_numpy(pc).to(dev)
        scale_d = torch.ones(B, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ann_d = ann.to(dev)
        torch.cuda.synchronize()
        t_up = (time.perf_counter() - t0) * 1e6
        call = lambda: build_targets(ann_d, trans_d, calib_d, cfg, pc_dep=pc_d, scale_factor=scale_d)

        # ---- the arms compute the same thing
        got = call()
        torch.cuda.synchronize()
        host = [host_image(anns[b], trans[b], calib[b], pc[b]) for b in range(B)]
        for k in ("mask", "classIds", "heatmap0", "pc_hm", "widthHeight", "rotbin"):
            ref = np.stack([it[k] for it in host])
            g = got[k].cpu().numpy()
            assert np.array_equal(g != 0, ref != 0) and np.allclose(g, ref, rtol=3e-7, atol=0), f"{k}: the two arms differ"
        painted = int((got["pc_hm"][:, 0] != 0).sum())

        for _ in range(warmup):
            call()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
        for a, b in ev:
            a.record()
            call()
            b.record()
        torch.cuda.synchronize()
        hip = stats([a.elapsed_time(b) * 1e3 for a, b in ev])
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        torch.cuda.synchronize()
        hip_wall = (time.perf_counter() - t0) * 1e6 / calls
        ts = []
        for _ in range(max(3, calls // 20)):
            t0 = time.perf_counter()
            for b in range(B):
                host_image(anns[b], trans[b], calib[b], pc[b])
            ts.append((time.perf_counter() - t0) * 1e6)
        cpu = stats(ts)
        result[f"objs{n_obj}"] = {"hip_events": hip, "hip_wall_per_call": hip_wall, "pack_annotations": t_pack, "upload_tables": t_up,
                                  "host_loop": cpu, "painted_px": painted, "drawn": int(got["mask"].sum())}
        print(f"{n_obj} annotations / image, B = {B}: drawn {int(got['mask'].sum())}, pc_hm painted {painted} px", flush=True)
        print(f"  hip   build_targets      median {hip['median']:9.1f} us  p95 {hip['p95']:9.1f}  min {hip['min']:9.1f}  (n = {hip['n']}; "
              f"host clock over {calls} back-to-back calls: {hip_wall:.1f} us / call)")
        print(f"        pack_annotations   {t_pack:9.1f} us (host, once)   table upload {t_up:9.1f} us")
        print(f"  host  numpy loop, {B} images median {cpu['median']:9.1f} us  p95 {cpu['p95']:9.1f}  min {cpu['min']:9.1f}  (n = {cpu['n']})", flush=True)
    line = json.dumps(result)
    print(line)
    if path:
        with open(path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
