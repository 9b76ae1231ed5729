"""Cases and a plain-torch restatement of the criterion (GenericLoss over one output layer), shared by tests/test_loss_cpu.py,
tests/test_gpu_loss.py, tests/golden/make_golden_loss.py and tools/bench_loss.py.

`generic_loss` is written from the semantics include/cf_hip.h states (layer mask, focal term, masked L1, bin / residual
rotation term, masked BCE, uncertainty-attenuated depth term) with gathers on the NCHW maps and `torch.where` for the
zero-count branches; it is differentiable, runs in any float dtype on any device, and holds no reference text.  In float64
on the CPU it is the oracle of the GPU tests; tests/golden/loss_cases.npz pins it to the reference's own code.

`make_case(i)` is seeded.  Every case but the all-masked ones holds, asserted: two objects on one pixel and class, a third
on that pixel with another class, objects on pixel (0,0) and (w-1,h-1), all four combinations of mask 0/1 and area 0/>0
(widthHeight drawn independently of mask), rotbin != 0 on a row with mask 0 and area > 0, and - with an uncertainty head -
u beyond both +10 and -10 at object pixels.  The L1 gradient jumps at pred == target and the clamp's at |u| == 10: such inputs
are moved 2e-3 away and the distance (>= 1e-3) is asserted on the fp32 values; no case is excluded.
"""
import functools

import torch

# (name, (B, C, h, w, M), head set, uncertainty head, training, every mask 0)
CASES = [
    ("dense", (2, 10, 16, 24, 32), "middle", False, True, False),
    ("tiny", (1, 10, 7, 9, 5), "middle", False, True, False),            # 630 heat-map elements: not a multiple of 4
    ("sparse", (3, 10, 13, 17, 128), "middle", False, True, False),
    ("fullmap", (2, 10, 112, 200, 128), "middle", False, True, False),   # many partial sums
    ("dense_mask0", (2, 10, 16, 24, 32), "middle", False, True, True),
    ("dense_unc_train", (2, 10, 16, 24, 32), "middle", True, True, False),
    ("dense_unc_eval", (2, 10, 16, 24, 32), "middle", True, False, False),
    ("dense_unc_mask0", (2, 10, 16, 24, 32), "middle", True, True, True),
    ("dense_camera", (2, 10, 16, 24, 32), "camera", False, True, False),
    ("dense_early", (2, 10, 16, 24, 32), "early", False, True, False),
    # R = B * M = 1280 rows on 221 pixels: the object kernel's 1024-thread loops run twice, many colliding atomic adds in the backward
    ("manyrows", (5, 10, 13, 17, 256), "middle", True, True, False),
    # 1,075,200 heat-map elements: just above the 1,048,576 at which the dense passes' 1024-workgroup cap binds (grid-stride loops
    # run twice, all 1024 partial sums enter the object kernel)
    ("bigmap", (3, 10, 160, 224, 128), "middle", False, True, False),
]
NAMES = [c[0] for c in CASES]

# not the defaults, so that a weight applied to the wrong term shows
LOSS_WEIGHTS = dict(HEATMAP=1.0, AMODAL_OFFSET=0.9, DIMENSION_2D=0.1, DEPTH=0.7, DIMENSION_3D=1.1, ROTATION=1.3,
                    NUSCENES_ATT=0.8, VELOCITY=1.2, BBOX_2D=0.0, BBOX_3D=0.0, LIDAR_DEPTH=0.0, RADAR_DEPTH=0.0)
L1_HEADS = ("reg", "widthHeight", "dimension", "amodal_offset", "velocity")
KINK = 1e-3


def config_for(i):
    """this package's config of case i (MODEL.OUTPUT_SIZE = the case's map, LOSS_WEIGHTS above)"""
    from centerfusiondetect3d_amd import config as cfgmod
    _, (B, C, h, w, M), heads, unc, _, _ = CASES[i]
    make = {"middle": cfgmod.centerfusion_middle_config, "camera": cfgmod.centernet_config,
            "early": cfgmod.centerfusion_early_config}[heads]
    c = make((4 * h, 4 * w))
    c.DATASET.NUM_CLASSES = C
    c.TRAIN.UNCERTAINTY_LOSS = unc
    cfgmod.update_heads(c)
    c.LOSS_WEIGHTS.update(LOSS_WEIGHTS)
    cfgmod.update_loss_weights(c)
    return c


def _object_rows(g, B, C, h, w, M, mask0, sparse):
    """centers (B,M,2), cls, mask, widthHeight; rows 0-4 (and 5 when there is one) of every image are the constructed ones"""
    xs = torch.randint(0, w, (B, M), generator=g)
    ys = torch.randint(0, h, (B, M), generator=g)
    cls = torch.randint(0, C, (B, M), generator=g)
    mask = (torch.rand(B, M, generator=g) < (0.15 if sparse else 0.6)).float()
    area = torch.rand(B, M, generator=g) < 0.7                       # drawn independently of mask
    # rows 0, 1: one pixel (the last one), one class, mask 1, area > 0; row 2: that pixel, another class, mask 0, area > 0
    xs[:, 0:3], ys[:, 0:3] = w - 1, h - 1
    cls[:, 0:2] = 3
    cls[:, 2] = 7
    mask[:, 0:2], mask[:, 2] = 1.0, 0.0
    area[:, 0:3] = True
    # row 3: pixel (0,0), mask 1, area 0; row 4: mask 0, area 0
    xs[:, 3], ys[:, 3] = 0, 0
    mask[:, 3], mask[:, 4] = 1.0, 0.0
    area[:, 3:5] = False
    if M > 5:                                                        # row 5: pixel (0,0), mask 1, area > 0
        xs[:, 5], ys[:, 5] = 0, 0
        mask[:, 5], area[:, 5] = 1.0, True
    frac = torch.rand(B, M, 2, generator=g) * 0.9
    centers = torch.stack([xs, ys], dim=-1).float() + frac
    wh = (torch.rand(B, M, 2, generator=g) * 20 + 0.5) * area[..., None].float()
    if mask0:
        mask = torch.zeros(B, M)
    return centers, cls, mask, wh


def _targets(g, B, M, gt, mask, cls, wh, centers):
    rn = lambda *s: torch.randn(*s, generator=g)
    return {"heatmap0": gt, "mask": mask, "classIds": cls, "widthHeight": wh, "target": {"heatCenters": centers},
            "depth": rn(B, M, 1).abs() * 20 + 1, "reg": torch.rand(B, M, 2, generator=g), "dimension": rn(B, M, 3).abs() + 0.5,
            "amodal_offset": rn(B, M, 2), "velocity": rn(B, M, 3) * 3,
            "rotbin": (torch.rand(B, M, 2, generator=g) < 0.5).long(), "rotres": rn(B, M, 2),
            "nuscenes_att": (torch.rand(B, M, 8, generator=g) < 0.3).float(),
            "nuscenes_att_mask": (torch.rand(B, M, 8, generator=g) < 0.5).float() * (torch.rand(B, M, 1, generator=g) < 0.7).float()}


def _move_l1_kinks(out, batch, pix, eff_mask, name):
    """pred == target at an object's pixel, on the rows that count (layer mask and mask != 0): the target is moved away, and the
    distance asserted on the fp32 values"""
    B, M = pix.shape

    def gathered(t):
        ch = t.shape[1]
        return t.flatten(2).gather(2, pix[:, None, :].expand(B, ch, M)).transpose(1, 2)
    for k in ("depth", "depth2") + L1_HEADS:
        if k not in out:
            continue
        tk = "depth" if k == "depth2" else k
        for _ in range(3):                                           # (depth's target serves two heads)
            d = gathered(out[k]) - batch[tk]
            close = (d.abs() < 2 * KINK) & (eff_mask[..., None] != 0)
            batch[tk] = torch.where(close, batch[tk] + 4 * KINK, batch[tk])
    for k in ("depth", "depth2") + L1_HEADS:
        if k in out:
            d = (gathered(out[k]) - batch["depth" if k == "depth2" else k]).abs()
            assert bool((d[eff_mask != 0] >= KINK).all()), (name, k)


def batch_for(outputs, M=16, seed=77):
    """a seeded batch (the constructed rows of `make_case` included) for maps that came from somewhere else, e.g. a model"""
    out = {k: v.detach().cpu() for k, v in outputs[0].items() if torch.is_tensor(v)}
    B, C, h, w = out["heatmap"].shape
    g = torch.Generator().manual_seed(seed)
    centers, cls, mask, wh = _object_rows(g, B, C, h, w, M, False, False)
    lm = (wh[..., 0] * wh[..., 1]) / float(h * w) > 0
    pix = ((centers[..., 1].long() * w + centers[..., 0].long()) * lm).clamp(0, h * w - 1)
    batch = _targets(g, B, M, torch.rand(B, C, h, w, generator=g) ** 4, mask, cls, wh, centers)
    _move_l1_kinks(out, batch, pix, mask * lm, "batch_for")
    return batch


@functools.lru_cache(maxsize=None)
def make_case(i):
    """-> (outputs, batch, training): CPU fp32 tensors (i64 where the reference's dataset has i64).  Cached: do not write to it."""
    name, (B, C, h, w, M), heads, unc, training, mask0 = CASES[i]
    g = torch.Generator().manual_seed(4100 + i)
    rn = lambda *s: torch.randn(*s, generator=g)
    centers, cls, mask, wh = _object_rows(g, B, C, h, w, M, mask0, name == "sparse")
    lm = (wh[..., 0] * wh[..., 1]) / float(h * w) > 0
    pix = ((centers[..., 1].long() * w + centers[..., 0].long()) * lm).clamp(0, h * w - 1)
    eff_mask = mask * lm

    out = {"heatmap": torch.sigmoid(rn(B, C, h, w) * 2).clamp(1e-4, 1 - 1e-4)}
    chans = {"reg": 2, "widthHeight": 2, "depth": 1, "rotation": 8, "dimension": 3, "amodal_offset": 2, "nuscenes_att": 8,
             "velocity": 3}
    if heads == "middle":
        chans.update({"depth2": 1, "rotation2": 8})
    for k, ch in chans.items():
        out[k] = rn(B, ch, h, w) * (1.5 if k.startswith("rotation") or k == "nuscenes_att" else 1.0)
    for k in ("depth", "depth2"):
        if k in out:
            out[k] = out[k].abs() * 20 + 1
    if unc:
        # under pixel (0,0) e^-u reaches e^10: keep |d| of row 5 small there, or that one row would be the whole total
        for k in ("depth", "depth2"):
            out[k][:, 0, 0, 0] = 5.0
        u = rn(B, 1, h, w) * 2
        u[:, 0, h - 1, w - 1] = 12.0                                 # beyond +10 under rows 0-2, beyond -10 under pixel (0,0)
        u[:, 0, 0, 0] = -11.5
        near = (u.abs() - 10).abs() < 2 * KINK
        u = torch.where(near, u + 4 * KINK * torch.sign(u), u)
        out["uncertainty"] = u
    if heads == "middle":                                            # keys the criterion ignores
        out["pc_hm"] = rn(B, 3, h, w)
        out["depthMap"] = rn(B, 1, h, w)

    gt = torch.rand(B, C, h, w, generator=g) ** 4
    for b in range(B):
        for m in range(M):
            if eff_mask[b, m] > 0:
                gt[b, cls[b, m], pix[b, m] // w, pix[b, m] % w] = 1.0
    batch = _targets(g, B, M, gt, mask, cls, wh, centers)
    if unc and M > 5:
        batch["depth"][:, 5, 0] = 5.01
    batch["rotbin"][:, 2, 0] = 1                                     # row 2: mask 0, area > 0, a residual term all the same

    _move_l1_kinks(out, batch, pix, eff_mask, name)
    if unc:
        assert float(((out["uncertainty"].abs() - 10).abs()).min()) >= KINK, name

    if not mask0:
        for b in range(B):
            e = [(int(pix[b, m]), int(cls[b, m])) for m in range(M)]
            assert e[0] == e[1] and eff_mask[b, 0] == eff_mask[b, 1] == 1
            assert e[2][0] == e[0][0] and e[2][1] != e[0][1] and e[0][0] == h * w - 1
            assert centers[b, 3].long().tolist() == [0, 0] and (M <= 5 or (e[5][0] == 0 and eff_mask[b, 5] == 1))
            combos = {(bool(mask[b, m] != 0), bool(lm[b, m])) for m in range(M)}
            assert len(combos) == 4, (name, combos)
            assert any(mask[b, m] == 0 and lm[b, m] and batch["rotbin"][b, m].any() for m in range(M))
            if unc:
                uu = out["uncertainty"][b, 0].flatten()[pix[b]]
                assert float(uu.max()) > 10 and float(uu.min()) < -10 and bool((uu.abs() < 10).any())
    else:
        assert float(mask.sum()) == 0
    return [out], batch, training


def clone_case(i, device=None, requires_grad=False, dtype=None):
    """a private copy of case i: maps as leaves (requires_grad) on `device`"""
    outputs, batch, training = make_case(i)

    def mv(t, leaf=False):
        t = t.clone()
        if dtype is not None and t.is_floating_point():
            t = t.to(dtype)
        if device is not None:
            t = t.to(device)
        return t.requires_grad_(True) if leaf and requires_grad else t
    out = {k: mv(v, leaf=True) for k, v in outputs[0].items()}
    b = {k: ({kk: mv(vv) for kk, vv in v.items()} if isinstance(v, dict) else mv(v)) for k, v in batch.items()}
    return [out], b, training


def key_order(cfg, output):
    """the keys of `losses` in the reference's order: config.heads, total, then depth heads the config does not name"""
    return list(cfg.heads) + ["total"] + [k for k in ("depth", "depth2") if k in output and k not in cfg.heads]


def generic_loss(outputs, batch, cfg, training, dtype=torch.float64):
    """-> (total, losses): the criterion in `dtype`, differentiable in the maps of outputs[0]"""
    assert len(outputs) == 1
    out = outputs[0]
    f = lambda t: t.to(dtype)
    heat = f(out["heatmap"])
    B, C, h, w = heat.shape
    weights = cfg.weights
    area = float(cfg.MODEL.OUTPUT_SIZE[0] * cfg.MODEL.OUTPUT_SIZE[1])
    wh = batch["widthHeight"]
    lm = (wh[..., 0] * wh[..., 1]) / area > 0                         # one layer: every object with a positive area

    def keep(t):                                                       # rows outside the layer count as zeros
        return t * lm.reshape(lm.shape + (1,) * (t.dim() - 2)).to(t.dtype)
    centers = batch["target"]["heatCenters"]
    pix = keep(centers[..., 1].long() * w + centers[..., 0].long())
    m = f(keep(batch["mask"]))
    cls = keep(batch["classIds"])
    M = m.shape[1]
    n_pos = m.sum()
    has_pos = n_pos != 0
    one = torch.ones((), dtype=dtype, device=heat.device)

    def at_objects(t):                                                 # (B,ch,h,w) -> (B,M,ch), straight from NCHW
        return t.flatten(2).gather(2, pix[:, None, :].expand(B, t.shape[1], M)).transpose(1, 2)

    losses = {k: torch.zeros((), dtype=dtype, device=heat.device) for k in key_order(cfg, out)}
    # focal term
    gt = f(batch["heatmap0"])
    neg = (torch.log(1 - heat) * heat ** 2 * (1 - gt) ** 4).sum()
    pp = at_objects(heat).gather(2, cls[..., None])[..., 0]
    pos = (torch.log(pp) * (1 - pp) ** 2 * m).sum()
    losses["heatmap"] = torch.where(has_pos, -(pos + neg) / torch.where(has_pos, n_pos, one), -neg)
    total = losses["heatmap"] * weights["heatmap"]

    def masked_l1(pred, target):
        mm = m[..., None]
        return (pred * mm - f(keep(target)) * mm).abs()

    uncertain = training and "uncertainty" in out
    for k in ("depth", "depth2"):
        if k not in out:
            continue
        l = masked_l1(at_objects(f(out[k])), batch["depth"])           # (B,M,1)
        if uncertain:
            u = at_objects(f(out["uncertainty"]).clamp(-10, 10))
            e = l * torch.exp(-u) + u
            sel = (m[..., None] != 0).to(dtype)
            cnt = torch.where(has_pos, sel.sum(), one)
            losses[k] = torch.where(has_pos, (l * sel).sum() / cnt, l.mean())
            total = total + torch.where(has_pos, (e * sel).sum() / cnt, e.mean()) * weights["depth"]
        else:
            n = n_pos * l.shape[2]
            losses[k] = l.sum() / torch.where(n == 0, 1e7 * one, n)
            total = total + losses[k] * weights["depth"]
    for k in L1_HEADS:
        if k in out:
            l = masked_l1(at_objects(f(out[k])), batch[k])
            n = n_pos * l.shape[2]
            losses[k] = l.sum() / torch.where(n == 0, 1e7 * one, n)
            total = total + losses[k] * weights[k]
    for k in ("rotation", "rotation2"):
        if k not in out:
            continue
        x = at_objects(f(out[k])).reshape(-1, 8)
        rb = keep(batch["rotbin"]).reshape(-1, 2)
        rr = f(keep(batch["rotres"])).reshape(-1, 2)
        sel = (m.reshape(-1) != 0).to(dtype)
        cnt = torch.where(has_pos, sel.sum(), one)
        value = torch.zeros((), dtype=dtype, device=heat.device)
        for j in range(2):
            logits = x[:, 4 * j:4 * j + 2]
            ce = torch.logsumexp(logits, dim=1) - logits.gather(1, rb[:, j:j + 1])[:, 0]
            value = value + (ce * sel).sum() / cnt
            valid = (rb[:, j] != 0).to(dtype)                          # whatever the row's mask
            nv = valid.sum()
            res = (torch.nn.functional.smooth_l1_loss(x[:, 4 * j + 2], torch.sin(rr[:, j]), reduction="none")
                   + torch.nn.functional.smooth_l1_loss(x[:, 4 * j + 3], torch.cos(rr[:, j]), reduction="none"))
            value = value + (res * valid).sum() / torch.where(nv == 0, one, nv)
        losses[k] = value * has_pos.to(dtype)                          # no positives: 0, and no gradient
        total = total + losses[k] * weights[k]
    if "nuscenes_att" in out:
        x = at_objects(f(out["nuscenes_att"]))
        t, am = f(keep(batch["nuscenes_att"])), f(keep(batch["nuscenes_att_mask"]))
        bce = x.clamp(min=0) - x * t + torch.log1p(torch.exp(-x.abs()))
        n = am.sum()
        losses["nuscenes_att"] = (am * bce).sum() / torch.where(n == 0, 1e7 * one, n)
        total = total + losses["nuscenes_att"] * weights["nuscenes_att"]
    losses["total"] = total
    return total, losses
