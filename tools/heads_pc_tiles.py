"""Dev tool (GPU box): share of the secondary heads' 128-pixel tiles whose pc_hm patch (tile + 1-pixel frame) is all zero
in one bench-shaped forward (bs 16, 448x800, bench.py's synthetic weights and inputs) - the workgroups of
head_patch16_kernel<.., PC> that leave the pc_hm taps out.   python tools/heads_pc_tiles.py [--batch 16] [--seed 1000]
--tuned: the small tuned model of tests/golden/cases.py (128x160, whose heat-map peaks the frustum association does match)
instead of the benchmark's random-weight model."""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F


def empty_share(pc_hm, th, tw):
    """pc_hm (B, C, H, W) -> (tiles per image, share of th x tw tiles whose (th + 2) x (tw + 2) patch holds no non-zero value)"""
    nz = (pc_hm != 0).any(1, keepdim=True).float()                        # -0.0 != 0 is False: as the kernel counts it
    H, W = nz.shape[-2:]
    ty, tx = -(-H // th), -(-W // tw)
    nz = F.pad(nz, (1, tx * tw - W + 1, 1, ty * th - H + 1))              # the frame and the ragged edge: zeros
    live = F.max_pool2d(nz, (th + 2, tw + 2), stride=(th, tw))            # one window per tile, with its frame
    assert live.shape[-2:] == (ty, tx), (live.shape, ty, tx)
    return ty * tx, float((live == 0).float().mean())


if __name__ == "__main__":
    import bench
    from centerfusiondetect3d_amd import getModel, centerfusion_middle_config
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--tuned", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.tuned:
        from tests.golden import cases
        H, W = 128, 160
        m = getModel(centerfusion_middle_config((H, W)))
        m.load_state_dict(cases.tuned_state_dict(radar=True, seed=0), strict=True)
        m = m.to(dev).eval()
        images, pc_dep, calib = (t.to(dev) for t in cases.model_inputs(a.batch, H, W, seed=a.seed, radar=True))
    else:
        H, W = 448, 800
        m = bench.synthetic_weights(getModel(centerfusion_middle_config((H, W)))).to(dev).eval()
        images, pc_dep, calib = bench.make_inputs(a.batch, H, W, dev, a.seed)
    with torch.no_grad():
        out = m(images, pc_dep=pc_dep, calib=calib)
    pc_hm = out[0]["pc_hm"].float().cpu()
    print(f"pc_hm {tuple(pc_hm.shape)}: {float((pc_hm != 0).any(1).float().mean()) * 100:.1f} % of the pixels are painted")
    for name, th, tw in (("8 x 16 (flat)", 8, 16), ("16 x 8 (upright)", 16, 8)):
        n, share = empty_share(pc_hm, th, tw)
        print(f"tiles {name:17s}: {n} per image, {share * 100:.1f} % with an all-zero patch")
