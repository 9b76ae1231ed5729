"""cf_head_fused_at computes only the tile rows that hold a centre (rows 0, 3 and 6 of the virtual tile = column tiles 0, 3, 6 of
the MFMA tile; in the hidden chain rows 0 and 3 of the first half, row 6 of the second).

The four forms (mx / bf16x3 first layer, without and with pc_hm source + hidden layers) on a two-image 16 x 24 map, with
hand-made tables whose only non-empty slots are (a) slot 0, (b) slots 12-17 - tile row 6, the second half of the hidden chain -,
(c) slots 6-11 - tile row 3 -, (d) all 18, image corners and edges among them.  Listed pixels: `torch.equal` with the dense
cf_head_fused output; everything else keeps the NaN the maps were filled with.  The forms without hidden layers run the
six-head group once per number of heads per workgroup the launcher's rule picks (1, 2, 3: it goes by the number of tiles, so
the table is padded with empty tiles)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_heads_at_peaks import _packed_heads, nhwc, rnd

gpu = pytest.mark.gpu
B, H, W = 2, 16, 24
HW = H * W
IMG1 = HW                                                      # flat pixel of image 1's first pixel

# slot -> flat pixel of the batch
CORNERS_EDGES = [0, W - 1, (H - 1) * W, HW - 1, 5, 7 * W, 9 * W + W - 1, (H - 1) * W + 11]
TABLES = {
    "slot0": {0: IMG1 + 8 * W + 8},
    "row6": dict(zip(range(12, 18), [HW - 1, IMG1, IMG1 + 4 * W + 4, IMG1 + 4 * W + 5, IMG1 + 10 * W + 10, IMG1 + 12 * W + 12])),
    "row3": dict(zip(range(6, 12), [(H - 1) * W, 3 * W + 3, IMG1 + W - 1, IMG1 + 6 * W + 6, IMG1 + 7 * W + 7, IMG1 + 13 * W])),
    "all": dict(zip(range(18), CORNERS_EDGES + [6 * W + 9, 6 * W + 10] +
                    [IMG1 + p for p in (2 * W + 2, 2 * W + 3, 3 * W + 2, 8 * W + 20, 11 * W + 1, 14 * W + 22, HW - 1, 0)])),
}
# (mx, pc_hm source, hidden layers, heads)
FORMS = [(True, False, 0, 6), (False, False, 0, 6), (True, True, 2, 2), (False, True, 2, 2)]
# tiles -> heads per workgroup of a six-head group without hidden layers, by the launcher's rule (512 workgroup slots, cost
# rounds * (heads + 0.25)): up to 85 tiles 1, up to 170 tiles 2, beyond 3
HLOOP_TILES = (1, 100, 180)


def _inputs():
    """features; pc_hm non-zero in a block of image 0 and all zero in image 1: virtual tiles with and without the radar k-step"""
    feat, pch = F.relu(rnd(B, 64, H, W, seed=1)) * 3.0, rnd(B, 3, H, W, seed=2) * 20.0
    keep = torch.zeros(B, 1, H, W)
    keep[0, :, 2:12, 4:20] = 1.0
    return feat, pch * keep


def _table(slots, n_tiles, at, dev):
    """[n_tiles][18] int32, tile `at` holding `slots`, every other tile empty"""
    t = torch.full((n_tiles, 18), -1, dtype=torch.int32)
    for s, p in slots.items():
        t[at, s] = p
    return t.to(dev)


@gpu
@pytest.mark.parametrize("mx,pc,n_hidden,n_heads", FORMS)
def test_centre_rows_get_the_dense_bits_and_nothing_else_is_written(mx, pc, n_hidden, n_heads):
    from centerfusiondetect3d_amd import _lib, ops
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    feat, pch = _inputs()
    packed, slots, k_pad = _packed_heads(dev, mx, pc, n_hidden, n_heads)
    heads = [dict(hd, out=torch.empty(B, hd["n_out"], H, W, device=dev),
                  out2=torch.empty(B, hd["n_out"], H, W, device=dev) if hd["act"] == 3 else None) for hd in packed]
    src0 = ops.pack_feat_mx(nhwc(feat).to(dev)) if mx else ops.split_bf16(nhwc(feat).to(dev))
    srcs = [src0] + ([ops.split_bf16(nhwc(pch).to(dev), cs=8)] if pc else [])
    f = ops.head_fused_args(srcs, [64, 8][:len(srcs)], slots, k_pad, B, H, W, heads)
    assert f.mx == int(mx) and f.n_src == len(srcs) and f.tail.n_hidden == n_hidden and f.tail.n_heads == n_heads
    maps = [hd["out"] for hd in heads] + [hd["out2"] for hd in heads if hd["out2"] is not None]
    ops.run_head_fused(f)
    dense = [m.clone() for m in maps]
    assert all(bool(torch.isfinite(d).all()) for d in dense)
    for name, tab in TABLES.items():
        for n_tiles in (HLOOP_TILES if n_hidden == 0 and name == "all" else (1,)):
            table = _table(tab, n_tiles, n_tiles // 2, dev)
            sel = torch.zeros(B * HW, dtype=torch.bool)
            sel[list(tab.values())] = True
            sel = sel.view(B, HW).to(dev)
            for m in maps:
                m.fill_(float("nan"))
            _lib.check(lib.cf_head_fused_at(C.byref(f), table.data_ptr(), n_tiles, _lib.stream_ptr()), "cf_head_fused_at")
            for m, d in zip(maps, dense):
                n = m.shape[1]
                got, want = m.view(B, n, HW).transpose(1, 2), d.view(B, n, HW).transpose(1, 2)     # (B, HW, n)
                assert torch.equal(got[sel], want[sel]), (name, n_tiles, n)
                assert bool(torch.isnan(got[~sel]).all()), (name, n_tiles, n)
