"""Heads at listed pixels (cf_head_fused_at, cf_head_slot_tables; model.heads_at_peaks).

Through the C ABI: the dense launch runs once per form; the at-pixels launch then writes into NaN-filled maps from hand-made
lists and must give `torch.equal` values at every listed pixel and leave everything else NaN.  Through the model: the forward
with `heads_at_peaks` against the dense forward - the decoded rows, the radar map and, once they are read, every map, bit for bit.
Map 32 x 40 (the 128 x 160 input of the other model tests), B = 3."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
B, H, W = 3, 32, 40
HW = H * W
N_OUTS, ACTS = (10, 1, 3, 8, 2, 2), (2, 3, 0, 0, 0, 0)       # heat-map-like, depth-like (two outputs), raw heads
KS = (1, 17, 18, 19, 37, 100)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------ lists and tables
def pixel_lists(K, seed=0):
    """(B, K) int32.  Image 0: the four corners, a pixel on each edge, two adjacent pixels, a duplicate, the out-of-range entries
    -1 and HW, then random pixels (K = 1: the top-left corner alone); image 1: random pixels, -1 in the middle; image 2: no
    valid entry at all."""
    g = np.random.default_rng(1000 * K + seed)
    special = [0, W - 1, (H - 1) * W, HW - 1,                 # corners
               17, 5 * W, 9 * W + W - 1, (H - 1) * W + 23,    # top, left, right, bottom edge
               12 * W + 20, 12 * W + 21,                      # adjacent
               12 * W + 20,                                   # duplicate
               -1, HW]
    img0 = (special + list(g.integers(0, HW, size=max(0, K - len(special)))))[:K]
    img1 = list(g.integers(0, HW, size=K))
    img1[K // 2] = -1
    img2 = [(-1, HW, HW + 7, -5)[j % 4] for j in range(K)]
    return np.array([img0, img1, img2], dtype=np.int32)


def tables_numpy(list_a, list_b, K):
    """restatement of cf_head_slot_tables: table_ab [B][ceil(2K/18)][18] = list_a then list_b, table_b [B][ceil(K/18)][18] = list_b;
    entry v of image b -> b * HW + v if 0 <= v < HW, else -1; padding -1"""
    def flat(v, b):
        return np.where((v >= 0) & (v < HW), b * HW + v, -1).astype(np.int32)
    n_ab, n_b = -(-2 * K // 18) * 18, -(-K // 18) * 18
    t_ab, t_b = np.full((B, n_ab), -1, np.int32), np.full((B, n_b), -1, np.int32)
    for b in range(B):
        if list_a is not None:
            t_ab[b, :K] = flat(list_a[b].astype(np.int64), b)
        if list_b is not None:
            t_ab[b, K:2 * K] = flat(list_b[b].astype(np.int64), b)
            t_b[b, :K] = flat(list_b[b].astype(np.int64), b)
    return t_ab, t_b


def slot_tables(dev, list_a, list_b, K, want_ab=True, want_b=True):
    from centerfusiondetect3d_amd import _lib
    lib = _lib.load()
    la = torch.from_numpy(list_a).to(dev) if list_a is not None else None
    lb = torch.from_numpy(list_b).to(dev) if list_b is not None else None
    t_ab = torch.full((B * -(-2 * K // 18) * 18,), 12345, device=dev, dtype=torch.int32) if want_ab else None
    t_b = torch.full((B * -(-K // 18) * 18,), 12345, device=dev, dtype=torch.int32) if want_b else None
    _lib.check(lib.cf_head_slot_tables(_lib.ptr(la), _lib.ptr(lb), B, K, HW, _lib.ptr(t_ab), _lib.ptr(t_b), _lib.stream_ptr()),
               "cf_head_slot_tables")
    return t_ab, t_b


@gpu
@pytest.mark.parametrize("K", KS)
def test_slot_tables_match_the_numpy_restatement(dev, K):
    a, b = pixel_lists(K, seed=1), pixel_lists(K, seed=2)
    for la, lb in ((a, b), (None, b)):
        t_ab, t_b = slot_tables(dev, la, lb, K)
        r_ab, r_b = tables_numpy(la, lb, K)
        assert np.array_equal(t_ab.cpu().numpy().reshape(B, -1), r_ab)
        assert np.array_equal(t_b.cpu().numpy().reshape(B, -1), r_b)
    t_ab, none = slot_tables(dev, a, None, K, want_b=False)       # list_a alone: the second half of each image stays empty
    assert none is None and np.array_equal(t_ab.cpu().numpy().reshape(B, -1), tables_numpy(a, None, K)[0])
    none, t_b = slot_tables(dev, None, b, K, want_ab=False)
    assert none is None and np.array_equal(t_b.cpu().numpy().reshape(B, -1), tables_numpy(None, b, K)[1])


def test_entry_points_refuse_bad_arguments():
    from centerfusiondetect3d_amd import _lib
    lib = _lib.load()
    f = _lib.HeadFusedArgs()
    assert lib.cf_head_fused_at(C.byref(f), None, 4, None) == -22 and b"slot table" in lib.cf_last_error()
    assert lib.cf_head_fused_at(None, None, 4, None) == -22
    assert lib.cf_head_slot_tables(None, None, 1, 100, HW, None, None, None) == -22 and b"no list" in lib.cf_last_error()
    assert lib.cf_head_slot_tables(None, None, 0, 100, HW, None, None, None) == -22
    assert lib.cf_head_slot_tables(None, None, 1 << 20, 100, 1 << 12, None, None, None) == -22 and b"2^31" in lib.cf_last_error()


# ------------------------------------------------------------------------------------------------ the launch, per form
def _weights(i, n_hidden, no):
    w1, b1 = rnd(256, 67, 3, 3, seed=300 + i, scale=(67 * 9) ** -0.5), rnd(256, seed=310 + i, scale=0.1)
    hid = [(rnd(256, 256, 1, 1, seed=10 * i + l, scale=1 / 16), rnd(256, seed=50 + 10 * i + l, scale=0.1)) for l in range(n_hidden)]
    return w1, b1, hid, rnd(no, 256, 1, 1, seed=100 + i, scale=1 / 16), rnd(no, seed=200 + i)


def _packed_heads(dev, mx, pc, n_hidden, n_heads):
    from centerfusiondetect3d_amd import packing
    heads, slots, k_pad = [], None, 0
    for i, (no, act) in enumerate(zip(N_OUTS[:n_heads], ACTS[:n_heads])):
        w1, b1, hid, w, b = _weights(i, n_hidden, no)
        if not pc:
            w1 = w1[:, :64].contiguous()
        if mx:
            d = packing.pack_head_first_mx(w1, b1, pc)
            first = dict(w_first=d["w_first"].to(dev), b_first=d["b_first"].to(dev), first_scale=d["first_scale"])
        else:
            p = packing.pack_conv_bf16(w1, b1, [packing.Source(64, 64)] + ([packing.Source(3, 8)] if pc else [])).to(dev)
            slots, k_pad = p.slots, p.k_pad
            first = dict(w_first=p.weight, b_first=p.bias[:256].contiguous())
        b32 = torch.zeros(32)
        b32[:no] = b
        heads.append(dict(first, w_hidden=[packing.pack_fragments16(wl.view(256, 256)).to(dev) for wl, _ in hid],
                          b_hidden=[bl.to(dev) for _, bl in hid], w_out=packing.pack_fragments16(w.view(no, 256)).to(dev),
                          b_out=b32.to(dev), w_out_perm=packing.pack_fragments16(w.view(no, 256), acc_order=True).to(dev),
                          mfma16=True, n_out=no, act=act))
    return heads, slots, k_pad


def _inputs():
    """features; a pc_hm map that is non-zero in a block of image 0 (around some of its listed pixels, not others) and of image
    2, and all zero in image 1: virtual tiles with and without the radar k-step in one launch"""
    feat, pch = F.relu(rnd(B, 64, H, W, seed=1)) * 3.0, rnd(B, 3, H, W, seed=2) * 20.0
    keep = torch.zeros(B, 1, H, W)
    keep[0, :, 8:20, 10:30] = 1.0
    keep[2] = 1.0
    return feat, pch * keep


# (mx, pc_hm source, hidden layers, heads in the block): the model's four forms, the chained early-fusion form (bf16x3, hidden,
# one source), the radar source without hidden layers, and 1 / 2 / 6 heads where a workgroup walks several heads on one patch
FORMS = [(True, False, 0, 1), (True, False, 0, 2), (True, False, 0, 6), (False, False, 0, 1), (False, False, 0, 2),
         (False, False, 0, 6), (True, True, 2, 2), (False, True, 2, 2), (False, False, 2, 2), (False, True, 0, 6)]


@gpu
@pytest.mark.parametrize("mx,pc,n_hidden,n_heads", FORMS)
def test_listed_pixels_get_the_dense_bits_and_nothing_else_is_written(dev, mx, pc, n_hidden, n_heads):
    from centerfusiondetect3d_amd import _lib, ops
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
    for K in KS:
        lists = pixel_lists(K)
        other = pixel_lists(K, seed=3)
        for la, lb in ((None, lists), (other, lists)) if K in (19, 100) else ((None, lists),):
            t_ab, t_b = slot_tables(dev, la, lb, K)
            table = t_b if la is None else t_ab
            listed = torch.zeros(B, HW, dtype=torch.bool)
            for l in (la, lb):
                if l is not None:
                    for b in range(B):
                        ok = l[b][(l[b] >= 0) & (l[b] < HW)]
                        listed[b, torch.from_numpy(ok.astype(np.int64))] = True
            assert int(listed[2].sum()) == 0 and int(listed[0].sum()) >= 1
            for m in maps:
                m.fill_(float("nan"))
            _lib.check(lib.cf_head_fused_at(C.byref(f), table.data_ptr(), table.numel() // 18, _lib.stream_ptr()), "cf_head_fused_at")
            sel = listed.to(dev)
            for m, d in zip(maps, dense):
                n = m.shape[1]
                got, want = m.view(B, n, HW).transpose(1, 2), d.view(B, n, HW).transpose(1, 2)     # (B, HW, n)
                assert torch.equal(got[sel], want[sel]), (K, la is not None, n)
                assert bool(torch.isnan(got[~sel]).all()), (K, la is not None, n)


# ------------------------------------------------------------------------------------------------ through the model
MH, MW = 4 * H, 4 * W                                         # 128 x 160 input -> the 32 x 40 map


def _model(dev, kind, at):
    from centerfusiondetect3d_amd import getModel, centerfusion_middle_config, centernet_config, centerfusion_early_config
    from tests.golden import cases
    if kind == "early":
        from tests.golden.make_golden_early import early_state_dict
        m = getModel(centerfusion_early_config((MH, MW)))
        m.load_state_dict(early_state_dict(0), strict=True)
    else:
        radar = kind != "camera"
        cfg = (centerfusion_middle_config if radar else centernet_config)((MH, MW))
        if kind == "nofrustum":
            cfg.MODEL.FRUSTUM = False
        m = getModel(cfg)
        m.load_state_dict(cases.tuned_state_dict(radar=radar, seed=0), strict=True)
    assert m.heads_at_peaks is True                            # the default
    m.heads_at_peaks = at
    return m.to(dev).eval()


def _forward(m, dev, kind, seed):
    """(the radar map is normalised in place without frustum association: every forward gets its own copy)"""
    from tests.golden import cases
    x, pc_dep, calib = cases.model_inputs(B, MH, MW, seed=seed, radar=True)
    kw = dict(calib=calib.to(dev))
    if kind != "camera":
        kw["pc_dep"] = pc_dep.to(dev)
    with torch.no_grad():
        return m(x.to(dev), **kw), kw["calib"]


def _decode(out, calib, dev, K=100):
    """-> [det (B,K,33), post (B,K,54) where the head set is complete]"""
    from centerfusiondetect3d_amd import decode_packed, decode_post_packed
    from centerfusiondetect3d_amd.postprocess import inverse_affine
    res = [decode_packed(out, (H, W), K=K)[0]]
    tinv = torch.from_numpy(inverse_affine(np.array([MW / 2, MH / 2], np.float32), float(max(MH, MW)), (W, H))).to(dev)
    try:
        res.append(decode_post_packed(out, calib, tinv, (H, W), K=K))
    except NotImplementedError:                                # (camera-only: no velocity / attribute heads)
        pass
    return res


def _clones(y):
    return {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in dict.items(y)}


def _same_maps(got, want):
    assert list(got.keys()) == list(want.keys())
    for k in want:
        if isinstance(want[k], torch.Tensor):
            assert torch.equal(got[k], want[k]), k


@gpu
@pytest.mark.parametrize("kind", ["middle", "nofrustum", "camera", "early"])
def test_model_at_peaks_equals_the_dense_forward(dev, kind):
    from centerfusiondetect3d_amd.pending import PendingOutputs
    m_at, m_dn = _model(dev, kind, True), _model(dev, kind, False)
    # the dense model: plain dicts, decoded rows of both inputs
    dn1, cal1 = _forward(m_dn, dev, kind, 4)
    assert type(dn1[0]) is dict
    keys = list(dn1[0].keys())
    ref1 = _clones(dn1[0])
    rows1 = _decode(dn1, cal1, dev)
    rows1_k = _decode([_clones(ref1)], cal1, dev, K=50)
    dn2, cal2 = _forward(m_dn, dev, kind, 5)
    rows2 = _decode(dn2, cal2, dev)
    # at the peaks: pending outputs with the same keys; decode leaves them pending and gives the same rows
    at1, _ = _forward(m_at, dev, kind, 4)
    y = at1[0]
    assert isinstance(y, PendingOutputs) and y.pending and list(y.keys()) == keys
    launched = [st[0].__name__ for plan in m_at._all_plans() for st in plan.steps if st and not isinstance(st[0], str)]
    assert launched.count("cf_head_fused") == (1 if kind == "camera" else 2)     # the plan's own steps stay the dense ones
    rows = _decode(at1, cal1, dev)
    assert y.pending
    assert len(rows) == len(rows1) and all(torch.equal(a, b) for a, b in zip(rows, rows1))
    if "pc_hm" in keys:
        assert torch.equal(y.peek("pc_hm"), dn1[0]["pc_hm"])
    # further forwards with other inputs while the first outputs are still held and unread: they stay pending (the forward
    # copies the operand buffers their dense launches read) and are the first inputs' maps when they are read at last
    at2, _ = _forward(m_at, dev, kind, 5)
    assert y.pending and at2[0].pending
    assert all(torch.equal(a, b) for a, b in zip(_decode(at2, cal2, dev), rows2))
    # another K: the forward's peaks do not cover it - the maps are completed before the decode
    at3, _ = _forward(m_at, dev, kind, 4)
    assert y.pending and at2[0].pending and at3[0].pending
    _same_maps(y, dn1[0])                                      # (both decoded: rotation2 renamed in both)
    assert not y.pending
    _same_maps(at2[0], dn2[0])                                 # (released when the third forward started)
    assert all(torch.equal(a, b) for a, b in zip(_decode(at3, cal1, dev, K=50), rows1_k))
    assert not at3[0].pending
    # a write into the heat map between forward and decode (reading the tensor completes the maps)
    at4, _ = _forward(m_at, dev, kind, 4)
    at4[0]["heatmap"].data[1, 3, 5, 7] = 0.99
    assert not at4[0].pending
    plain = _clones(ref1)
    plain["heatmap"][1, 3, 5, 7] = 0.99
    assert all(torch.equal(a, b) for a, b in zip(_decode(at4, cal1, dev), _decode([plain], cal1, dev)))
    # reading every map of fresh pending outputs: the dense maps; dict(y) copies completed maps
    at5, _ = _forward(m_at, dev, kind, 4)
    d = dict(at5[0])
    assert not at5[0].pending and type(d) is dict
    _same_maps(d, ref1)


@gpu
def test_pending_outputs_outlive_the_model_and_write_nothing_they_do_not_own(dev):
    """The dense launches of a late read need the plan's buffers, the packed weights and EVERY tensor they write - also the raw
    `depth` logits a radar model does not hand out: all of them stay alive with the pending dict, so a read after the model is
    gone gives the dense maps and touches no memory that was handed to someone else in between."""
    import gc
    y = _forward(_model(dev, "middle", True), dev, "middle", 4)[0][0]          # (the model and its plans are dropped here)
    ref = _forward(_model(dev, "middle", False), dev, "middle", 4)[0][0]
    gc.collect()
    junk = [torch.full((B, c, H, W), 7.0, device=dev) for c in (1, 2, 3, 8, 10) for _ in range(6)]   # takes freed blocks of these sizes
    assert y.pending
    maps = dict(y)
    torch.cuda.synchronize()
    _same_maps(maps, ref)
    assert all(float(j.min()) == 7.0 == float(j.max()) for j in junk)
