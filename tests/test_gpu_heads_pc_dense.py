"""The radar taps of the heads' first layer (cf_head_fused with a pc_hm source): ONE dense 32-deep k-step, k = 3 tap + channel,
read from an operand image the workgroup builds in LDS - and left out altogether by a workgroup whose pc_hm patch (tile +
1-pixel frame) holds nothing but (+-) zeros.  Through the C ABI, both first-layer forms (mx: fp16 + FP6; bf16x3), both tile
orientations, with and without hidden layers.

Bars (tests/test_gpu_heads_mx.py's, unchanged): against the float64 evaluation of the same operands 2e-5 * max|ref| (+ 1e-5 per
hidden layer) - for the mx form that is oracle/mx_emul.py, for bf16x3 (whose split operands carry 16 significant bits: the
operands ARE the fp32 values to 2^-17) float64 torch; against plain fp32 torch 2e-4 * max|ref|; sigmoid heads rtol 1e-4 /
atol 1e-5.  Everything that only moves work (skip on / off, tile orientation, batch sharding) is compared with torch.equal.

Measured on the MI355X, worst head of each case, error vs float64 / vs fp32 (the 3-k-step kernel before this layout in
brackets): mx (2, 2x13x19) 1.33e-5 / 2.19e-5 (1.42e-5 / 2.13e-5), mx (1, 1x8x40) 1.57e-5 / 1.68e-5 (1.56e-5 / 1.66e-5),
mx (0, 1x21x37) 6.05e-6 / 8.82e-6 (6.05e-6 / 8.72e-6), bf16x3 (2, 2x13x19) 1.55e-5 / 1.53e-5 (the same), bf16x3 (0, 1x21x37)
8.49e-6 / 8.52e-6 (the same); every head: docs/experiments/heads_pc_dense_ab.txt."""
import pytest
import torch
import torch.nn.functional as F

from oracle import mx_emul

gpu = pytest.mark.gpu
N_OUTS, ACTS = (10, 1, 3, 8), (2, 3, 0, 0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _weights(i, n_hidden, no):
    """head i's layers (the seeds of tests/test_gpu_heads_mx.py::_heads_case)"""
    w1, b1 = rnd(256, 67, 3, 3, seed=300 + i, scale=(67 * 9) ** -0.5), rnd(256, seed=310 + i, scale=0.1)
    hid = [(rnd(256, 256, 1, 1, seed=10 * i + l, scale=1 / 16), rnd(256, seed=50 + 10 * i + l, scale=0.1)) for l in range(n_hidden)]
    return w1, b1, hid, rnd(no, 256, 1, 1, seed=100 + i, scale=1 / 16), rnd(no, seed=200 + i)


_packed = {}


def _packed_heads(dev, mx, n_hidden):
    """the packed weights of the four heads, once per (form, depth): every case of this file runs the same heads"""
    from centerfusiondetect3d_amd import packing
    key = (mx, n_hidden)
    if key not in _packed:
        heads, slots, k_pad = [], None, 0
        for i, (no, act) in enumerate(zip(N_OUTS, ACTS)):
            w1, b1, hid, w, b = _weights(i, n_hidden, no)
            if mx:
                d = packing.pack_head_first_mx(w1, b1, True)
                first = dict(w_first=d["w_first"].to(dev), b_first=d["b_first"].to(dev), first_scale=d["first_scale"])
            else:
                pc = packing.pack_conv_bf16(w1, b1, [packing.Source(64, 64), packing.Source(3, 8)]).to(dev)
                slots, k_pad = pc.slots, pc.k_pad
                first = dict(w_first=pc.weight, b_first=pc.bias[:256].contiguous())
            b32 = torch.zeros(32); b32[:no] = b
            heads.append(dict(first, w_hidden=[packing.pack_fragments16(wl.view(256, 256)).to(dev) for wl, _ in hid],
                              b_hidden=[bl.to(dev) for _, bl in hid], w_out=packing.pack_fragments16(w.view(no, 256)).to(dev),
                              b_out=b32.to(dev), w_out_perm=packing.pack_fragments16(w.view(no, 256), acc_order=True).to(dev),
                              mfma16=True, n_out=no, act=act))
        _packed[key] = (heads, slots, k_pad)
    return _packed[key]


def _inputs(B, H, W):
    feat, pch = F.relu(rnd(B, 64, H, W, seed=1)) * 3.0, rnd(B, 3, H, W, seed=2) * 20.0
    feat[:, :, 0, :3] = 0.0
    return feat, pch


def _launch(dev, mx, n_hidden, feat, pch):
    """-> run(tile=None, pc_skip=None): launches the four heads on (feat, pch), with that tile orientation / skip forced, and
    returns every output map (out of each head, then the out2 maps)"""
    from centerfusiondetect3d_amd import ops
    B, _, H, W = feat.shape
    packed, slots, k_pad = _packed_heads(dev, mx, n_hidden)
    heads = [dict(hd, out=torch.empty(B, hd["n_out"], H, W, device=dev),
                  out2=torch.empty(B, hd["n_out"], H, W, device=dev) if hd["act"] == 3 else None) for hd in packed]
    src0 = ops.pack_feat_mx(nhwc(feat).to(dev)) if mx else ops.split_bf16(nhwc(feat).to(dev))
    srcs = [src0, ops.split_bf16(nhwc(pch).to(dev), cs=8)]
    f = ops.head_fused_args(srcs, [64, 8], slots, k_pad, B, H, W, heads)
    assert f.mx == int(mx) and f.mfma16 == 1 and f.layout3x3 == 1 and f.n_src == 2
    f._keep = srcs

    def run(tile=None, pc_skip=None):
        for hd in heads:
            hd["out"].fill_(float("nan"))
            if hd["out2"] is not None:
                hd["out2"].fill_(float("nan"))
        ops.run_head_fused(f, tile=tile, pc_skip=pc_skip)
        return [hd["out"].clone() for hd in heads] + [hd["out2"].clone() for hd in heads if hd["out2"] is not None]
    return run


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _refs(mx, n_hidden, feat, pch):
    """per head (float64 evaluation of the form's own operands, fp32 torch)"""
    out = []
    for i, no in enumerate(N_OUTS):
        w1, b1, hid, w, b = _weights(i, n_hidden, no)
        xin = torch.cat([feat, pch], 1)
        x64 = torch.relu(mx_emul.first_layer_mx(feat, pch, w1, b1) if mx else F.conv2d(xin.double(), w1.double(), b1.double(), 1, 1))
        x32 = F.relu(F.conv2d(xin, w1, b1, 1, 1))
        for wl, bl in hid:
            x64 = torch.relu(F.conv2d(x64, wl.double(), bl.double()))
            x32 = F.relu(F.conv2d(x32, wl, bl))
        out.append((F.conv2d(x64, w.double(), b.double()), F.conv2d(x32, w, b)))
    return out


@gpu
@pytest.mark.parametrize("mx,n_hidden,B,H,W", [
    (True, 2, 2, 13, 19),        # hidden layers: both 64-pixel halves, ragged tiles, two frames
    (True, 1, 1, 8, 40),
    (True, 0, 1, 21, 37),        # output layer from the registers, ragged in both directions
    (False, 2, 2, 13, 19),
    (False, 0, 1, 21, 37),
])
def test_dense_pc_step_against_float64(dev, mx, n_hidden, B, H, W):
    """dense random pc_hm (x 20): every tile runs the radar k-step; both tile orientations give the same bits"""
    feat, pch = _inputs(B, H, W)
    run = _launch(dev, mx, n_hidden, feat, pch)
    flat = run(tile=0)
    assert _same(flat, run(tile=1))
    outs = run()
    assert _same(flat, outs)
    out2 = iter(outs[len(N_OUTS):])
    for (r64, r32), got, no, act in zip(_refs(mx, n_hidden, feat, pch), outs, N_OUTS, ACTS):
        got = got.cpu().double()
        assert bool(torch.isfinite(got).all())
        if act == 2:
            torch.testing.assert_close(got, torch.clamp(torch.sigmoid(r64), 1e-4, 1 - 1e-4), rtol=1e-4, atol=1e-5)
            continue
        scale = float(r64.abs().max())
        e_emul = float((got - r64).abs().max()) / scale
        e_fp32 = float((got - r32.double()).abs().max()) / scale
        print(f"[pc dense {'mx' if mx else 'bf16x3'} n_hidden {n_hidden} {B}x{H}x{W}] n_out {no:2d}: vs float64 of the operands "
              f"{e_emul:.2e}, vs fp32 torch {e_fp32:.2e}")
        assert e_emul < 2e-5 + 1e-5 * n_hidden, e_emul
        assert e_fp32 < 2e-4, e_fp32
        if act == 3:
            torch.testing.assert_close(next(out2).cpu().double(), 1.0 / (torch.sigmoid(r64) + 1e-6) - 1.0, rtol=1e-3, atol=1e-3)


FORMS = [(mx, n_hidden) for mx in (True, False) for n_hidden in (0, 2)]
H3, W3 = 16, 48                  # two rows of three 8 x 16 tiles / one row of six 16 x 8 tiles


def _skip_on_off(run):
    """every output with the skip off and on, for both tile orientations: all equal; -> the outputs"""
    first = None
    for tile in (0, 1):
        off = run(tile=tile, pc_skip=0)
        on = run(tile=tile)
        assert _same(off, on), f"skip on != skip off (tile orientation {tile})"
        first = first or off
        assert _same(first, off)
    return first


@gpu
@pytest.mark.parametrize("mx,n_hidden", FORMS)
def test_skip_equals_no_skip(dev, mx, n_hidden):
    """pc_hm non-zero in x = 20..27 only: the middle 8 x 16 tile column is live, the outer two - whose frame columns x = 16 and
    x = 31 are zero - are empty"""
    feat, pch = _inputs(1, H3, W3)
    pch[..., :20] = 0.0
    pch[..., 28:] = 0.0
    outs = _skip_on_off(_launch(dev, mx, n_hidden, feat, pch))
    assert all(bool(torch.isfinite(o).all()) for o in outs)


@gpu
@pytest.mark.parametrize("mx,n_hidden", FORMS)
def test_a_value_in_the_frame_keeps_the_tile(dev, mx, n_hidden):
    """one non-zero pc_hm value at (y 3, x 16): the left 8 x 16 tile holds it in its frame only and must run the radar taps -
    its pixels (2..4, 15) see it"""
    feat, pch = _inputs(1, H3, W3)
    pch.zero_()
    pch[0, :, 3, 16] = torch.tensor([20.0, -7.0, 3.0])
    outs = _skip_on_off(_launch(dev, mx, n_hidden, feat, pch))
    zero = _launch(dev, mx, n_hidden, feat, torch.zeros_like(pch))()
    for o, z, act in zip(outs, zero, ACTS):
        if act == 0:                                           # raw outputs: nothing squashes the difference
            assert bool((o[0, :, 2:5, 15] != z[0, :, 2:5, 15]).any(0).all()), "the frame's value did not reach the tile"
            assert torch.equal(o[0, :, :, :14], z[0, :, :, :14]) and torch.equal(o[0, :, 6:, :], z[0, :, 6:, :])


@gpu
@pytest.mark.parametrize("mx,n_hidden", FORMS)
def test_zero_maps_of_either_sign(dev, mx, n_hidden):
    feat, pch = _inputs(1, H3, W3)
    res = []
    for z in (-0.0, 0.0):
        outs = _skip_on_off(_launch(dev, mx, n_hidden, feat, torch.full_like(pch, z)))
        assert all(bool(torch.isfinite(o).all()) for o in outs)
        res.append(outs)
    assert _same(*res)


@gpu
@pytest.mark.parametrize("mx", [True, False])
def test_batch_equals_single_frames(dev, mx):
    feat, pch = _inputs(3, 13, 19)
    pch[1] = 0.0                                               # one frame without radar: all of its tiles are empty
    full = _launch(dev, mx, 2, feat, pch)()
    for b in range(3):
        one = _launch(dev, mx, 2, feat[b:b + 1].clone(), pch[b:b + 1].clone())()
        assert _same([o[b:b + 1] for o in full], one), b


# ------------------------------------------------------------------------------------------------ packers (no GPU)
def _bf16_pair(w):
    hi = w.to(torch.bfloat16)
    return hi, (w - hi.float()).to(torch.bfloat16)


def test_packers_place_the_radar_weights_in_one_dense_k_step():
    """W[o, 64 + c, ty, tx] sits at k = 3 (3 ty + tx) + c of the fragment row o's lanes load: lane 16 (k >> 3) + (o & 15), element
    k & 7 of row tile o >> 4; k = 27..31 are zero; the streams have the documented lengths"""
    from centerfusiondetect3d_amd import packing
    w, b = rnd(256, 67, 3, 3, seed=7, scale=0.04), rnd(256, seed=8, scale=0.1)
    k = torch.tensor([3 * t + c for t in range(9) for c in range(3)])
    dense = lambda t: t.permute(0, 2, 3, 1).reshape(256, 27)   # (o, k = 3 tap + c)

    # mx stream: the feature slabs, then the pc_hm container [wv 4][ks 3][rt 4][hi, lo][lane 64][8 bf16] of W * 2^s * feat_scale (its
    # length and per-tap positions are what tests/test_oracle_mx.py decodes); the dense k-step is threaded through its padding:
    # lane group 0 in the g = 0 lanes of k-step 0, groups 1-3 in the g = 1..3 lanes of k-step 2
    d = packing.pack_head_first_mx(w, b, True, feat_scale=8.0)
    assert d["w_first"].dtype == torch.uint8 and d["w_first"].numel() == 4 * 9 * packing.MX_SLAB + 4 * 3 * 4 * 2 * 1024
    assert packing.pack_head_first_mx(w[:, :64], b, False)["w_first"].numel() == 4 * 9 * packing.MX_SLAB
    s = round(torch.log2(torch.tensor(1.0 / (d["first_scale"] * 8.0))).item())
    assert d["first_scale"] == 2.0 ** -s / 8.0
    c = d["w_first"][4 * 9 * packing.MX_SLAB:].view(torch.bfloat16).view(4, 3, 4, 2, 4, 16, 8)    # wv, ks, rt, plane, g, i, j
    f = torch.cat([c[:, 0, :, :, :1], c[:, 2, :, :, 1:]], 3)                                     # wv, rt, plane, G, i, j: what a lane loads
    rows = f.permute(2, 0, 1, 4, 3, 5).reshape(2, 256, 32)                                       # plane, o, k = 8 G + j
    hi, lo = _bf16_pair((dense(w[:, 64:]).double() * 2.0 ** s * 8.0).float())
    assert torch.equal(rows[0][:, k], hi) and torch.equal(rows[1][:, k], lo)
    assert not bool(rows[:, :, 27:].float().any())
    taps = c.permute(3, 0, 2, 5, 1, 4, 6).reshape(2, 256, 12, 8)[:, :, :9, :3].reshape(2, 256, 27)   # the per-tap reading still holds
    assert torch.equal(taps[0], hi) and torch.equal(taps[1], lo)

    # bf16x3 fragments [16 rt][n_ks][hi, lo][lane 64][8 bf16]: 18 feature k-steps, the dense radar k-step, padding to K_pad % 64
    pc = packing.pack_conv_bf16(w, b, [packing.Source(64, 64), packing.Source(3, 8)])
    assert pc.k_pad == 640 and tuple(pc.weight.shape) == (16, 20, 2, 64, 8) and pc.slots.shape == (80, 4)
    rows = pc.weight[:, 18].reshape(16, 2, 4, 16, 8).permute(1, 0, 3, 2, 4).reshape(2, 256, 32)
    hi, lo = _bf16_pair(dense(w[:, 64:]))
    assert torch.equal(rows[0][:, k], hi) and torch.equal(rows[1][:, k], lo)
    assert not bool(rows[:, :, 27:].float().any()) and not bool(pc.weight[:, 19].float().any())
    # the feature part is untouched: k-step 2 tap + half holds channels 32 half .. + 32 of that tap
    fr = pc.weight[:, :18].reshape(16, 9, 2, 2, 4, 16, 8).permute(3, 0, 5, 1, 2, 4, 6).reshape(2, 256, 9, 64)
    hi, lo = _bf16_pair(w[:, :64].permute(0, 2, 3, 1).reshape(256, 9, 64))
    assert torch.equal(fr[0], hi) and torch.equal(fr[1], lo)
