"""GPU: the grouped launches of the neck (cf_conv3x3_f16x3_grouped, cf_dcn_v2_f16x3_grouped, model.neck_groups) against the
ungrouped launches they replace.  A group changes no arithmetic, no K order and no tile form that enters a sum, so every
comparison here is bit for bit (torch.equal)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.golden import cases


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X box"
    from centerfusiondetect3d_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _offset_convs(dev, G, B, H, W, Ci, seed):
    from centerfusiondetect3d_amd import ops, packing
    pcs = [packing.pack_conv_f16(rnd(27, Ci, 3, 3, seed=seed + 10 * g, scale=(Ci * 9) ** -0.5), rnd(27, seed=seed + 10 * g + 1),
                                 [packing.Source(Ci, Ci)]).to(dev) for g in range(G)]
    assert all(pc.patch and pc.n_pad == 32 for pc in pcs)
    xs = [rnd(B, H, W, Ci, seed=seed + 10 * g + 2).to(dev) for g in range(G)]
    out = torch.full((G, B, H, W, 32), float("nan"), device=dev)
    blocks = [ops.conv_args(pc, [x], [Ci], B, H, W, out[g], 32, 0, None, 0, 0, None, 0, False) for g, (pc, x) in enumerate(zip(pcs, xs))]
    return pcs, xs, out, blocks


def _check_offset_convs(dev, G, B, H, W, Ci, seed, form):
    from centerfusiondetect3d_amd import ops
    pcs, xs, out, blocks = _offset_convs(dev, G, B, H, W, Ci, seed)
    got = ops.conv3x3_grouped_form(blocks)
    assert {k: got[k] for k in form} == form, got
    ops.conv3x3_f16x3_grouped(pcs, xs, out=out)
    for g in range(G):
        one = torch.full((B, H, W, 32), float("nan"), device=dev)
        ops.conv2d_f16x3(pcs[g], [xs[g]], B, H, W, out=one, patch=True)
        assert torch.equal(out[g, ..., :27], one[..., :27]), (Ci, g)
        assert bool(torch.isnan(out[g, ..., 27:]).all())          # the padding channels of a row are nobody's
    assert not bool(torch.isnan(out[..., :27]).any())


@pytest.mark.parametrize("Ci", [128, 32])
def test_offset_conv_groups_flat_form(dev, Ci):
    """G = 3, B = 2, 13 x 19 maps: M = 494 is no multiple of the tile, so every group's last tile is partial - a tile that ran
    on would write (and its patch would read) the next group's rows.  Flat form with K split over waves (a map below 4096
    pixels; 8 slices: conv3x3_f16x3_kernel_grouped<1,1,4,1,8>, 2 slices: <1,2,2,1,12>).  Each group's rows equal the ungrouped call."""
    form = dict(WC=1, WP=1, WK=4, NU=8, T2=0, CT=2) if Ci == 128 else dict(WC=1, WP=2, WK=2, NU=12, T2=0, CT=2)
    _check_offset_convs(dev, 3, 2, 13, 19, Ci, seed=Ci, form=form)


def test_offset_conv_groups_wk4_small_map(dev):
    """7 x 9 maps, 256 channels (16 slices): the launcher reports conv3x3_f16x3_kernel_grouped<1,1,4,1,8,true,2> - WK = 4, the
    form of the 28 x 50 offset convolutions - and M = 126 fills less than two of its 64-pixel tiles."""
    _check_offset_convs(dev, 3, 2, 7, 9, 256, seed=7, form=dict(WC=1, WP=1, WK=4, NU=8, T2=0, CT=2))


@pytest.mark.parametrize("G,B,H,W,form", [(2, 4, 65, 67, dict(WC=1, WP=4, WK=1, NU=8, T2=0, CT=2)),
                                          (2, 5, 64, 64, dict(WC=1, WP=4, WK=1, NU=6, T2=1, CT=2)),
                                          (2, 1, 64, 64, dict(WC=1, WP=4, WK=1, NU=4, T2=1, CT=1))],
                         ids=["flat_256_pixel_runs", "tiled_8x16", "tiled_small_grid"])
def test_offset_conv_groups_on_maps_of_4096_pixels_and_more(dev, G, B, H, W, form):
    """The forms without a K split (32 channels, maps of 4096+ pixels): the flat 256-pixel runs of the 56 x 100 projections
    (<1,4,1,1,8>; 65 x 67 x 4 frames = 68.05 runs per group: the last one is partial), the 16-wide tiles where they cover the
    map (<1,4,1,1,6,T2>) and their half-height form while the whole grid - all groups - fits one round (<1,4,1,1,4,T2,CT=1>).
    The ungrouped calls choose their tile by their own grid; the tile shape enters no sum, so the rows are equal all the same."""
    _check_offset_convs(dev, G, B, H, W, 32, seed=H + W, form=form)


def _dcn_case(dev, G, B, H, W, Ci, Co, mag, shared, seed):
    from centerfusiondetect3d_amd import packing
    pds = [packing.pack_dcn_f16(rnd(Co, Ci, 3, 3, seed=seed + 10 * g, scale=(Ci * 9) ** -0.5), rnd(Co, seed=seed + 10 * g + 1)).to(dev)
           for g in range(G)]
    xs = [rnd(B, H, W, Ci, seed=seed + 10 * g + 2).to(dev) for g in range(G)]
    for a, b in shared:
        xs[b] = xs[a]                                  # two groups read ONE tensor (ida_2.proj_3 and ida_up.proj_1)
    # offsets as in tests/test_gpu_deform_conv2d.py: normal, scaled so that many samples leave the image; raw mask logits
    om = torch.zeros(G, B, H, W, 32)
    om[..., :27] = rnd(G, B, H, W, 27, seed=seed + 5)
    om[..., :18] *= mag
    return pds, xs, om.to(dev)


def test_dcn_groups_four_members_shared_input(dev):
    """G = 4, 128 -> 64, B = 2, 9 x 14 (M = 252: partial last tiles), groups 2 and 3 on one input pointer: bit-equal to four
    ungrouped calls - with the K split + one reduction over all rows, and without a workspace (no K split)."""
    from centerfusiondetect3d_amd import ops
    pds, xs, om = _dcn_case(dev, 4, 2, 9, 14, 128, 64, 4.0, [(2, 3)], seed=3)
    assert xs[2].data_ptr() == xs[3].data_ptr()
    for k_split in (True, False):
        out = ops.dcn_v2_f16x3_grouped(pds, xs, om, k_split=k_split)
        for g in range(4):
            assert torch.equal(out[g], ops.dcn_v2_fused(pds[g], xs[g], om[g].contiguous(), k_split=k_split)), (k_split, g)


def test_dcn_groups_half_size_tiles(dev):
    """G = 4, 128 -> 64, B = 2, 41 x 52: 66.6 tiles of 64 pixels per group and 267 workgroups in all - past the one-round rule, so
    the grouped launch is dcn_f16x3_kernel_grouped<2,2,1,true,1>, the form of the 56 x 100 projections at bs = 16 (no K split
    above 2048 pixels per image); the ungrouped calls take <4,1,1,true> on their own small grids - same K order, same bits."""
    from centerfusiondetect3d_amd import ops
    pds, xs, om = _dcn_case(dev, 4, 2, 41, 52, 128, 64, 8.0, [(2, 3)], seed=5)
    out = ops.dcn_v2_f16x3_grouped(pds, xs, om)
    for g in range(4):
        assert torch.equal(out[g], ops.dcn_v2_fused(pds[g], xs[g], om[g].contiguous())), g


def test_dcn_groups_k_split_and_reduce(dev):
    """G = 2, 256 -> 128, B = 1, 7 x 10: at most 512 pixels, so the launch splits K (four parts) and the grouped reduction runs once
    over both groups' rows, each with its own bias and scale: bit-equal to the two ungrouped calls including their reductions."""
    from centerfusiondetect3d_amd import _lib, ops
    assert _lib.load().cf_dcn_v2_workspace_bytes(1, 7, 10, 256, 128) == 4 * 70 * 128 * 4
    pds, xs, om = _dcn_case(dev, 2, 1, 7, 10, 256, 128, 6.0, [], seed=11)
    out = ops.dcn_v2_f16x3_grouped(pds, xs, om)
    for g in range(2):
        assert torch.equal(out[g], ops.dcn_v2_fused(pds[g], xs[g], om[g].contiguous())), g


def test_grouped_entry_points_refuse_bad_groups(dev):
    """n_groups = 0 / 5, a null group pointer, and a second output with n_groups > 1: CF_EINVAL, nothing is launched (the
    outputs keep their NaN fill)."""
    from centerfusiondetect3d_amd import _lib, ops
    lib = _lib.load()
    st = _lib.stream_ptr()
    pcs, xs, out, blocks = _offset_convs(dev, 2, 1, 7, 9, 32, seed=1)
    ptrs = ops.group_ptrs(blocks)
    null2 = (C.POINTER(_lib.ConvArgs) * 2)(C.pointer(blocks[0]), None)
    for rc in (lib.cf_conv3x3_f16x3_grouped(ptrs, 0, st), lib.cf_conv3x3_f16x3_grouped(ptrs, 5, st),
               lib.cf_conv3x3_f16x3_grouped(null2, 2, st)):
        assert rc == -22
    pds, dxs, om = _dcn_case(dev, 2, 1, 7, 9, 32, 64, 1.0, [], seed=2)
    dout = torch.full((2, 1, 7, 9, 64), float("nan"), device=dev)
    split = torch.full((1, 7, 9, 2, 64), float("nan"), device=dev, dtype=torch.bfloat16)
    mk = lambda **kw: [ops.dcn_args(pds[g], dxs[g], om[g], 32, 1, 7, 9, dout[g], 64, **(kw if g == 1 else {})) for g in range(2)]
    plain = mk()
    dnull = (C.POINTER(_lib.DcnArgs) * 2)(C.pointer(plain[0]), None)
    with_split, with_mx = mk(out_split=split), mk(out_mx=torch.zeros(1, 7, 9, 272, device=dev, dtype=torch.uint8))
    for rc in (lib.cf_dcn_v2_f16x3_grouped(ops.group_ptrs(plain), 0, st), lib.cf_dcn_v2_f16x3_grouped(ops.group_ptrs(plain), 5, st),
               lib.cf_dcn_v2_f16x3_grouped(dnull, 2, st), lib.cf_dcn_v2_f16x3_grouped(ops.group_ptrs(with_split), 2, st),
               lib.cf_dcn_v2_f16x3_grouped(ops.group_ptrs(with_mx), 2, st)):
        assert rc == -22
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(dout).all()) and bool(torch.isnan(split.float()).all())
    # ... and the same blocks are accepted as they are
    assert lib.cf_conv3x3_f16x3_grouped(ptrs, 2, st) == 0 and lib.cf_dcn_v2_f16x3_grouped(ops.group_ptrs(plain), 2, st) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out[..., :27]).any()) and not bool(torch.isnan(dout).any())


def _kernel_launches(plan):
    """kernel launches of a plan's steps: a DCN step on a K-split map (it has a workspace) is the DCN kernel + its reduction"""
    n = 0
    for st in plan.steps:
        if not st or isinstance(st[0], str):
            continue
        n += 1
        name = st[0].__name__
        if name == "cf_dcn_v2_f16x3" and st[1]._obj.workspace:
            n += 1
        elif name == "cf_dcn_v2_f16x3_grouped" and st[1][0].contents.workspace:
            n += 1
    return n


def test_model_neck_groups_on_and_off(dev):
    """The small CenterFusion model of the goldens (2 x 128 x 160), model.neck_groups on against off, one stream and two: every output
    tensor bit-equal.  `lanes` is off in both arms - with lanes (small batches) the projections keep their own launches on the
    side stream, so there would be nothing to compare.  At this size both sets sit on K-split maps: 8 steps = 12 kernel
    launches fewer per trunk; a trunk plan of the flagship's maps (448 x 800, built, not run) holds the 9 launches fewer."""
    from centerfusiondetect3d_amd import getModel, centerfusion_middle_config
    from centerfusiondetect3d_amd.plan import _Plan
    B, H, W = 2, 128, 160
    x, pc_dep, calib = cases.model_inputs(B, H, W, seed=1, radar=True)
    outs, plans, models = {}, {}, {}
    for groups in (True, False):
        m = getModel(centerfusion_middle_config((H, W)))
        m.neck_groups, m.lanes = groups, False
        m.load_state_dict(cases.tuned_state_dict(radar=True, seed=0), strict=True)
        m = models[groups] = m.to(dev).eval()
        for streams in (1, 2):
            m.streams, m.min_sub_batch = streams, 0
            with torch.no_grad():
                outs[groups, streams] = m(x.to(dev), pc_dep=pc_dep.clone().to(dev), calib=calib.to(dev))[0]
        trunks = [p for k, p in m._plans.items() if "trunk" in k]
        assert len(trunks) == 2                                            # the split path really ran
        plans[groups] = trunks[0]
    names = lambda p: {st[0].__name__ for st in p.steps if st and not isinstance(st[0], str)}
    assert "cf_conv3x3_f16x3_grouped" in names(plans[True]) and "cf_dcn_v2_f16x3_grouped" in names(plans[True])
    assert not any(n.endswith("_grouped") for n in names(plans[False]))
    assert len(plans[False].steps) - len(plans[True].steps) == 8
    assert _kernel_launches(plans[False]) - _kernel_launches(plans[True]) == 12
    assert set(plans[True].step_index) == set(plans[False].step_index)     # every layer keeps its name
    assert sum(plans[True].step_flops.values()) == sum(plans[False].step_flops.values())
    for streams in (1, 2):
        for k, v in outs[False, streams].items():
            if k != "calib":
                assert torch.equal(outs[True, streams][k], v), (streams, k)
    big = {g: _Plan(models[g], 1, 448, 800, dev, part="trunk") for g in (True, False)}
    assert _kernel_launches(big[False]) - _kernel_launches(big[True]) == 9
