"""Argument blocks for the host-only form exports of the split-fp16 launchers (cf_conv3x3_tile_form, cf_dcn_v2_f16x3_form) and
the rows they are asked about (tests/test_f16x3_forms_cpu.py, tests/golden/make_f16x3_forms.py).

The exports validate a block as the launch does and read no memory behind its pointers, so every buffer here is a dummy
non-null address.  A conv row is (entry, B, H, W, Ci, N, stride, G, extra):
    entry 0  cf_conv3x3_f16x3          extra = 1: with a residual
    entry 1  cf_conv3x3_root_f16x3     Ci = N = the Tree's channels; extra = number of 64-channel children (or their channels)
    entry 2  cf_conv3x3_proj_f16x3     extra = channels of the projected tensor
    entry 3  cf_conv3x3_f16x3_grouped  G groups
a DCN row (B, H, W, C, N, G, workspace): G groups (1: cf_dcn_v2_f16x3), workspace = 1: the K split may be taken."""
import ctypes as C

from centerfusiondetect3d_amd import _lib, ops

PLAIN, ROOT, PROJ, GROUPED = 0, 1, 2, 3
ENTRY_NAMES = {PLAIN: "plain", ROOT: "root", PROJ: "proj", GROUPED: "grouped"}
REFUSED = -22                                     # CF_EINVAL
P = 0x10000000                                    # dummy device addresses, 256 MiB apart
X, X2, WGT, BIAS, SLOTS, RES, OUT, ROOT_OUT, WS, OM = (P * i for i in range(1, 11))
KIDS = (P * 11, P * 12)


def conv_n_pad(n):
    """packing.pack_conv_f16's padding"""
    return 32 if n <= 32 else -(-n // 64) * 64


def _conv_block(B, H, W, Ci, N, stride=1, residual=False, proj=0, out=OUT, out_stride=None):
    a = _lib.ConvArgs()
    a.src[0], a.src_c[0], a.n_src = X, Ci, 1
    slices = Ci // 16
    a.K_pad = -(-slices * 144 // 32) * 32
    if proj:
        a.src[1], a.src_c[1], a.n_src = X2, proj, 2
        a.K_pad = slices * 144 + proj
    a.B, a.H, a.W, a.stride = B, H, W, stride
    a.Ho, a.Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    a.weight, a.slots, a.bias = WGT, SLOTS, BIAS
    a.N, a.N_pad = N, conv_n_pad(N)
    a.out_stride = out_stride or -(-N // 4) * 4
    a.out, a.out_layout, a.act, a.out_scale = out, _lib.LAYOUT_NHWC, _lib.ACT_RELU, 2.0 ** -18
    if residual:
        a.residual, a.res_stride = RES, a.out_stride
    return a


def conv_call(row):
    """-> (entry name, blocks, channels) of one conv row: the arguments of ops.conv3x3_tile_form"""
    entry, B, H, W, Ci, N, stride, G, extra = row
    if entry == PLAIN:
        return "plain", [_conv_block(B, H, W, Ci, N, stride, bool(extra))], None
    if entry == ROOT:
        kids = (64,) * extra if isinstance(extra, int) else tuple(extra)
        a = _conv_block(B, H, W, Ci, N, 1, True)
        r = _conv_block(B, H, W, 16, N, 1, False, out=ROOT_OUT)
        chans = [N, N, *kids]
        r.n_src = len(chans)
        r.src[0], r.src[1], r.src_c[0], r.src_c[1] = a.out, a.residual, a.out_stride, a.res_stride
        for i, c in enumerate(kids):
            r.src[2 + i], r.src_c[2 + i] = KIDS[i], c
        r.K_pad = sum(chans)
        return "root", [a, r], chans
    if entry == PROJ:
        return "proj", [_conv_block(B, H, W, Ci, N, 1, False, proj=extra)], [Ci, extra]
    M = B * H * W
    return "grouped", [_conv_block(B, H, W, Ci, N, 1, False, out=OUT + 4 * g * M * 32, out_stride=32) for g in range(G)], None


def conv_form(row):
    """cf_conv3x3_tile_form's answer for a conv row as a tuple in ops.CONV3_FORM_FIELDS order, or REFUSED"""
    entry, blocks, channels = conv_call(row)
    try:
        return tuple(ops.conv3x3_tile_form(entry, blocks, channels).values())
    except _lib.CfHipError:
        return REFUSED


def dcn_blocks(row):
    B, H, W, Cc, N, G, ws = row
    M, out_stride = B * H * W, -(-N // 4) * 4
    blocks = []
    for g in range(G):
        a = _lib.DcnArgs()
        a.x, a.offmask, a.om_stride = X, OM + 4 * g * M * 32, 32
        a.B, a.H, a.W, a.C = B, H, W, Cc
        a.weight, a.bias, a.N, a.N_pad = WGT, BIAS, N, -(-N // 32) * 32          # (packing.pack_dcn_f16's padding)
        a.out, a.out_stride, a.act, a.out_scale = OUT + 4 * g * M * out_stride, out_stride, _lib.ACT_RELU, 2.0 ** -18
        if ws:
            a.workspace, a.workspace_bytes = WS, 1 << 40
        blocks.append(a)
    return blocks


def dcn_form(row):
    """cf_dcn_v2_f16x3_form's answer for a DCN row as a tuple in ops.DCN_FORM_FIELDS order, or REFUSED"""
    try:
        return tuple(ops.dcn_v2_f16x3_form(dcn_blocks(row)).values())
    except _lib.CfHipError:
        return REFUSED
