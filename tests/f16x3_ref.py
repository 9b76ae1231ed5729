"""Cases and CPU references of the split-fp16 ("f16x3") range tests (tests/test_gpu_f16x3_range.py, tests/test_f16x3_cpu.py).

The f16x3 kernels multiply an activation by a power of two `in_scale`, clamp it to +-65504, split it into fp16 hi + lo
(cf_f16x3.h: split2 / split8), multiply hi and lo with the packer's fp16 hi / lo weights (the lo * lo term is dropped) and undo
both scales in the epilogue.  This module restates that arithmetic in float64 sums on the CPU - the only rounding it keeps is
the split itself - together with the host rule that picks `in_scale` (ops.in_scale_for), the case tables both test files
walk, their seeded inputs and the two error metrics.  No GPU, plain torch."""
import functools
import math

import torch
import torch.nn.functional as F

from oracle import dcn_ref

ACT_NONE, ACT_RELU = 0, 1
F16_MAX = 65504.0
DEFAULT_IN_SCALE = 16.0
CONV_TOL, DCN_TOL = 1e-6, 2e-6                  # relerr gates: test_conv3x3_in_scale_matches_fp32_oracle / test_deform_conv2d_operator_accepts_any_range
CONV_CH_CEILING, DCN_CH_CEILING = 1.5e-6, 5e-6   # no per-channel gate may come out above these (a condition on the inputs)
AMPS = (2.0 ** -24, 2.0 ** -12, 1.0, 2.0 ** 10)
HAZARD_AMP = 2.0 ** -12                         # at this amplitude the default pre-scale must MISS the relerr gate
KS = (-12, 5)                                   # scale invariance: inputs * 2^k, in_scale * 2^-k
GROUP_KS = {2: (-12, 5), 3: (0, -12, 5), 4: (0, -12, 5, 5)}   # ... one k per group of a grouped launch (groups 2 and 3 of the
                                                              # four-member DCN case read ONE tensor: one k for both)
ROOT_ONLY_KS = (-3, 5)                          # the Root's scale alone: x2 keeps its magnitude, so 2^12 would push it into the clamp

# (e, max|x|, error at the default pre-scale 16, error with the pre-scale following the range): max|err| / max|ref| of a 64 -> 32
# 3x3 convolution (float64 sums, exact weights) on x = relu(randn) * 3 * 2^e after the split; torch's fp32 conv: 2.4e-7 on every row
HAZARD_TABLE = ((0, 13.7, 3.9e-8, 3.9e-8), (-8, 5.3e-2, 9.8e-8, 9.8e-8), (-12, 3.3e-3, 1.65e-6, 3.9e-8), (-16, 2.1e-4, 2.6e-5, 3.9e-8),
                (-20, 1.3e-5, 3.8e-4, 3.9e-8), (-24, 8.2e-7, 6.4e-3, 3.9e-8))
HAZARD_FP32 = 2.4e-7


# ------------------------------------------------------------------------------------------------ the host rule, restated
def in_scale_rule(absmax, headroom=8.0):
    """ops.in_scale_for restated on mantissa / exponent: 16 for absmax == 0 and while 2^-6 <= absmax and absmax * 16 <= 65504 / 4;
    otherwise the largest power of two s with absmax * s <= 65504 / headroom, below 2^-6 capped at 2^32."""
    a = float(absmax)
    if a != a or a == float("inf"):
        raise ValueError("not finite")
    if a == 0.0 or (a >= 2.0 ** -6 and a * DEFAULT_IN_SCALE <= F16_MAX / 4.0):
        return DEFAULT_IN_SCALE
    m, e = math.frexp(a)                         # a = m 2^e, 0.5 <= m < 1
    lm, le = math.frexp(F16_MAX / headroom)
    s = 2.0 ** (le - e if m <= lm else le - e - 1)
    return min(s, 2.0 ** 32) if a < 2.0 ** -6 else s


# ------------------------------------------------------------------------------------------------ the split
def split_parts(x, scale):
    """-> (hi, lo) of x * scale as float64: clamp to +-65504, hi = fp16(v), lo = fp16(v - hi), all in fp32 as split2 does"""
    v = (x.float() * float(scale)).clamp(-F16_MAX, F16_MAX)
    hi = v.to(torch.float16)
    lo = (v - hi.float()).to(torch.float16)
    return hi.double(), lo.double()


def split_model(x, scale):
    """What the kernels see of x: (hi + lo) / scale in float64"""
    hi, lo = split_parts(x, scale)
    return (hi + lo) / float(scale)


def weight_exp(*ws):
    """The packer's per-layer weight exponent s (packing.pack_conv_f16 / pack_dcn_f16 / _f16_split): max|w| 2^s in [2^13, 2^14)"""
    wmax = max(float(w.abs().max()) for w in ws)
    return int(torch.floor(torch.log2(torch.tensor(16384.0 / wmax)))) if wmax > 0 else 0


def weight_parts(w, s_exp):
    ws = (w.double() * 2.0 ** s_exp).float()
    hi = ws.to(torch.float16)
    lo = (ws - hi.float()).to(torch.float16)
    return hi.double(), lo.double()


def _conv3(x, w, in_scale, s_exp, stride, pad):
    """conv(x, w) in float64 on split operands without the lo * lo term, scales undone"""
    xh, xl = split_parts(x, in_scale)
    wh, wl = weight_parts(w, s_exp)
    y = F.conv2d(xh, wh, None, stride, pad) + F.conv2d(xh, wl, None, stride, pad) + F.conv2d(xl, wh, None, stride, pad)
    return y / (float(in_scale) * 2.0 ** s_exp)


def _finish(y, b, residual, act):
    if b is not None:
        y = y + b.double().view(1, -1, 1, 1)
    if residual is not None:
        y = y + residual.double()
    return F.relu(y) if act else y


def conv_model(x, w, b, in_scale=DEFAULT_IN_SCALE, stride=1, pad=None, residual=None, act=ACT_NONE, proj=None):
    """The f16x3 convolution (NCHW) in float64 on split operands.  proj = (weight (Co, Cp, 1, 1), bias, pooled): the projection
    summed into the same accumulators - one in_scale and one weight exponent for both parts."""
    pad = w.shape[-1] // 2 if pad is None else pad
    s_exp = weight_exp(w) if proj is None else weight_exp(w, proj[0])
    y = _conv3(x, w, in_scale, s_exp, stride, pad)
    if proj is not None:
        y = y + _conv3(proj[2], proj[0], in_scale, s_exp, 1, 0)
        b = b + proj[1]
    return _finish(y, b, residual, act)


def root_model(t, x1, kids, w2, b2, wr, br, in_scale=DEFAULT_IN_SCALE, root_in_scale=DEFAULT_IN_SCALE):
    """x2 = ReLU(conv3x3(t) + x1) (an fp32 value), out = ReLU(Root([x2, x1, *kids]))"""
    x2 = conv_model(t, w2, b2, in_scale, residual=x1, act=ACT_RELU).float()
    return conv_model(torch.cat([x2, x1, *kids], 1), wr, br, root_in_scale, act=ACT_RELU)


def dcn_model(x, off, mask, w, b, in_scale=DEFAULT_IN_SCALE, act=ACT_NONE):
    """The f16x3 DCN in float64: the bilinear sample times (mask * in_scale) is what the kernel splits."""
    cols, Ho, Wo = dcn_ref.bilinear_columns(x.double(), off.double(), mask.double(), 3, 3, (1, 1), (1, 1), (1, 1))
    B, Cc = x.shape[:2]
    s_exp = weight_exp(w)
    ch, cl = split_parts(cols.reshape(B, Cc * 9, Ho * Wo), in_scale)
    wh, wl = (p.reshape(1, w.shape[0], Cc * 9) for p in weight_parts(w, s_exp))
    y = (torch.matmul(wh, ch) + torch.matmul(wl, ch) + torch.matmul(wh, cl)).view(B, -1, Ho, Wo) / (float(in_scale) * 2.0 ** s_exp)
    return _finish(y, b, None, act)


STEM_LAYERS = ((1, 3), (1, 1), (2, 1))          # (stride, pad) of base_layer, level0, level1


def combine(x, pc):
    """the six-channel image of the early stem: channels 3-5 the radar map, nearest-upsampled to the image size"""
    return torch.cat([x, F.interpolate(pc.to(x.dtype), size=x.shape[-2:], mode="nearest")], dim=1)


def stem_chain(x, w, dtype=torch.float64):
    """base_layer + level0 + level1 (bias + ReLU each) in `dtype` -> (the three layer INPUTS' max |x|, the level1 map)"""
    t, tops = x.to(dtype), []
    for i, (stride, pad) in enumerate(STEM_LAYERS):
        tops.append(float(t.abs().max()))
        t = F.relu(F.conv2d(t, w[2 * i].to(dtype), w[2 * i + 1].to(dtype), stride, pad))
    return tops, t


def stem_model(x, w, in_scales):
    t = x
    for i, (stride, pad) in enumerate(STEM_LAYERS):
        t = conv_model(t, w[2 * i], w[2 * i + 1], in_scales[i], stride, pad, act=ACT_RELU).float()
    return t.double()


# ------------------------------------------------------------------------------------------------ metrics
def relerr(got, ref):
    """max|err| / max|ref|"""
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-300))


def relerr_per_channel(got, ref):
    """NCHW: the worst over output channels of max|err_c| / max|ref_c| - a large channel cannot hide a wrong small one"""
    e = (got.double() - ref.double()).abs().amax(dim=(0, 2, 3))
    r = ref.double().abs().amax(dim=(0, 2, 3))
    if float(r.min()) <= 0:
        return float("inf")                      # a channel of the reference is all zero: the inputs need other seeds
    return float((e / r).max())


# ------------------------------------------------------------------------------------------------ the case tables
# Every launch form the f16x3 entry points are run in off the default pre-scale; a case names the form it is there for.
FORMS = (
    "slot:n_pad32_stride2", "slot:n27_ragged", "slot:residual", "slot:multi_source",
    "patch:wk4", "patch:wk2", "patch:wk1", "patch:residual", "patch:wave_pairs", "patch:512_channels", "patch:forwarded_to_slot",
    "patch:2d", "patch:tiled",
    "patch_s2:odd_sizes", "patch_s2:ragged", "patch_s2:one_slice", "patch_s2:two_channel_blocks",
    "root:fused_half_tiles", "root:fused_children", "root:fused_three_pieces", "root:two_launches", "root:root_scale_only",
    "proj:one_and_a_half_pieces", "proj:second_round", "proj:wave_pairs",
    "grouped_conv:flat_wk4", "grouped_conv:flat_wk2", "grouped_conv:tiled_small_grid",
    "grouped_dcn:k_split_reduce", "grouped_dcn:shared_input_k_split", "grouped_dcn:shared_input_no_split",
    "dcn:k_split_reduce", "dcn:two_row_tiles", "dcn:ragged_64", "dcn:48_of_64_rows",
    "stem:one_tile", "stem:ragged", "stem_early:ragged",
)


def _conv(entry, B, Ci, Co, H, W, stride, act, res, form):
    return dict(entry=entry, B=B, Ci=Ci, Co=Co, H=H, W=W, stride=stride, act=act, res=res, form=form)


# cf_conv2d_f16x3 (slot kernel) and cf_conv3x3_f16x3 (LDS patch, stride 1 and 2): rows of the tables of tests/test_gpu_ops.py
CONV_CASES = {
    "slot_16x32_s2": _conv("slot", 2, 16, 32, 40, 56, 2, 1, False, "slot:n_pad32_stride2"),
    "slot_64x27": _conv("slot", 3, 64, 27, 23, 31, 1, 0, False, "slot:n27_ragged"),
    "slot_128x256_res": _conv("slot", 2, 128, 256, 14, 25, 1, 1, True, "slot:residual"),
    "patch_64x27_wk4": _conv("patch", 3, 64, 27, 23, 31, 1, 0, False, "patch:wk4"),
    "patch_96x27_wk2": _conv("patch", 2, 96, 27, 20, 30, 1, 0, False, "patch:wk2"),
    "patch_48x27_wk1": _conv("patch", 2, 48, 27, 9, 11, 1, 0, False, "patch:wk1"),
    "patch_64x64_res": _conv("patch", 1, 64, 64, 28, 50, 1, 1, True, "patch:residual"),
    "patch_256_wave_pairs": _conv("patch", 2, 256, 256, 14, 25, 1, 1, True, "patch:wave_pairs"),
    "patch_512": _conv("patch", 1, 512, 512, 7, 13, 1, 1, False, "patch:512_channels"),
    "patch_5x300_forwarded": _conv("patch", 14, 64, 64, 5, 300, 1, 1, False, "patch:forwarded_to_slot"),
    "patch_127x127_2d": _conv("patch", 2, 32, 27, 127, 127, 1, 0, False, "patch:2d"),
    "patch_37x150_tiled": _conv("patch", 3, 128, 128, 37, 150, 1, 1, False, "patch:tiled"),
    "s2_32x64_45x67": _conv("patch", 1, 32, 64, 45, 67, 2, 1, False, "patch_s2:odd_sizes"),
    "s2_64x128_17x31": _conv("patch", 3, 64, 128, 17, 31, 2, 1, False, "patch_s2:ragged"),
    "s2_16x64_8x6": _conv("patch", 2, 16, 64, 8, 6, 2, 1, False, "patch_s2:one_slice"),
    "s2_256x512_28x50": _conv("patch", 3, 256, 512, 28, 50, 2, 1, False, "patch_s2:two_channel_blocks"),
}
ROOT_CONCAT_CASE = dict(B=2, H=14, W=25, chans=(128, 128, 64, 128), Co=128, form="slot:multi_source")
# cf_conv3x3_root_f16x3: C, B, H, W, children, form
ROOT_CASES = {
    "root_64_28x50": (64, 1, 28, 50, (), "root:fused_half_tiles"),
    "root_256_children": (256, 1, 28, 50, (128, 256), "root:fused_children"),
    "root_128_one_child": (128, 12, 37, 41, (192,), "root:fused_three_pieces"),
    "root_256_14x25_fallback": (256, 1, 14, 25, (), "root:two_launches"),
}
ROOT_SCALE_ONLY_CASE, ROOT_SCALE_ONLY_FORM = "root_256_children", "root:root_scale_only"
# cf_conv3x3_proj_f16x3: B, Cp, C, H, W, form
PROJ_CASES = {
    "proj_96_64": (3, 96, 64, 45, 67, "proj:one_and_a_half_pieces"),
    "proj_320_256": (2, 320, 256, 31, 23, "proj:second_round"),
    "proj_256_512": (1, 256, 512, 14, 25, "proj:wave_pairs"),
}
# cf_conv3x3_f16x3_grouped: G, B, H, W, Ci, the launcher's form (cf_conv3x3_grouped_form), form
GROUPED_CONV_CASES = {
    "gconv_128": (3, 2, 13, 19, 128, dict(WC=1, WP=1, WK=4, NU=8, T2=0, CT=2), "grouped_conv:flat_wk4"),
    "gconv_32": (3, 2, 13, 19, 32, dict(WC=1, WP=2, WK=2, NU=12, T2=0, CT=2), "grouped_conv:flat_wk2"),
    "gconv_32_64x64": (2, 1, 64, 64, 32, dict(WC=1, WP=4, WK=1, NU=4, T2=1, CT=1), "grouped_conv:tiled_small_grid"),
}
# cf_dcn_v2_f16x3_grouped: G, B, H, W, Ci, Co, offset magnitude, shared inputs, k_split, form
GROUPED_DCN_CASES = {
    "gdcn_256_128": (2, 1, 7, 10, 256, 128, 6.0, (), True, "grouped_dcn:k_split_reduce"),
    "gdcn_shared_split": (4, 2, 9, 14, 128, 64, 4.0, ((2, 3),), True, "grouped_dcn:shared_input_k_split"),
    "gdcn_shared_nosplit": (4, 2, 9, 14, 128, 64, 4.0, ((2, 3),), False, "grouped_dcn:shared_input_no_split"),
}
# cf_dcn_v2_f16x3: B, Ci, Co, H, W, offset magnitude, form
DCN_CASES = {
    "dcn_128_64_ksplit": (1, 128, 64, 14, 25, 8.0, "dcn:k_split_reduce"),
    "dcn_512_256": (1, 512, 256, 7, 13, 1.0, "dcn:two_row_tiles"),
    "dcn_64_64_37x70": (1, 64, 64, 37, 70, 0.5, "dcn:ragged_64"),
    "dcn_32_48": (1, 32, 48, 50, 45, 1.0, "dcn:48_of_64_rows"),
}


def _tile(WC, WP, WK, RT, NU, T2, CT, **more):
    return dict(patch=1, WC=WC, WP=WP, WK=WK, RT=RT, NU=NU, T2=T2, CT=CT, **more)


# The tiling every row above is there for, as the launchers report it (cf_conv3x3_tile_form: ops.CONV3_FORM_FIELDS;
# cf_dcn_v2_f16x3_form: ops.DCN_FORM_FIELDS) - tests/test_f16x3_forms_cpu.py asserts it, so a moved threshold cannot move a case onto
# another kernel unseen.  patch = 0: forwarded to the slot kernel; fused: conv2 + Root as one launch.
CONV_TILINGS = {
    "patch_64x27_wk4": _tile(1, 1, 4, 1, 8, 0, 2), "patch_96x27_wk2": _tile(1, 2, 2, 1, 12, 0, 2), "patch_48x27_wk1": _tile(1, 4, 1, 1, 12, 0, 2),
    "patch_64x64_res": _tile(1, 4, 1, 2, 4, 1, 1), "patch_256_wave_pairs": _tile(2, 1, 2, 2, 4, 0, 1, grid_y=2),
    "patch_512": _tile(2, 1, 2, 2, 4, 0, 1, grid_y=4), "patch_5x300_forwarded": dict(patch=0),
    "patch_127x127_2d": _tile(1, 4, 1, 1, 4, 1, 1), "patch_37x150_tiled": _tile(2, 2, 1, 2, 4, 1, 2),
    "s2_32x64_45x67": _tile(1, 4, 1, 2, 9, 1, 1, S2=1), "s2_64x128_17x31": _tile(2, 2, 1, 2, 5, 1, 1, S2=1),
    "s2_16x64_8x6": _tile(1, 4, 1, 2, 9, 1, 1, S2=1, n_rounds=1), "s2_256x512_28x50": _tile(4, 1, 1, 2, 3, 1, 1, S2=1, grid_y=2),
}
ROOT_TILINGS = {
    "root_64_28x50": _tile(1, 4, 1, 2, 4, 1, 1, fused=1, ROOT=1), "root_256_children": _tile(4, 1, 1, 2, 4, 0, 1, fused=1, ROOT=1),
    "root_128_one_child": _tile(2, 2, 1, 2, 6, 0, 2, fused=1, ROOT=1), "root_256_14x25_fallback": _tile(2, 1, 2, 2, 4, 0, 1, fused=0, ROOT=0),
}
PROJ_TILINGS = {
    "proj_96_64": _tile(1, 4, 1, 2, 4, 1, 1, PROJ=1), "proj_320_256": _tile(4, 1, 1, 2, 4, 0, 1, PROJ=1),
    "proj_256_512": _tile(2, 1, 2, 2, 4, 0, 1, PROJ=1),
}
DCN_TILINGS = {
    "dcn_128_64_ksplit": dict(WC=4, WP=1, RT=1, COAL=1, CT=2, ks=4), "dcn_512_256": dict(WC=4, WP=1, RT=2, COAL=1, CT=2, ks=4),
    "dcn_64_64_37x70": dict(WC=4, WP=1, RT=1, COAL=1, CT=2, ks=1, tiles=41), "dcn_32_48": dict(WC=4, WP=1, RT=1, COAL=1, CT=2, ks=1, grid_y=1),
}

# cf_stem_fused (B, C, H, W) and cf_stem_fused_early (B, H, W)
STEM_CASES = {"stem_16x16": (1, 3, 16, 16, "stem:one_tile"), "stem_34x50": (1, 3, 34, 50, "stem:ragged")}
EARLY_CASES = {"early_36x52": (1, 36, 52, "stem_early:ragged")}

# part B: one row per entry point, the smallest of each
# seeds of the part-B inputs where seed 0 leaves an output channel all zero behind its ReLU (the per-channel metric needs every
# channel alive) or breaks the ceiling of the per-channel gate
SMALL_SEEDS = {"s2_16x64_8x6": 300, "stem_16x16": 200, "early_36x52": 418}
SMALL_CASES = (("conv", "slot_16x32_s2"), ("conv", "patch_48x27_wk1"), ("conv", "s2_16x64_8x6"), ("root", "root_64_28x50"),
               ("proj", "proj_96_64"), ("gconv", "gconv_32"), ("gdcn", "gdcn_256_128"), ("dcn", "dcn_128_64_ksplit"),
               ("stem", "stem_16x16"), ("early", "early_36x52"))


def claimed_forms():
    """every form a case table names, in table order (with repetitions)"""
    out = [c["form"] for c in CONV_CASES.values()] + [ROOT_CONCAT_CASE["form"]]
    out += [c[-1] for c in ROOT_CASES.values()] + [ROOT_SCALE_ONLY_FORM]
    for table in (PROJ_CASES, GROUPED_CONV_CASES, GROUPED_DCN_CASES, DCN_CASES, STEM_CASES, EARLY_CASES):
        out += [c[-1] for c in table.values()]
    return out


# ------------------------------------------------------------------------------------------------ seeded inputs
def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def out_hw(H, W, stride):
    return (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1


def conv_inputs(c, amp=1.0, seed=0):
    """x = relu(randn) * 3 * amp, w, b * amp, residual * amp (or None): the recipe of test_conv3x3_f16x3_patch"""
    Ho, Wo = out_hw(c["H"], c["W"], c["stride"])
    x = F.relu(rnd(c["B"], c["Ci"], c["H"], c["W"], seed=seed + 1)) * 3 * amp
    w = rnd(c["Co"], c["Ci"], 3, 3, seed=seed + 2, scale=(c["Ci"] * 9) ** -0.5)
    b = rnd(c["Co"], seed=seed + 3) * amp
    r = rnd(c["B"], c["Co"], Ho, Wo, seed=seed + 6) * amp if c["res"] else None
    return x, w, b, r


def root_concat_inputs(amp=1.0):
    c = ROOT_CONCAT_CASE
    xs = [F.relu(rnd(c["B"], n, c["H"], c["W"], seed=10 + i)) * 3 * amp for i, n in enumerate(c["chans"])]
    K = sum(c["chans"])
    return xs, rnd(c["Co"], K, 1, 1, seed=20, scale=K ** -0.5), rnd(c["Co"], seed=21) * amp


def root_inputs(case, amp=1.0, seed=0):
    """t, x1, children, (w2, b2), (wr, br): the seeds of test_conv3x3_root_fused_equals_two_launches; amp scales every
    activation and both biases"""
    C_, B, H, W, kids, _ = case
    t, x1 = F.relu(rnd(B, C_, H, W, seed=seed + 1)) * 3 * amp, F.relu(rnd(B, C_, H, W, seed=seed + 2)) * 3 * amp
    ch = [F.relu(rnd(B, c, H, W, seed=seed + 10 + i)) * 3 * amp for i, c in enumerate(kids)]
    K = 2 * C_ + sum(kids)
    w2, b2 = rnd(C_, C_, 3, 3, seed=seed + 3, scale=(C_ * 9) ** -0.5), rnd(C_, seed=seed + 4) * amp
    wr, br = rnd(C_, K, 1, 1, seed=seed + 5, scale=K ** -0.5), rnd(C_, seed=seed + 6) * amp
    return t, x1, ch, (w2, b2), (wr, br)


def proj_inputs(case, amp=1.0, seed=0):
    B, Cp, C_, H, W, _ = case
    t, pooled = F.relu(rnd(B, C_, H, W, seed=seed + 1)) * 3 * amp, F.relu(rnd(B, Cp, H, W, seed=seed + 2)) * 3 * amp
    w2, b2 = rnd(C_, C_, 3, 3, seed=seed + 3, scale=(C_ * 9) ** -0.5), rnd(C_, seed=seed + 4) * amp
    wp, bp = rnd(C_, Cp, 1, 1, seed=seed + 5, scale=Cp ** -0.5), rnd(C_, seed=seed + 6) * amp
    return t, pooled, (w2, b2), (wp, bp)


def grouped_conv_inputs(case, amps, seed=0):
    """per group: x (NCHW), w (27, Ci, 3, 3), b; amps: one amplitude per group"""
    G, B, H, W, Ci = case[:5]
    return [(F.relu(rnd(B, Ci, H, W, seed=seed + 10 * g + 2)) * 3 * amps[g],
             rnd(27, Ci, 3, 3, seed=seed + 10 * g, scale=(Ci * 9) ** -0.5), rnd(27, seed=seed + 10 * g + 1) * amps[g]) for g in range(G)]


def dcn_inputs(B, Ci, Co, H, W, mag, amp=1.0, seed=0):
    """x = relu(randn) * 3 * amp, offsets = randn * mag, mask logits, w, b * amp"""
    om = rnd(B, 27, H, W, seed=seed + 2)
    return (F.relu(rnd(B, Ci, H, W, seed=seed + 1)) * 3 * amp, om[:, :18] * mag, om[:, 18:].contiguous(),
            rnd(Co, Ci, 3, 3, seed=seed + 3, scale=(Ci * 9) ** -0.5), rnd(Co, seed=seed + 4) * amp)


def grouped_dcn_inputs(case, amps, seed=0):
    """per group (x, off, mask logits, w, b); amps: one amplitude per group; groups named in `shared` read the first one's x"""
    G, B, H, W, Ci, Co, mag, shared = case[:8]
    gs = [list(dcn_inputs(B, Ci, Co, H, W, mag, amps[g], seed=seed + 10 * g)) for g in range(G)]
    for a, b in shared:
        assert amps[a] == amps[b]
        gs[b][0] = gs[a][0]
    return gs


def offmask32(off, mask_logits):
    """NHWC (B,H,W,32): offsets in 0..17, mask logits in 18..26, the rest zero"""
    B, _, H, W = off.shape
    om = torch.zeros(B, H, W, 32)
    om[..., :18] = nhwc(off)
    om[..., 18:27] = nhwc(mask_logits)
    return om


def stem_inputs(B, Cc, H, W, amp=1.0, early=False, seed=0):
    """image (randn * 2) [, radar map], (wb, bb, w0, b0, w1, b1): the seeds of test_stem_fused / tests/test_gpu_early.py; amp
    scales the image, the radar planes and the three biases"""
    x = rnd(B, 3 if early else Cc, H, W, seed=seed + 1) * 2 * amp
    ci = 6 if early else Cc
    wb, bb = rnd(16, ci, 7, 7, seed=seed + 2, scale=(ci * 49) ** -0.5), rnd(16, seed=seed + 3, scale=0.3) * amp
    w0, b0 = rnd(16, 16, 3, 3, seed=seed + 4, scale=144 ** -0.5), rnd(16, seed=seed + 5, scale=0.3) * amp
    w1, b1 = rnd(32, 16, 3, 3, seed=seed + 6, scale=144 ** -0.5), rnd(32, seed=seed + 7, scale=0.3) * amp
    pc = None
    if early:
        pc = rnd(B, 3, H // 4, W // 4, seed=seed + 8) * 3
        pc[:, 0] = torch.rand(B, H // 4, W // 4, generator=torch.Generator().manual_seed(seed + 9))
        pc = pc * amp
    return x, pc, (wb, bb, w0, b0, w1, b1)


# ------------------------------------------------------------------------------------------------ part B: references and gates
def _worst(metric, gots, refs):
    return max(metric(g, r) for g, r in zip(gots, refs))


def _entry(ref, torch32, model, absmax, default_model, tol, ceiling):
    """One small-input evaluation (every tensor argument: a list, one entry per group of the launch): float64 reference, the two
    yardsticks (torch fp32, the split model at the rule's scale), the split model at the DEFAULT scale (the hazard), the relerr
    gate and the per-channel gate.  The metrics are the worst over the groups."""
    y_t, y_m = _worst(relerr_per_channel, torch32, ref), _worst(relerr_per_channel, model, ref)
    return dict(ref=ref, absmax=absmax, in_scales=[in_scale_rule(a) for a in absmax], tol=tol, ceiling=ceiling, torch_ch=y_t, model_ch=y_m, gate_ch=2.0 * max(y_t, y_m),
                torch_rel=_worst(relerr, torch32, ref), model_rel=_worst(relerr, model, ref),
                default_rel=_worst(relerr, default_model, ref))


@functools.lru_cache(maxsize=None)
def small_case(kind, name, amp):
    """-> dict(ref (list of NCHW float64 maps, one per group), in_scales (list), tol, ceiling, the yardsticks and gates).
    The scale of every launch is in_scale_rule(max |x|) of its input."""
    S = in_scale_rule
    D = DEFAULT_IN_SCALE
    seed = SMALL_SEEDS.get(name, 0)
    if kind == "conv":
        c = CONV_CASES[name]
        x, w, b, r = conv_inputs(c, amp, seed)
        s = S(float(x.abs().max()))
        f = lambda dt: _finish(F.conv2d(x.to(dt), w.to(dt), None, c["stride"], 1), b.to(dt), None if r is None else r.to(dt), c["act"])
        m = lambda sc: conv_model(x, w, b, sc, c["stride"], residual=r, act=c["act"])
        return _entry([f(torch.float64)], [f(torch.float32)], [m(s)], [float(x.abs().max())], [m(D)], CONV_TOL, CONV_CH_CEILING)
    if kind == "root":
        t, x1, ch, (w2, b2), (wr, br) = root_inputs(ROOT_CASES[name], amp, seed)

        def f(dt):
            x2 = F.relu(F.conv2d(t.to(dt), w2.to(dt), b2.to(dt), 1, 1) + x1.to(dt))
            return x2, F.relu(F.conv2d(torch.cat([x2, x1.to(dt)] + [c.to(dt) for c in ch], 1), wr.to(dt), br.to(dt)))
        x2, ref = f(torch.float64)
        a2, ar = float(t.abs().max()), max(float(v.abs().max()) for v in [x2, x1, *ch])
        s2, sr = S(a2), S(ar)
        m = lambda a, b_: root_model(t, x1, ch, w2, b2, wr, br, a, b_)
        return _entry([ref], [f(torch.float32)[1]], [m(s2, sr)], [a2, ar], [m(D, D)], CONV_TOL, CONV_CH_CEILING)
    if kind == "proj":
        t, pooled, (w2, b2), (wp, bp) = proj_inputs(PROJ_CASES[name], amp, seed)
        f = lambda dt: F.relu(F.conv2d(t.to(dt), w2.to(dt), b2.to(dt), 1, 1) + F.conv2d(pooled.to(dt), wp.to(dt), bp.to(dt)))
        top = max(float(t.abs().max()), float(pooled.abs().max()))
        s = S(top)
        m = lambda sc: conv_model(t, w2, b2, sc, act=ACT_RELU, proj=(wp, bp, pooled))
        return _entry([f(torch.float64)], [f(torch.float32)], [m(s)], [top], [m(D)], CONV_TOL, CONV_CH_CEILING)
    if kind == "gconv":
        gs = grouped_conv_inputs(GROUPED_CONV_CASES[name], [amp] * GROUPED_CONV_CASES[name][0], seed)
        tops = [float(x.abs().max()) for x, _, _ in gs]
        ss = [S(a) for a in tops]
        f = lambda dt: [F.conv2d(x.to(dt), w.to(dt), b.to(dt), 1, 1) for x, w, b in gs]
        m = lambda scs: [conv_model(x, w, b, sc) for (x, w, b), sc in zip(gs, scs)]
        return _entry(f(torch.float64), f(torch.float32), m(ss), tops, m([D] * len(gs)), CONV_TOL, CONV_CH_CEILING)
    if kind in ("dcn", "gdcn"):
        if kind == "dcn":
            B, Ci, Co, H, W, mag, _ = DCN_CASES[name]
            gs = [dcn_inputs(B, Ci, Co, H, W, mag, amp, seed)]
        else:
            gs = grouped_dcn_inputs(GROUPED_DCN_CASES[name], [amp] * GROUPED_DCN_CASES[name][0], seed)
        tops = [float(g[0].abs().max()) for g in gs]
        ss = [S(a) for a in tops]
        # (no activation in part B: behind a ReLU a DCN channel with a negative bias is all zero on these small maps)
        f = lambda dt: [dcn_ref.deform_conv2d(x.to(dt), off.to(dt), w.to(dt), b.to(dt), (1, 1), (1, 1), (1, 1),
                                              torch.sigmoid(ml.to(dt))) for x, off, ml, w, b in gs]
        m = lambda scs: [dcn_model(x, off, torch.sigmoid(ml.double()), w, b, sc, ACT_NONE)
                         for (x, off, ml, w, b), sc in zip(gs, scs)]
        return _entry(f(torch.float64), f(torch.float32), m(ss), tops, m([D] * len(gs)), DCN_TOL, DCN_CH_CEILING)
    if kind in ("stem", "early"):
        if kind == "stem":
            B, Cc, H, W, _ = STEM_CASES[name]
            x, pc, w = stem_inputs(B, Cc, H, W, amp, seed=seed)
            x6 = x
        else:
            B, H, W, _ = EARLY_CASES[name]
            x, pc, w = stem_inputs(B, 3, H, W, amp, early=True, seed=seed)
            x6 = combine(x, pc)
        tops, ref = stem_chain(x6, w)
        ss = [S(a) for a in tops]
        return _entry([ref], [stem_chain(x6, w, torch.float32)[1]], [stem_model(x6, w, ss)], tops, [stem_model(x6, w, [D] * 3)],
                      CONV_TOL, CONV_CH_CEILING)
    raise ValueError(kind)
