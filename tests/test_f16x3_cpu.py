"""CPU side of the split-fp16 range tests (tests/f16x3_ref.py; the GPU side is tests/test_gpu_f16x3_range.py): the hazard of a
fixed pre-scale on small inputs pinned on the restated split, ops.in_scale_for against the restated rule, the reference's own
error across amplitudes (the condition the GPU gates rely on), the ceilings of the per-channel gates, and the case tables."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import f16x3_ref as R


def _hazard_inputs():
    x = F.relu(R.rnd(2, 64, 28, 50, seed=2)) * 3
    w = R.rnd(32, 64, 3, 3, seed=3, scale=(64 * 9) ** -0.5).double()
    return x, w


def test_split_model_reproduces_the_hazard_table():
    """A 64 -> 32 3x3 convolution in float64 with exact weights whose input went through the split: at the default pre-scale
    the error grows as the input shrinks (the lo half turns fp16-subnormal: an absolute floor of 2^-25 / 16 per activation),
    with the pre-scale following the range it does not.  Every figure within a factor 2 of the recorded table."""
    x0, w = _hazard_inputs()
    for e, absmax, err, err_following in R.HAZARD_TABLE:
        x = x0 * 2.0 ** e
        ref = F.conv2d(x.double(), w, None, 1, 1)
        top = float(x.abs().max())
        assert absmax / 2 < top < absmax * 2, (e, top)
        fixed = R.relerr(F.conv2d(R.split_model(x, 16.0), w, None, 1, 1), ref)
        following = R.relerr(F.conv2d(R.split_model(x, R.in_scale_rule(top)), w, None, 1, 1), ref)
        fp32 = R.relerr(F.conv2d(x, w.float(), None, 1, 1), ref)
        print(f"[hazard] max|x| = {top:.2e}: scale 16 {fixed:.2e}, following {following:.2e}, torch fp32 {fp32:.2e}")
        assert err / 2 < fixed < err * 2, (e, fixed, err)
        assert err_following / 2 < following < err_following * 2, (e, following)
        assert R.HAZARD_FP32 / 2 < fp32 < R.HAZARD_FP32 * 2, (e, fp32)
    # the branch point: at max|x| = 2^-6 the default pre-scale is still at fp32 level
    x = x0 * (2.0 ** -6 / float(x0.abs().max()))
    ref = F.conv2d(x.double(), w, None, 1, 1)
    assert R.relerr(F.conv2d(R.split_model(x, 16.0), w, None, 1, 1), ref) < 3e-7


def _sweep_points():
    pts = []
    for e in range(-60, 21):
        a = 2.0 ** e
        pts += [a, math.nextafter(a, 0.0), math.nextafter(a, math.inf), a * 1.5]
    for headroom in (2.0, 4.0, 8.0, 16.0):
        # the branch points: 2^-6, 65504 / 64 (where 16 stops), and every absmax at which the scale of a branch steps
        for b in [2.0 ** -6, R.F16_MAX / 64.0] + [R.F16_MAX / headroom / 2.0 ** p for p in range(-8, 34)]:
            pts += [b, math.nextafter(b, 0.0), math.nextafter(b, math.inf)]
    return pts


def test_in_scale_for_against_the_restated_rule():
    from centerfusiondetect3d_amd import ops, _lib
    assert ops.in_scale_for(0.0) == 16.0 == R.in_scale_rule(0.0)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(_lib.CfHipError, match="not finite"):
            ops.in_scale_for(bad)
        with pytest.raises(ValueError):
            R.in_scale_rule(bad)
    seen = set()
    for headroom in (2.0, 4.0, 8.0, 16.0):
        for a in _sweep_points():
            s = ops.in_scale_for(a, headroom)
            assert s == R.in_scale_rule(a, headroom), (a, headroom, s)
            assert s > 0 and math.frexp(s)[0] == 0.5, (a, s)                       # a power of two
            assert s <= 2.0 ** 32
            if s != 16.0:
                assert a * s <= R.F16_MAX / headroom, (a, headroom, s)
                if s < 2.0 ** 32:
                    assert a * s * 2.0 > R.F16_MAX / headroom, (a, headroom, s)     # ... and the largest one
            else:
                assert a * 16.0 <= R.F16_MAX / 4.0 or headroom < 8.0
            if headroom == 8.0:
                assert (s == 16.0) == (2.0 ** -6 <= a <= R.F16_MAX / 64.0), (a, s)
                seen.add(s)
    assert 2.0 ** 32 in seen and 2.0 ** 19 in seen and 2.0 ** -8 in seen and 16.0 in seen
    # the upper branch alone (the heads' mx rows keep it): never above 16
    for a in _sweep_points():
        s = ops.in_scale_for_large(a)
        assert s == (16.0 if a * 16.0 <= R.F16_MAX / 4.0 else R.in_scale_rule(a)) and s <= 16.0


def test_argument_blocks_keep_out_scale_a_normal_fp32():
    """out_scale = 2^-s / in_scale must stay a normal fp32 at the cap of the rule, and the host refuses one that would not."""
    from centerfusiondetect3d_amd import ops, packing, _lib
    w, b = torch.randn(32, 16, 3, 3) * 0.05, torch.zeros(32)
    pc = packing.pack_conv_f16(w, b, [packing.Source(16, 16)])
    x = torch.zeros(1, 8, 8, 16)
    a = ops.conv_args(pc, [x], [16], 1, 8, 8, torch.zeros(1, 8, 8, 32), 32, in_scale=2.0 ** 32)
    assert a.in_scale == 2.0 ** 32 and a.out_scale == pc.out_scale * 2.0 ** -28 and a.out_scale >= 2.0 ** -126
    tiny = packing.pack_conv_f16(w * 2.0 ** -80, b, [packing.Source(16, 16)])        # weights of 2^-83: out_scale near 2^-100 by itself
    assert 0 < tiny.out_scale < 2.0 ** -98
    with pytest.raises(_lib.CfHipError, match="normal fp32"):
        ops.conv_args(tiny, [x], [16], 1, 8, 8, torch.zeros(1, 8, 8, 32), 32, in_scale=2.0 ** 32)
    pd = packing.pack_dcn_f16(torch.randn(32, 32, 3, 3) * 0.05, torch.zeros(32))
    om = torch.zeros(1, 8, 8, 32)
    xd = torch.zeros(1, 8, 8, 32)
    d = ops.dcn_args(pd, xd, om, 32, 1, 8, 8, torch.zeros(1, 8, 8, 32), 32, in_scale=2.0 ** 32)
    assert d.in_scale == 2.0 ** 32 and d.out_scale == pd.out_scale * 2.0 ** -28


def test_conv_model_with_the_rules_scale_is_flat_across_amplitudes():
    """For every amplitude 2^-32 .. 2^12 the restated kernel arithmetic with the rule's pre-scale stays within 2x of its error at
    amplitude 1 (both metrics): the small-input gates of the GPU tests ask nothing the arithmetic cannot give."""
    c = R.CONV_CASES["patch_48x27_wk1"]
    x0, w, b0, _ = R.conv_inputs(c)
    base = None
    for e in [0] + list(range(-32, 13, 4)):
        amp = 2.0 ** e
        x, b = x0 * amp, b0 * amp
        ref = F.conv2d(x.double(), w.double(), b.double(), 1, 1)
        got = R.conv_model(x, w, b, R.in_scale_rule(float(x.abs().max())))
        errs = (R.relerr(got, ref), R.relerr_per_channel(got, ref))
        if base is None:
            base = errs
            assert base[0] < 2e-7
        assert errs[0] <= 2 * base[0] and errs[1] <= 2 * base[1], (e, errs, base)


@pytest.mark.parametrize("kind,name", R.SMALL_CASES)
def test_small_input_gates_stay_below_their_ceilings(kind, name):
    """The per-channel gate of each small-input case (twice the larger of the torch fp32 and the split-model yardstick) may
    not come out above 1.5e-6 (convolutions) / 5e-6 (DCN); the split model itself meets the relerr gate with a factor 2 to
    spare; and at amp = 2^-12 the DEFAULT pre-scale misses that gate - the GPU test's hazard assertion is not vacuous."""
    for amp in R.AMPS:
        e = R.small_case(kind, name, amp)
        print(f"[{name} amp {amp:g}] in_scales {e['in_scales']}: per channel torch {e['torch_ch']:.2e} model {e['model_ch']:.2e} "
              f"gate {e['gate_ch']:.2e}; relerr torch {e['torch_rel']:.2e} model {e['model_rel']:.2e} default scale {e['default_rel']:.2e}")
        assert e["gate_ch"] <= e["ceiling"], (amp, e["gate_ch"])
        assert e["model_rel"] < e["tol"] / 2
        assert all((s == 16.0) == (amp == 1.0) for s in e["in_scales"]), e["in_scales"]      # off the default wherever amp is not 1
    assert R.small_case(kind, name, R.HAZARD_AMP)["default_rel"] > R.small_case(kind, name, R.HAZARD_AMP)["tol"]


def test_case_tables_name_every_form_once():
    claimed = R.claimed_forms()
    assert sorted(claimed) == sorted(R.FORMS), set(claimed) ^ set(R.FORMS)          # every form, each by exactly one case
    for kind, name in R.SMALL_CASES:
        table = dict(conv=R.CONV_CASES, root=R.ROOT_CASES, proj=R.PROJ_CASES, gconv=R.GROUPED_CONV_CASES, gdcn=R.GROUPED_DCN_CASES,
                     dcn=R.DCN_CASES, stem=R.STEM_CASES, early=R.EARLY_CASES)[kind]
        assert name in table
    assert {k for k, _ in R.SMALL_CASES} >= {"conv", "root", "proj", "gconv", "gdcn", "dcn", "stem", "early"}
    # the packer's view of the convolution rows: slice-major (patch) packing wherever the patch kernel is asked for
    from centerfusiondetect3d_amd import packing
    for name, c in R.CONV_CASES.items():
        pc = packing.pack_conv_f16(torch.zeros(c["Co"], c["Ci"], 3, 3), torch.zeros(c["Co"]), [packing.Source(c["Ci"], c["Ci"])],
                                   stride=c["stride"])
        assert pc.patch, name
