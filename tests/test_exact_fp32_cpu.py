"""CPU: the tile form of the exact-fp32 kernels (csrc/cf_gemm.hip) as the library itself reports it, and the yardsticks the
GPU tests of those kernels are gated by (tests/exact_fp32_ref.py).

`cf_gemm_tile_form` is the function `cf_conv2d_fused` and `cf_dcn_v2_fused` choose their launch through.  Swept over M, N_pad,
both `precise` values, convolution and DCN it reaches these forms, and the case tables of tests/exact_fp32_ref.py (with the
shapes of test_conv2d_fused / test_dcn_v2_fused) reach exactly the same set, so a later change of a threshold fails here
instead of silently un-testing a form:

    convolution, plain    128x128  128x64  128x32  64x128  64x64  16-channel kernel
    convolution, precise                   128x32  64x128  64x64  16-channel kernel
    DCN, plain and precise                 128x32  64x128  64x64

Compiled but never launched (removing them is a separate piece of work): `conv_igemm_kernel<128,128,..,true>` and
`<128,64,..,true>` (precise takes 64 rows on every tile 64 or more wide), `dcn_igemm_kernel<128,128,..>` and `<128,64,..>` in both
modes (the DCN always does)."""
import ctypes as C

import pytest

from tests import exact_fp32_ref as R

N_PADS = (32, 64, 96, 128, 192, 256, 512)


@pytest.fixture(scope="module")
def lib():
    from centerfusiondetect3d_amd import _lib
    return _lib.load()


def _m_values():
    ms = {1, 2, 63, 64, 65, 127, 128, 129, 70000}
    ms.update(range(1, 70001, 997))
    for n_tiles in (1, 2, 3, 4, 6, 8, 16):           # N_pad / bn of the N_PADS above
        need = -(-512 // n_tiles)                      # row tiles at which the grid reaches 512 workgroups
        for rows in (64, 128):
            for d in (-1, 0, 1, 2):
                ms.add(rows * (need - 1) + d)
                ms.add(rows * need + d)
    return sorted(m for m in ms if 1 <= m <= 70000)


def _sweep():
    """(M, N, N_pad, layout, act, precise, dcn) over everything the rule looks at"""
    for M in _m_values():
        for n_pad in N_PADS:
            for precise in (False, True):
                yield (M, n_pad, n_pad, R.NHWC, R.ACT_RELU, precise, True)
                yield (M, n_pad, n_pad, R.NHWC, R.ACT_RELU, precise, False)
                yield (M, n_pad, n_pad, R.NCHW, R.ACT_NONE, precise, False)
        for n in (1, 10, 16, 17, 27):                   # the 16-channel kernel's own conditions (N_pad = 32)
            for layout in (R.NHWC, R.NCHW):
                for act in (R.ACT_NONE, R.ACT_RELU, R.ACT_SIGMOID_CLAMP, R.ACT_RAW_AND_SIGDEPTH):
                    for precise in (False, True):
                        for dcn in (False, True):
                            yield (M, n, 32, layout, act, precise, dcn)


def test_the_export_is_the_restated_rule(lib):
    n = 0
    for key in _sweep():
        assert R.tile_form(lib, *key) == R.tile_rule(*key), key
        n += 1
    assert n > 10000
    kind, bm, bn = C.c_int32(), C.c_int32(), C.c_int32()
    assert lib.cf_gemm_tile_form(100, 32, 32, 0, 0, 0, 0, None, None, None) == -22        # refused, not answered
    assert lib.cf_gemm_tile_form(100, 40, 32, 0, 0, 0, 0, C.byref(kind), C.byref(bm), C.byref(bn)) == -22


def test_the_case_tables_reach_every_reachable_form(lib):
    reachable = {(key[6],) + R.tile_form(lib, *key) + (bool(key[5]),) for key in _sweep()}
    T, N16 = R.KIND_TILE, R.KIND_N16
    expected = {(False, T, bm, bn, False) for bm, bn in ((128, 128), (128, 64), (128, 32), (64, 128), (64, 64))}
    expected |= {(False, T, bm, bn, True) for bm, bn in ((128, 32), (64, 128), (64, 64))}
    expected |= {(False, N16, 128, 16, p) for p in (False, True)}
    expected |= {(True, T, bm, bn, p) for bm, bn in ((128, 32), (64, 128), (64, 64)) for p in (False, True)}
    assert reachable == expected                      # (the docstring's list of unreachable instantiations is its complement)
    covered = R.table_forms(lambda *key: R.tile_form(lib, *key))
    assert covered == reachable, (sorted(reachable - covered), sorted(covered - reachable))
    # every case is there for one form: the library must say it launches that one
    for name, c in R.CONV_CASES.items():
        assert R.tile_form(lib, *R.conv_case_key(c)) == c["form"], name
    for name, case in R.DCN_CASES.items():
        for precise in (False, True):
            assert R.tile_form(lib, *R.dcn_case_key(case, precise)) == case[6], (name, precise)
    # the shard launches of the bit-exactness test sit on the other side of the threshold: 64x64
    for name in R.SHARD_CONV_CASES:
        c = R.CONV_CASES[name]
        for frames in (1, 2):
            assert R.tile_form(lib, *R.conv_case_key(dict(c, B=frames)))[1:] == (64, 64) != c["form"][1:]
    B, Ci, Co, H, W, mag, form = R.DCN_CASES[R.SHARD_DCN_CASE]
    for frames in (1, 2):
        for precise in (False, True):
            assert R.tile_form(lib, *R.dcn_case_key((frames, Ci, Co, H, W, mag, form), precise))[1:] == (64, 64) != form[1:]


def _model_errors(c):
    from centerfusiondetect3d_amd import packing
    x, w, b, r = R.conv_inputs(c)
    srcs, tensors = R.conv_sources(c, x)
    pc = packing.pack_conv(w, b, [packing.Source(*s) for s in srcs], stride=c["stride"])
    ref = R.conv_ref(x, w, b, r, c["stride"], c["act"])
    res = None if r is None else R.nhwc(r)
    return [R.relerr(R.nchw(R.summation_model(pc, tensors, c["B"], c["H"], c["W"], precise, res, c["act"])), ref)
            for precise in (False, True)]


def test_the_summation_models_are_convolutions_and_blocked_beats_chain_at_long_k():
    """Both orders of the yardstick must BE the convolution (1e-5 of float64 catches any wrong tap, stride, source or pad
    slot); at K = 4608 the blocked order must be the closer one - the reason the kernels have a precise mode at all."""
    for name in ("c128x32_plain_stride2", "hconv_two_sources_offset", "n16_stem7x7", "head_out_9x7_raw"):
        chain, blocked = _model_errors(R.CONV_CASES[name])
        assert chain < 1e-5 and blocked < 1e-5, (name, chain, blocked)
    small = dict(R.CONV_CASES["c64x128_precise_res"], B=1, H=9, W=11, Co=32)      # residual + ReLU
    chain, blocked = _model_errors(small)
    assert chain < 1e-5 and blocked < 1e-5, (chain, blocked)
    chain, blocked = _model_errors(R.CONV_CASES["c64x64_plain_k4608"])
    print(f"[exact fp32] K = 4608: chain model {chain:.2e}, blocked model {blocked:.2e} of max|ref64|")
    assert chain < 1e-5 and blocked < chain, (chain, blocked)


def test_the_dcn_gate_rule():
    assert R.dcn_gate([1.4e-6, 4e-7]) == 5e-6
    assert R.dcn_gate([1.4e-6, 3e-6]) == 6e-6
