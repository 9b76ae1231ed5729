"""CPU: what the neck-training tests stand on (tests/neck_train_ref.py).  (1) The fp32 CPU graph of every case is within the gate
rule's reach of the float64 graph (tests/dcn_backward_ref.case_gate refuses a case above 1.25e-5).  (2) The chosen draws keep every
sampling coordinate and every ReLU input 1e-5 from its kink, as float64 and as fp32 see them.  (3) The header's new entry points
are the binding's.  (4) The launch geometry each launch-size case is there for, against the library's own workspace functions."""
import os
import re

import pytest
import torch

from tests import neck_train_ref as T
from tests.dcn_backward_ref import CEILING, case_gate, relerr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("cf_offmask_activate", "cf_conv3x3_bwd_workspace_bytes", "cf_conv3x3_bwd_weight", "cf_conv3x3_bwd_data", "cf_bn_relu_workspace_bytes",
               "cf_bn_relu_train_forward", "cf_bn_relu_backward", "cf_upsample_dw_bwd_workspace_bytes", "cf_upsample_dw_bwd")


def errors(g32, g64, names):
    return {n: relerr(g32[n], g64[n]) for n in names}


@pytest.mark.parametrize("i", range(len(T.CONV_CASES)))
def test_offset_conv_fp32_graph_against_float64(i):
    inp = T.conv_inputs(i)
    e = errors(T.conv_graph(inp, torch.float32)[0], T.conv_graph(inp, torch.float64)[0], ("gx", "gw", "gbias"))
    print(T.CONV_CASES[i], e)
    assert all(case_gate(v) <= 2 * CEILING for v in e.values())


@pytest.mark.parametrize("i", range(len(T.BN_CASES)))
def test_bn_relu_fp32_graph_against_float64(i):
    inp = T.bn_inputs(i)
    (g32, m32), (g64, m64) = T.bn_graph(inp, torch.float32), T.bn_graph(inp, torch.float64)
    e = errors(g32, g64, ("y", "gx", "ggamma", "gbeta", "running_mean", "running_var"))
    print(T.BN_CASES[i], e, m64)
    assert m64 >= T.KINK and m32 > 0
    assert all(case_gate(v) <= 2 * CEILING for v in e.values())
    B, C, H, W = T.BN_CASES[i]
    assert B * H * W > 2                          # (M = 2: fp32 itself is at 6.7e-6 - not a gated case)


def test_bn_conditioning_case_is_beyond_the_ceiling_in_fp32_and_breaks_a_single_pass_variance():
    inp = T.bn_inputs(0, cond=True)
    (g32, _), (g64, m64) = T.bn_graph(inp, torch.float32), T.bn_graph(inp, torch.float64)
    e = errors(g32, g64, ("y", "gx", "ggamma", "gbeta"))
    print(e)
    assert m64 >= T.KINK
    assert max(e.values()) < 1e-3                 # its own rule: twice the fp32 error, no ceiling - but the yardstick must mean something
    x = inp[0].float()
    single = (x * x).mean((0, 2, 3)) - x.mean((0, 2, 3)) ** 2            # E[x^2] - E[x]^2 in fp32
    true = inp[0].double().var((0, 2, 3), unbiased=False)
    assert float(((single.double() - true).abs() / true).max()) > 1e-2   # orders above any gate of this case


@pytest.mark.parametrize("i", range(len(T.UP_CASES)))
def test_upsample_fp32_graph_against_float64(i):
    inp, f = T.up_inputs(i), T.UP_CASES[i][4]
    g32, g64 = T.up_graph(inp, f, torch.float32), T.up_graph(inp, f, torch.float64)
    e = errors(g32, g64, ("out", "gx", "gw", "gskip"))
    print(T.UP_CASES[i], e)
    assert all(case_gate(v) <= 2 * CEILING for v in e.values())
    assert torch.equal(g64["gskip"], inp[3].double())


@pytest.mark.parametrize("i", range(len(T.BLOCK_CASES)))
def test_block_draws_keep_their_distance_from_every_kink(i):
    inp = T.block_inputs(i)
    (g32, m32), (g64, m64) = T.block_graph(inp, torch.float32), T.block_graph(inp, torch.float64)
    e = errors(g32, g64, ("y",) + tuple(n for n in T.BLOCK_NAMES if n != "b"))
    print(T.BLOCK_CASES[i], e, m64, m32)
    assert m64 >= T.KINK and m32 >= T.KINK / 2
    assert max(e.values()) < T.BLOCK_GATE / 2     # the fp32 graph itself sits well inside the block gate
    # under batch statistics the DCN bias cancels: its gradient is zero in exact arithmetic
    assert float(g64["b"].abs().max()) < 1e-12 * float(g64["bn_b"].abs().max())


def test_ida_stage_draw_keeps_its_distance_from_every_kink():
    inp = T.ida_inputs()
    (g32, m32), (g64, m64) = T.ida_graph(inp, torch.float32), T.ida_graph(inp, torch.float64)
    e = errors(g32, g64, ("y",) + tuple(n for n in T.IDA_NAMES if not n.endswith(".b")))
    print(e, m64, m32)
    assert m64 >= T.KINK and m32 >= T.KINK / 2
    assert max(e.values()) < 1e-4


def test_header_names_the_new_entry_points_and_the_binding_has_them():
    from centerfusiondetect3d_amd import _lib
    header = open(os.path.join(ROOT, "include", "cf_hip.h")).read()
    declared = set(re.findall(r"\b(cf_\w+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SYMBOLS, name
    assert set(_lib.SYMBOLS) <= declared
    assert _lib.ABI_VERSION == 7 and _lib.load().cf_abi_version() == 7


def test_entry_points_validate_without_a_gpu():
    from centerfusiondetect3d_amd import _lib
    lib = _lib.load()
    assert lib.cf_conv3x3_bwd_data(None, None, None, 1, 4, 4, 48, None, None) == -22 and b"multiple of 32" in lib.cf_last_error()
    assert lib.cf_conv3x3_bwd_weight(None, None, None, 1, 4, 4, 32, None, None, None, 0, None) == 0      # nothing wanted
    assert lib.cf_bn_relu_backward(None, None, None, None, None, None, 1, 8, 64, None, None, None, None, 0, None) == 0
    assert lib.cf_upsample_dw_bwd(None, None, None, 1, 4, 4, 64, 3, None, None, None, 0, None) == -22 and b"2 or 4" in lib.cf_last_error()
    assert lib.cf_upsample_dw_bwd(None, None, None, 1, 4, 4, 64, 2, None, None, None, 0, None) == 0
    assert lib.cf_bn_relu_train_forward(None, None, None, None, None, 1, 0.1, 1e-5, 8, 66, None, None, None, None, 0, None) == -22


def test_cases_reach_the_launch_geometry_they_are_there_for():
    from centerfusiondetect3d_amd import _lib
    lib = _lib.load()
    for i, (B, C, H, W) in enumerate(T.CONV_CASES):
        M = B * H * W
        assert lib.cf_conv3x3_bwd_workspace_bytes(B, H, W, C) == T.conv_workspace_bytes(M, C), T.CONV_CASES[i]
        geo = T.conv_geometry(M, C)
        assert geo == T.CONV_GEOMETRY[i], (T.CONV_CASES[i], geo)
        slabs, cap, slab_px, last = geo[:4]
        assert slab_px % 2 == 0 and 0 < last <= slab_px and (slabs - 1) * slab_px + last == M
    geos = list(T.CONV_GEOMETRY.values())
    assert {g[5] for g in geos} == {1, 2, 4} and {g[4] for g in geos} == {1, 2, 4}       # chunks per wave, waves
    assert any(g[0] == g[1] < (B * H * W + 255) // 256 for g, (B, C, H, W) in zip(geos, T.CONV_CASES))   # the cap binds
    assert any(g[0] > 1 and g[3] < g[2] for g in geos)                                                # a short last slab
    assert sum((B * H * W) % 32 != 0 for B, C, H, W in T.CONV_CASES) >= 5                             # partial 32-pixel tiles
    for i, (B, C, H, W) in enumerate(T.BN_CASES):
        assert lib.cf_bn_relu_workspace_bytes(B * H * W, C) == T.bn_workspace_bytes(B * H * W, C)
        assert T.red_slabs(B * H * W, C) == T.BN_GEOMETRY[i], (T.BN_CASES[i], T.red_slabs(B * H * W, C))
    assert {g[2] for g in T.BN_GEOMETRY.values()} == {4, 8, 16}                  # rows per trip: 256, 128, 64 channels
    assert max(g[0] for g in T.BN_GEOMETRY.values()) > 32 and min(g[0] for g in T.BN_GEOMETRY.values()) == 1
    for i, (B, C, H, W, f) in enumerate(T.UP_CASES):
        assert lib.cf_upsample_dw_bwd_workspace_bytes(B, H, W, C, f) == T.up_workspace_bytes(B, H, W, C, f)
        assert T.red_slabs(B * H * W, C) == T.UP_GEOMETRY[i], (T.UP_CASES[i], T.red_slabs(B * H * W, C))
    assert {c[4] for c in T.UP_CASES} == {2, 4} and max(g[0] for g in T.UP_GEOMETRY.values()) > 1


def test_argument_checks_need_no_gpu():
    from centerfusiondetect3d_amd import _lib, ops
    x, p = torch.zeros(1, 32, 4, 4), T.block_params(32, 32, 0)
    with pytest.raises(_lib.CfHipError):
        ops.deform_conv_block(x, *p)
    with pytest.raises(NotImplementedError):
        ops.deform_conv_block(x.double(), *p)
    with pytest.raises(NotImplementedError):
        ops.deform_conv_block(torch.zeros(1, 48, 4, 4), *T.block_params(48, 32, 0))
    with pytest.raises(_lib.CfHipError):
        ops.upsample_dw_add(torch.zeros(1, 64, 2, 2), torch.zeros(64, 1, 4, 4), 2, torch.zeros(1, 64, 4, 4))
    with pytest.raises(NotImplementedError):
        ops.upsample_dw_add(torch.zeros(1, 64, 2, 2), torch.zeros(64, 1, 6, 6), 3, torch.zeros(1, 64, 6, 6))
    with pytest.raises(NotImplementedError):
        ops.upsample_dw_add(torch.zeros(1, 64, 2, 2).half(), torch.zeros(64, 1, 4, 4), 2, torch.zeros(1, 64, 4, 4))
