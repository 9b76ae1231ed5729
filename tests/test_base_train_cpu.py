"""CPU: what the base-training tests stand on (tests/base_train_ref.py).  (1) The header declares the new entry points, the library
exports them, the ABI is 7.  (2) The workspace mirrors equal the C functions, and every launch-size case reaches the geometry it is
there for.  (3) The fp32 CPU graph of every case is within the gate rule's reach of the float64 graph
(tests/dcn_backward_ref.case_gate refuses a case above 1.25e-5), and the chosen draws keep every ReLU input 1e-5 from zero.
(4) The max-pool inputs hold the ties they are there for, and torch's CPU backward sends a tie's gradient to the first maximum in
row-major order in both memory formats.  (5) The operators' argument checks."""
import os
import re

import pytest
import torch

from tests import base_train_ref as T
from tests.dcn_backward_ref import CEILING, case_gate, relerr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("cf_conv_bwd_workspace_bytes", "cf_conv_bwd_weight", "cf_conv_bwd_data", "cf_bn_act_workspace_bytes",
               "cf_bn_act_train_forward", "cf_bn_act_backward", "cf_maxpool2x2_bwd")


def errors(g32, g64, names):
    return {n: relerr(g32[n], g64[n]) for n in names}


def test_header_names_the_new_entry_points_and_the_library_exports_them():
    import ctypes
    from centerfusiondetect3d_amd import _lib
    header = open(os.path.join(ROOT, "include", "cf_hip.h")).read()
    declared = set(re.findall(r"\b(cf_\w+)\s*\(", header))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SYMBOLS, name
        assert getattr(raw, name) is not None
    assert set(_lib.SYMBOLS) <= declared
    assert _lib.ABI_VERSION == 7 and _lib.load().cf_abi_version() == 7


def test_workspace_mirrors_equal_the_c_functions_and_the_cases_reach_their_geometry():
    from centerfusiondetect3d_amd import _lib
    lib = _lib.load()
    for i, (B, Ci, Co, H, W, k, s) in enumerate(T.CONV_CASES):
        assert lib.cf_conv_bwd_workspace_bytes(B, H, W, Ci, Co, k, s) == T.conv_workspace_bytes(B, H, W, Ci, Co, k, s), T.CONV_CASES[i]
        ho, wo = T.out_hw(H, W, k, s)
        geo = T.conv_slabs(B * ho * wo, Ci, Co, k)
        assert geo == T.CONV_GEOMETRY[i], (T.CONV_CASES[i], geo)
        slabs, cap, slab_px, last = geo
        assert slab_px % 2 == 0 and 0 < last <= slab_px and (slabs - 1) * slab_px + last == B * ho * wo
    geos = [T.CONV_GEOMETRY[i] for i in range(len(T.CONV_CASES))]
    assert any(g[0] > 1 and g[0] < g[1] for g in geos)                                                # several slabs under the cap
    assert any(g[0] == g[1] < (g[2] * (g[0] - 1) + g[3] + 255) // 256 for g in geos)                 # the cap binds
    assert any(g[0] > 1 and g[3] < g[2] for g in geos)                                                # a short last slab
    assert {(k, s) for *_, k, s in T.CONV_CASES} == {(1, 1), (3, 1), (3, 2)}
    assert any(H % 2 and W % 2 and s == 2 for _, _, _, H, W, _, s in T.CONV_CASES)
    assert max(c[1] for c in T.CONV_CASES) == 1280 and max(c[2] for c in T.CONV_CASES) == 512
    for B, C, H, W in T.BN_CASES:
        assert lib.cf_bn_act_workspace_bytes(B * H * W, C) == T.bn_workspace_bytes(B * H * W, C) \
            == lib.cf_bn_relu_workspace_bytes(B * H * W, C)
    assert lib.cf_conv_bwd_workspace_bytes(1, 4, 4, 48, 32, 3, 1) == 0 and lib.cf_conv_bwd_workspace_bytes(1, 4, 4, 32, 32, 5, 1) == 0


def test_entry_points_validate_without_a_gpu():
    from centerfusiondetect3d_amd import _lib
    lib = _lib.load()
    assert lib.cf_conv_bwd_data(None, None, 1, 4, 4, 48, 32, 3, 1, None, None) == -22 and b"multiple of 32" in lib.cf_last_error()
    assert lib.cf_conv_bwd_data(None, None, 1, 4, 4, 1312, 32, 1, 1, None, None) == -22 and b"1280" in lib.cf_last_error()
    assert lib.cf_conv_bwd_weight(None, None, 1, 4, 4, 32, 544, 3, 1, None, None, 0, None) == -22 and b"512" in lib.cf_last_error()
    assert lib.cf_conv_bwd_weight(None, None, 1, 4, 4, 32, 32, 1, 2, None, None, 0, None) == -22 and b"stride" in lib.cf_last_error()
    assert lib.cf_conv_bwd_weight(None, None, 1, 4, 4, 32, 32, 3, 1, None, None, 0, None) == -22 and b"null" in lib.cf_last_error()
    assert lib.cf_bn_act_backward(None, None, None, None, None, 1, None, None, 1, 8, 64, None, None, None, None, None, 0, None) == 0
    assert lib.cf_bn_act_train_forward(None, None, None, None, 1, None, None, 1, 0.1, 1e-5, 8, 66, None, None, None, None, 0, None) == -22
    assert lib.cf_maxpool2x2_bwd(None, None, 1, 4, 4, 30, None, None) == -22


@pytest.mark.parametrize("i", range(len(T.CONV_CASES)))
def test_conv_fp32_graph_against_float64(i):
    B, Ci, Co, H, W, k, s = T.CONV_CASES[i]
    inp = T.conv_inputs(i)
    e = errors(T.conv_graph(inp, k, s, torch.float32)[0], T.conv_graph(inp, k, s, torch.float64)[0], ("gx", "gw"))
    print(T.CONV_CASES[i], e)
    assert all(case_gate(v) <= 2 * CEILING for v in e.values())
    if s == 2:
        e = errors(T.conv_graph(inp, k, s, torch.float32, True)[0], T.conv_graph(inp, k, s, torch.float64, True)[0], ("gx", "gw"))
        assert all(case_gate(v) <= 2 * CEILING for v in e.values())


@pytest.mark.parametrize("i", range(len(T.BN_CASES)))
@pytest.mark.parametrize("residual,relu", T.BN_MODES)
def test_bn_act_fp32_graph_against_float64(i, residual, relu):
    inp = T.bn_inputs(i, residual, relu)
    (g32, m32), (g64, m64) = T.bn_graph(inp, torch.float32, residual, relu), T.bn_graph(inp, torch.float64, residual, relu)
    names = ("y", "gx", "ggamma", "gbeta", "running_mean", "running_var") + (("gres",) if residual else ())
    e = errors(g32, g64, names)
    print(T.BN_CASES[i], residual, relu, e, m64)
    assert m64 >= T.KINK and m32 > 0
    assert all(case_gate(v) <= 2 * CEILING for v in e.values())


@pytest.mark.parametrize("i", range(len(T.POOL_CASES)))
def test_pool_inputs_hold_their_ties_and_aten_takes_the_first_maximum(i):
    x, R = T.pool_input(i)
    B, C, H, W = x.shape
    win = x.view(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)
    mx = win.max(dim=-1, keepdim=True).values
    zero = (mx.squeeze(-1) == 0)
    tied = ((win == mx).sum(-1) > 1) & ~zero
    print(T.POOL_CASES[i], "all-zero windows", float(zero.float().mean()), "positive ties", int(tied.sum()))
    assert 0.3 < float(zero.float().mean()) < 0.7 and int(tied.sum()) > 0 and float(x.min()) >= 0
    first = (win == mx).float().argmax(dim=-1)                                   # (argmax of a 0/1 map: the first 1)
    want = torch.zeros_like(win).scatter_(-1, first.unsqueeze(-1), R.unsqueeze(-1))
    want = want.view(B, C, H // 2, W // 2, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H, W)
    for cl in (False, True):
        out, gx = T.pool_graph(x, R, channels_last=cl)
        assert torch.equal(gx, want), cl


@pytest.mark.parametrize("kind", sorted(T.BLOCK_CASES))
def test_block_draws_keep_their_distance_from_the_kink(kind):
    inp = T.block_inputs(kind)
    (g32, m32), (g64, m64) = T.block_graph(kind, inp, torch.float32), T.block_graph(kind, inp, torch.float64)
    e = errors(g32, g64, [n for n in g64 if not n.startswith("running")])
    print(kind, e, m64, m32)
    assert m64 >= T.KINK and m32 >= T.KINK / 2
    assert max(e.values()) < T.BLOCK_GATE / 2     # the fp32 graph itself sits well inside the block gate
    cins = T.BLOCK_CASES[kind][1]
    assert all(c in (32, 64, 128) for c in cins + (T.BLOCK_CASES[kind][2],))


def test_levels_graph_has_the_shapes_of_dla34():
    from centerfusiondetect3d_amd import config as cfg, getModel
    c = cfg.centernet_config((64, 96))
    c.MODEL.FREEZE_BACKBONE = True
    torch.manual_seed(11)
    sd = getModel(cfg.update_loss_weights(c)).state_dict()
    names = T.level_param_names(sd)
    assert len(names) == sum(n.startswith(("base.level2.", "base.level3.", "base.level4.", "base.level5."))
                             for n, _ in getModel(cfg.update_loss_weights(c)).named_parameters())
    x = torch.relu(T.rnd(1, 32, 32, 32, seed=1))
    Rs = [T.rnd(1, ch, 32 >> (j + 1), 32 >> (j + 1), seed=2 + j) for j, ch in enumerate((64, 128, 256, 512))]
    out, _ = T.levels_graph(sd, x, Rs, torch.float32)
    assert [tuple(out[f"level{l}"].shape) for l in (2, 3, 4, 5)] == [(1, 64, 16, 16), (1, 128, 8, 8), (1, 256, 4, 4), (1, 512, 2, 2)]
    assert all(out[n] is not None and tuple(out[n].shape) == tuple(sd[n].shape) for n in names)


def test_argument_checks_need_no_gpu():
    from centerfusiondetect3d_amd import _lib, ops
    x, p = torch.zeros(1, 32, 4, 4), T.block_params(32, 32, 3, 0)
    with pytest.raises(_lib.CfHipError):
        ops.conv_bn_act(x, *p)
    with pytest.raises(NotImplementedError):
        ops.conv_bn_act(x.double(), *p)
    with pytest.raises(NotImplementedError):
        ops.conv_bn_act(torch.zeros(1, 48, 4, 4), *T.block_params(48, 32, 3, 0))
    with pytest.raises(NotImplementedError):
        ops.conv_bn_act(x, *T.block_params(32, 32, 1, 0), stride=2)                 # stride 2 with k = 3 only
    with pytest.raises(NotImplementedError):
        ops.conv_bn_act(x, *T.block_params(32, 32, 5, 0))
    with pytest.raises(ValueError):
        ops.conv_bn_act(x, p[0], p[1][:16], *p[2:])
    with pytest.raises(ValueError):
        ops.conv_bn_act(x, *p, residual=torch.zeros(1, 32, 2, 2))
    with pytest.raises(_lib.CfHipError):
        ops.max_pool2x2(x)
    with pytest.raises(NotImplementedError):
        ops.max_pool2x2(x.double())
    with pytest.raises(NotImplementedError):
        ops.max_pool2x2(torch.zeros(1, 32, 1, 4))
