"""CPU: what the stem-training tests stand on (tests/stem_train_ref.py).  (1) The header declares the new entry points, the library
exports them, the ABI stays 7.  (2) The eval-mode fp32 graph of the ref file on a model's state dict IS the reference's stem
(tests/early_ref.stem, held to the reference-generated fixture by tests/test_early_cpu.py) - on six channels for the early model,
the same composition on three for the middle one.  (3) The restated launch geometry equals cf_stem_conv_bwd_workspace_bytes and
every launch-size case reaches the branch it is there for.  (4) The new entry points and the operator refuse bad arguments without
a GPU.  (5) The chosen draws keep every ReLU input 1e-5 from zero and their fp32 graphs sit inside the gates."""
import os
import re

import pytest
import torch

from tests import early_ref
from tests import stem_train_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("cf_stem_conv_bwd_workspace_bytes", "cf_stem_conv_forward", "cf_stem_conv_bwd_weight", "cf_stem_conv_bwd_data")
STEM_SEED_HINT = {"middle_nofrustum": 1, "early": 0}     # tests/test_gpu_stem_train.SEED_HINT


def _sd(kind):
    from centerfusiondetect3d_amd import config as cfg, getModel
    c = {"middle_nofrustum": cfg.centerfusion_middle_config, "early": cfg.centerfusion_early_config}[kind]((64, 96))
    c.MODEL.FREEZE_BACKBONE = True
    torch.manual_seed(11)
    return getModel(cfg.update_loss_weights(c)).state_dict()


def test_header_names_the_new_entry_points_and_the_library_exports_them():
    import ctypes
    from centerfusiondetect3d_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "cf_hip.h")).read()
    declared = set(re.findall(r"\b(cf_\w+)\s*\(", header))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SYMBOLS, name
        assert getattr(raw, name) is not None
    assert _lib.ABI_VERSION == 7 and _lib.load().cf_abi_version() == 7
    assert "cf_stem_train.hip" in [s for s, _ in build.SOURCES]


@pytest.mark.parametrize("kind", ["middle_nofrustum", "early"])
def test_eval_graph_on_a_state_dict_is_the_reference_stem(kind):
    sd = _sd(kind)
    g = torch.Generator().manual_seed(3)
    for n in list(sd):                                      # running statistics and affine that are not the identity
        if n.startswith(("base.base_layer.1.", "base.level0.1.", "base.level1.1.")) and sd[n].is_floating_point():
            sd[n] = torch.rand(sd[n].shape, generator=g) + 0.5
    x = T.rnd(2, 3, 32, 32, seed=1)
    x6 = early_ref.combine(x, torch.relu(T.rnd(2, 3, 8, 8, seed=2))) if kind == "early" else x
    assert sd["base.base_layer.0.weight"].shape[1] == x6.shape[1]
    want = early_ref.stem(sd, x6)
    got = T.stem_eval(sd, x6)
    assert tuple(got.shape) == (2, 32, 16, 16) and float(got.max()) > 0
    assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())
    assert len(T.stem_param_names(sd)) == 9


def test_restated_geometry_equals_the_c_function_and_the_cases_reach_their_branches():
    from centerfusiondetect3d_amd import _lib
    lib = _lib.load()
    for i, (B, Ci, Co, H, W, k, s) in enumerate(T.CONV_CASES):
        assert lib.cf_stem_conv_bwd_workspace_bytes(B, H, W, Ci, Co, k, s) == T.conv_workspace_bytes(B, Ci, Co, H, W, k, s), T.CONV_CASES[i]
        geo = T.conv_geometry(B, Ci, Co, H, W, k, s)
        assert geo == T.CONV_GEOMETRY[i], (T.CONV_CASES[i], geo)
        slabs, cap, slab_px, last = geo[:4]
        ho, wo = T.out_hw(H, W, k, s)
        assert slab_px % 4 == 0 and 0 < last <= slab_px and (slabs - 1) * slab_px + last == B * ho * wo and slabs <= cap
    geos = [T.CONV_GEOMETRY[i] for i in range(len(T.CONV_CASES))]
    assert any(1 < g[0] and (g[2] * (g[0] - 1) + g[3] + 255) // 256 <= g[1] and g[3] < g[2] for g in geos)   # several slabs, short last one
    assert any((g[2] * (g[0] - 1) + g[3] + 255) // 256 > g[1] for g in geos)                                # the cap binds
    assert any(g[4] > 1 and c[5] == 3 and c[6] == 1 for g, c in zip(geos, T.CONV_CASES))                    # the grid's second dimension
    assert any(g[4] > 1 and c[5] == 7 for g, c in zip(geos, T.CONV_CASES))
    assert any(g[5] > 1 and c[6] == 2 for g, c in zip(geos, T.CONV_CASES))
    assert any(B * T.out_hw(H, W, k, s)[0] % T.TILE_ROWS and B > 1 for B, _, _, H, W, k, s in T.CONV_CASES)  # batch boundary in a tile
    assert {(c[1], c[5], c[6], c[2]) for c in T.CONV_CASES} >= {(3, 7, 1, 16), (6, 7, 1, 16), (16, 3, 1, 16), (16, 3, 2, 32)}
    assert lib.cf_stem_conv_bwd_workspace_bytes(1, 8, 8, 16, 24, 3, 1) == 0 and lib.cf_stem_conv_bwd_workspace_bytes(1, 8, 8, 16, 16, 5, 1) == 0
    assert lib.cf_stem_conv_bwd_workspace_bytes(1, 8, 8, 3, 16, 7, 2) == 0
    # batch 16 at 448 x 800: one 16-channel map is 92 M floats; the slab count stays under its cap
    assert T.weight_slabs(16 * 448 * 800, 3, 7)[0] <= 512 and lib.cf_stem_conv_bwd_workspace_bytes(16, 448, 800, 3, 16, 7, 1) \
        == T.conv_workspace_bytes(16, 3, 16, 448, 800, 7, 1)


def test_entry_points_validate_without_a_gpu():
    from centerfusiondetect3d_amd import _lib
    lib = _lib.load()
    fwd = lambda *geo: lib.cf_stem_conv_forward(None, None, None, *geo, None, None)
    bww = lambda *geo: lib.cf_stem_conv_bwd_weight(None, None, None, *geo, None, None, 0, None)
    bwd = lambda *geo: lib.cf_stem_conv_bwd_data(None, None, *geo, None, None)
    for call in (fwd, bww, bwd):
        assert call(1, 8, 8, 16, 24, 3, 1) == -22 and b"16 or 32" in lib.cf_last_error()            # Cout 24
        assert call(1, 8, 8, 16, 16, 5, 1) == -22 and b"stride" in lib.cf_last_error()              # k 5
        assert call(1, 8, 8, 3, 16, 7, 2) == -22 and b"stride" in lib.cf_last_error()               # stride 2 with k 7
        assert call(1, 8, 8, 32, 16, 3, 1) == -22 and b"Cin" in lib.cf_last_error()
        assert call(1, 8, 8, 9, 16, 7, 1) == -22 and b"Cin" in lib.cf_last_error()
        assert call(0, 8, 8, 16, 16, 3, 1) == -22
        assert call(1, 8, 8, 16, 16, 3, 1) == -22 and b"null" in lib.cf_last_error()                # null pointers
    assert bwd(1, 8, 8, 3, 16, 7, 1) == -22 and b"input gradient" in lib.cf_last_error()            # the 7x7 layer has none


def test_argument_checks_need_no_gpu():
    from centerfusiondetect3d_amd import _lib, ops
    x3, x16 = torch.zeros(1, 3, 8, 8), torch.zeros(1, 16, 8, 8)
    p7, p3 = T.block_params(3, 16, 7, 0), T.block_params(16, 16, 3, 0)
    with pytest.raises(_lib.CfHipError):
        ops.stem_conv_bn_relu(x3, *p7)
    with pytest.raises(_lib.CfHipError):
        ops.stem_conv_bn_relu(x16, *p3)
    with pytest.raises(NotImplementedError):
        ops.stem_conv_bn_relu(x3.double(), *p7)
    with pytest.raises(NotImplementedError):
        ops.stem_conv_bn_relu(x3.clone().requires_grad_(True), *p7)                                 # no data gradient for k = 7
    with pytest.raises(NotImplementedError):
        ops.stem_conv_bn_relu(x3, *T.block_params(6, 16, 7, 0), radar=torch.zeros(1, 3, 2, 2, requires_grad=True))
    with pytest.raises(NotImplementedError):
        ops.stem_conv_bn_relu(x3, *p7, stride=2)
    with pytest.raises(NotImplementedError):
        ops.stem_conv_bn_relu(x16, *T.block_params(16, 24, 3, 0))
    with pytest.raises(NotImplementedError):
        ops.stem_conv_bn_relu(x16, *T.block_params(16, 16, 5, 0))
    with pytest.raises(NotImplementedError):
        ops.stem_conv_bn_relu(torch.zeros(1, 32, 8, 8), *T.block_params(32, 32, 3, 0))
    with pytest.raises(NotImplementedError):
        ops.stem_conv_bn_relu(x16, *p3, radar=torch.zeros(1, 3, 2, 2))                              # a radar map goes with k = 7
    with pytest.raises(ValueError):
        ops.stem_conv_bn_relu(x3, *T.block_params(6, 16, 7, 0), radar=torch.zeros(1, 3, 4, 4))
    with pytest.raises(ValueError):
        ops.stem_conv_bn_relu(x16, p3[0], p3[1][:8], *p3[2:])
    with pytest.raises(_lib.CfHipError):
        ops.stem_conv_bn_relu_nhwc(torch.zeros(1, 8, 8, 16), *p3)


@pytest.mark.parametrize("i", range(len(T.CONV_CASES)))
def test_conv_fp32_graph_against_float64(i):
    B, Ci, Co, H, W, k, s = T.CONV_CASES[i]
    inp = T.conv_inputs(i)
    for mask_odd in (False, True):
        g32, g64 = T.conv_all(inp, k, s, torch.float32, mask_odd)[0], T.conv_all(inp, k, s, torch.float64, mask_odd)[0]
        e = {n: T.relerr(g32[n], g64[n]) for n in ("z", "gx", "gw")}
        print(T.CONV_CASES[i], mask_odd, e)
        assert max(e.values()) <= 1.25e-5                   # (tests/dcn_backward_ref.CEILING: above it a case measures nothing)


@pytest.mark.parametrize("kind", sorted(T.BLOCK_CASES))
def test_block_draws_keep_their_distance_from_the_kink(kind):
    inp = T.block_inputs(kind)
    (g32, m32), (g64, m64) = T.block_graph(kind, inp, torch.float32), T.block_graph(kind, inp, torch.float64)
    e = {n: T.relerr(g32[n], g64[n]) for n in g64 if not n.startswith("running")}
    print(kind, e, m64, m32)
    assert m64 >= T.KINK and m32 >= T.KINK / 2
    assert max(e.values()) < T.BLOCK_GATE / 2               # the fp32 graph itself sits well inside the block gate
    assert ("x" in g64) == (T.BLOCK_CASES[kind][5] == 3)


@pytest.mark.parametrize("kind", ["middle_nofrustum", "early"])
def test_stem_draw_keeps_its_distance_from_the_kink_and_the_hint_is_current(kind):
    sd = _sd(kind)
    x, pc, R, seed = T.stem_input(sd, kind == "early", hint=STEM_SEED_HINT[kind])
    assert seed == STEM_SEED_HINT[kind] == T.stem_input(sd, kind == "early")[3]       # the hint is what the search finds
    assert (pc is None) == (kind != "early") and tuple(x.shape) == T.STEM_SHAPE
    (g64, m64), (g32, m32) = T.stem_graph(sd, x, pc, R, torch.float64), T.stem_graph(sd, x, pc, R, torch.float32)
    assert m64 >= T.KINK and m32 > 0
    assert set(g64) == {"level1", *T.stem_param_names(sd)} and len(g64) == 10
    e = {n: T.relerr(g32[n], g64[n]) for n in g64}
    print(kind, e)
    assert max(e.values()) < 1e-4
