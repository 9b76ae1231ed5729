"""CPU side of the head training path: the constructions of tests/heads_train_ref.py hold what they promise, the cases reach the
geometry they are named for (the replicated ones too), the fp32 oracle is usable on every case, `ops.head_stack` and `DLASeg` refuse what they do not
implement before any device is touched, construction sets the requires_grad flags, and the ctypes mirror of
cf_head_train_args has the C compiler's layout."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from tests import heads_train_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(T.CASES))
def test_construction_keeps_the_relu_masks(name):
    case = T.build(name)
    assert len(case["checks"]) == T.CASES[name][3] + 1
    r64, r32 = T.reference(name)
    if case["family"] == "dyadic":
        for v in case["checks"]:
            assert v < 2 ** 24, "a hidden pre-activation is not exact in fp32"
        # the hidden maps of fp32 and float64 agree on every element, and exact zeros occur
        x = case["x"] if case["x2"] is None else torch.cat([case["x"], case["x2"]], 1)
        cur64, cur32, zeros = x, x.float(), 0
        for w, b in zip(case["weights"][:-1], case["biases"][:-1]):
            cur64, cur32 = T._conv(cur64, w, b), T._conv(cur32, w.float(), b.float())
            assert torch.equal(cur64, cur32.double())
            zeros += int((cur64 == 0).sum())
            cur64, cur32 = torch.relu(cur64), torch.relu(cur32)
        assert zeros > 0
    else:
        for v in case["checks"]:
            assert v > 1.0, "a hidden pre-activation is within reach of a sign flip"
    for t in [case["x"], case["dy"], *case["weights"], *case["biases"]]:
        assert torch.equal(t, t.float().double()), "a case value is not fp32-representable"
    # the fp32 oracle is usable on every quantity (case_gate raises above 1.25e-5)
    for label, e in T.oracle_errors(name).items():
        T.case_gate(e)
    if case["final"] == "heatmap":
        out = r64["out"]
        clamped = (out == 1e-4) | (out == 1 - 1e-4)
        assert clamped.any() and not clamped.all()


def test_cases_reach_their_geometry():
    g = {n: T.geometry(n) for n in T.CASES}
    assert g["dy_3x5_c1"]["M"] < T.TILE and T.TILE < g["dy_5x7_c1"]["M"] < T.OUT_SLAB
    assert g["dy_one_tile_c2"]["M"] == T.TILE and g["dy_one_tile_c2"]["tiles"] == 1
    big = g["dy_17x33_sec_c3"]
    assert big["M"] % T.TILE and big["M"] % T.SLAB and big["slabs"] > 1 and big["chunks"] == 1
    assert g["dy_17x33_sparse_c8"]["active"] == 3 and g["dy_zero_c10"]["active"] == 0
    assert g["lin_tile32_c16"]["active"] == T.TILE and g["lin_tile33_c10"]["active"] == T.TILE + 1
    assert g["lin_tile33_c10"]["tiles"] == 2
    assert g["lin_slab257_c2"]["active"] == T.SLAB + 1 and g["lin_slab257_c2"]["slabs"] == 2
    two = g["lin_two_chunks_c2"]
    assert two["chunks"] == 2 and two["chunk"] == 576 and two["M"] - two["chunk"] not in (0, two["chunk"])
    assert {T.CASES[n][4] for n in T.CASES} >= {1, 2, 3, 8, 10, 16}
    # one-pixel-high / -wide maps, the depths, the widths of the first layer's k loop
    assert g["dy_1x40_c2"]["taps_inside"] == 3 == g["dy_40x1_sec_c2"]["taps_inside"] and g["dy_1x1_c3"]["taps_inside"] == 1
    assert g["dy_1x1_c3"]["M"] == 2 and g["dy_40x1_sec_c2"]["K"] == 67
    assert {g[n]["n_hidden"] for n in T.CASES} == {0, 1, 2} and g["dy_nh1_c4"]["n_hidden"] == 1
    cx72, cx8, c512 = g["dy_cx72_sec_c3"], g["dy_cx8_c2"], g["lin_cin512_c2"]
    assert 0 < cx72["kvec"] == 64 < T.CASES["dy_cx72_sec_c3"][1] == 72 < cx72["K"] == 75        # the k-tail reads both sources
    assert cx8["kvec"] == 0 and cx8["K"] == 8
    assert c512["K"] == 512 and (c512["K"] + 31) // 32 == 16 and c512["kvec"] == 448
    # a dense list above the grid of head_out_bwd_data_kernel, in one chunk
    for n in ("lin_8img_dense_c3", "lin_8img_heat_c10"):
        assert g[n]["chunks"] == 1 and g[n]["chunk"] == 4544 and g[n]["bwd_data_grid"] == T.OUT_BWD_GRID_CAP < g[n]["active"] == 4488
    assert T.CASES["lin_8img_heat_c10"][4] == 10 and T.CASES["lin_8img_heat_c10"][10] == "heatmap"
    # five chunks, the last ragged; a list that ends strictly inside chunk 1 with three empty chunks behind it
    five, part = g["lin_8img_5chunks_c2"], g["lin_8img_1500_c2"]
    assert five["chunks"] == 5 and five["chunk"] == 1088 and five["M"] - 4 * five["chunk"] == 136 and five["empty_chunks"] == 0
    assert five["list_end_chunk"] == 4 and five["list_end_at"] == 136
    assert part["chunks"] == 5 and part["list_end_chunk"] == 1 and 0 < part["list_end_at"] == 412 < part["chunk"]
    assert part["empty_chunks"] == 3
    # every earlier case is below the caps: the loops are reached by the cases named for them alone
    assert max(g[n]["active"] for n in T.CASES if not n.startswith("lin_8img")) < T.OUT_BWD_GRID_CAP
    assert max(g[n]["chunk"] * T.CASES[n][4] for n in T.CASES) <= T.OUT_FWD_THREAD_CAP
    assert max(g[n]["chunk"] // T.TILE for n in T.CASES) <= T.GEMM_GRID_CAP
    # the dY patterns are what geometry() counts
    for n in T.CASES:
        dy = T.build(n)["dy"]
        assert int((dy != 0).any(dim=1).sum()) == g[n]["active"]
    sp = T.build("dy_17x33_sparse_c8")["dy"]
    assert (sp[0, :, 0, 0] != 0).any() and (sp[0, :, -1, -1] != 0).any() and not (sp[1] != 0).any()
    # the chunk lengths are the library's own
    from centerfusiondetect3d_amd import _lib
    lib = _lib.load()
    for n, (B, _, _, _, _, h, w, _, _, chunk_px, _) in T.CASES.items():
        assert lib.cf_head_bwd_chunk_px(B, h, w, chunk_px) == g[n]["chunk"]
    for n, (base, R, chunk_px, _) in T.REPLICATED.items():
        B, _, _, _, _, h, w = T.CASES[base][:7]
        assert lib.cf_head_bwd_chunk_px(R * B, h, w, chunk_px) == T.rep_geometry(n)["chunk"]
    assert lib.cf_head_bwd_workspace_bytes(2, 17, 33, 67, 2, 576) < lib.cf_head_bwd_workspace_bytes(2, 17, 33, 67, 2, 0)
    assert lib.cf_head_train_workspace_bytes(2, 17, 33, 67, 2, 0) < lib.cf_head_bwd_workspace_bytes(2, 17, 33, 67, 2, 0)


def test_replicated_cases_reach_their_geometry():
    caps, dflt = T.rep_geometry("rep234_gridcaps"), T.rep_geometry("rep64_default_chunk")
    # both forward grid caps bind in the first chunk, and a second chunk follows it
    assert caps["M"] == 131274 and caps["chunk"] == 131136 and caps["chunks"] == 2 and caps["M"] - caps["chunk"] == 138
    assert caps["tiles"] == 4098 > T.GEMM_GRID_CAP and caps["out_elems"] > T.OUT_FWD_THREAD_CAP
    assert caps["chunk"] > T.GEMM_GRID_CAP * T.TILE                     # positions only the second pass of the loop reaches
    # the list: 33 + 3 + 561 positions out of the first, a middle and the last of 513 compaction blocks
    assert caps["active"] == 597 and caps["compact_blocks"] == 513
    blocks = caps["active_blocks"]
    assert blocks[0] == 0 and blocks[-1] == 512 and any(200 < b < 300 for b in blocks)
    # the default chunk: 32768 + 3136, the boundary strictly inside image 58, which carries a gradient as do the first and last
    assert dflt["M"] == 35904 and dflt["chunk"] == T.DEFAULT_CHUNK and dflt["chunks"] == 2 and dflt["M"] - dflt["chunk"] == 3136
    assert dflt["split_images"] == [58] and T.rep_build("rep64_default_chunk")["images"] == [0, 58, 63] and dflt["images"] == 64
    assert dflt["active"] == 33 + 2 * 561
    for n in T.REPLICATED:
        rep, (base, R, _, dys) = T.rep_build(n), T.REPLICATED[n]
        B = T.CASES[base][0]
        # the dY is zero outside the named images, fp32-representable, and the small batch is those images of the replicated one
        live = (rep["dy_full"] != 0).flatten(1).any(dim=1).nonzero().flatten().tolist()
        assert live == rep["images"] == sorted(dys)
        assert torch.equal(rep["dy_full"][rep["images"]].double(), rep["small"]["dy"])
        x, x2 = T.rep_sources(n)
        assert x.shape[0] == R * B and torch.equal(x[rep["images"]].double(), rep["small"]["x"])
        assert torch.equal(x.view(R, B, *x.shape[1:]), rep["base"]["x"].float().expand(R, *rep["base"]["x"].shape))
        if x2 is not None:
            assert torch.equal(x2[rep["images"]].double(), rep["small"]["x2"])
        for img, pattern in dys.items():
            n_act = int((rep["dy_full"][img] != 0).any(dim=0).sum())
            assert n_act == (x.shape[2] * x.shape[3] if pattern == "base" else 3 if pattern == "sparse" else pattern[1])
        # linear family: the masks cannot flip; the fp32 oracle is usable on every quantity (case_gate raises above 1.25e-5)
        assert rep["base"]["family"] == "linear"
        for label, e in T.rep_oracle_errors(n).items():
            T.case_gate(e)


def test_head_train_struct_layout_matches_c(tmp_path):
    from centerfusiondetect3d_amd import _lib
    prog = tmp_path / "szh.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cf_hip.h"\nint main(){'
                    'printf("%zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(cf_head_train_args), offsetof(cf_head_train_args, chunk_px),'
                    'offsetof(cf_head_train_args, weight), offsetof(cf_head_train_args, y), offsetof(cf_head_train_args, gw),'
                    'offsetof(cf_head_train_args, gb), offsetof(cf_head_train_args, workspace_bytes), CF_HEAD_TRAIN_MAX_HIDDEN);'
                    'return 0;}')
    exe = tmp_path / "szh"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    A = _lib.HeadTrainArgs
    assert got == [ctypes.sizeof(A), A.chunk_px.offset, A.weight.offset, A.y.offset, A.gw.offset, A.gb.offset,
                   A.workspace_bytes.offset, _lib.CF_HEAD_TRAIN_MAX_HIDDEN]


def test_entry_points_validate_before_the_device():
    from centerfusiondetect3d_amd import _lib
    lib = _lib.load()
    a = _lib.HeadTrainArgs()
    assert lib.cf_head_train_forward(ctypes.byref(a), None) == -22
    assert lib.cf_head_backward(ctypes.byref(a), None) == -22
    a.B, a.h, a.w, a.n_hidden, a.n_out, a.hidden = 1, 4, 8, 3, 1, 256
    assert lib.cf_head_backward(ctypes.byref(a), None) == -22 and b"n_hidden" in lib.cf_last_error()
    a.n_hidden, a.n_out = 0, 17
    assert lib.cf_head_backward(ctypes.byref(a), None) == -22 and b"n_out" in lib.cf_last_error()
    a.n_out, a.hidden = 16, 128
    assert lib.cf_head_backward(ctypes.byref(a), None) == -22 and b"256" in lib.cf_last_error()
    assert lib.cf_head_bwd_workspace_bytes(0, 1, 1, 64, 0, 0) == 0


def _head(cin=64, n_hidden=0, cout=2, dtype=torch.float32, hid=256):
    ws = [torch.zeros(hid, cin, 3, 3, dtype=dtype)] + [torch.zeros(hid, hid, 1, 1, dtype=dtype)] * n_hidden + \
        [torch.zeros(cout, hid, 1, 1, dtype=dtype)]
    return ws, [torch.zeros(w.shape[0], dtype=dtype) for w in ws]


def test_head_stack_error_paths_without_a_device():
    from centerfusiondetect3d_amd import _lib, ops
    x = torch.zeros(1, 64, 4, 8)
    ws, bs = _head()
    with pytest.raises(_lib.CfHipError):
        ops.head_stack(x, ws, bs)                                   # CPU tensors
    with pytest.raises(NotImplementedError, match="float32"):
        ops.head_stack(x.double(), *_head(dtype=torch.float64))
    with pytest.raises(NotImplementedError, match="float32"):
        ops.head_stack(x, [w.half() for w in ws], bs)
    with pytest.raises(NotImplementedError, match="256"):
        ops.head_stack(x, *_head(hid=128))                          # hidden width
    with pytest.raises(NotImplementedError, match="16"):
        ops.head_stack(x, *_head(cout=17))                          # outputs
    with pytest.raises(NotImplementedError, match="hidden"):
        ops.head_stack(x, *_head(n_hidden=3))                       # depth
    with pytest.raises(NotImplementedError):
        ops.head_stack(x, *_head(cin=67))                           # the first layer does not fit the sources
    with pytest.raises(ValueError):
        ops.head_stack(x, ws, bs, final="softmax")


def _config(kind, freeze=True):
    from centerfusiondetect3d_amd import config as cfg
    make = {"middle": cfg.centerfusion_middle_config, "centernet": cfg.centernet_config, "early": cfg.centerfusion_early_config}
    c = make[kind]((64, 64))
    c.MODEL.FREEZE_BACKBONE = bool(freeze)
    return c


@pytest.mark.parametrize("kind", ["middle", "centernet"])
def test_freeze_backbone_sets_requires_grad_at_construction(kind):
    from centerfusiondetect3d_amd.model import getModel
    m = getModel(_config(kind, freeze=True))
    heads = [n for n, p in m.named_parameters() if n.startswith("detectHead_0.")]
    assert heads and all(p.requires_grad == n.startswith("detectHead_0.") for n, p in m.named_parameters())
    assert not m.training
    frozen = getModel(_config(kind, freeze=False))
    assert not any(p.requires_grad for p in frozen.parameters())      # as before: an inference model
    # training without FREEZE_BACKBONE keeps raising, and names the one mode that is implemented
    frozen.train()
    with pytest.raises(NotImplementedError, match="FREEZE_BACKBONE"):
        frozen(torch.zeros(1, 3, 64, 64))
