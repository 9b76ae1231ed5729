"""CPU side of the head training path: the constructions of tests/heads_train_ref.py hold what they promise, the cases reach the
geometry they are named for, the fp32 oracle is usable on every case, `ops.head_stack` and `DLASeg` refuse what they do not
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
    assert lib.cf_head_bwd_workspace_bytes(2, 17, 33, 67, 2, 576) < lib.cf_head_bwd_workspace_bytes(2, 17, 33, 67, 2, 0)
    assert lib.cf_head_train_workspace_bytes(2, 17, 33, 67, 2, 0) < lib.cf_head_bwd_workspace_bytes(2, 17, 33, 67, 2, 0)


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
