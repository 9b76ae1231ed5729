"""CPU side of the heads' input gradient (cf_head_backward_dx, `ops.head_stack(..., input_grad=True)`): the fp32 oracle of
tests/heads_dgrad_ref.py is usable on every case, the two exports validate their arguments before any device is touched and the
ABI number stands."""
import ctypes

import pytest
import torch

from tests import heads_dgrad_ref as D


@pytest.mark.parametrize("name", list(D.CASES))
def test_oracle_is_usable(name):
    case, errors = D.build(name), D.oracle_errors(name)
    assert ("gx2" in errors) == (case["x2"] is not None)
    for label, gate in D.gates(errors).items():           # (case_gate raises above 1.25e-5)
        print(f"[head dgrad oracle] {name:20s} {label:3s}: fp32 oracle {errors[label]:.2e}   gate {gate:.1e}")
    r64, _ = D.reference(name)
    assert r64["gx"].shape == case["x"].shape and (r64["gx2"] is None or r64["gx2"].shape == case["x2"].shape)
    if name == "dy_zero_c10":
        assert not r64["gx"].any() and errors["gx"] == 0.0
    else:
        assert r64["gx"].abs().max() > 0


@pytest.mark.parametrize("name", list(D.REPLICATED))
def test_replicated_oracle_is_usable(name):
    D.gates(D.rep_oracle_errors(name))


def test_sparse_case_reaches_only_the_neighbourhoods():
    """what the GPU test pins, on the float64 reference itself: gx vanishes outside the 3x3 neighbourhoods of the active pixels"""
    case, (r64, _) = D.build("dy_17x33_sparse_c8"), D.reference("dy_17x33_sparse_c8")
    near = torch.nn.functional.max_pool2d((case["dy"] != 0).any(dim=1, keepdim=True).double(), 3, 1, 1) > 0
    assert int(near.sum()) == 4 + 4 + 9 and not near[1].any()
    assert not (r64["gx"] * (~near)).any() and not (r64["gx2"] * (~near)).any()


def _args(_lib, c_x=64, c_x2=0):
    """an argument block that passes every check in front of the source-gradient ones (no pointer is ever followed)"""
    a = _lib.HeadTrainArgs()
    a.B, a.h, a.w, a.n_hidden, a.n_out, a.hidden = 1, 4, 8, 0, 1, 256
    a.x, a.c_x, a.x_stride = 4096, c_x, c_x
    if c_x2:
        a.x2, a.c_x2, a.x2_stride = 8192, c_x2, c_x2
    return a


def test_entry_points_validate_before_the_device():
    from centerfusiondetect3d_amd import _lib
    lib = _lib.load()
    assert lib.cf_abi_version() == 7
    empty = _lib.HeadTrainArgs()
    assert lib.cf_head_backward_dx(ctypes.byref(empty), 4096, 64, None, 0, None) == -22
    assert lib.cf_head_backward_dx(None, 4096, 64, None, 0, None) == -22 and b"null args" in lib.cf_last_error()
    a = _args(_lib)
    assert lib.cf_head_backward_dx(ctypes.byref(a), None, 64, None, 0, None) == -22 and b"both null" in lib.cf_last_error()
    assert lib.cf_head_backward_dx(ctypes.byref(a), 4096, 63, None, 0, None) == -22 and b"gx_stride" in lib.cf_last_error()
    assert lib.cf_head_backward_dx(ctypes.byref(a), 4096, 64, 8192, 4, None) == -22 and b"gx2 without x2" in lib.cf_last_error()
    a2 = _args(_lib, 64, 3)
    assert lib.cf_head_backward_dx(ctypes.byref(a2), None, 0, 8192, 2, None) == -22 and b"gx2_stride" in lib.cf_last_error()
    # past the source-gradient checks the shared ones go on: no weights were given
    assert lib.cf_head_backward_dx(ctypes.byref(a2), 4096, 64, 8192, 4, None) == -22 and b"layer 0" in lib.cf_last_error()
    assert b"cf_head_backward_dx" in lib.cf_last_error()
    # the plain backward is unchanged by the same block
    assert lib.cf_head_backward(ctypes.byref(a2), None) == -22 and b"cf_head_backward:" in lib.cf_last_error()


def test_workspace_bytes():
    from centerfusiondetect3d_amd import _lib
    lib = _lib.load()
    for bad in [(0, 1, 1, 64, 0, 0), (1, 0, 1, 64, 0, 0), (1, 1, 0, 64, 0, 0), (1, 1, 1, 0, 0, 0), (1, 1, 1, 64, -1, 0),
                (1, 1, 1, 64, 0, -64)]:
        assert lib.cf_head_bwd_dx_workspace_bytes(*bad) == 0
    for geo in [(1, 5, 7, 64, 0, 0), (2, 17, 33, 67, 2, 576), (16, 112, 200, 64, 0, 0), (1, 5, 7, 512, 0, 0), (1, 1, 1, 1, 0, 0)]:
        plain, dx = lib.cf_head_bwd_workspace_bytes(*geo), lib.cf_head_bwd_dx_workspace_bytes(*geo)
        # the second packed copy of the first layer's weights, [tap][o][c] fp32, rounded up to 16 bytes
        assert dx == plain + (9 * geo[3] * 256 * 4 + 15) // 16 * 16 and dx % 16 == 0


def test_input_grad_needs_device_tensors():
    from centerfusiondetect3d_amd import _lib, ops
    x = torch.zeros(1, 64, 4, 8, requires_grad=True)
    ws = [torch.zeros(256, 64, 3, 3), torch.zeros(2, 256, 1, 1)]
    bs = [torch.zeros(256), torch.zeros(2)]
    with pytest.raises(_lib.CfHipError):
        ops.head_stack(x, ws, bs, input_grad=True)
