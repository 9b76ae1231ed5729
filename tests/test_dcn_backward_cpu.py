"""CPU: what the deformable convolution's backward tests stand on.  (1) The yardstick: float64 autograd through
oracle/dcn_ref.deform_conv2d equals central finite differences in float64 for all five arguments (needs no library).
(2) The ctypes mirror of cf_dcn_bwd_args has the C compiler's layout."""
import ctypes
import os
import subprocess

import torch

from oracle import dcn_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_oracle_autograd_equals_central_differences():
    B, Ci, Co, H, W = 1, 2, 3, 4, 5
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x, w, b, R = r(B, Ci, H, W), r(Co, Ci, 3, 3), r(Co), r(B, Co, H, W)
    mask = torch.sigmoid(r(B, 9, H, W))
    # offsets whose sampling coordinates keep 0.1 from every integer: the differences (h = 1e-6) never cross a kink
    ys = torch.arange(H, dtype=torch.float64).view(H, 1).expand(H, W)
    xs = torch.arange(W, dtype=torch.float64).view(1, W).expand(H, W)
    base = torch.stack([(ys - 1 + k // 3) if c == 0 else (xs - 1 + k % 3) for k in range(9) for c in (0, 1)])
    pos = base + 1.5 * r(B, 18, H, W)
    off = torch.floor(pos) + (pos - torch.floor(pos)).clamp(0.1, 0.9) - base
    assert float(((base + off) - torch.round(base + off)).abs().min()) >= 0.1 - 1e-12
    args = [x, off, w, b, mask]

    def loss(a):
        return (dcn_ref.deform_conv2d(a[0], a[1], a[2], a[3], (1, 1), (1, 1), (1, 1), a[4]) * R).sum()

    leaves = [t.clone().requires_grad_(True) for t in args]
    loss(leaves).backward()
    h = 1e-6
    for i, name in enumerate(("input", "offset", "weight", "bias", "mask")):
        fd = torch.zeros_like(args[i])
        flat, fdf = args[i].reshape(-1), fd.view(-1)           # (a view: the perturbation is written in place and taken back)
        for j in range(flat.numel()):
            v = float(flat[j])
            flat[j] = v + h
            up = float(loss(args))
            flat[j] = v - h
            dn = float(loss(args))
            flat[j] = v
            fdf[j] = (up - dn) / (2 * h)
        err = float((leaves[i].grad - fd).abs().max() / fd.abs().max())
        # the loss is piecewise bilinear / linear in every argument between the kinks: central differences are exact up to
        # rounding, eps * |loss| / h ~ 1e-16 * 1e2 / 1e-6 = 1e-8 absolute
        assert err < 1e-6, (name, err)


def test_dcn_bwd_args_layout_matches_c(tmp_path):
    from centerfusiondetect3d_amd import _lib
    fields = [n for n, _ in _lib.DcnBwdArgs._fields_]
    prog = tmp_path / "bwd.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cf_hip.h"\nint main(){'
                    'printf("%zu", sizeof(cf_dcn_bwd_args));'
                    + "".join(f'printf(" %zu", offsetof(cf_dcn_bwd_args, {n}));' for n in fields)
                    + 'printf("\\n");return 0;}')
    exe = tmp_path / "bwd"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(_lib.DcnBwdArgs)] + [getattr(_lib.DcnBwdArgs, n).offset for n in fields]


def test_dcn_bwd_entry_points_validate_without_a_gpu():
    """bad arguments are refused before the device is touched; a launch with no output wanted succeeds and does nothing"""
    from centerfusiondetect3d_amd import _lib
    lib = _lib.load()
    a = _lib.DcnBwdArgs()
    a.B, a.H, a.W, a.C, a.N = 1, 4, 4, 48, 8
    assert lib.cf_dcn_v2_bwd_data(ctypes.byref(a), None) == -22 and b"multiple of 32" in lib.cf_last_error()
    a.C = 32
    assert lib.cf_dcn_v2_bwd_data(ctypes.byref(a), None) == 0
    assert lib.cf_dcn_v2_bwd_weight(ctypes.byref(a), None) == 0
    n = lib.cf_dcn_v2_bwd_workspace_bytes(1, 4, 4, 32, 8)
    assert n >= (9 * 8 * 32 + 8) * 4 and n % ((9 * 8 * 32 + 8) * 4) == 0
    assert lib.cf_dcn_v2_bwd_workspace_bytes(0, 4, 4, 32, 8) == 0


def test_new_cases_reach_the_launch_size_branches_they_are_there_for():
    """the comments on the cases of tests/dcn_backward_ref.py, as assertions: the restated slab geometry of every case added for
    a launch-size branch is the one listed, and the restatement's slab count is the library's (its workspace size says it)"""
    from centerfusiondetect3d_amd import _lib
    from tests import dcn_backward_ref as T
    lib = _lib.load()
    assert sorted(T.SLAB_GEOMETRY) == list(T.NEW_CASES)
    for i, (B, C, N, H, W, _, _) in enumerate(T.CASES):
        slabs = T.slab_geometry(B * H * W, C, N)[0]
        assert lib.cf_dcn_v2_bwd_workspace_bytes(B, H, W, C, N) == slabs * (9 * N * C + N) * 4, T.CASES[i]
    for i in T.NEW_CASES:
        B, C, N, H, W, _, _ = T.CASES[i]
        slabs, cap, slab_px, last = geo = T.slab_geometry(B * H * W, C, N)
        assert geo == T.SLAB_GEOMETRY[i], (T.CASES[i], geo)
        assert slab_px % 2 == 0 and 0 < last <= slab_px and (slabs - 1) * slab_px + last == B * H * W
    old = [T.slab_geometry(B * H * W, C, N) for B, C, N, H, W, _, _ in T.CASES[:6]]
    assert max(g[0] for g in old) == 3 and all(g[0] < g[1] for g in old)          # the cap never bound before
    for i in (7, 8, 9):                                                            # the cap binds: fewer slabs than 256-pixel ones
        B, C, N, H, W, _, _ = T.CASES[i]
        slabs, cap, _, _ = T.SLAB_GEOMETRY[i]
        assert slabs == cap < (B * H * W + 255) // 256
    assert -(-35 * 53 // 7) % 2 == 1                                               # (35,53): an odd length, rounded up
    assert 113 * 256 < 116 * 250 <= 114 * 256                                      # (116,250): one 256-pixel slab more than the cap
    # the data kernel: chunks per wave, dynamic LDS against the 32768-byte floor and the 64 KB default, the most that fits
    assert max(T.data_kernel_geometry(C, N)[0] for _, C, N, _, _, _, _ in T.CASES[:6]) == 2
    assert T.data_kernel_geometry(512, 256) == (4, 32768, 58368)
    assert T.data_kernel_geometry(64, 320)[2] == 66560 > 65536
    assert T.data_kernel_geometry(32, 1024)[2] == 156672 <= 163840
    assert all((B * H * W) % 32 for B, _, _, H, W, _, _ in (T.CASES[6], T.CASES[13], T.CASES[14]))     # partial 32-pixel tiles
