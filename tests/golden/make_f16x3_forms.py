#!/usr/bin/env python3
"""The INPUTS of tests/golden/f16x3_forms.npz: the sweep the launch rules of the split-fp16 3x3 convolution
(cf_conv3x3_f16.hip) and DCN (cf_gemm_f16.hip: dcn_f16x3_impl) were recorded on.

The fixture's `conv_out` / `dcn_out` columns are NOT made here: they are what the launchers of the commit before the rule
became one reported function chose for these rows, written down by a probe in front of their launch calls
(docs/experiments/f16x3_tile_form_rule.md has the probe).  They stay as recorded: tests/test_f16x3_forms_cpu.py holds the
exports cf_conv3x3_tile_form / cf_dcn_v2_f16x3_form to them row by row.  This script regenerates the input rows only

    python tests/golden/make_f16x3_forms.py            # compare the fixture's input rows with the sweep below
    python tests/golden/make_f16x3_forms.py --inputs F # write the input rows alone to F (.npz), for a recorder

Row formats: tests/f16x3_forms.py.  The sweep sits on both sides of everything the rules read: one round of <= 256 workgroups
in each variant (8x16 tiles x B, x 2 for 128 channels, x G for groups; 32-pixel runs x channel blocks; stride-2 half tiles),
H W >= 4096, H W <= 512, the 6 % tile cover (124x124 / 125x125), 128-pixel tiles >= 160 (28x50 at B = 14 / 15, 7 / 8 with 512
channels), the widths where each flat patch stops fitting (31/32, 63/64, 95/96, 127/128, 255/256) and 150, 300, 512; for the
DCN one round of 64-pixel tiles x ks x G, the K-split maps of 512 / 513 and 2048 / 2050 pixels, N not a multiple of 4, and
N_pad of 32, 64, 96, 128, 192, 256, 512."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "f16x3_forms.npz")

BATCHES = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 15, 16)
SMALL_MAPS = ((7, 13), (8, 6), (9, 11), (14, 25), (16, 32), (19, 27), (13, 19), (23, 31), (20, 30), (28, 50), (31, 23), (37, 41),
              (45, 67), (17, 31), (56, 60))
WIDTH_MAPS = tuple((5, w) for w in (31, 32, 63, 64, 95, 96, 127, 128, 150, 255, 256, 300, 512))
BIG_MAPS = ((64, 64), (63, 65), (56, 100), (37, 150), (40, 150), (40, 300), (112, 200), (124, 124), (125, 125), (127, 127),
            (96, 128), (40, 512), (28, 150))
MAPS = SMALL_MAPS + WIDTH_MAPS + BIG_MAPS


def conv_sweep():
    rows = []
    for H, W in MAPS:
        for B in BATCHES:
            for Ci in (16, 32, 48, 64, 96, 128, 256, 512):                  # cf_conv3x3_f16x3, stride 1
                for N in (27, 64, 128, 192, 256, 512):
                    rows.append((0, B, H, W, Ci, N, 1, 1, 0))
            for Ci in (16, 64, 256):                                        # ... stride 2 (with a residual: forwarded)
                for N in (27, 64, 128, 192, 256, 512):
                    rows.append((0, B, H, W, Ci, N, 2, 1, 0))
            rows.append((0, B, H, W, 64, 64, 2, 1, 1))
            for Cc in (64, 128, 192, 256, 512):                             # cf_conv3x3_root_f16x3, 0-2 children
                for kids in (0, 1, 2):
                    rows.append((1, B, H, W, Cc, Cc, 1, 1, kids))
            for Ci, N, Cp in ((64, 64, 32), (64, 128, 64), (128, 128, 96), (96, 192, 32), (256, 256, 128), (512, 512, 256)):
                rows.append((2, B, H, W, Ci, N, 1, 1, Cp))                  # cf_conv3x3_proj_f16x3
            for G in (1, 2, 3, 4):                                          # cf_conv3x3_f16x3_grouped
                for Ci in (16, 32, 48, 64, 128):
                    rows.append((3, B, H, W, Ci, 27, 1, G, 0))
    # what the launch refuses: a projection onto 32 outputs, a grouped launch of 64 outputs, a stride of 3
    rows += [(2, 1, 14, 25, 64, 27, 1, 1, 32), (3, 2, 14, 25, 64, 64, 1, 2, 0), (0, 1, 14, 25, 64, 64, 3, 1, 0)]
    return np.asarray(rows, dtype=np.int32)


DCN_MAPS = ((7, 10), (7, 13), (9, 14), (14, 25), (16, 32), (19, 27), (32, 64), (41, 50), (28, 50), (37, 70), (50, 45), (56, 100),
            (112, 200))


def dcn_sweep():
    rows = []
    for H, W in DCN_MAPS:
        for B in BATCHES:
            for Cc in (32, 64, 128, 256, 512):
                for N in (27, 30, 48, 64, 96, 126, 128, 192, 254, 256, 512):
                    for ws in (0, 1):
                        for G in (1, 2, 3, 4):
                            if G == 1 or (N in (48, 64, 128) and Cc <= 256):
                                rows.append((B, H, W, Cc, N, G, ws))
    rows += [(1, 14, 25, 64, 30, 2, 1), (1, 14, 25, 64, 256, 2, 1), (1, 14, 25, 48, 64, 1, 1)]      # refused
    return np.asarray(rows, dtype=np.int32)


def main():
    conv, dcn = conv_sweep(), dcn_sweep()
    print(f"{len(conv)} conv rows, {len(dcn)} DCN rows")
    if "--inputs" in sys.argv:
        np.savez_compressed(sys.argv[sys.argv.index("--inputs") + 1], conv_in=conv.T, dcn_in=dcn.T)
        return 0
    fx = np.load(FIXTURE)
    same = np.array_equal(fx["conv_in"].T, conv) and np.array_equal(fx["dcn_in"].T, dcn)      # (stored by column: it compresses 5x better)
    print("the fixture's input rows are this sweep" if same else "the fixture's input rows DIFFER from this sweep")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
