"""CPU: the launch rule of the split-fp16 3x3 convolution (csrc/cf_conv3x3_f16.hip: conv3_pick) and DCN (csrc/cf_gemm_f16.hip:
dcn_pick) as the library itself reports it - `cf_conv3x3_tile_form` and `cf_dcn_v2_f16x3_form`, the functions every launching
entry point chooses its kernel through.

*The export is the recorded rule.*  tests/golden/f16x3_forms.npz holds, for 66,423 conv calls (cf_conv3x3_f16x3 at stride 1 and
2, _root_ with 0-2 children, _proj_, _grouped with 1-4 groups; 41 maps, batches 1-16, 16-512 channels) and 35,493 DCN calls,
what the launchers chose before the rule was one function: form, grid, threads, LDS bytes, patch rows, tile counts, rounds
(tests/golden/make_f16x3_forms.py regenerates the inputs; docs/experiments/f16x3_tile_form_rule.md says how the answers were
recorded).  Every row is reproduced exactly, refusals included, so moving a threshold or a candidate fails here.

*The case tables reach what they claim*: every row of CONV_CASES (entry "patch"), ROOT_CASES, PROJ_CASES and DCN_CASES of
tests/f16x3_ref.py sits on the tiling its table names.

*Coverage*: the sweep reaches all 50 instantiations of conv3x3_f16x3_kernel / _grouped (the 23 tile shapes of CF_CONV3_TILES in
their plain, projection, fused-Root, grouped and stride-2 variants) and all 8 of dcn_f16x3_kernel / _grouped: none is compiled
but not reached."""
import os

import numpy as np
import pytest

from tests import f16x3_forms as FM
from tests import f16x3_ref as R
from tests.golden import make_f16x3_forms as MK

FIELDS = ("WC", "WP", "WK", "RT", "NU", "DB", "MINB", "T2", "CT", "S2", "ROOT", "PROJ", "GRP")


@pytest.fixture(scope="module")
def record():
    fx = np.load(os.path.join(os.path.dirname(__file__), "golden", "f16x3_forms.npz"))
    return {k: fx[k].T.tolist() for k in fx.files}             # (stored by column)


@pytest.fixture(scope="module")
def ops():
    from centerfusiondetect3d_amd import ops
    return ops


def _expected(rec):
    """a fixture row (status, answer...) as the export's answer"""
    return FM.REFUSED if rec[0] == FM.REFUSED else tuple(rec[1:])


def test_the_fixture_rows_are_the_sweep(record):
    assert record["conv_in"] == MK.conv_sweep().tolist() and record["dcn_in"] == MK.dcn_sweep().tolist()
    assert len(record["conv_in"]) == len(record["conv_out"]) > 29376 and len(record["dcn_in"]) == len(record["dcn_out"]) > 10000


def test_the_conv_export_is_the_recorded_rule(record, ops):
    assert len(ops.CONV3_FORM_FIELDS) == len(record["conv_out"][0]) - 1
    n_forwarded = n_refused = 0
    for row, rec in zip(record["conv_in"], record["conv_out"]):
        got, want = FM.conv_form(tuple(row)), _expected(rec)
        assert got == want, (row, got, want)
        n_refused += want == FM.REFUSED
        n_forwarded += want != FM.REFUSED and want[0] == 0
    assert (n_forwarded, n_refused) == (6501, 1123)              # both answers are exercised, not only "patch"


def test_the_dcn_export_is_the_recorded_rule(record, ops):
    assert len(ops.DCN_FORM_FIELDS) == len(record["dcn_out"][0]) - 1
    for row, rec in zip(record["dcn_in"], record["dcn_out"]):
        got, want = FM.dcn_form(tuple(row)), _expected(rec)
        assert got == want, (row, got, want)
    assert sum(rec[0] == FM.REFUSED for rec in record["dcn_out"]) == 3


def test_the_sweep_reaches_every_instantiation(record, ops):
    f0 = ops.CONV3_FORM_FIELDS.index("WC") + 1                    # (+ 1: the status column)
    reached = {tuple(rec[f0:f0 + 13]) for rec in record["conv_out"] if rec[0] == 0 and rec[1] == 1}

    def variants(shapes, **flag):
        return {s + tuple(int(flag.get(k, 0)) for k in ("S2", "ROOT", "PROJ", "GRP")) for s in shapes}
    #          WC WP WK RT NU DB MINB T2 CT
    offset = {(1, 4, 1, 1, 4, 1, 2, 1, 1), (1, 4, 1, 1, 6, 1, 2, 1, 2), (1, 4, 1, 1, 8, 1, 2, 0, 2), (1, 4, 1, 1, 12, 1, 1, 0, 2),
              (1, 1, 4, 1, 8, 1, 2, 0, 2), (1, 1, 4, 1, 12, 1, 2, 0, 2), (1, 2, 2, 1, 12, 1, 2, 0, 2)}
    rooted = {(1, 4, 1, 2, 4, 1, 2, 1, 1), (1, 4, 1, 2, 6, 1, 2, 1, 2), (1, 4, 1, 2, 6, 1, 2, 0, 2), (2, 2, 1, 2, 4, 1, 2, 1, 2),
              (2, 2, 1, 2, 6, 1, 2, 0, 2), (4, 1, 1, 2, 4, 1, 2, 0, 1), (4, 1, 1, 2, 4, 1, 2, 0, 2), (4, 1, 1, 2, 2, 1, 2, 1, 2)}
    wide = rooted | {(2, 1, 2, 2, 4, 1, 2, 0, 1), (2, 1, 2, 2, 4, 1, 2, 0, 2), (4, 2, 1, 2, 2, 1, 1, 0, 2), (4, 2, 1, 2, 2, 1, 1, 1, 2)}
    stride2 = {(1, 4, 1, 2, 9, 0, 2, 1, 1), (2, 2, 1, 2, 5, 1, 2, 1, 1), (4, 1, 1, 2, 3, 1, 2, 1, 1), (4, 1, 1, 2, 5, 1, 2, 1, 2)}
    expected = (variants(offset) | variants(offset, GRP=1) | variants(wide) | variants(wide, PROJ=1) | variants(rooted, ROOT=1) |
                variants(stride2, S2=1))
    assert len(expected) == 50 and reached == expected, (sorted(expected - reached), sorted(reached - expected))
    #                   WC WP RT COAL CT grouped
    dcn = {tuple(rec[1:6]) + (row[5] > 1,) for row, rec in zip(record["dcn_in"], record["dcn_out"]) if rec[0] == 0}
    assert dcn == {(4, 1, 1, 1, 2, False), (4, 1, 1, 0, 2, False), (2, 2, 1, 1, 1, False), (2, 2, 1, 0, 2, False), (4, 1, 2, 1, 2, False),
                   (4, 1, 2, 0, 2, False), (4, 1, 1, 1, 2, True), (2, 2, 1, 1, 1, True)}


def _assert_tiling(ops, answer, fields, tiling, what):
    assert answer != FM.REFUSED, what
    got = dict(zip(fields, answer))
    assert {k: got[k] for k in tiling} == tiling, (what, got)
    return got


def test_the_case_tables_reach_the_tiling_they_name(ops):
    assert set(R.CONV_TILINGS) == {n for n, c in R.CONV_CASES.items() if c["entry"] == "patch"}
    assert set(R.ROOT_TILINGS) == set(R.ROOT_CASES) and set(R.PROJ_TILINGS) == set(R.PROJ_CASES) and set(R.DCN_TILINGS) == set(R.DCN_CASES)
    for name, t in R.CONV_TILINGS.items():
        c = R.CONV_CASES[name]
        got = _assert_tiling(ops, FM.conv_form((FM.PLAIN, c["B"], c["H"], c["W"], c["Ci"], c["Co"], c["stride"], 1, int(c["res"]))),
                             ops.CONV3_FORM_FIELDS, t, name)
        assert (got["patch"] == 0) == (c["form"] == "patch:forwarded_to_slot"), name
        assert got["patch"] == 0 or (got["S2"] == (c["stride"] == 2) and got["ROOT"] == got["PROJ"] == got["GRP"] == 0), name
    for name, t in R.ROOT_TILINGS.items():
        C_, B, H, W, kids, form = R.ROOT_CASES[name]
        got = _assert_tiling(ops, FM.conv_form((FM.ROOT, B, H, W, C_, C_, 1, 1, kids)), ops.CONV3_FORM_FIELDS, t, name)
        assert (got["fused"] == 0) == (form == "root:two_launches") and got["fused"] == got["ROOT"], name
    for name, t in R.PROJ_TILINGS.items():
        B, Cp, C_, H, W, _ = R.PROJ_CASES[name]
        got = _assert_tiling(ops, FM.conv_form((FM.PROJ, B, H, W, C_, C_, 1, 1, Cp)), ops.CONV3_FORM_FIELDS, t, name)
        assert got["PROJ"] == 1, name
    for name, t in R.DCN_TILINGS.items():
        B, Ci, Co, H, W, _, form = R.DCN_CASES[name]
        got = _assert_tiling(ops, FM.dcn_form((B, H, W, Ci, Co, 1, 1)), ops.DCN_FORM_FIELDS, t, name)
        assert (got["ks"] > 1) == (form in ("dcn:k_split_reduce", "dcn:two_row_tiles")), name
    # the grouped tables through the same export: the six-int answer of cf_conv3x3_grouped_form is a view of it
    for name, (G, B, H, W, Ci, t, _) in R.GROUPED_CONV_CASES.items():
        _assert_tiling(ops, FM.conv_form((FM.GROUPED, B, H, W, Ci, 27, 1, G, 0)), ops.CONV3_FORM_FIELDS, dict(t, patch=1, GRP=1), name)
        assert ops.conv3x3_grouped_form(FM.conv_call((FM.GROUPED, B, H, W, Ci, 27, 1, G, 0))[1]) == t, name
    for name, c in R.GROUPED_DCN_CASES.items():
        G, B, H, W, Ci, Co, k_split = *c[:6], c[8]
        got = _assert_tiling(ops, FM.dcn_form((B, H, W, Ci, Co, G, int(k_split))), ops.DCN_FORM_FIELDS, dict(COAL=1), name)
        assert (got["ks"] > 1) == k_split and got["grid_x"] == G * got["tiles"], name


def test_what_the_launch_refuses_is_refused_and_nothing_is_written(ops):
    import ctypes as C
    from centerfusiondetect3d_amd import _lib
    lib = _lib.load()
    blocks = FM.conv_call((FM.PLAIN, 1, 14, 25, 64, 64, 1, 1, 0))[1]
    form = (C.c_int32 * 23)(*([7] * 23))
    assert lib.cf_conv3x3_tile_form(4, ops.group_ptrs(blocks), 1, None, form) == FM.REFUSED           # no such entry point
    assert lib.cf_conv3x3_tile_form(0, ops.group_ptrs(blocks), 2, None, form) == FM.REFUSED           # one block, not two
    assert lib.cf_conv3x3_tile_form(0, ops.group_ptrs(blocks), 1, None, None) == FM.REFUSED
    assert lib.cf_conv3x3_tile_form(1, ops.group_ptrs(blocks * 2), 2, None, form) == FM.REFUSED       # a Root without its channels
    blocks[0].in_scale = 3.0                                                                          # not a power of two
    assert lib.cf_conv3x3_tile_form(0, ops.group_ptrs(blocks), 1, None, form) == FM.REFUSED
    assert list(form) == [7] * 23
    d = FM.dcn_blocks((1, 14, 25, 64, 64, 1, 1))
    assert lib.cf_dcn_v2_f16x3_form(ops.group_ptrs(d), 1, None) == FM.REFUSED
    assert lib.cf_dcn_v2_f16x3_form(ops.group_ptrs(d), 5, form) == FM.REFUSED                         # more than CF_MAX_GROUPS
    d[0].workspace_bytes = 16                                                                         # a K-split map, too small a workspace
    assert lib.cf_dcn_v2_f16x3_form(ops.group_ptrs(d), 1, form) == FM.REFUSED
