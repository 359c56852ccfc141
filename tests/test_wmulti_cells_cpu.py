"""CPU: the case table of tests/test_gpu_weight_multi_cells.py covers the launch plan of the model-wide weight launches
(tests/wmulti_cells.py restates the host rules of csrc/fq_pc.hip as integers): every cell, every row body a cell can hold,
both sides of every threshold -- and what the suite covered before that table, pinned as data."""
import os
import re

from tests import wmulti_cells as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case_cells(case):
    return WC.Plan.of(case.layers).cells()


def test_every_cell_and_every_reachable_row_body_has_a_case():
    seen = set()
    for case in WC.CASES:
        plan = WC.Plan.of(case.layers)
        f, b = plan.cells()
        for bf, bb in plan.bodies():
            seen.add((f, bf))
            seen.add((b, bb))
    for cell in WC.FWD_CELLS + WC.BWD_CELLS:
        for body in WC.reachable_bodies(cell):
            assert (cell, body) in seen, (cell, body)
    assert {c for c, _ in seen} == set(WC.FWD_CELLS + WC.BWD_CELLS)
    # every estimator, AEWGS included (per-channel plans only), reaches every backward cell and each of its bodies
    for method in ("STE", "LSQ", "EWGS", "AEWGS"):
        got = set()
        for case in WC.CASES:
            if method in WC.estimators(case):
                plan = WC.Plan.of(case.layers)
                got.update((plan.cells()[1], bb) for _, bb in plan.bodies())
        assert got == {(cell, body) for cell in WC.BWD_CELLS for body in WC.reachable_bodies(cell)}, method
    # ... and nothing the rules call unreachable turns up in a plan
    assert all(body in WC.reachable_bodies(cell) for cell, body in seen)


def test_reachable_bodies_follow_from_the_rules():
    """An aligned row beyond NV * TB float4 exists only in the open-ended 8 x 256 cells and the generic kernels: swept over
    every max_row a plan can have, on both sides of the whole-tensor rule."""
    for max_row in range(1, 70001):
        for total_co, nlayers in ((8, 4), (9, 4)):
            for cell in (WC.fwd_cell(max_row, total_co, nlayers), WC.bwd_cell(max_row, total_co, nlayers)):
                row = max_row - max_row % 4              # the longest aligned row such a launch can hold
                if row:
                    assert WC.row_body(row, True, cell) in WC.reachable_bodies(cell), (max_row, cell)
                assert WC.row_body(max_row, False, cell) == "dword"


def test_each_case_is_a_small_plan_with_one_group_and_the_bodies_its_cell_can_hold():
    assert 14 <= len(WC.CASES) <= 22 and len(WC.CASE) == len(WC.CASES)
    for case in WC.CASES:
        plan = WC.Plan.of(case.layers)
        assert 3 <= plan.nlayers <= 5, case.name
        for layer, co in zip(case.layers, plan.co):
            assert (2 <= co <= 5) if layer[1] == "pc" else co == 1, (case.name, layer)
        assert plan.row[case.defining] == plan.max_row, case.name
        f, b = plan.cells()
        bodies = plan.bodies()
        for k, cell in ((0, f), (1, b)):
            # (an 8 x 256 cell holds an unstaged row only where the plan's longest row overflows it)
            want = {bd for bd in WC.reachable_bodies(cell)
                    if bd != "unstaged" or WC.row_body(plan.max_row - plan.max_row % 4, True, cell) == "unstaged"}
            assert {bd[k] for bd in bodies} == want, (case.name, cell)
        # a short aligned row, a 27-float row, and an aligned-length layer that starts off the 16-byte grid
        aligned = [i for i in range(plan.nlayers) if plan.row[i] % 4 == 0 and plan.elem_off[i] % 4 == 0]
        assert any(plan.row[i] == 36 for i in aligned), case.name
        odd = [i for i in range(plan.nlayers) if plan.row[i] == 27]
        assert len(odd) == 1 and odd[0] + 1 < plan.nlayers, case.name
        nxt = odd[0] + 1
        assert plan.row[nxt] % 4 == 0 and plan.elem_off[nxt] % 4 != 0, case.name
        # a default plan keeps per-channel rows of more than 8192 floats out (multi.py MAX_PLAN_ROW)
        long = any(layer[1] == "pc" and r > 8192 for layer, r in zip(case.layers, plan.row))
        assert case.long_rows == long, case.name
        assert all(r <= WC.PT_MAX_ELEMS for layer, r in zip(case.layers, plan.row) if layer[1] == "pt")
        assert WC.estimators(case) == (("STE", "LSQ", "EWGS") if case.per_tensor else ("STE", "LSQ", "EWGS", "AEWGS"))
    assert any(c.channels_last for c in WC.CASES if c.per_tensor)
    assert any(c.channels_last for c in WC.CASES if not c.per_tensor)


def test_every_threshold_has_a_case_on_each_side_four_floats_apart():
    for kind, below, above in WC.THRESHOLDS:
        lo, hi = WC.Plan.of(WC.CASE[below].layers), WC.Plan.of(WC.CASE[above].layers)
        assert hi.max_row - lo.max_row == 4 and lo.max_row % 4 == 0, (below, above)
        assert (lo.total_co, lo.nlayers) == (hi.total_co, hi.nlayers)
        (fl, bl), (fh, bh) = lo.cells(), hi.cells()
        if kind in ("fwd", "both"):
            assert fl != fh, (below, above)
        if kind in ("bwd", "both"):
            assert bl != bh, (below, above)
    # the thresholds of the rules, each met by the pair above: the forward's per128 steps, the backward's per256 steps, the
    # whole-tensor rule's 8192 and the register limit of 9 x 1024 float4
    pairs = {(WC.Plan.of(WC.CASE[a].layers).max_row, k) for k, a, _ in WC.THRESHOLDS}
    assert pairs == {(1024, "fwd"), (2048, "fwd"), (4608, "fwd"), (2048, "bwd"), (4096, "bwd"), (5120, "bwd"),
                     (8188, "both"), (36864, "both")}
    for total_co, n in ((100, 4),):      # per-channel steps as the rules state them, one float4 apart
        assert [WC.fwd_cell(r, total_co, n) for r in (1024, 1025, 2048, 2049, 4608, 4609)] == \
            ["F2x128", "F4x128", "F4x128", "F9x128", "F9x128", "F8x256"]
        assert [WC.bwd_cell(r, total_co, n) for r in (2048, 2049, 4096, 4097, 5120, 5121, 8192, 8193)] == \
            ["B2x256", "B4x256", "B4x256", "B5x256", "B5x256", "B8x256", "B8x256", "B8x256"]
    # the one maximum that is no multiple of 4: the dword layer sets the forward cell, aligned 1024-float rows beside it
    p = WC.Plan.of(WC.CASE["pc1025"].layers)
    assert p.max_row == 1025 and p.cells() == ("F4x128", "B2x256")
    assert ("reg", "reg") in [bd for bd, r in zip(p.bodies(), p.row) if r == 1024]
    # the top of the range: both in the generic kernels, and nothing longer rides a plan as PER_TENSOR
    lo, hi = (WC.Plan.of(WC.CASE[n].layers) for n in WC.TOP_PAIR)
    assert (lo.max_row, hi.max_row) == (WC.PT_MAX_ELEMS - 4, WC.PT_MAX_ELEMS)
    assert lo.cells() == hi.cells() == ("Fgen1024", "Bgen1024")
    # total_co on the two sides of 2 * nlayers, the same rows
    a, b = (WC.Plan.of(WC.CASE[n].layers) for n in WC.CO_PAIR)
    assert a.row[0] == b.row[0] == a.max_row == b.max_row == 8192 and a.nlayers == b.nlayers
    assert a.total_co == 2 * a.nlayers and b.total_co == 2 * b.nlayers + 1
    assert a.cells() == ("F9x1024", "B9x1024") and b.cells() == ("F8x256", "B8x256")
    # one per-channel row above 8192
    p = WC.Plan.of(WC.CASE["pc8196"].layers)
    assert WC.CASE["pc8196"].long_rows and p.cells() == ("F8x256", "B8x256")
    assert p.bodies()[0] == ("unstaged", "unstaged")


def test_the_replica_reproduces_the_cells_of_the_earlier_tests():
    """What the suite selected before the case table: four forward and four backward cells.  The other two of each
    direction -- WC.NEW_CELLS -- were selected by no test that compares with the per-layer bits."""
    fwd, bwd = set(), set()
    for where, layers, groups, f_want, b_want in WC.EXISTING_PLANS:
        plan = WC.Plan.of(layers)
        assert plan.cells()[0] == f_want, where
        got = tuple(plan.cells(first, last)[1] for first, last in groups)
        assert got == b_want, (where, got)
        fwd.add(f_want)
        bwd.update(b_want)
    assert fwd == {"F2x128", "F9x128", "F8x256", "F9x1024"}
    assert bwd == {"B2x256", "B5x256", "B8x256", "B9x1024"}
    assert set(WC.FWD_CELLS + WC.BWD_CELLS) - fwd - bwd == set(WC.NEW_CELLS)
    # their plan maxima: short per-channel rows up to 425 floats, 4608, 40004, and 36864 as a whole tensor; a group's 288
    assert sorted({WC.Plan.of(p[1]).max_row for p in WC.EXISTING_PLANS}) == [72, 180, 231, 425, 4608, 36864, 40004]
    assert max(WC.Plan.of(WC.EXISTING_PLANS[0][1]).row[1:5]) == 288


def test_the_256_thread_forward_launches_of_two_and_four_float4_are_unreachable():
    """mhaq_fq_wlayer_fwd_multi instantiates pc_fwd_multi_reg_kernel<2,256> and <4,256>, and no max_row selects them:
    per128 <= 9 takes every max_row <= 4608, and beyond that a row has at least 5 float4 per thread at 256 threads
    (recorded here and in DESIGN.md section 4; the instantiations are left in place)."""
    seen = set()
    for max_row in range(1, 70001):
        for total_co, nlayers in ((8, 4), (9, 4), (1, 1), (4000, 16)):
            seen.add(WC.fwd_cell(max_row, total_co, nlayers))
    assert seen == set(WC.FWD_CELLS)
    assert not seen & set(WC.FWD_UNREACHABLE)
    assert WC.multi_reg_nv(4609, False) == 8 and (4609 + 3) // 4 > 9 * 128 - 1
    # the launch code still names them: if that changes, this record and DESIGN.md go with it
    src = open(os.path.join(ROOT, "mhaq_amd", "csrc", "fq_pc.hip")).read()
    assert re.search(r"MHAQ_LAUNCH_MFR\(2, kBlock\)", src) and re.search(r"MHAQ_LAUNCH_MFR\(4, kBlock\)", src)


def test_the_replica_matches_the_constants_of_the_source():
    src = open(os.path.join(ROOT, "mhaq_amd", "csrc", "fq_pc.hip")).read()
    common = open(os.path.join(ROOT, "mhaq_amd", "csrc", "fq_common.hpp")).read()
    assert re.search(r"constexpr int kBlock = (\d+);", common).group(1) == str(WC.K_BLOCK)
    assert 64 * int(re.search(r"constexpr int kMaxWaves = (\d+);", src).group(1)) == WC.K_WIDE
    assert re.search(r"max_row >= (\d+) && total_co <= 2 \* \(int64_t\)nlayers", src).group(1) == str(WC.WHOLE_MIN_ROW)
    assert "constexpr int64_t kSmallMaxElems = 64 * 1024;" in src and WC.PT_MAX_ELEMS == 64 * 1024
