"""GPU: the branches and constants of mhaq_amd.od_assign that tests/test_gpu_od_assign.py does not reach -- how the exponents
are taken, the ends of the ranges, selection inside one thread's column, the quirk of step 4, padding rows that are not last,
label and mask values, non-finite inputs, eps and the box edge, and which expand kernel runs.  The bars are those of
od_assign_ref.check(): discrete outputs equal the fp64 restatement, target_scores lies within twice the error of the fp32
restatement against fp64 on the same case, scores_sum within its own bar (sr_metrics_ref.within_bar, factor 1).

Measured on an MI355X, as fractions of those bars (target_scores of 2x the fp32 chain's error / scores_sum of its bar); the
fp32 chain takes every exponent by torch.pow, and no case needed another bar:
  exp-powf-0.75-2.5 0.500 / 0.063    exp-odd-3-identity-1 0.500 / 0.018    exp-odd-7-5 0.524 / 0.076
  exp-2-last-integer-64 0.629 / 0.349    exp-2-powf-65 0.500 / 0.314    exp-alpha0-zero-scores 0.473 / 0.154
  exp-beta0 0.500 / 0.004    exp-6-sqrt-beta 0.700 / 0.088    exp-both-0 0.500 / 0.029    exp-bf16-powf-0.75-2.5 0.500 / 0.164
  k32-full-selection 0.586 / 0.087    nc2 0.462 / 0.301    nc4 0.468 / 0.050    nc5 0.477 / 0.223    nc8 0.500 / 0.164
  a24576 0.686 / 0.085    g1024-identical 0.874 / 0.220    g1024-distinct 0.556 / 0.228    a24576-g1024 0.686 / 0.085
  column ties and descending, k = 1..4: 0.500 / at most 0.028    few positives: corner 0.513 / 0.077, inside 0.372 / 0.073
  step-4 quirk, all 14: 0 / 0 (every norm is 0 on both sides) except row 0 valid elsewhere, whose own positives count
  padding flipped and interleaved 0.558 / 0.238    labels 0.449 / at most 0.242    masks 0.449 / at most 0.223
  non-finite: fp32 cases 0.449 / at most 0.128, f16 beyond 65504 0.513 / 0.018    edge eps 0: 0.500 / 0.058, 1e-9: 0.500 / 0.061,
  4.0: 0.676 / 0.292
(0.500 means that the kernel and the fp32 chain have the same largest error.)  The largest-LDS case runs the restatement on
the whole [1, 1024, 24576] problem on the device: 0.02 s for fp64 and fp32 together, 2.96 GiB at its peak.  The whole file takes
3.2 s, its slowest test 1.2 s (the first one, which loads the library).
"""
import time

import pytest
import torch

from mhaq_amd import ops
from tests import od_assign_ref as R

pytestmark = pytest.mark.gpu
F32 = torch.float32
run, check = R.run, R.check


def fg_of(rec, image=0):
    return rec["fg_mask"][image].nonzero().flatten().tolist()


# ---------------------------------------------------------------- 1. exponents, 2. top_k == 32, 9. the row lengths of expand
@pytest.mark.parametrize("name", R.EDGE_CASES)
def test_edge_table_row_against_the_restatement(name):
    c, nc, k, alpha, beta, need_margin = R.edge_case(name)
    dev, rec = run(c, nc, k, alpha, beta)
    r64 = check(rec, dev, nc, k, alpha, beta, need_margin, label=name)
    assert bool(r64["fg_mask"].any()) and bool(r64["target_scores"].any())
    if name == "exp-alpha0-zero-scores":                # powf(0, 0) == 1: an anchor whose gathered score is 0 is a positive
        assert bool((r64["fg_mask"] & (dev["pd_scores"].amax(-1) == 0)).any())
    if name == "exp-beta0":                             # the one place where m > 0 meets ov == 0 (step 8)
        m0 = R.assign_ref(dev, nc, k, alpha, 1.0)       # beta = 1: the metric is 0 exactly where the overlap is
        assert bool((r64["fg_mask"] & ~m0["fg_mask"]).any()) or bool((r64["fg_mask"] & (r64["target_scores"].amax(-1) == 0)).any())
    if nc in (4, 8):                                    # the label hit falls in each of the four lanes of a 16-byte store
        assert sorted(set(((r64["target_scores"] != 0).nonzero()[:, 2] % 4).tolist())) == [0, 1, 2, 3]


# ---------------------------------------------------------------- 2. the ends of the ranges
BIG = [16.5, 24.5, 1200.5, 900.5]                       # on the 192 x 128 grid of stride 8: 24 576 anchors


def test_a24576_the_largest_anchor_count():
    rows = {0: (BIG, 3.0, 1.0), 1: ([400.5, 300.5, 1500.5, 1000.5], 7.0, 1.0), 2: ([700.0, 500.0, 703.0, 503.0], 1.0, 1.0),
            3: ([100.5, 600.5, 460.5, 1010.5], 3.0, 1.0)}
    c = R.hand_case(R.grid(192, 128), 80, rows, 4, seed=31, extent=1536.0)
    assert c["anc_points"].shape[0] == 24576
    dev, rec = run(c, 80, 13, 1.0, 6.0)
    r64 = check(rec, dev, 80, 13, 1.0, 6.0, True, label="a24576")
    assert int(r64["fg_mask"].sum()) > 13 and int(r64["fg_mask"][0].nonzero().max()) > 16384


def test_g1024_identical_rows_count_1024_on_one_anchor():
    """Every row chooses the same ten anchors: the packed word holds count 1024 (bit 30) and the index sum 523 776 (all 20
    low bits short of a carry); the arg-max over 1024 equal overlaps is row 0."""
    c = R.hand_case(R.anchors(64), 80, {j: ([4.5, 7.0, 53.0, 50.0], 5.0, 1.0) for j in range(1024)}, 1024, seed=32, extent=64.0)
    dev, rec = run(c, 80, 10, 0.5, 6.0)
    check(rec, dev, 80, 10, 0.5, 6.0, False, label="g1024-identical")
    assert len(fg_of(rec)) == 10 and int(rec["target_gt_idx"].max()) == 0 and float(rec["scores_sum"]) > 0


def test_g1024_distinct_rows_single_claims_by_high_indices():
    """Rows 1014..1023 each hold one stride-8 anchor of their own: cnt == 1 and the index sum is an index up to 1023."""
    anc = R.anchors(64)
    rows = {j: ([4.5, 7.0, 53.0, 50.0], float(j % 80), 1.0) for j in range(1014)}
    own = [56, 57, 58, 59, 60, 61, 62, 63, 0, 1]        # stride-8 anchors outside the large box, each in a 3 px box
    for a, j in zip(own, range(1014, 1024)):
        x, y = float(anc[a, 0]), float(anc[a, 1])
        rows[j] = ([x - 1.5, y - 1.5, x + 1.5, y + 1.5], float(j % 80), 1.0)
    c = R.hand_case(anc, 80, rows, 1024, seed=33, extent=64.0)
    for a, j in zip(own, range(1014, 1024)):            # predicted exactly: a positive metric, or anchors 0..9 would go first
        c["pd_bboxes"][0, a] = c["gt_bboxes"][0, j]
    dev, rec = run(c, 80, 10, 0.5, 6.0)
    r64 = check(rec, dev, 80, 10, 0.5, 6.0, False, label="g1024-distinct")
    assert rec["target_gt_idx"][0, own].tolist() == list(range(1014, 1024)) and bool(rec["fg_mask"][0, own].all())
    assert bool((rec["target_scores"][0, own].amax(-1) > 0).all())


def test_a24576_g1024_the_largest_dynamic_lds():
    """4 * A + 28 * G = 126 976 bytes in the resolve kernel; valid rows at 0, 511 and 1023.  The restatement runs on the
    device on the whole [1, 1024, 24576] problem (its time and peak memory are printed and stand in the module docstring)."""
    rows = {0: (BIG, 3.0, 1.0), 511: ([400.5, 300.5, 1500.5, 1000.5], 7.0, 1.0), 1023: ([100.5, 600.5, 460.5, 1010.5], 3.0, 1.0)}
    c = R.hand_case(R.grid(192, 128), 80, rows, 1024, seed=31, extent=1536.0)
    dev, rec = run(c, 80, 13, 1.0, 6.0)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    r64 = check(rec, dev, 80, 13, 1.0, 6.0, True, label="a24576-g1024")
    torch.cuda.synchronize()
    print(f"restatement fp64 + fp32 on the device: {time.perf_counter() - t0:.2f} s, peak "
          f"{torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
    assert set(r64["target_gt_idx"][0].tolist()) == {0, 511, 1023}


@pytest.mark.parametrize("b,a", [(0, 84), (3, 0), (0, 0)])
def test_no_images_or_no_anchors_writes_only_the_sum_and_the_flags(b, a):
    c = R.make_case(14, 160, (4, 2), 4, 80)
    c["gt_labels"][0, 1] = 80.0
    dev, rec = run(c, 80, 10, 0.5, 6.0)                # leaves a non-zero sum and flag word behind in the allocator's blocks
    assert float(rec["scores_sum"]) > 0 and int(rec["flags"]) == 4
    del rec
    z = lambda *s: torch.zeros(*s, device="cuda")
    tb, ts, fg, gi, ssum, flags = ops.od_assign(z(b, a, 80), z(b, a, 4), z(a, 2), z(b, 4), z(b, 4, 4), z(b, 4), 10, 0.5, 6.0, 1e-9)
    assert (tuple(tb.shape), tuple(ts.shape), tuple(fg.shape), tuple(gi.shape)) == ((b, a, 4), (b, a, 80), (b, a), (b, a))
    assert float(ssum) == 0.0 and int(flags) == 0


# ---------------------------------------------------------------- 3. selection inside one thread's column
def column_case(scores):
    """One ground truth over the whole 160^2 image; anchors 5, 69 (another wavefront), 261 and 517 (thread 5's column again)
    predict the box itself with `scores`: the four largest metrics."""
    c = R.hand_case(R.anchors(160), 80, {0: ([0.0, 0.0, 160.0, 160.0], 9.0, 1.0)}, 1, seed=34)
    c["pd_scores"].clamp_(max=0.9)
    for a, s in zip((5, 69, 261, 517), scores):
        c["pd_bboxes"][0, a], c["pd_scores"][0, a, 9] = torch.tensor([0.0, 0.0, 160.0, 160.0]), s
    return c


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_equal_metrics_in_one_column_and_across_wavefronts(k):
    dev, rec = run(column_case((0.99, 0.99, 0.99, 0.99)), 80, k, 0.5, 6.0)
    check(rec, dev, 80, k, 0.5, 6.0, False, label=f"column-ties-k{k}")
    assert fg_of(rec) == [5, 69, 261, 517][:k]


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_a_column_whose_later_anchors_win_first(k):
    """The owner of anchors 5, 261 and 517 gives up 517 first, then 261, then 5: every rescan must see the whole column."""
    dev, rec = run(column_case((0.96, 0.97, 0.98, 0.99)), 80, k, 0.5, 6.0)
    check(rec, dev, 80, k, 0.5, 6.0, True, label=f"column-descending-k{k}")
    assert fg_of(rec) == sorted([517, 261, 69, 5][:k])


@pytest.mark.parametrize("where", ["corner", "inside"])
def test_fewer_positive_metrics_than_k(where):
    """11 (corner) or 10 (inside) anchors lie in the box and two of them have a zero score; k = 13.  The rounds after the
    positive metrics take zero-metric anchors by index: at the corner anchor 0 is in the box and becomes a positive with a
    zero norm, every later one is outside; inside, the zero-metric anchors of the box are never reached."""
    box, zeros = ([0.0, 0.0, 22.0, 22.0], (0, 41)) if where == "corner" else ([17.0, 17.0, 39.0, 39.0], (42, 63))
    c = R.hand_case(R.anchors(160), 80, {0: (box, 9.0, 1.0)}, 1, seed=35)
    anc = c["anc_points"]
    inb = ((anc > torch.tensor(box[:2])) & (anc < torch.tensor(box[2:]))).all(-1).nonzero().flatten().tolist()
    c["pd_bboxes"][0, inb] = torch.tensor(box) + torch.arange(len(inb))[:, None] * 0.25      # distinct positive overlaps
    for a in zeros:
        assert a in inb
        c["pd_scores"][0, a, 9] = 0.0
    assert len(inb) < 13
    dev, rec = run(c, 80, 13, 0.5, 6.0)
    r64 = check(rec, dev, 80, 13, 0.5, 6.0, False, label=f"few-positives-{where}")
    assert fg_of(rec) == sorted(set(inb) - set(zeros) | ({0} if where == "corner" else set()))
    assert int((r64["target_scores"][0] != 0).sum()) == len(inb) - 2


# ---------------------------------------------------------------- 4. the quirk of step 4
@pytest.mark.parametrize("beta", [6.0, 0.0])
@pytest.mark.parametrize("row0", ["elsewhere", "padding", 80.0, -1.0, 1e10, float("inf"), float("nan")])
def test_an_argmax_over_zero_overlaps_gives_the_anchor_to_row_0_which_does_not_hold_it(row0, beta):
    """Rows 1 and 2 cover anchors 0..19 and 2..19 of the top row of the stride-8 grid; every prediction is far away and every
    score is 0.25, so row 1 chooses anchors 0..9 and row 2 anchors 2..9 of those (2..11 with beta == 0, where its metrics are
    positive).  Anchors 2..9 are claimed twice, the arg-max over
    zeros is row 0: foreground, index 0, norm 0 -- whether row 0 is a valid box elsewhere, a padding row, or has a label out
    of range (flag 4; 1e10, inf and NaN pass through the label's clamp).  With beta == 0 the metrics are positive and the
    overlaps 0: the singly claimed anchors 0, 1, 10, 11 have norm 0 through pov == 0."""
    first = {"elsewhere": ([40.0, 40.0, 120.0, 120.0], 3.0, 1.0), "padding": ([0.0, 0.0, 0.0, 0.0], 0.0, 0.0)}.get(
        row0, ([40.0, 40.0, 120.0, 120.0], row0, 1.0))
    c = R.hand_case(R.anchors(160), 80, {0: first, 1: ([0.0, 0.0, 160.0, 7.0], 4.0, 1.0), 2: ([16.0, 0.0, 160.0, 7.0], 6.0, 1.0)},
                    3, seed=36, far=True)
    c["pd_scores"].fill_(0.25)
    if row0 == "elsewhere":                             # row 0's own anchors predict its box: pov(0) > 0, so a metric taken
        anc = c["anc_points"]                           # for row 0 on an anchor it does not hold would show in the norm
        c["pd_bboxes"][0, ((anc > 40.0) & (anc < 120.0)).all(-1)] = c["gt_bboxes"][0, 0]
    dev, rec = run(c, 80, 10, 0.5, beta)
    check(rec, dev, 80, 10, 0.5, beta, False, label=f"quirk-{row0}-beta{beta:g}")
    assert bool(rec["fg_mask"][0, :10].all()) and rec["target_gt_idx"][0, :10].tolist() == [1, 1] + [0] * 8
    if beta == 0.0:                                     # row 2's metrics are positive: it chooses its own first ten, 2..11
        assert bool(rec["fg_mask"][0, 10:12].all()) and rec["target_gt_idx"][0, 10:12].tolist() == [2, 2]
    assert not bool(rec["target_scores"][0, :12].any())
    assert (float(rec["scores_sum"]) > 0.0) == (row0 == "elsewhere")
    assert int(rec["flags"]) == (4 if isinstance(row0, float) else 0)
    assert torch.equal(rec["target_bboxes"][0, 5], dev["gt_bboxes"][0, 0])


# ---------------------------------------------------------------- 5. padding rows that are not last
@pytest.mark.parametrize("order", ["flipped", "interleaved"])
def test_padding_rows_first_and_between_valid_rows(order):
    base = R.make_case(3, 160, (7, 4, 0), 7, 80)
    if order == "flipped":
        perm = list(range(6, -1, -1))                   # image 1: rows 0..2 are padding
    else:
        perm = [7, 0, 8, 1, 2, 9, 3, 10, 4, 5, 11, 6]   # 7..11: padding rows in front and in between
    c = dict(base)
    for n in ("gt_labels", "gt_bboxes", "mask_gt"):
        t = torch.cat((base[n], torch.zeros(3, 5, base[n].shape[2])), 1)
        c[n] = t[:, perm].contiguous()
    dev, rec = run(c, 80, 10, 0.5, 6.0)
    check(rec, dev, 80, 10, 0.5, 6.0, True, label=f"padding-{order}")
    r0 = R.assign_ref(base, 80, 10, 0.5, 6.0)           # the same assignment, indexed by the rows as they now stand
    fg = r0["fg_mask"]
    assert torch.equal(rec["fg_mask"].cpu(), fg)
    where = torch.tensor([perm.index(j) for j in range(7)])
    assert torch.equal(rec["target_gt_idx"].cpu().long()[fg], where[r0["target_gt_idx"]][fg])
    assert not bool(rec["target_gt_idx"].cpu()[~fg].any())
    assert torch.equal(rec["target_bboxes"].cpu()[~fg], c["gt_bboxes"][:, 0][:, None].expand(3, 525, 4)[~fg])   # row 0's box
    assert torch.equal(rec["target_scores"].cpu() != 0, r0["target_scores"] != 0)


# ---------------------------------------------------------------- 6. labels and masks
@pytest.mark.parametrize("label,flag", [(-1.0, 4), (-0.5, 4), (float("nan"), 4), (float("inf"), 4), (1e10, 4), (2.7, 0)])
def test_label_values(label, flag):
    c = R.make_case(14, 160, (4, 2), 4, 80)
    c["gt_labels"][0, 1] = label
    dev, rec = run(c, 80, 10, 0.5, 6.0)
    check(rec, dev, 80, 10, 0.5, 6.0, False, label=f"label-{label}")
    assert int(rec["flags"]) == flag
    mine = rec["target_gt_idx"][0] == 1
    if flag:                                            # an invalid row has no anchor, and so no row of target_scores
        assert not bool(mine.any())
    else:                                               # 2.7 is class 2 in the gather and in the output
        c["gt_labels"][0, 1] = 2.0
        _, rec2 = run(c, 80, 10, 0.5, 6.0)
        assert bool(mine.any()) and all(torch.equal(rec[n], rec2[n]) for n in ("target_scores", "fg_mask", "target_gt_idx"))
        assert bool((rec["target_scores"][0][mine][:, 2] > 0).any())


@pytest.mark.parametrize("mask,counts", [(0.5, True), (-1.0, True), (float("nan"), True), (-0.0, False)])
def test_mask_values(mask, counts):
    c = R.make_case(14, 160, (4, 2), 4, 80)
    c["mask_gt"][0, 1] = mask
    dev, rec = run(c, 80, 10, 0.5, 6.0)
    check(rec, dev, 80, 10, 0.5, 6.0, False, label=f"mask-{mask}")
    c["mask_gt"][0, 1] = 1.0 if counts else 0.0
    _, rec2 = run(c, 80, 10, 0.5, 6.0)
    assert all(torch.equal(rec[n], rec2[n]) for n in rec) and bool((rec["target_gt_idx"][0] == 1).any()) == counts


def test_a_bad_label_on_a_padding_row_sets_no_flag():
    c = R.make_case(14, 160, (4, 2), 4, 80)
    c["gt_labels"][1, 2], c["gt_labels"][1, 3] = 80.0, float("nan")
    dev, rec = run(c, 80, 10, 0.5, 6.0)
    check(rec, dev, 80, 10, 0.5, 6.0, True, label="bad-label-padding-row")
    assert int(rec["flags"]) == 0


# ---------------------------------------------------------------- 7. non-finite inputs
NAN, INF = float("nan"), float("inf")


def nonfinite_case(what):
    """-> (case, expected flag word, the (image, anchor) that was touched or None)."""
    c = R.make_case(14, 160, (4, 1), 4, 80)
    r = R.assign_ref(c, 80, 10, 0.5, 6.0)
    anc, gb = c["anc_points"], c["gt_bboxes"]
    inb = ((anc[None, None] > gb[:, :, None, :2]) & (anc[None, None] < gb[:, :, None, 2:])).all(-1)       # [B, G, A]
    outside = (~inb[0].any(0)).nonzero().flatten()
    img = 1                                             # a positive of image 1, whose one ground truth alone can hold it
    pos = int(r["fg_mask"][img].nonzero()[0])
    row = int(r["target_gt_idx"][img, pos])
    lab = int(c["gt_labels"][img, row])
    if what == "score-of-a-class-not-gathered":
        free = sorted(set(range(80)) - {int(v) for v in c["gt_labels"][0].flatten()})[0]
        c["pd_scores"][0, :, free] = NAN
        return c, 0, None
    if what == "box-of-an-anchor-outside-every-ground-truth":
        c["pd_bboxes"][0, int(outside[0])], c["pd_bboxes"][0, int(outside[-1]), 1] = NAN, INF
        return c, 0, None
    if what == "padding-row":
        c["gt_bboxes"][1, 3], c["gt_labels"][1, 2], c["gt_bboxes"][1, 2, 2] = NAN, NAN, INF
        return c, 0, None
    if what == "anchor-point":
        c["anc_points"][int(outside[0]), 1] = NAN       # in the box of nobody, before and after
        return c, 0, None
    if what == "anchor-point-of-a-positive":            # the anchor (shared by all images) is in the box of nobody any more
        c["anc_points"][pos, 0] = NAN
        return c, 0, (img, pos)
    if what in ("gathered-score-nan", "gathered-score-inf"):
        c["pd_scores"][img, pos, lab] = NAN if what.endswith("nan") else INF
        return c, 1, (img, pos)
    if what == "gt-box-inf":
        c["gt_bboxes"][img, row, 2] = INF
        return c, 1, None
    assert what == "f16-box-beyond-65504"
    c["pd_bboxes"][img, pos, 2] = 70000.0
    c["pd_scores"], c["pd_bboxes"] = c["pd_scores"].half(), c["pd_bboxes"].half()
    return c, 1, (img, pos)


@pytest.mark.parametrize("what", ["score-of-a-class-not-gathered", "box-of-an-anchor-outside-every-ground-truth", "padding-row",
                                  "anchor-point", "anchor-point-of-a-positive", "gathered-score-nan", "gathered-score-inf", "gt-box-inf", "f16-box-beyond-65504"])
def test_nonfinite_inputs_flag_only_in_a_pair_that_counts(what):
    c, flag, touched = nonfinite_case(what)
    dev, rec = run(c, 80, 10, 0.5, 6.0)
    check(rec, dev, 80, 10, 0.5, 6.0, False, label=what)
    assert int(rec["flags"]) == flag and bool(rec["fg_mask"].any())
    assert bool(torch.isfinite(rec["target_scores"]).all()) and bool(torch.isfinite(rec["scores_sum"]).all())
    if touched is not None:                             # the pair counts as zero: the anchor is no positive any more (k = 10
        assert not bool(rec["target_scores"][touched].any())          # positive metrics remain in the box that held it)
    if flag == 0 and touched is None:                   # nothing that counts was touched: the clean case's assignment
        _, clean = run(R.make_case(14, 160, (4, 1), 4, 80), 80, 10, 0.5, 6.0)
        assert all(torch.equal(rec[n], clean[n]) for n in ("fg_mask", "target_gt_idx", "target_scores", "scores_sum"))


# ---------------------------------------------------------------- 8. eps and the box edge
RING = ((12.0, 36.0), (12.0, 60.0), (100.0, 44.0), (100.0, 68.0), (36.0, 20.0), (60.0, 20.0), (44.0, 92.0), (68.0, 92.0))


@pytest.mark.parametrize("eps", [0.0, 1e-9, 4.0])
def test_anchors_on_the_box_edge_and_a_ring_of_eps(eps):
    """Image 0's box has its four edges on stride-8 anchor centres, image 1's lies 4 px further out.  Two anchors per edge
    predict their image's box with the largest scores, so they are chosen wherever they count as inside: never in image 0
    (the difference is 0), in image 1 unless eps is 4.0 (the difference is exactly 4).  Every coordinate is a multiple of
    0.5, so the fp32 and the fp64 differences are the same numbers."""
    c = R.make_case(37, 160, (1, 1), 1, 80)
    c["gt_bboxes"][0, 0], c["gt_bboxes"][1, 0] = torch.tensor([12.0, 20.0, 100.0, 92.0]), torch.tensor([8.0, 16.0, 104.0, 96.0])
    c["pd_scores"].clamp_(max=0.8)
    ring = [int(((c["anc_points"] == torch.tensor(p)).all(-1)).nonzero()[0]) for p in RING]
    for i in (0, 1):
        lab = int(c["gt_labels"][i, 0])
        for j, a in enumerate(ring):
            c["pd_bboxes"][i, a], c["pd_scores"][i, a, lab] = c["gt_bboxes"][i, 0], 0.99 - 0.01 * j
    dev, rec = run(c, 80, 10, 0.5, 6.0, eps)
    check(rec, dev, 80, 10, 0.5, 6.0, True, eps=eps, label=f"edge-eps{eps:g}")
    assert not bool(rec["fg_mask"][0, ring].any()) and len(fg_of(rec, 0)) == 10
    assert rec["fg_mask"][1, ring].tolist() == [eps < 4.0] * 8 and len(fg_of(rec, 1)) == 10


# ---------------------------------------------------------------- 9. which expand kernel runs
def expand_run(dev, nc, off_tb, off_ts, band=64):
    """ops.od_assign into guarded buffers whose target_bboxes / target_scores views start `off` floats past 256 bytes."""
    b, a, g = dev["pd_scores"].shape[0], dev["anc_points"].shape[0], dev["gt_bboxes"].shape[1]
    bufs, outs = [], []
    for shape, dt, fill, off in (((b, a, 4), F32, -7.0, off_tb), ((b, a, nc), F32, -7.0, off_ts), ((b, a), torch.uint8, 77, 0),
                                 ((b, a), torch.int32, -7, 0)):
        n = b * a * (shape[2] if len(shape) == 3 else 1)
        bufs.append(torch.full((n + 2 * band + off,), fill, dtype=dt, device="cuda"))
        outs.append(bufs[-1][band + off:band + off + n].view(shape))
        assert outs[-1].data_ptr() % 16 == 4 * off
    res = ops.od_assign(dev["pd_scores"], dev["pd_bboxes"], dev["anc_points"], dev["gt_labels"].reshape(b, g), dev["gt_bboxes"],
                        dev["mask_gt"].reshape(b, g), 10, 0.5, 6.0, 1e-9, out=tuple(outs))
    for buf, off in zip(bufs, (off_tb, off_ts, 0, 0)):
        assert bool((buf[:band + off] == buf[0]).all()) and bool((buf[-band:] == buf[0]).all()) and buf[0] in (-7, 77)
    return [t.clone() for t in res]


@pytest.fixture(scope="module")
def aligned_runs():
    runs = {}
    for nc in (4, 8, 80):
        dev = {n: t.cuda() for n, t in R.make_case(21, 160, (7, 3, 0), 7, nc).items()}
        runs[nc] = (dev, expand_run(dev, nc, 0, 0))
    return runs


@pytest.mark.parametrize("which", ["scores", "bboxes", "both"])
@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("nc", [4, 8, 80])
def test_an_output_off_16_bytes_takes_the_scalar_expand_and_writes_the_same_bits(aligned_runs, nc, off, which):
    dev, aligned = aligned_runs[nc]
    assert bool(aligned[1].any()) and bool(aligned[2].any())
    res = expand_run(dev, nc, off if which != "scores" else 0, off if which != "bboxes" else 0)
    for x, y in zip(res, aligned):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
