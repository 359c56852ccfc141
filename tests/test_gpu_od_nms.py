"""GPU (-m gpu): the YOLO head's non-maximum suppression (mhaq_fq_od_keys / torch.sort / mhaq_fq_od_nms, csrc/od_nms.hip)
through mhaq_amd.od_metrics.od_nms against the contract restated in numpy (tests/od_ref.py).  The contract has only singly
rounded fp32 operations and integer results, so every comparison is on bits.  Shapes are the smallest at which the kernel can
go wrong: candidate counts around the chunk width W of the workgroup's sweep, more than one chunk, several images."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import od_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FAR = 40.0            # pitch of a grid of 10 px boxes that do not touch


@functools.lru_cache(maxsize=None)
def chunk():
    from mhaq_amd import ops
    return ops.od_nms_chunk()


def _bits(t):
    """The words of a tensor; every NaN as the one quiet NaN (the contract says where a NaN stands, not its payload)."""
    if t.is_floating_point():
        t = torch.where(torch.isnan(t), torch.full_like(t, float("nan")), t)
    return t.contiguous().view(torch.int32)


def run(pred, **kw):
    from mhaq_amd.od_metrics import od_nms
    return od_nms(pred.to(DEV), **kw)


def check(pred, rec=None, **kw):
    """od_nms on the device against the oracle on the exactly up-converted prediction: all four outputs, on bits."""
    rec = run(pred, **kw) if rec is None else rec
    ref = R.nms(R.to_f32(pred), **kw)
    assert torch.equal(rec["count"].cpu(), torch.from_numpy(ref["count"])), (rec["count"], ref["count"])
    assert torch.equal(rec["n_candidates"].cpu(), torch.from_numpy(ref["n_cand"]))
    assert torch.equal(_bits(rec["det"]).cpu(), _bits(torch.from_numpy(ref["det"])))
    assert int(rec["flags"].item()) == ref["flags"]
    assert rec["det"].dtype == torch.float32 and rec["count"].dtype == torch.int32 and rec["flags"].dtype == torch.int32
    return rec, ref


def ordered(boxes, nc=1, cls=0, A=None, top=0.9, step=0.001):
    """One image whose anchor j holds boxes[j] = (x1, y1, x2, y2) with score top - j * step in class `cls`: the sorted order
    of the candidates is the order of the list."""
    A = len(boxes) if A is None else A
    rows = []
    for j, (x1, y1, x2, y2) in enumerate(boxes):
        rows.append((j, (x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1, {cls: top - j * step}))
    return R.make_pred([rows], nc, A)


def cell(i, size=10.0):
    """The i-th box of a grid of boxes that do not touch one another (all coordinates exact in fp32)."""
    x, y = FAR * (i % 32), FAR * (i // 32)
    return (x, y, x + size, y + size)


def with_candidates(n, A, seed):
    """One image, one class, random boxes in a 60 px field, exactly n scores above the threshold."""
    pred = R.random_pred(1, 1, A, seed=seed)
    drop = torch.randperm(A, generator=torch.Generator().manual_seed(seed + 1))[n:]
    pred[0, 4, drop] = 0.0
    return pred


@pytest.mark.parametrize("n", ["0", "1", "W-1", "W", "W+1", "2*W+1"])
def test_candidate_counts_around_the_chunk_width(n):
    W = chunk()
    n = eval(n, {"W": W})
    rec, ref = check(with_candidates(n, 2 * W + 8, seed=n), conf_thr=0.05)
    assert int(ref["n_cand"][0]) == n and (n == 0) == (int(ref["count"][0]) == 0)


def test_a_box_in_chunk_two_is_suppressed_by_a_box_kept_in_chunk_zero():
    W = chunk()
    first, filler = cell(0), cell(1)
    boxes = [first] + [filler] * (2 * W + 2) + [(2.0, 0.0, 12.0, 10.0), cell(2)]      # IoU with `first`: 8 / 12
    rec, ref = check(ordered(boxes, step=0.0005), conf_thr=0.05, iou_thr=0.5)
    assert int(ref["count"][0]) == 3 and list(ref["det"][0, :3, 0]) == [0.0, FAR, 2 * FAR]


def test_a_box_overlapping_only_a_suppressed_box_survives():
    boxes = [(0.0, 0.0, 10.0, 10.0), (4.0, 0.0, 14.0, 10.0), (8.0, 0.0, 18.0, 10.0)]      # IoU 6/14, 6/14 and 2/18
    rec, ref = check(ordered(boxes), conf_thr=0.05, iou_thr=0.4)
    assert int(ref["count"][0]) == 2 and list(ref["det"][0, :2, 0]) == [0.0, 8.0]


@pytest.mark.parametrize("max_det,where", [(1, "W-1"), (1, "W-2"), (5, "W-1"), (5, "W-2")])
def test_the_list_fills_at_a_chunk_end_and_one_candidate_before_it(max_det, where):
    W = chunk()
    p = eval(where, {"W": W})
    early = list(range(max(max_det - 1, 1)))                  # sorted positions of the first kept boxes
    kept_at = early + [p, p + 2, W + 3]                       # distinct boxes: kept unless the list is full
    boxes = [cell(j + 1) if j in kept_at else cell(0) for j in range(W + 8)]
    boxes[0] = cell(0)
    pred = ordered(boxes, step=0.0005)
    pred[0, 0, p + 1] = float("nan")                          # just behind the box that fills the list of max_det = 5
    rec, ref = check(pred, conf_thr=0.05, max_det=max_det)
    assert int(ref["count"][0]) == max_det
    if max_det == 5:
        assert ref["det"][0, 4, 0] == cell(p + 1)[0] and ref["flags"] == 0      # the walk ended at p: the NaN was not walked
    assert tuple(rec["det"].shape) == (1, max_det, 6)


def test_rows_beyond_the_count_are_written_as_zeros_and_nothing_else_is_touched():
    """The C entry points on poisoned buffers between bands of ones."""
    from mhaq_amd import _lib
    L = _lib.lib()
    B, nc, A, max_det, band = 2, 2, 70, 9, 64
    pred = R.random_pred(B, nc, A, seed=21, frac=0.2)
    pred[1, 4:, 6:] = 0.0                                     # the second image keeps fewer boxes than max_det
    pred = pred.to(DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def banded(n, dtype):
        buf = torch.ones(band + n + band, dtype=dtype, device=DEV)
        buf[band:band + n] = -7
        return buf, buf[band:band + n]

    kbuf, keys = banded(B * A * nc, torch.int64)
    assert L.mhaq_fq_od_keys(pred.data_ptr(), 0, B, nc, A, 0.05, keys.data_ptr(), stream) == 0
    skeys = torch.sort(keys.reshape(B, A * nc), dim=1).values.contiguous()
    dbuf, det = banded(B * max_det * 6, torch.float32)
    cbuf, count = banded(B, torch.int32)
    nbuf, ncand = banded(B, torch.int32)
    fbuf, flags = banded(1, torch.int32)
    nb = L.mhaq_fq_od_nms_workspace_bytes(B)
    wbuf, ws = banded(nb // 4, torch.int32)
    assert L.mhaq_fq_od_nms(pred.data_ptr(), 0, skeys.data_ptr(), B, nc, A, 0.65, 7680.0, 30000, max_det, det.data_ptr(),
                            count.data_ptr(), ncand.data_ptr(), flags.data_ptr(), ws.data_ptr(), nb, stream) == 0
    torch.cuda.synchronize()
    for buf, n in ((kbuf, B * A * nc), (dbuf, B * max_det * 6), (cbuf, B), (nbuf, B), (fbuf, 1), (wbuf, nb // 4)):
        assert bool((buf[:band] == 1).all()) and bool((buf[band + n:] == 1).all())
        assert not bool((buf[band:band + n] == -7).any())
    ref = R.nms(R.to_f32(pred), conf_thr=0.05, max_det=max_det)
    assert (ref["count"] < max_det).any()
    assert torch.equal(_bits(det).cpu(), torch.from_numpy(ref["det"].view(np.int32).reshape(-1)))
    assert torch.equal(count.cpu(), torch.from_numpy(ref["count"])) and int(flags.item()) == ref["flags"]


def test_more_candidates_than_max_nms_sets_bit_1_and_walks_the_truncated_list():
    pred = with_candidates(200, 260, seed=3)
    rec, ref = check(pred, conf_thr=0.05, max_nms=70)
    assert ref["flags"] == 2 and int(ref["n_cand"][0]) == 200
    full = R.nms(R.to_f32(pred), conf_thr=0.05)
    assert int(full["count"][0]) > int(ref["count"][0])       # the truncation is visible in this case


def test_three_images_with_different_counts_and_an_empty_one_in_the_middle():
    W = chunk()
    A = W + 40
    pred = torch.cat([with_candidates(W + 5, A, seed=31), with_candidates(0, A, seed=32), with_candidates(17, A, seed=33)])
    rec, ref = check(pred, conf_thr=0.05)
    assert list(ref["n_cand"]) == [W + 5, 0, 17] and ref["count"][1] == 0 and not ref["det"][1].any()


def test_the_same_box_at_the_same_score_in_two_classes_is_kept_twice_in_class_order():
    rows = [(5, 20.0, 20.0, 10.0, 10.0, {2: 0.8, 0: 0.8}), (1, 100.0, 20.0, 10.0, 10.0, {1: 0.9})]
    rec, ref = check(R.make_pred([rows], 3, 12), conf_thr=0.05)
    assert int(ref["count"][0]) == 3 and list(ref["det"][0, :3, 5]) == [1.0, 0.0, 2.0]


def test_equal_scores_across_anchors_are_ordered_by_anchor():
    rows = [(a, FAR * a, 5.0, 10.0, 10.0, {0: 0.5}) for a in (7, 3, 11)]
    rec, ref = check(R.make_pred([rows], 1, 16), conf_thr=0.05)
    assert list(ref["det"][0, :3, 0]) == [FAR * 3 - 5, FAR * 7 - 5, FAR * 11 - 5]


def class79_case(cls):
    """Three 1/8 px boxes 0.01 px and 0.04 px apart in x: at class 79 the offset coordinates sit on a grid of 1/16 px."""
    rows = [(0, 100.0, 50.0, 0.125, 0.125, {cls: 0.9}), (1, 100.01, 50.0, 0.125, 0.125, {cls: 0.8}),
            (2, 100.04, 50.0, 0.125, 0.125, {cls: 0.7})]
    return R.make_pred([rows], 80, 4)


def test_the_class_offset_is_applied_in_fp32_before_the_iou():
    rec, ref = check(class79_case(79), conf_thr=0.05, iou_thr=0.4)
    low = R.nms(R.to_f32(class79_case(0)), conf_thr=0.05, iou_thr=0.4)
    # un-offset, the third box overlaps the first by 0.515 and goes; on the 1/16 px grid of class 79 by 1/3, and stays
    assert int(low["count"][0]) == 1 and int(ref["count"][0]) == 2 and ref["det"][0, 1, 4] == np.float32(0.7)
    check(class79_case(0), conf_thr=0.05, iou_thr=0.4)


def test_a_zero_area_pair_is_not_suppressed():
    rows = [(0, 30.0, 30.0, 0.0, 0.0, {0: 0.9}), (1, 30.0, 30.0, 0.0, 0.0, {0: 0.8})]
    rec, ref = check(R.make_pred([rows], 1, 4), conf_thr=0.05, iou_thr=0.0)
    assert int(ref["count"][0]) == 2


def test_a_nan_score_is_no_candidate_and_an_infinite_one_sorts_first():
    rows = [(0, 10.0, 10.0, 8.0, 8.0, {0: float("nan")}), (1, 60.0, 10.0, 8.0, 8.0, {0: 0.99}),
            (2, 110.0, 10.0, 8.0, 8.0, {0: float("inf")})]
    rec, ref = check(R.make_pred([rows], 1, 4), conf_thr=0.05)
    assert int(ref["n_cand"][0]) == 2 and list(ref["det"][0, :2, 4]) == [np.inf, np.float32(0.99)] and ref["flags"] == 0


def test_a_nan_coordinate_sets_bit_0_and_leaves_the_other_images_alone():
    clean = with_candidates(30, 64, seed=41)
    dirty = with_candidates(30, 64, seed=42)
    a = int(torch.nonzero(dirty[0, 4] > 0.05)[3])
    dirty[0, 2, a] = float("nan")
    rec, ref = check(torch.cat([clean, dirty, clean]), conf_thr=0.05)
    assert ref["flags"] == 1
    alone = run(clean, conf_thr=0.05)
    assert int(alone["flags"].item()) == 0
    for b in (0, 2):
        assert torch.equal(_bits(rec["det"][b]), _bits(alone["det"][0])) and int(rec["count"][b]) == int(alone["count"][0])
    inf = with_candidates(30, 64, seed=43)
    inf[0, 0, int(torch.nonzero(inf[0, 4] > 0.05)[0])] = float("inf")
    assert check(inf, conf_thr=0.05)[1]["flags"] == 1


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bfloat16", "float16"])
def test_sixteen_bit_predictions_are_converted_up_exactly(dtype):
    W = chunk()
    pred = R.random_pred(2, 3, W // 2, seed=51, frac=0.8).to(dtype)      # rounded scores tie: the order falls to (a, c)
    rec, ref = check(pred, conf_thr=0.05)
    assert int(ref["n_cand"].max()) > W


def test_bad_predictions_are_refused_on_the_host():
    from mhaq_amd.od_metrics import od_nms
    good = R.random_pred(1, 2, 8).to(DEV)
    with pytest.raises(ValueError):
        od_nms(good.transpose(1, 2))
    with pytest.raises(ValueError):
        od_nms(good[:, :, ::2])
    with pytest.raises(ValueError):
        od_nms(good[0])
    with pytest.raises(TypeError):
        od_nms(good.double())
    with pytest.raises(TypeError):
        od_nms(good.to(torch.int32))


def test_two_calls_give_the_same_bits_and_nothing_waits_for_the_device():
    W = chunk()
    pred = R.random_pred(2, 2, W, seed=61).to(DEV)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = run(pred, conf_thr=0.05)
        b = run(pred, conf_thr=0.05)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    for k in ("det", "count", "n_candidates", "flags"):
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
    assert int(a["count"].min()) > 0


def test_a_captured_call_replays_the_eager_bits():
    W = chunk()
    pred = R.random_pred(2, 2, W, seed=71).to(DEV)
    other = R.random_pred(2, 2, W, seed=72).to(DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                # warm-up on the side stream, as torch.cuda.graph requires
        run(pred, conf_thr=0.05)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                             # keys, sort, NMS, flags: one linear chain on one stream
        captured = run(pred, conf_thr=0.05)
    pred.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    replayed = {k: captured[k].clone() for k in ("det", "count", "n_candidates", "flags")}
    eager = run(other, conf_thr=0.05)
    for k, v in replayed.items():
        assert torch.equal(_bits(v), _bits(eager[k])), k
    assert not torch.equal(_bits(replayed["det"]), _bits(run(R.random_pred(2, 2, W, seed=71), conf_thr=0.05)["det"]))
