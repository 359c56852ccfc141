"""GPU: mhaq_amd.od_assign against the fp64 restatement of its contract (tests/od_assign_ref.py).  Discrete outputs are equal;
each continuous one has its own bar, the error of the framework's own fp32 chain against fp64 on the case: target_scores may use
twice its largest element error (measured on an MI355X: at most 1.31 of it), scores_sum once its error plus the suite's 8 ulp32
floor for a scalar (sr_metrics_ref.within_bar; measured: at most 0.47 of that, so the factor there is 1)."""
import pytest
import torch

from mhaq_amd import od_assign as OA
from mhaq_amd import ops
from tests import od_assign_ref as R

pytestmark = pytest.mark.gpu
CASES, F32 = R.CASES, torch.float32


run, check = R.run, R.check                  # shared with tests/test_gpu_od_assign_edges.py


@pytest.mark.parametrize("name", CASES)
def test_random_case_against_the_restatement(name):
    seed, size, counts, g, nc, k, alpha, beta, dtype = CASES[name]
    dev, rec = run(R.make_case(seed, size, counts, g, nc, dtype), nc, k, alpha, beta)
    r64 = check(rec, dev, nc, k, alpha, beta, True)
    assert g == 0 or bool(r64["fg_mask"].any())


@pytest.mark.parametrize("lower", [True, False])
def test_equal_metrics_at_the_cut_go_to_the_lower_anchor(lower):
    c = R.make_case(11, 160, (1,), 1, 80)
    best = int(R.assign_ref(c, 80, 1, 0.5, 6.0)["fg_mask"][0].nonzero()[0])
    gb, anc = c["gt_bboxes"][0, 0], c["anc_points"]
    inb = ((anc > gb[:2]) & (anc < gb[2:])).all(-1).nonzero().flatten()
    twin = int(inb[inb < best][0] if lower else inb[inb > best][-1])
    c["pd_bboxes"][0, twin], c["pd_scores"][0, twin] = c["pd_bboxes"][0, best], c["pd_scores"][0, best]
    dev, rec = run(c, 80, 1, 0.5, 6.0)
    check(rec, dev, 80, 1, 0.5, 6.0, False)
    assert rec["fg_mask"][0].nonzero().flatten().tolist() == [min(best, twin)]


def test_identical_ground_truth_goes_to_the_lower_index():
    c = R.make_case(12, 160, (2,), 2, 80)
    c["gt_bboxes"][0, 1], c["gt_labels"][0, 1] = c["gt_bboxes"][0, 0], c["gt_labels"][0, 0]
    dev, rec = run(c, 80, 10, 0.5, 6.0)
    check(rec, dev, 80, 10, 0.5, 6.0, False)
    assert bool(rec["fg_mask"].any()) and int(rec["target_gt_idx"].max()) == 0


def test_all_scores_zero_selects_the_lowest_anchor_indices():
    c = R.make_case(13, 64, (4, 2), 4, 80)
    c["pd_scores"].zero_()
    dev, rec = run(c, 80, 10, 0.5, 6.0)
    check(rec, dev, 80, 10, 0.5, 6.0, False)
    assert not bool(rec["target_scores"].any()) and float(rec["scores_sum"]) == 0.0


@pytest.mark.parametrize("what,bit", [("nan", 1), ("label", 4)])
def test_flags(what, bit):
    c = R.make_case(14, 160, (4, 2), 4, 80)
    if what == "nan":       # a positive of image 0: its pairs now count as zero
        c["pd_bboxes"][0, int(R.assign_ref(c, 80, 10, 0.5, 6.0)["fg_mask"][0].nonzero()[0]), 2] = float("nan")
    else:
        c["gt_labels"][0, 1] = 80.0
    dev, rec = run(c, 80, 10, 0.5, 6.0)
    check(rec, dev, 80, 10, 0.5, 6.0, False)
    assert int(rec["flags"].item()) == bit
    if what == "label":
        with pytest.raises(ValueError):
            OA.check_od_flags(rec["flags"])


@pytest.mark.parametrize("name", ["a525-crosses-tiles-b3", "nc3-scalar-stores-b3"])
def test_no_stray_writes_and_the_same_bits_twice(name):
    seed, size, counts, g, nc, k, alpha, beta, dtype = CASES[name]
    dev = {n: t.cuda() for n, t in R.make_case(seed, size, counts, g, nc, dtype).items()}
    b, a, band = len(counts), dev["anc_points"].shape[0], 64
    args = (dev["pd_scores"], dev["pd_bboxes"], dev["anc_points"], dev["gt_labels"].reshape(b, g), dev["gt_bboxes"],
            dev["mask_gt"].reshape(b, g), k, alpha, beta, 1e-9)
    results = []
    for _ in range(2):
        bufs, outs = [], []
        for shape, dt, fill in (((b, a, 4), F32, -7.0), ((b, a, nc), F32, -7.0), ((b, a), torch.uint8, 77), ((b, a), torch.int32, -7)):
            n = b * a * (shape[2] if len(shape) == 3 else 1)
            bufs.append(torch.full((n + 2 * band,), fill, dtype=dt, device="cuda"))
            outs.append(bufs[-1][band:band + n].view(shape))
        res = ops.od_assign(*args, out=tuple(outs))
        for buf in bufs:
            assert bool((buf[:band] == buf[0]).all()) and bool((buf[-band:] == buf[0]).all()) and buf[0] in (-7, 77)
        results.append([t.clone() for t in res])
    for x, y in zip(*results):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))


def test_assigner_is_a_drop_in_and_can_be_captured():
    nc, dev = 80, {n: t.cuda() for n, t in R.make_case(3, 160, (7, 4, 0), 7, 80).items()}
    assigner = OA.Assigner(nc, top_k=10, alpha=0.5, beta=6.0)
    args = [dev[n] for n in ("pd_scores", "pd_bboxes", "anc_points", "gt_labels", "gt_bboxes", "mask_gt")]
    eager = [t.clone() for t in assigner(*args)] + [assigner.last["scores_sum"].clone()]
    assert [tuple(t.shape) for t in eager[:3]] == [(3, 525, 4), (3, 525, nc), (3, 525)] and eager[2].dtype == torch.bool
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        assigner(*args)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            out = list(assigner(*args)) + [assigner.last["scores_sum"]]
    torch.cuda.current_stream().wait_stream(stream)
    for _ in range(3):
        for t in out:
            t.zero_()
        graph.replay()
        for x, y in zip(out, eager):
            assert torch.equal(x, y)


def test_shapes_beyond_the_ranges_raise_value_error():
    c = {n: t.cuda() for n, t in R.make_case(1, 1152, (1,), 1, 1).items()}          # 27 216 anchors > 24 576
    with pytest.raises(ValueError):
        run(c, 1, 10, 0.5, 6.0)
    with pytest.raises(ValueError):
        run(R.make_case(1, 64, (1,), 1, 1), 1, 33, 0.5, 6.0)                        # top_k > 32
