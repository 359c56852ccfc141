"""Checker code for the classification head (mhaq_fq_cls_head_fwd, mhaq_amd/cls_metrics.py, mhaq_amd/loss.py:
FusedCrossEntropy): the definitions of include/mhaq_fq.h restated in float64 torch on the CPU.

  valid_rows(y, cols, ii)       target != ignore_index and 0 <= target < cols
  sort_rank(x, y, ii)           the label's position in torch.sort(x, descending=True, stable=True); cols on other rows
  count_rank(x, y, ii)          the counting form of the header: #{x_c > x_y} + #{c < y: x_c == x_y}, NaN above +inf
  head64(x, y, ii, topk)        loss, nll, gunit, rank, counts, acc
  chain32(x, y, ii, g)          the framework's float32 cross_entropy (loss, per-row nll, gx) where x lives
  loss_bar / grad_bar / nll_bar the accuracy bars of the GPU tests
  plain_case / edge_case        seeded inputs

No kernel is involved in any of them."""
import math

import torch
import torch.nn.functional as F

IGNORE = -100
MARGIN = 4.0                                     # the issue's factor on the framework chain's own error
# register path (37, 1001: unaligned row bases), its edge at 4096 / 4097, a re-walked row; more rows than the finalize has
# threads (257: one of them, 600: a third trip); 1028 and 4092 columns: the first 4-element group of a thread's second trip
# over the row and the last group of its fourth; 10 and 100 columns: the CIFAR heads (the kernel has no narrower body)
SHAPES = [(3, 1), (1, 2), (5, 37), (16, 10), (16, 100), (16, 1001), (250, 1000), (257, 4), (600, 3), (3, 1028), (2, 4092),
          (2, 4096), (4, 4097), (2, 10007)]
CPU_SHAPES = [(3, 1), (1, 2), (5, 37), (16, 10), (16, 100), (16, 1001), (257, 4), (3, 1028), (2, 4097)]
SCALES = {(3, 1): 2.0, (1, 2): 1.0, (5, 37): 8.0, (16, 10): 3.0, (16, 100): 4.0, (16, 1001): 4.0, (250, 1000): 4.0,
          (257, 4): 4.0, (600, 3): 2.0, (3, 1028): 4.0, (2, 4092): 2.0, (2, 4096): 2.0, (4, 4097): 8.0, (2, 10007): 1.0,
          (2, 4097): 2.0}


def valid_rows(y, cols, ignore_index=IGNORE):
    y = y.cpu()
    return (y != ignore_index) & (y >= 0) & (y < cols)


def _safe(y, valid):
    return torch.where(valid, y.cpu(), torch.zeros_like(y.cpu()))


def sort_rank(x, y, ignore_index=IGNORE):
    """int64 [rows]: where the stable descending sort of row i puts column y_i (NaN first, as torch sorts); cols elsewhere."""
    x = x.detach().double().cpu()
    rows, cols = x.shape
    valid = valid_rows(y, cols, ignore_index)
    order = torch.sort(x, dim=1, descending=True, stable=True).indices
    pos = (order == _safe(y, valid)[:, None]).int().argmax(1)
    return torch.where(valid, pos, torch.full_like(pos, cols))


def count_rank(x, y, ignore_index=IGNORE):
    x = x.detach().double().cpu()
    rows, cols = x.shape
    valid = valid_rows(y, cols, ignore_index)
    ys = _safe(y, valid)
    xy = x.gather(1, ys[:, None])
    nx, ny = x.isnan(), xy.isnan()
    above = ~ny & (nx | (x > xy))
    same = torch.where(ny, nx, x == xy) & (torch.arange(cols)[None, :] < ys[:, None])
    r = above.sum(1) + same.sum(1)
    return torch.where(valid, r, torch.full_like(r, cols))


def head64(x, y, ignore_index=IGNORE, topk=5):
    """The header's definitions in float64 from the bits of x -> dict(loss, nll [rows], gunit [rows, cols], rank, counts, acc)."""
    x = x.detach().double().cpu()
    rows, cols = x.shape
    valid = valid_rows(y, cols, ignore_index)
    ys = _safe(y, valid)
    m = x.max(1, keepdim=True).values
    e = (x - m).exp()
    s = e.sum(1, keepdim=True)
    nll = (m + s.log() - x.gather(1, ys[:, None]))[:, 0]
    nll = torch.where(valid, nll, torch.zeros_like(nll))
    v = int(valid.sum())
    onehot = torch.zeros_like(x).scatter_(1, ys[:, None], 1.0)
    gunit = torch.where(valid[:, None], (e / s - onehot) / max(v, 1), torch.zeros_like(x))
    rank = sort_rank(x, y, ignore_index)
    counts = torch.tensor([v, int((valid & (rank == 0)).sum()), int((valid & (rank < topk)).sum())])
    f32 = lambda n: torch.tensor(float(n), dtype=torch.float32)      # noqa: E731
    acc = torch.stack([f32(counts[1]) / f32(v), f32(counts[2]) / f32(v)]) if v else torch.zeros(2)
    loss = nll[valid].sum() / v if v else torch.tensor(float("nan"), dtype=torch.float64)
    return dict(loss=loss, nll=nll, gunit=gunit, rank=rank, counts=counts, acc=acc, valid=valid)


def chain32(x, y, ignore_index=IGNORE, g=1.0):
    """The framework's float32 chain where x lives (the GPU tests run it on the device) -> (loss, nll [rows], gx).  Only
    for labels that are ignore_index or in range: the framework's device code asserts on any other."""
    xf = x.detach().float().requires_grad_(True)
    loss = F.cross_entropy(xf, y, ignore_index=ignore_index)
    (gx,) = torch.autograd.grad(loss * g, xf)
    with torch.no_grad():
        nll = F.cross_entropy(xf, y, ignore_index=ignore_index, reduction="none")
    return loss.detach(), nll, gx


def ulp32(v):
    v = abs(float(v))
    if v == 0.0 or not math.isfinite(v):
        return 2.0 ** -149
    return max(2.0 ** (math.floor(math.log2(v)) - 23), 2.0 ** -149)


def loss_bar(l_torch, l64):
    return MARGIN * abs(float(l_torch) - float(l64)) + 8 * ulp32(l64)


def grad_bar(g_torch, g64):
    g64 = g64.double().cpu()
    return MARGIN * float((g_torch.double().cpu() - g64).abs().max()) + 8 * 2.0 ** -24 * float(g64.abs().max())


def nll_bar(nll_torch, nll64):
    nll64 = nll64.double().cpu()
    return MARGIN * float((nll_torch.double().cpu() - nll64).abs().max()) + 8 * ulp32(nll64.abs().max())


def plain_case(shape, dtype=torch.float32, seed=0):
    """Finite seeded normal logits of the shape's scale in `dtype`, random labels with the first and the last column among
    them and (from four rows on) one ignored row -> (x, y) on the CPU."""
    rows, cols = shape
    gen = torch.Generator().manual_seed(7000 + 1000 * rows + cols + seed)
    x = (torch.randn(shape, generator=gen) * SCALES[shape]).to(dtype)
    y = torch.randint(0, cols, (rows,), generator=gen)
    y[0] = 0
    if rows > 1:
        y[1] = cols - 1
    if rows > 3:
        y[3] = IGNORE
    return x, y


N_EDGES = 13


def edge_case(shape, dtype=torch.float32, variant=0):
    """plain_case with planted rows: row r gets treatment r + variant (rows beyond the thirteen treatments stay random) ->
    (x, y) on the CPU.  Treatments: label in the first / last column, a tied maximum at a lower / at a higher index than the
    label, an all-equal row, a row of +0 and -0, a NaN beside / at the label, +inf beside the label, +inf at the label and
    after it, -inf at the label, an all-NaN row, an ignored row."""
    rows, cols = shape
    x, y = plain_case(shape, torch.float32, seed=31 + variant)
    gen = torch.Generator().manual_seed(99 + variant)
    y = torch.randint(0, cols, (rows,), generator=gen)
    other = lambda r: (int(y[r]) + 1 + int(torch.randint(0, max(cols - 1, 1), (1,), generator=gen))) % cols     # noqa: E731
    for r in range(rows):
        t = r + variant
        big = float(x[r].abs().max()) + 1.0
        if t == 0:
            y[r] = 0
        elif t == 1:
            y[r] = cols - 1
        elif t == 2:                      # the label is the second of two equal maxima: rank 1 (0 where cols == 1)
            y[r] = cols - 1
            x[r, 0] = x[r, cols - 1] = big
        elif t == 3:                      # the label is the first of two equal maxima: rank 0
            y[r] = 0
            x[r, 0] = x[r, cols - 1] = big
        elif t == 4:
            x[r] = 0.5
        elif t == 5:
            x[r] = 0.0
            x[r, ::2] = -0.0
        elif t == 6 and cols > 1:
            x[r, other(r)] = float("nan")
        elif t == 7:
            x[r, int(y[r])] = float("nan")
            x[r, other(r)] = float("nan")
        elif t == 8 and cols > 1:
            x[r, other(r)] = float("inf")
        elif t == 9:
            y[r] = cols // 2
            x[r, cols // 2] = x[r, cols - 1] = float("inf")
        elif t == 10:
            x[r, int(y[r])] = float("-inf")
        elif t == 11:
            x[r] = float("nan")
        elif t == 12:
            y[r] = IGNORE
    return x.to(dtype), y


def edge_variants(shape):
    """The variants of edge_case that between them plant every treatment in a tensor of this many rows."""
    return list(range(0, N_EDGES, min(shape[0], N_EDGES)))
