"""GPU (-m gpu): the classification head (mhaq_fq_cls_head_fwd, csrc/cls_head.hip) through the C ABI, mhaq_amd.cls_metrics and
mhaq_amd.loss.FusedCrossEntropy, against the definitions restated in float64 on the CPU (tests/cls_head_ref.py).  Ranks and
counts are exact integers; the bars of the floating-point outputs are the framework's own float32 chain on the device:
    |L - L64| <= 4 |L_torch - L64| + 8 ulp32(L64),   max|gx - g64| <= 4 max|g_torch - g64| + 8 2^-24 max|g64|,
    max|nll - nll64| <= 4 max|nll_torch - nll64| + 8 ulp32(max|nll64|).
Every C-ABI call here has its outputs and its workspace between bands of ones, poisoned: nothing outside them may be written,
every element inside them must be.  A label out of range is only ever handed to the new entry point."""
import ctypes
import functools

import pytest
import torch

from tests import cls_head_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAND = 64                                  # elements of ones planted before and after every output
POISON = -7.0
G_UP = 0.375                               # a non-trivial upstream gradient
DT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
ids_shape = lambda s: "%dx%d" % s          # noqa: E731
ids_dtype = lambda d: str(d).split(".")[1]  # noqa: E731


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Banded:
    """n poisoned elements between two bands of ones, the view 16-byte aligned plus `shift` elements."""

    def __init__(self, n, dtype, shift=0):
        self.buf = torch.ones(BAND + shift + n + BAND, dtype=dtype, device=DEV)
        self.lo, self.n = BAND + shift, n
        self.view = self.buf[self.lo:self.lo + n]
        self.view.fill_(POISON)

    def intact(self):
        return bool((self.buf[:self.lo] == 1).all()) and bool((self.buf[self.lo + self.n:] == 1).all())

    def written(self):
        return not bool((self.view == POISON).any())


def capi(x, y, topk=5, ignore_index=R.IGNORE, want_grad=True, want_rows=True, shift=0):
    """One call of mhaq_fq_cls_head_fwd on device tensors -> dict of its outputs; asserts that nothing around an output or the
    workspace was written and that every element of them was."""
    from mhaq_amd import _lib
    lib = _lib.lib()
    rows, cols = x.shape
    assert x.is_contiguous() and y.is_contiguous() and y.dtype == torch.int64
    wsb = lib.mhaq_fq_cls_head_workspace_bytes(rows)
    assert wsb == rows * 16
    o = dict(ws=Banded(2 * rows, torch.float64), loss=Banded(1, torch.float32), acc=Banded(2, torch.float32),
             counts=Banded(3, torch.int64), flags=Banded(1, torch.int32))
    if want_rows:
        o.update(nll=Banded(rows, torch.float32, shift), rank=Banded(rows, torch.int32, shift))
    if want_grad:
        o["gunit"] = Banded(rows * cols, torch.float32, shift)
    p = lambda k: _ptr(o[k].view) if k in o else None      # noqa: E731
    _lib.check(lib.mhaq_fq_cls_head_fwd(_ptr(x), DT[x.dtype], _ptr(y), rows, cols, ignore_index, topk, p("loss"), p("acc"),
                                        p("counts"), p("nll"), p("rank"), p("gunit"), p("flags"), p("ws"), wsb, _stream()),
               "mhaq_fq_cls_head_fwd")
    torch.cuda.synchronize()
    for k, b in o.items():
        assert b.intact(), f"{k}: written outside"
        assert b.written(), f"{k}: an element was not written"
    out = {k: b.view.clone() for k, b in o.items() if k != "ws"}
    if want_grad:
        out["gunit"] = out["gunit"].reshape(rows, cols)
    return out


def capi_bwd(gunit, g, dtype, shift=0):
    from mhaq_amd import _lib
    lib = _lib.lib()
    gx = Banded(gunit.numel(), dtype, shift)
    gdev = torch.tensor([g], dtype=torch.float32, device=DEV)
    _lib.check(lib.mhaq_fq_distill_loss_bwd(_ptr(gunit), _ptr(gdev), _ptr(gx.view), DT[dtype], gunit.numel(), _stream()),
               "mhaq_fq_distill_loss_bwd")
    torch.cuda.synchronize()
    assert gx.intact() and gx.written()
    return gx.view.reshape(gunit.shape).clone()


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same_bits(a, b, keys):
    return [k for k in keys if not torch.equal(_bits(a[k]), _bits(b[k]))]


@functools.lru_cache(maxsize=None)
def _plain(shape):
    """-> (x, y on the device, the framework's float32 chain there, the float64 reference): computed once, never modified."""
    x, y = R.plain_case(shape)
    xd, yd = x.to(DEV), y.to(DEV)
    return xd, yd, R.chain32(xd, yd, g=G_UP), R.head64(x, y)


# ---------------------------------------------------------------------------------------------- exact integers
@pytest.mark.parametrize("dtype", DTYPES, ids=ids_dtype)
@pytest.mark.parametrize("shape", R.SHAPES, ids=ids_shape)
def test_rank_and_counts_equal_the_stable_sort_on_ties_zeros_nan_and_inf(shape, dtype):
    rows, cols = shape
    cases = [R.plain_case(shape, dtype)] + [R.edge_case(shape, dtype, v) for v in R.edge_variants(shape)]
    for i, (x, y) in enumerate(cases):
        ref = R.head64(x, y, topk=5)
        xd, yd = x.to(DEV), y.to(DEV)
        out = capi(xd, yd, topk=5, want_grad=False)
        assert torch.equal(out["rank"].cpu().long(), ref["rank"]), i
        assert out["counts"].cpu().tolist() == ref["counts"].tolist(), i
        assert torch.equal(_bits(out["acc"].cpu()), _bits(ref["acc"])), i
        valid = ref["valid"]
        hits = int(((xd.float().argmax(1) == yd).cpu() & valid).sum())          # the framework's argmax on the device
        assert int(out["counts"][1]) == hits, i
        finite = torch.isfinite(out["nll"].cpu())
        assert torch.equal(finite[valid], torch.isfinite(ref["nll"])[valid]), i
        assert int(out["flags"]) == (0 if bool(finite[valid].all()) else 2), i
        assert not bool(out["nll"].cpu()[~valid].any()), i
    # topk = 1 counts the top-1 hits twice; topk >= cols counts every valid row
    x, y = cases[-1]
    ref = R.head64(x, y)
    one = capi(x.to(DEV), y.to(DEV), topk=1, want_grad=False, want_rows=False)
    every = capi(x.to(DEV), y.to(DEV), topk=cols + 3, want_grad=False, want_rows=False)
    assert one["counts"].tolist() == [int(ref["counts"][0]), int(ref["counts"][1]), int(ref["counts"][1])]
    assert every["counts"].tolist() == [int(ref["counts"][0]), int(ref["counts"][1]), int(ref["counts"][0])]


def test_sixteen_bit_rows_of_a_thousand_logits_all_hold_ties():
    """... so the tie rule is exercised by ordinary data, not only by planted rows."""
    x, _ = R.plain_case((250, 1000), torch.bfloat16)
    assert all(len(torch.unique(r.float())) < 1000 for r in x)


# ---------------------------------------------------------------------------------------------- accuracy
@pytest.mark.parametrize("shape", R.SHAPES, ids=ids_shape)
def test_loss_nll_and_gradient_meet_the_bar_through_the_c_abi_the_module_and_cls_metrics(shape):
    from mhaq_amd.cls_metrics import check_cls_flags, cls_metrics
    from mhaq_amd.loss import FusedCrossEntropy, cls_head_launches
    x, y, (l_t, nll_t, g_t), ref = _plain(shape)
    out = capi(x, y)
    gx = capi_bwd(out["gunit"], G_UP, torch.float32)
    g64 = ref["gunit"] * G_UP
    el, bl = abs(float(out["loss"]) - float(ref["loss"])), R.loss_bar(l_t, ref["loss"])
    eg, bg = float((gx.double().cpu() - g64).abs().max()), R.grad_bar(g_t, g64)
    en, bn = float((out["nll"].double().cpu() - ref["nll"]).abs().max()), R.nll_bar(nll_t, ref["nll"])
    share = lambda e, b: e / b if b else 0.0      # noqa: E731
    print("bar shares", shape, dict(loss=share(el, bl), grad=share(eg, bg), nll=share(en, bn), loss_err=el,
                                    loss_err_torch=abs(float(l_t) - float(ref["loss"])), grad_err=eg, nll_err=en))
    assert el <= bl and eg <= bg and en <= bn, (el, bl, eg, bg, en, bn)
    assert torch.equal(out["rank"].cpu().long(), ref["rank"]) and out["counts"].cpu().tolist() == ref["counts"].tolist()
    # the same inputs give the same bits: again, without the gradient, without the per-row outputs
    keys = ("loss", "acc", "counts", "nll", "rank", "flags")
    assert not _same_bits(out, capi(x, y), keys + ("gunit",))
    assert not _same_bits(out, capi(x, y, want_grad=False), keys)
    assert not _same_bits(out, capi(x, y, want_rows=False), ("loss", "acc", "counts", "flags", "gunit"))
    # outputs at another alignment (gunit no longer takes 16-byte stores): the integers exactly, the rest within the bars
    off = capi(x, y, shift=1)
    assert not _same_bits(out, off, ("rank", "counts", "acc", "flags"))
    assert abs(float(off["loss"]) - float(ref["loss"])) <= bl
    assert float((off["gunit"].double().cpu() * G_UP - g64).abs().max()) <= bg
    # the module: the same entry points behind autograd
    n0 = cls_head_launches()
    xm = x.clone().requires_grad_(True)
    crit = FusedCrossEntropy()
    lm = crit(xm, y)
    assert lm.dim() == 0 and lm.dtype == torch.float32 and cls_head_launches() - n0 == 2
    (lm * G_UP).backward()
    assert cls_head_launches() - n0 == 3
    assert torch.equal(_bits(lm.detach().reshape(1)), _bits(out["loss"])) and torch.equal(_bits(xm.grad), _bits(gx))
    assert check_cls_flags(crit.last_flags) == 0
    with torch.no_grad():
        assert torch.equal(_bits(FusedCrossEntropy()(xm, y).reshape(1)), _bits(out["loss"]))
    assert cls_head_launches() - n0 == 5
    # the validation face
    m = cls_metrics(x, y)
    assert list(m) == ["loss", "Accuracy_top1", "Accuracy_top5", "counts", "nll", "rank", "flags"]
    got = dict(loss=m["loss"].reshape(1), acc=torch.stack([m["Accuracy_top1"], m["Accuracy_top5"]]), counts=m["counts"],
               nll=m["nll"], rank=m["rank"], flags=m["flags"])
    assert not _same_bits(out, got, keys)
    assert check_cls_flags(m["flags"], nonfinite=True) == 0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=ids_dtype)
@pytest.mark.parametrize("shape", R.SHAPES, ids=ids_shape)
def test_16_bit_logits_equal_the_fp32_entry_on_the_upcast_logits(shape, dtype):
    from mhaq_amd.loss import FusedCrossEntropy
    x, y = R.plain_case(shape, dtype)
    x, y = x.to(DEV), y.to(DEV)
    lo, up = capi(x, y), capi(x.float(), y)
    assert not _same_bits(lo, up, ("loss", "acc", "counts", "nll", "rank", "flags", "gunit"))
    gx = capi_bwd(lo["gunit"], G_UP, dtype)
    assert torch.equal(_bits(gx), _bits((up["gunit"] * G_UP).to(dtype)))        # one rounding to nearest-even
    xm = x.clone().requires_grad_(True)
    lm = FusedCrossEntropy()(xm, y)
    (lm * G_UP).backward()
    assert xm.grad.dtype == dtype and torch.equal(_bits(xm.grad), _bits(gx))
    assert torch.equal(_bits(lm.detach().reshape(1)), _bits(up["loss"]))


def test_module_on_other_shapes_and_another_ignore_index():
    from mhaq_amd.loss import FusedCrossEntropy
    x, y = R.plain_case((16, 100))
    x, y = x.to(DEV), y.to(DEV)
    flat = FusedCrossEntropy()(x, y)
    assert torch.equal(_bits(FusedCrossEntropy()(x.reshape(2, 8, 100), y.reshape(2, 8)).reshape(1)), _bits(flat.reshape(1)))
    assert torch.equal(_bits(FusedCrossEntropy()(x.t().contiguous().t(), y).reshape(1)), _bits(flat.reshape(1)))
    y7 = y.clone()
    y7[3] = 5
    y7[5:9] = 7
    got = FusedCrossEntropy(ignore_index=7)(x, y7)
    l_t = torch.nn.functional.cross_entropy(x, y7, ignore_index=7)
    ref = R.head64(x, y7, ignore_index=7)
    assert int(ref["counts"][0]) == int((y7 != 7).sum()) < 16
    assert abs(float(got) - float(ref["loss"])) <= R.loss_bar(l_t, ref["loss"])
    with pytest.raises(ValueError):
        FusedCrossEntropy()(x, y[:15])
    with pytest.raises(ValueError):
        FusedCrossEntropy()(x, y.int())


# ---------------------------------------------------------------------------------------------- ignored and out-of-range rows
@pytest.mark.parametrize("shape", [(16, 100), (5, 37), (4, 4097)], ids=ids_shape)
def test_ignored_rows_contribute_nothing(shape):
    x, y = R.plain_case(shape)
    y[1::2] = R.IGNORE
    ref = R.head64(x, y)
    xd, yd = x.to(DEV), y.to(DEV)
    l_t, nll_t, g_t = R.chain32(xd, yd)
    out = capi(xd, yd)
    assert out["counts"].cpu().tolist() == ref["counts"].tolist() and int(out["counts"][0]) == (shape[0] + 1) // 2
    assert not bool(out["gunit"][1::2].any()) and not bool(out["nll"][1::2].any())
    assert bool((out["rank"][1::2] == shape[1]).all()) and int(out["flags"]) == 0
    assert abs(float(out["loss"]) - float(ref["loss"])) <= R.loss_bar(l_t, ref["loss"])
    assert float((out["gunit"].double().cpu() - ref["gunit"]).abs().max()) <= R.grad_bar(g_t, ref["gunit"])
    assert float((out["nll"].double().cpu() - ref["nll"]).abs().max()) <= R.nll_bar(nll_t, ref["nll"])
    # the ignored rows' logits do not matter, NaN included: the same bits everywhere else
    x2 = xd.clone()
    x2[1::2] = float("nan")
    out2 = capi(x2, yd)
    assert not _same_bits(out, out2, ("loss", "acc", "counts", "nll", "rank", "flags", "gunit"))
    # every row ignored: a NaN loss as the framework's, zero accuracy and gradient
    none = capi(xd, torch.full_like(yd, R.IGNORE))
    assert bool(torch.isnan(none["loss"]).all()) and none["acc"].tolist() == [0.0, 0.0] and none["counts"].tolist() == [0, 0, 0]
    assert not bool(none["gunit"].any()) and int(none["flags"]) == 0 and bool((none["rank"] == shape[1]).all())


@pytest.mark.parametrize("bad", [-1, "cols", 1 << 40], ids=["minus1", "cols", "2pow40"])
@pytest.mark.parametrize("shape", [(16, 100), (4, 4097)], ids=ids_shape)
def test_a_label_out_of_range_raises_a_flag_and_is_treated_as_ignored(shape, bad):
    """The label goes to the new entry point only; the comparison values come from a run with ignore_index in its place and
    from the CPU reference."""
    from mhaq_amd.cls_metrics import check_cls_flags, cls_metrics
    from mhaq_amd.loss import FusedCrossEntropy
    bad = shape[1] if bad == "cols" else bad
    x, y = R.plain_case(shape)
    y_ign, y_bad = y.clone(), y.clone()
    y_ign[2], y_bad[2] = R.IGNORE, bad
    xd = x.to(DEV)
    a, b = capi(xd, y_ign.to(DEV)), capi(xd, y_bad.to(DEV))
    assert int(a["flags"]) == 0 and int(b["flags"]) == 4
    assert not _same_bits(a, b, ("loss", "acc", "counts", "nll", "rank", "gunit"))
    ref = R.head64(x, y_bad)
    assert torch.equal(b["rank"].cpu().long(), ref["rank"]) and b["counts"].cpu().tolist() == ref["counts"].tolist()
    assert int(b["rank"][2]) == shape[1] and not bool(b["gunit"][2].any())
    with pytest.raises(IndexError, match=r"Target .* is out of bounds\."):
        check_cls_flags(b["flags"])
    m = cls_metrics(xd, y_bad.to(DEV))
    assert torch.equal(_bits(m["loss"].reshape(1)), _bits(a["loss"]))
    with pytest.raises(IndexError):
        check_cls_flags(m["flags"])
    crit = FusedCrossEntropy()
    assert torch.equal(_bits(crit(xd, y_bad.to(DEV)).reshape(1)), _bits(a["loss"]))
    with pytest.raises(IndexError):
        check_cls_flags(crit.last_flags)


# ---------------------------------------------------------------------------------------------- no host sync
def test_no_host_synchronisation_in_cls_metrics_nor_in_the_loss_forward_and_backward():
    from mhaq_amd.cls_metrics import cls_metrics
    from mhaq_amd.loss import FusedCrossEntropy
    x, y, _, ref = _plain((250, 1000))
    xm = x.clone().requires_grad_(True)
    crit = FusedCrossEntropy()
    cls_metrics(x, y)                                   # library and extension are loaded before the mode is switched on
    crit(xm, y).backward()
    xm.grad = None
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        m = cls_metrics(x, y)
        loss = crit(xm, y)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert m["counts"].cpu().tolist() == ref["counts"].tolist() and bool(torch.isfinite(xm.grad).all())
