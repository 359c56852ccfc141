"""GPU (-m gpu): the 16-bit BatchNorm backward (mhaq_fq_bn_bwd_x16, csrc/bn_bwd.hip) through the C ABI, the compiled node
and the module, in bf16 and fp16, against the contract of tests/bn_bwd16_contract.py: the fp64 closed form from the SAVED
fp32 mean / invstd on the exactly upcast 16-bit x and dy, an elementwise bound of 1e-6 of the term sum plus the one rounding,
and the nearest-even 16-bit value of the reference wherever that is decided beyond the bound.

Inputs are those of tests/test_gpu_bn_backward.py cast to the dtype; the forward is aten._batch_norm_impl_index on the
16-bit x with fp32 gamma / beta, so the statistics are the framework's own.  The framework's own 16-bit backward is evaluated
on the same inputs and its figures are printed next to ours: recorded, not asserted.
"""
import copy
import ctypes

import pytest
import torch
from torch import nn

from tests import bn_bwd16_contract as K
from tests.test_gpu_bn_backward import _inputs as _inputs32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5
BF16, F16 = torch.bfloat16, torch.float16
DTYPES = [BF16, F16]
_ids = lambda s: "x".join(map(str, s))
_dt = lambda d: "bf16" if d is BF16 else "fp16"

# the smallest shapes that reach each code path (a lane owns 8 channels, a block 16 column vectors = 128 channels)
SHAPES = [(2, 8, 1, 1),            # one vector, M = 2
          (2, 64, 3, 3),
          (3, 24, 5, 5),           # 3 column vectors: idle lanes, constants re-fetched per vector
          (5, 512, 7, 7),          # column split
          (1, 8, 1, 9),
          (8, 64, 56, 56),         # several row chunks
          (7, 8, 389, 385),        # one column vector, ragged last chunk and ragged last dx block
          (3, 136, 5, 5)]          # 17 vectors: a ragged last column group
# one case just above each size threshold of the launcher (csrc/bn_bwd.hip: kBn16BigElems = 20 Mi elements,
# kBn16ReduceNtElems = kBn16DxNtElems = 56 Mi): the smallest [1, 64, H, W] with 64 H W >= the threshold
THRESHOLD_SHAPES = [(1, 64, 640, 512), (1, 64, 896, 1024)]


@pytest.fixture(autouse=True)
def _deterministic_miopen():
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = det


def _inputs(shape, dtype, seed=0):
    x, dy, gamma, beta = _inputs32(shape, seed)
    return x.to(dtype), dy.to(dtype), gamma, beta


def _forward(x, gamma, beta):
    c = x.shape[1]
    rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
    fwd = torch.ops.aten._batch_norm_impl_index(x, gamma, beta, rm, rv, True, 0.1, EPS, True)
    assert fwd[1].dtype == torch.float32 and fwd[2].dtype == torch.float32
    return fwd, rm, rv


def _stock_backward(x, dy, gamma, fwd, rm, rv):
    _, mean, invstd, reserve, impl = fwd
    return torch.ops.aten._batch_norm_impl_index_backward(impl, x, dy, gamma, rm, rv, mean, invstd, True, EPS,
                                                          [True, True, True], reserve)


def _code(dtype):
    from mhaq_amd import _lib
    return _lib.DT_BF16 if dtype is BF16 else _lib.DT_F16


def _hip_backward(x, dy, mean, invstd, gamma, want=(True, True, True)):
    from mhaq_amd import _lib
    L = _lib.lib()
    c = x.shape[1]
    m = x.numel() // c
    nb = L.mhaq_fq_bn_bwd_x16_workspace_bytes(m, c)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    dx = torch.empty_like(x) if want[0] else None
    dw = torch.empty(c, device=DEV) if want[1] else None
    db = torch.empty(c, device=DEV) if want[2] else None
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    rc = L.mhaq_fq_bn_bwd_x16(p(x), p(dy), p(mean), p(invstd), p(gamma), p(dx), p(dw), p(db), m, c, _code(x.dtype), p(ws),
                              nb, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    return dx, dw, db


def _same_bits(a, b):
    if a is None or b is None:
        return a is b
    return a.dtype == b.dtype and torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def _stock_figure(got, ref, ref_abs):
    """The framework's 16-bit dx in the checker's unit: the largest |got - ref| - spacing16(got) / 2 over ref_abs."""
    g = got.double()
    ok = torch.isfinite(ref) & torch.isfinite(g) & (ref_abs > 0) & torch.isfinite(ref_abs)
    if not bool(ok.any()):
        return 0.0
    return float((((g - ref).abs() - K.spacing16(got) / 2)[ok] / ref_abs[ok]).max())


def _check(x, dy, gamma, fwd, rm, rv, label, got=None):
    """dx by check_dx16, dgamma / dbeta within 1e-6 of their term sums; the framework's figures printed beside ours."""
    _, mean, invstd, _, _ = fwd
    m = x.numel() // x.shape[1]
    cf = K.closed_form(x, dy, gamma, mean, invstd)
    new = got if got is not None else _hip_backward(x, dy, mean, invstd, gamma)
    old = _stock_backward(x, dy, gamma, fwd, rm, rv)
    f_old = _stock_figure(K.rows(old[0]), cf["dx"], cf["dx_abs"])
    fig = K.check_dx16(K.rows(new[0]), cf["dx"], cf["dx_abs"], x.dtype, cap=m >= 9)
    print(f"{label} dx: new {fig['err']:.3e}  stock {f_old:.3e}  (term sums beyond the rounding)  excluded {fig['excluded']:.4f}")
    for name, a, b, ref, ref_abs in (("dgamma", new[1], old[1], cf["dg"], cf["dg_abs"]),
                                     ("dbeta", new[2], old[2], cf["db"], cf["db_abs"])):
        f_new = K.check_sums(a, ref, ref_abs, (label, name))
        ok = torch.isfinite(ref) & (ref_abs > 0)
        f_stock = float(((b.double() - ref).abs()[ok] / ref_abs[ok]).max()) if bool(ok.any()) else 0.0
        print(f"{label} {name}: new {f_new:.3e}  stock {f_stock:.3e}  (units of the term sum)")
    return new, cf


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_c_abi_against_the_fp64_closed_form(shape, dtype):
    x, dy, gamma, beta = _inputs(shape, dtype)
    fwd, rm, rv = _forward(x, gamma, beta)
    new, _ = _check(x, dy, gamma, fwd, rm, rv, f"{shape} {_dt(dtype)}")
    # a second run gives the same bits; gamma = NULL is gamma = 1; each output is optional
    again = _hip_backward(x, dy, fwd[1], fwd[2], gamma)
    assert all(_same_bits(a, b) for a, b in zip(new, again))
    one = _hip_backward(x, dy, fwd[1], fwd[2], None)
    ones = _hip_backward(x, dy, fwd[1], fwd[2], torch.ones_like(gamma))
    assert all(_same_bits(a, b) for a, b in zip(one, ones))
    only = _hip_backward(x, dy, fwd[1], fwd[2], gamma, want=(False, True, False))
    assert only[0] is None and only[2] is None and _same_bits(only[1], new[1])
    only = _hip_backward(x, dy, fwd[1], fwd[2], gamma, want=(False, False, True))
    assert _same_bits(only[2], new[2])
    only = _hip_backward(x, dy, fwd[1], fwd[2], gamma, want=(True, False, False))
    assert _same_bits(only[0], new[0])


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("kind", ["constant_channel", "gamma_sign", "far_mean", "zero_dy"])
def test_planted_cases(kind, dtype):
    x, dy, gamma, beta = _planted24(kind, dtype)
    fwd, rm, rv = _forward(x, gamma, beta)
    new, cf = _check(x, dy, gamma, fwd, rm, rv, f"{kind} {_dt(dtype)}")
    if kind == "constant_channel":
        assert float(fwd[2][7]) == pytest.approx(EPS ** -0.5, rel=1e-3)      # variance 0: invstd = eps^-1/2
    if kind == "gamma_sign":
        assert bool((new[0][:, 0] == 0).all()) and bool((new[0][:, 2] == 0).all())
    if kind == "zero_dy":
        assert all(bool((t == 0).all()) for t in new)


def _planted24(kind, dtype):
    """The planted cases of the fp32 suite on (3, 24, 5, 5) -- its 20 channels are no multiple of 8 --, planted the same way
    and then cast."""
    shape = (3, 24, 5, 5)
    x, dy, gamma, beta = _inputs32(shape, seed=5)
    if kind == "constant_channel":
        x[:, 3] = 3.0
        x[:, 7] = 0.0
    elif kind == "gamma_sign":
        gamma[0], gamma[1], gamma[2] = 0.0, -1.5, -0.0
    elif kind == "far_mean":
        x[:, 4] = 1e4 + torch.randn(3, 5, 5, generator=torch.Generator().manual_seed(6)).to(DEV)
        x[:, 9] = -1e4 + torch.randn(3, 5, 5, generator=torch.Generator().manual_seed(7)).to(DEV)
    elif kind == "far_mean_spread":
        # around 1e4 adjacent bf16 values are 64 apart: 1e4 + randn is ONE value, a constant channel.  This one keeps a
        # spread after the cast, and a dy that follows x (dgamma / M of order one): tests/test_bn_backward16_cpu.py
        for ch, mu, seed in ((4, 1e4, 6), (9, -1e4, 7)):
            z = torch.randn(3, 5, 5, generator=torch.Generator().manual_seed(seed)).to(DEV)
            x[:, ch] = mu + 64 * z
            dy[:, ch] = z + 0.5 * dy[:, ch]
    elif kind == "zero_dy":
        dy.zero_()
    return x.to(dtype), dy.to(dtype), gamma, beta


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_far_mean_with_a_spread_that_survives_the_cast(dtype):
    x, dy, gamma, beta = _planted24("far_mean_spread", dtype)
    fwd, rm, rv = _forward(x, gamma, beta)
    assert float(fwd[1][4]) > 9e3 and float(fwd[1][9]) < -9e3 and float(fwd[2][4]) < 0.1
    _check(x, dy, gamma, fwd, rm, rv, f"far_mean_spread {_dt(dtype)}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_one_nan_in_dy_poisons_its_own_channel_only(dtype):
    x, dy, gamma, beta = _inputs((3, 24, 5, 5), dtype, seed=8)
    fwd, rm, rv = _forward(x, gamma, beta)
    clean = _hip_backward(x, dy, fwd[1], fwd[2], gamma)
    dy2 = dy.clone()
    dy2[1, 6, 2, 3] = float("nan")
    got = _hip_backward(x, dy2, fwd[1], fwd[2], gamma)
    others = [c for c in range(24) if c != 6]
    assert bool(torch.isnan(got[0][:, 6]).all()) and bool(torch.isnan(got[1][6])) and bool(torch.isnan(got[2][6]))
    assert _same_bits(got[0][:, others], clean[0][:, others])
    assert _same_bits(got[1][others], clean[1][others]) and _same_bits(got[2][others], clean[2][others])


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_infinities_and_a_negative_zero_in_dy(dtype):
    """+inf and -inf in dy (different channels) make their channels' sums infinite and every dx of those channels NaN or
    infinite as the closed form has it; a -0.0 is a zero.  All other channels keep their bits."""
    x, dy, gamma, beta = _inputs((3, 24, 5, 5), dtype, seed=9)
    gamma = gamma.abs() + 0.5
    fwd, rm, rv = _forward(x, gamma, beta)
    dy[0, 2, 0, 0] = -0.0
    clean = _hip_backward(x, dy, fwd[1], fwd[2], gamma)
    dy2 = dy.clone()
    dy2[1, 5, 2, 3] = float("inf")
    dy2[2, 11, 4, 1] = float("-inf")
    got = _hip_backward(x, dy2, fwd[1], fwd[2], gamma)
    cf = K.closed_form(x, dy2, gamma, fwd[1], fwd[2])
    K.check_dx16(K.rows(got[0]), cf["dx"], cf["dx_abs"], dtype, cap=False)
    assert float(got[2][5]) == float("inf") and float(got[2][11]) == float("-inf")
    assert not bool(torch.isfinite(got[0][:, 5]).any()) and not bool(torch.isfinite(got[0][:, 11]).any())
    others = [c for c in range(24) if c not in (5, 11)]
    assert _same_bits(got[0][:, others], clean[0][:, others]) and _same_bits(got[2][others], clean[2][others])
    # the -0.0 counts as a zero: the same results as with +0.0 in its place
    dy3 = dy.clone()
    dy3[0, 2, 0, 0] = 0.0
    assert all(_same_bits(a, b) for a, b in zip(clean, _hip_backward(x, dy3, fwd[1], fwd[2], gamma)))


def test_fp16_dx_overflows_to_infinity():
    """gamma * invstd large enough that one element's dx leaves the fp16 range: +-inf there (a plain conversion), as the
    checker allows at the top of the range only; the rest of the channel stays finite and inside the bound."""
    x, dy, gamma, beta = _inputs((3, 24, 5, 5), F16, seed=10)
    fwd, rm, rv = _forward(x, gamma, beta)
    dy[:, 3] = 0.0
    dy[1, 3, 2, 2] = 60000.0
    gamma[3] = 4.0 * float(1.0 / fwd[2][3])          # gamma * invstd ~ 4: dx ~ 4 * 60000 * (1 - 1 / M - xhat^2 / M)
    got = _hip_backward(x, dy, fwd[1], fwd[2], gamma)
    cf = K.closed_form(x, dy, gamma, fwd[1], fwd[2])
    K.check_dx16(K.rows(got[0]), cf["dx"], cf["dx_abs"], F16, cap=False)
    assert float(cf["dx"].abs().max()) > 65520.0
    assert float(got[0][1, 3, 2, 2]) == float("inf") and int(torch.isinf(got[0]).sum()) == 1
    assert bool(torch.isfinite(got[1]).all()) and bool(torch.isfinite(got[2]).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_argument_errors_leave_the_outputs_untouched(dtype):
    from mhaq_amd import _lib
    L = _lib.lib()
    x, dy, gamma, beta = _inputs((2, 64, 3, 3), dtype)
    fwd, _, _ = _forward(x, gamma, beta)
    m, c = 18, 64
    nb = L.mhaq_fq_bn_bwd_x16_workspace_bytes(m, c)
    sent = 0x5A
    ws = torch.full((nb + 16,), sent, dtype=torch.uint8, device=DEV)
    dx = torch.full((x.numel() * 2 + 16,), sent, dtype=torch.uint8, device=DEV)
    dw = torch.full((c * 4,), sent, dtype=torch.uint8, device=DEV)
    db = torch.full((c * 4,), sent, dtype=torch.uint8, device=DEV)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = [p(x), p(dy), p(fwd[1]), p(fwd[2]), p(gamma), p(dx), p(dw), p(db), m, c, _code(dtype), p(ws), nb, st]
    for k, off in ((0, 2), (1, 8), (5, 4), (11, 8)):                 # misaligned x / dy / dx / workspace
        bad = list(args)
        bad[k] = ctypes.c_void_p(args[k].value + off)
        assert L.mhaq_fq_bn_bwd_x16(*bad) == -3, k
    short = list(args)
    short[12] = nb - 1
    assert L.mhaq_fq_bn_bwd_x16(*short) == -2
    for cc in (60, 68):                                              # C % 8 != 0 (C % 4 == 0: the fp32 entry takes it)
        odd = list(args)
        odd[9] = cc
        odd[12] = 1 << 30
        assert L.mhaq_fq_bn_bwd_x16(*odd) == -4, cc
    for dt in (0, 3):
        bad = list(args)
        bad[10] = dt
        assert L.mhaq_fq_bn_bwd_x16(*bad) == -1, dt
    torch.cuda.synchronize()
    for buf in (ws, dx, dw, db):
        assert bool((buf == sent).all())                             # refused before any launch


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("shape", [(3, 24, 5, 5), (8, 64, 56, 56), (5, 512, 7, 7)], ids=_ids)
def test_sentinel_guards_around_dx_and_the_workspace(shape, dtype):
    from mhaq_amd import _lib
    L = _lib.lib()
    x, dy, gamma, beta = _inputs(shape, dtype)
    fwd, _, _ = _forward(x, gamma, beta)
    c = shape[1]
    m = x.numel() // c
    nb = L.mhaq_fq_bn_bwd_x16_workspace_bytes(m, c)
    guard = 4096                                               # bytes on either side, a multiple of 16
    sent = 0x5A
    wsbuf = torch.full((nb + 2 * guard,), sent, dtype=torch.uint8, device=DEV)
    dxbuf = torch.full((x.numel() * 2 + 2 * guard,), sent, dtype=torch.uint8, device=DEV)
    outbuf = torch.full((2 * c * 4 + 3 * 64,), sent, dtype=torch.uint8, device=DEV)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    rc = L.mhaq_fq_bn_bwd_x16(p(x), p(dy), p(fwd[1]), p(fwd[2]), p(gamma), p(dxbuf, guard), p(outbuf, 64),
                              p(outbuf, 128 + c * 4), m, c, _code(dtype), p(wsbuf, guard), nb,
                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    for buf, body in ((wsbuf, nb), (dxbuf, x.numel() * 2)):
        assert bool((buf[:guard] == sent).all()) and bool((buf[guard + body:] == sent).all())
    assert bool((outbuf[:64] == sent).all()) and bool((outbuf[64 + c * 4:128 + c * 4] == sent).all())
    assert bool((outbuf[128 + 2 * c * 4:] == sent).all())
    ref = _hip_backward(x, dy, fwd[1], fwd[2], gamma)
    assert torch.equal(dxbuf[guard:guard + x.numel() * 2].view(torch.int16), K.rows(ref[0]).reshape(-1).view(torch.int16))
    assert torch.equal(outbuf[64:64 + c * 4].view(torch.float32), ref[1])
    assert torch.equal(outbuf[128 + c * 4:128 + 2 * c * 4].view(torch.float32), ref[2])


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("shape", THRESHOLD_SHAPES, ids=_ids)
def test_one_case_just_above_each_size_threshold(shape, dtype):
    """The launcher changes kernels at 20 Mi elements (occupancy of the dx kernel) and at 56 Mi (non-temporal loads in both
    passes).  Inputs are drawn on the device; the fp64 closed form is evaluated in row blocks (sums first), so the
    reference stays well under 4 GB."""
    n, c, h, w = shape
    m = n * h * w
    assert m * c in (20 << 20, 56 << 20)
    gen = torch.Generator(device=DEV).manual_seed(12)
    x = (torch.randn((m, c), device=DEV, generator=gen) * (0.5 + 3 * torch.rand(c, device=DEV, generator=gen))
         + 2 * torch.randn(c, device=DEV, generator=gen)).to(dtype)
    dy = torch.randn((m, c), device=DEV, generator=gen).to(dtype)
    gamma, beta = torch.randn(c, device=DEV, generator=gen), torch.randn(c, device=DEV, generator=gen)
    as4d = lambda t: t.view(n, h, w, c).permute(0, 3, 1, 2)             # channels_last [N, C, H, W] over the same memory
    x4, dy4 = as4d(x), as4d(dy)
    assert x4.is_contiguous(memory_format=torch.channels_last)
    fwd, rm, rv = _forward(x4, gamma, beta)
    mean, invstd = fwd[1], fwd[2]
    new = _hip_backward(x4, dy4, mean, invstd, gamma)
    again = _hip_backward(x4, dy4, mean, invstd, gamma)
    assert all(_same_bits(a, b) for a, b in zip(new, again))
    mu, iv, ga = mean.double(), invstd.double(), gamma.double()
    step = 1 << 17
    db = torch.zeros(c, dtype=torch.float64, device=DEV)
    db_abs, s2, s2_abs = db.clone(), db.clone(), db.clone()
    for r in range(0, m, step):
        G, d = dy[r:r + step].double(), x[r:r + step].double() - mu
        db += G.sum(0)
        db_abs += G.abs().sum(0)
        s2 += (G * d).sum(0)
        s2_abs += (G * d).abs().sum(0)
    dg, dg_abs = iv * s2, iv * s2_abs
    f_g = K.check_sums(new[1], dg, dg_abs, "dgamma")
    f_b = K.check_sums(new[2], db, db_abs, "dbeta")
    got = K.rows(new[0])
    worst, excluded = -1.0, 0.0
    for r in range(0, m, step):
        G, xh = dy[r:r + step].double(), (x[r:r + step].double() - mu) * iv
        ref = ga * iv * (G - db / m - xh * dg / m)
        ref_abs = ga.abs() * iv * (G.abs() + db.abs() / m + xh.abs() * dg.abs() / m)
        fig = K.check_dx16(got[r:r + step], ref, ref_abs, dtype)
        worst, excluded = max(worst, fig["err"]), max(excluded, fig["excluded"])
    print(f"{shape} {_dt(dtype)}: dx {worst:.3e} (excluded <= {excluded:.4f})  dgamma {f_g:.3e}  dbeta {f_b:.3e}")


# ------------------------------------------------------------------------------------------------ the node and the module
def _pair(c, x16=True, **kw):
    from mhaq_amd import bn_backward
    torch.manual_seed(4)
    stock = nn.BatchNorm2d(c, **kw).to(DEV)
    with torch.no_grad():
        stock.weight.uniform_(-1.5, 1.5)
        stock.bias.uniform_(-1, 1)
    mine = copy.deepcopy(stock)
    assert bn_backward.install(mine, x16=x16) == 1
    return stock, mine


def _step(bn, x, g):
    x = x.clone().requires_grad_(True)
    for p in bn.parameters():
        p.grad = None
    y = bn(x)
    y.backward(g)
    own = lambda t: None if t is None else t.clone()          # a later backward accumulates into .grad in place
    return dict(y=y.detach(), dx=x.grad, dw=own(bn.weight.grad), db=own(bn.bias.grad), rm=bn.running_mean.clone(),
                rv=bn.running_var.clone(), nb=bn.num_batches_tracked.clone())


def _counts():
    from mhaq_amd import _ext
    E = _ext.ext()
    return E.bn_hip_backwards(), E.bn_hip_backwards_x16()


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("shape", [(2, 64, 3, 3), (3, 24, 5, 5), (5, 512, 7, 7), (8, 64, 56, 56)], ids=_ids)
def test_module_keeps_the_forward_bits_and_runs_the_16_bit_backward(shape, dtype):
    x, dy, _, _ = _inputs(shape, dtype, seed=2)
    stock, mine = _pair(shape[1])
    n0 = _counts()
    a, b = _step(stock, x, dy), _step(mine, x, dy)
    assert _counts() == (n0[0], n0[1] + 1)                      # never a silent fallback, and not the fp32 route
    for k in ("y", "rm", "rv", "nb"):
        assert _same_bits(a[k], b[k]), k
    assert b["dx"].dtype == dtype and b["dw"].dtype == torch.float32
    gamma, beta = stock.weight.detach(), stock.bias.detach()
    fwd, rm, rv = _forward(x, gamma, beta)
    _check(x, dy, gamma, fwd, rm, rv, f"module {shape} {_dt(dtype)}", got=(b["dx"], b["dw"], b["db"]))


@pytest.mark.parametrize("case", ["flag_off", "c_not_multiple_of_8", "nchw", "bf16_weights", "fp32_dy", "eval"])
def test_fallback_equals_stock_batchnorm_bit_for_bit(case):
    shape = (2, 12, 4, 4) if case == "c_not_multiple_of_8" else (4, 8, 6, 5)
    x, dy, _, _ = _inputs(shape, BF16, seed=3)
    if case == "nchw":
        x, dy = x.contiguous(), dy.contiguous()
    stock, mine = _pair(shape[1], x16=case != "flag_off")
    if case == "bf16_weights":
        stock, mine = stock.bfloat16(), mine.bfloat16()
    if case == "eval":
        stock, mine = stock.eval(), mine.eval()
    n0 = _counts()
    if case == "fp32_dy":
        _direct_fp32_dy(x, dy, stock)
    else:
        a, b = _step(stock, x, dy), _step(mine, x, dy)
        for k in a:
            assert _same_bits(a[k], b[k]), k
    assert _counts() == n0


def _direct_fp32_dy(x, dy, stock):
    """An fp32 gradient for the node's bf16 output.  The autograd engine casts a gradient to its output's dtype before a
    node sees it, so this reaches the node only when its backward is called directly: it must then take the framework's
    backward on that very dy -- the same bits, or the same refusal."""
    from mhaq_amd import _ext
    m1, m2 = copy.deepcopy(stock), copy.deepcopy(stock)
    fwd = torch.ops.aten._batch_norm_impl_index(x, m1.weight, m1.bias, m1.running_mean, m1.running_var, True, 0.1, EPS, True)
    xi = x.clone().requires_grad_(True)
    y = _ext.ext().bn_train(xi, m2.weight, m2.bias, m2.running_mean, m2.running_var, 0.1, EPS, True, True)
    assert _same_bits(y.detach(), fwd[0])
    stock_bwd = lambda: torch.ops.aten._batch_norm_impl_index_backward(
        fwd[4], x, dy.float(), m1.weight, m1.running_mean, m1.running_var, fwd[1], fwd[2], True, EPS, [True, True, True], fwd[3])
    try:
        ref = stock_bwd()
    except RuntimeError:
        with pytest.raises(RuntimeError):
            y.grad_fn(dy.float())
        return
    got = y.grad_fn(dy.float())
    assert all(_same_bits(p, q) for p, q in zip(ref, got[:3]))


def test_frozen_weight_or_bias_follows_needs_input_grad():
    x, dy, _, _ = _inputs((3, 24, 5, 5), BF16, seed=4)
    _, mine = _pair(24)
    full = _step(mine, x, dy)
    mine.weight.requires_grad_(False)
    got = _step(mine, x, dy)
    assert got["dw"] is None and _same_bits(got["dx"], full["dx"]) and _same_bits(got["db"], full["db"])
    mine.weight.requires_grad_(True)
    mine.bias.requires_grad_(False)
    got = _step(mine, x, dy)
    assert got["db"] is None and _same_bits(got["dx"], full["dx"]) and _same_bits(got["dw"], full["dw"])
    mine.bias.requires_grad_(True)
    n0 = _counts()
    got = _step(mine, x, dy.contiguous())                       # the same values, NCHW strides
    assert _counts() == (n0[0], n0[1] + 1)
    for k in ("dx", "dw", "db"):
        assert _same_bits(got[k], full[k]), k


def test_forward_and_backward_in_a_captured_graph_replay_like_eager():
    x, dy, _, _ = _inputs((8, 64, 56, 56), BF16, seed=6)
    _, mine = _pair(64)
    state = {k: v.clone() for k, v in mine.state_dict().items()}
    eager = [_step(mine, x, dy) for _ in range(3)]
    mine.load_state_dict(state)
    xs = x.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                               # warm-up off the capturing stream
        mine(xs).backward(dy)
    torch.cuda.current_stream().wait_stream(side)
    mine.load_state_dict(state)
    xs.grad = mine.weight.grad = mine.bias.grad = None
    n0 = _counts()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ys = mine(xs)
        ys.backward(dy)
    assert _counts() == (n0[0], n0[1] + 1)
    mine.load_state_dict(state)
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        e = eager[k]
        assert _same_bits(ys, e["y"]) and _same_bits(xs.grad, e["dx"])
        assert _same_bits(mine.weight.grad, e["dw"]) and _same_bits(mine.bias.grad, e["db"])
        assert _same_bits(mine.running_mean, e["rm"]) and _same_bits(mine.running_var, e["rv"])


# ------------------------------------------------------------------------------------------------ the trainer
STEPS = 4


def _trainer(x16=None, capture=False):
    import mhaq_amd as M
    from mhaq_amd import nets, ops
    from mhaq_amd.qat import QATConfig, QATTrainer
    torch.manual_seed(3)
    ops.manual_seed(3)
    net = nets.resnet18(10).to(memory_format=torch.channels_last)
    g = torch.Generator().manual_seed(2)
    calib = torch.randn(4, 3, 64, 64, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    kw = {} if x16 is None else dict(hip_bn_backward_16bit=x16)
    cfg = QATConfig(qscheme=M.QScheme.PER_CHANNEL, qnmethod=M.QNMethod.LSQ, distillation=True, warmup=2,
                    learning_rate=1e-3, autocast_dtype=BF16, **kw)
    return QATTrainer(net, cfg, DEV, calib_batches=[calib], distributed=False, capture_graph=capture)


def _batches(n):
    gen = torch.Generator().manual_seed(9)
    return [(torch.randn(4, 3, 64, 64, generator=gen).to(DEV).contiguous(memory_format=torch.channels_last),
             torch.randint(0, 10, (4,), generator=gen).to(DEV)) for _ in range(n)]


def _run(tr, batches):
    losses = [float(tr.train_step(x, y)) for x, y in batches]
    return losses, [p.detach().clone() for p in tr.net.parameters()]


def test_trainer_default_is_off_and_equals_the_explicit_off(monkeypatch):
    from mhaq_amd import bn_backward
    monkeypatch.delenv(bn_backward.ENV_SWITCH_X16, raising=False)
    batches = _batches(STEPS)
    n0 = _counts()
    tr = _trainer()
    assert not any(m.takes_x16() for m in tr.net.modules() if type(m) is bn_backward.HipBackwardBatchNorm2d)
    default = _run(tr, batches)
    assert _counts()[1] == n0[1]
    monkeypatch.setenv(bn_backward.ENV_SWITCH_X16, "0")
    off = _run(_trainer(), batches)
    assert _counts()[1] == n0[1]
    assert default[0] == off[0] and all(_same_bits(a, b) for a, b in zip(default[1], off[1]))
    # the environment decides when it is set, either way
    assert not any(m.takes_x16() for m in _trainer(x16=True).net.modules() if hasattr(m, "takes_x16"))
    monkeypatch.setenv(bn_backward.ENV_SWITCH_X16, "1")
    assert all(m.takes_x16() for m in _trainer().net.modules() if hasattr(m, "takes_x16"))


def test_trainer_with_the_16_bit_backward(monkeypatch):
    from mhaq_amd import bn_backward, fused_blocks
    monkeypatch.delenv(bn_backward.ENV_SWITCH_X16, raising=False)
    batches = _batches(STEPS)
    default = _run(_trainer(), batches)
    tr = _trainer(x16=True)
    assert type(tr.net) is fused_blocks.FusedResNet18
    layers = sum(type(m) is bn_backward.HipBackwardBatchNorm2d for m in tr.net.modules())
    assert layers == 20 and all(m.takes_x16() for m in tr.net.modules() if hasattr(m, "takes_x16"))
    assert not any(hasattr(m, "takes_x16") for m in tr.teacher.modules())
    n0 = _counts()
    eager = _run(tr, batches)
    assert _counts() == (n0[0], n0[1] + layers * STEPS)          # every student BatchNorm, the stem's included, every step
    assert eager[0][0] == default[0][0]                          # the forward is untouched
    assert all(v == v and abs(v) != float("inf") for v in eager[0]), eager[0]
    assert any(not _same_bits(a, b) for a, b in zip(default[1], eager[1]))       # (the gradients did change)
    graphed = _run(_trainer(x16=True, capture=True), batches)
    assert eager[0] == graphed[0] and all(_same_bits(a, b) for a, b in zip(eager[1], graphed[1]))
