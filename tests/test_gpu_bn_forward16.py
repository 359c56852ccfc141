"""GPU (-m gpu): the opt-in 16-bit HIP BatchNorm training forward (mhaq_fq_bn_fwd_x16, csrc/bn_bwd.hip) through the C ABI, the
compiled node (`hip_forward_x16` of bn_train), the module and the trainer, in bf16 and fp16, against the contract of
tests/bn_fwd16_contract.py: the fp64 textbook formulas on the exactly upcast input,

    mean = sum x / M,  var = sum (x - mean)^2 / M,  invstd = (var + eps)^-1/2,  y = (x - mean) * invstd * gamma + beta

y within 1e-6 * T + half a 16-bit spacing elementwise and equal to the nearest-even rounding of y64 wherever that is decided
beyond 1e-6 * T; the saved statistics within one fp32 ulp of the rounded fp64 value (the mean by value); the running statistics
within 1e-6 of their term sum.  The framework's own 16-bit forward (MIOpen) is run on the same inputs and its figures are printed
beside ours: recorded, not asserted.

Trainer loss (measured on an MI355X, 4 steps of the small ResNet-18 trainer under bf16 autocast, against the fp32 trainer on the
same batches): see DESIGN.md section 12f.
"""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from tests import bn_bwd16_contract as KB
from tests import bn_fwd16_contract as K
from tests import bn_fwd_contract as K32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5
BF16, F16 = torch.bfloat16, torch.float16
DTYPES = [BF16, F16]
_ids = lambda s: "x".join(map(str, s))
_dt = lambda d: "bf16" if d is BF16 else "fp16"

# the smallest shapes at which each path can go wrong (a lane owns 8 channels, a block 16 column vectors = 128 channels)
SHAPES = [(2, 8, 1, 1),            # M = 2
          (3, 24, 5, 5),           # 3 column vectors, a partial block
          (2, 136, 7, 9),          # 17 column vectors: a second, ragged column block
          (4, 64, 28, 28),         # 256 % (C / 8) == 0: no refetch of the constants
          (5, 40, 33, 31),         # the refetch arm, several row chunks, a ragged last chunk and a partial last norm block
          (9, 512, 7, 7)]          # wide C
# one case just above each size threshold of the launcher (csrc/bn_bwd.hip: kBnBigElems = 20 Mi elements for the occupancy of
# the normalisation, kBnFwd16ReduceNtElems = kBnFwd16NormNtElems = 112 Mi for the cache policy): the smallest [1, 64, H, W] there
THRESHOLD_SHAPES = [(1, 64, 640, 512), (1, 64, 1792, 1024)]


@pytest.fixture(autouse=True)
def _deterministic_miopen():
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = det


def _code(dtype):
    from mhaq_amd import _lib
    return _lib.DT_BF16 if dtype is BF16 else _lib.DT_F16


def _cl(x_rows, shape):
    """[M, C] rows -> the channels_last [N, C, H, W] tensor on the device with those rows."""
    n, c, h, w = shape
    if h == 1 and w == 1:
        # NCHW and NHWC are one memory order here.  The tensor carries torch's default strides (C, 1, 1, 1), as the 16-bit
        # backward suite hands this shape to the framework: with (C, 1, C, C) the framework's own 16-bit forward, which these
        # tests run beside ours, ended in a host segmentation fault.  The HIP entry point reads the memory, not the strides.
        return x_rows.reshape(n, c, 1, 1).to(DEV)
    return x_rows.reshape(n, h, w, c).to(DEV).permute(0, 3, 1, 2)


def _inputs(shape, dtype, kind="plain", seed=0):
    n, c, h, w = shape
    x, gamma, beta = K.planted(kind, n * h * w, c, dtype, seed)
    g = torch.Generator().manual_seed(seed + 100)
    rm, rv = torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5
    x = _cl(x, shape)
    assert x.dtype == dtype and x.is_contiguous(memory_format=torch.channels_last)
    return x, gamma.to(DEV), beta.to(DEV), rm.to(DEV), rv.to(DEV)


def _hip_forward(x, gamma, beta, rm=None, rv=None, f=0.1, eps=EPS, want_y=True):
    """One call of the C ABI on copies of the running statistics: dict(y, mean, invstd, rm, rv, ws)."""
    from mhaq_amd import _lib
    L = _lib.lib()
    c = x.shape[1]
    m = x.numel() // c
    nb = L.mhaq_fq_bn_fwd_x16_workspace_bytes(m, c)
    assert nb > 0
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    y = torch.empty_like(x) if want_y else None
    mean, invstd = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
    rm, rv = (None, None) if rm is None else (rm.clone(), rv.clone())
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    rc = L.mhaq_fq_bn_fwd_x16(p(x), p(gamma), p(beta), p(y), p(mean), p(invstd), p(rm), p(rv), f, eps, m, c, _code(x.dtype),
                              p(ws), nb, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    return dict(y=y, mean=mean, invstd=invstd, rm=rm, rv=rv, ws=ws)


def _rowsed(out):
    return dict(out, y=None if out["y"] is None else K.rows(out["y"]))


def _bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def _same(a, b, keys=("y", "mean", "invstd", "rm", "rv", "ws")):
    for k in keys:
        if a[k] is None or b[k] is None:
            assert a[k] is b[k], k
        else:
            assert a[k].dtype == b[k].dtype and torch.equal(_bits(a[k]), _bits(b[k])), k
    return True


def _stock(x, gamma, beta, rm, rv, f=0.1, eps=EPS):
    rm, rv = rm.clone(), rv.clone()
    out = torch.ops.aten._batch_norm_impl_index(x, gamma, beta, rm, rv, True, f, eps, True)
    return dict(y=out[0], mean=out[1], invstd=out[2], rm=rm, rv=rv)


def _record_stock(x, gamma, beta, rm, rv, f, eps, cf, label):
    """The framework's own 16-bit forward in the checker's units: printed, never asserted."""
    old = _stock(x, gamma, beta, rm, rv, f, eps)
    ok = ~cf["bad"]
    if not bool(ok.any()):
        return
    g = K.rows(old["y"])
    e = ((g.double() - cf["y"]).abs() - KB.spacing16(g) / 2) / cf["T"].clamp_min(1e-300)
    e = e[:, ok]
    fy = float(e[torch.isfinite(e)].max()) if bool(torch.isfinite(e).any()) else 0.0
    rel = lambda a, r: float(((a.double() - r).abs()[ok] / r.abs()[ok].clamp_min(1e-300)).max())
    print(f"{label}: miopen  y {fy:.3e} T beyond the rounding  mean {rel(old['mean'].float(), cf['mean']):.3e}  "
          f"invstd {rel(old['invstd'].float(), cf['invstd']):.3e}")


def _check(x, gamma, beta, rm, rv, label, f=0.1, eps=EPS, cap=True, got=None):
    cf = K.closed_form(K.rows(x), gamma, beta, eps, rm, rv, f)
    got = got if got is not None else _hip_forward(x, gamma, beta, rm, rv, f, eps)
    _record_stock(x, gamma, beta, rm, rv, f, eps, cf, label)
    fig = K.check_all(_rowsed(got), cf, x.dtype, cap=cap)
    print(f"{label}: new     " + "  ".join(f"{k} {v:.3e}" for k, v in fig.items()))
    return got, cf


# ------------------------------------------------------------------------------------------------ the C ABI
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_c_abi_against_the_fp64_closed_form(shape, dtype):
    x, gamma, beta, rm, rv = _inputs(shape, dtype)
    m = x.numel() // shape[1]
    got, _ = _check(x, gamma, beta, rm, rv, f"{shape} {_dt(dtype)}", cap=K.capped("plain", m))
    assert got["y"].dtype == dtype and got["mean"].dtype == torch.float32
    # two calls: equal bits in y, the statistics and every byte of the workspace
    assert _same(got, _hip_forward(x, gamma, beta, rm, rv))
    # weight NULL = 1, bias NULL = 0; no running statistics and no y change nothing else
    assert _same(_hip_forward(x, None, beta, rm, rv), _hip_forward(x, torch.ones_like(gamma), beta, rm, rv))
    assert _same(_hip_forward(x, gamma, None, rm, rv), _hip_forward(x, gamma, torch.zeros_like(beta), rm, rv))
    assert _same(_hip_forward(x, gamma, beta), got, keys=("y", "mean", "invstd", "ws"))
    stats = _hip_forward(x, gamma, beta, rm, rv, want_y=False)
    assert stats["y"] is None and _same(stats, got, keys=("mean", "invstd", "rm", "rv", "ws"))


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("shape", THRESHOLD_SHAPES, ids=_ids)
def test_just_above_each_size_threshold(shape, dtype):
    """The statistics in full (fp64 sums in row blocks), y on a strided sample of the rows and on the last rows."""
    n, c, h, w = shape
    m = n * h * w
    assert m * c in (20 << 20, 112 << 20)
    gen = torch.Generator(device=DEV).manual_seed(3)
    x = torch.empty((m, c), dtype=dtype, device=DEV)
    scale = 0.5 + 3 * torch.rand(c, device=DEV, generator=gen)
    shift = 2 * torch.randn(c, device=DEV, generator=gen)
    step = 1 << 18
    for r in range(0, m, step):
        k = min(step, m - r)
        x[r:r + k] = (torch.randn((k, c), device=DEV, generator=gen) * scale + shift).to(dtype)
    gamma, beta = torch.randn(c, device=DEV, generator=gen), torch.randn(c, device=DEV, generator=gen)
    rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
    x4 = x.view(n, h, w, c).permute(0, 3, 1, 2)                      # channels_last [N, C, H, W] over the same memory
    assert x4.is_contiguous(memory_format=torch.channels_last)
    got = _hip_forward(x4, gamma, beta, rm, rv)
    s1 = torch.zeros(c, dtype=torch.float64, device=DEV)
    xmax = torch.zeros(c, dtype=torch.float64, device=DEV)
    for r in range(0, m, step):
        X = x[r:r + step].double()
        s1 += X.sum(0)
        xmax = torch.maximum(xmax, X.abs().amax(0))
    mean = s1 / m
    s2 = torch.zeros_like(s1)
    for r in range(0, m, step):
        s2 += (x[r:r + step].double() - mean).square().sum(0)
    var = s2 / m
    invstd = (var + EPS) ** -0.5
    bad = torch.zeros(c, dtype=torch.bool, device=DEV)
    f_m = K32.check_stat(got["mean"], mean, bad, "save_mean", xmax)
    f_i = K32.check_stat(got["invstd"], invstd, bad, "save_invstd")
    unb = var * m / (m - 1)
    K32.check_running(got["rm"], 0.9 * rm.double() + 0.1 * mean, 0.9 * rm.double().abs() + 0.1 * mean.abs(), bad, "running_mean")
    K32.check_running(got["rv"], 0.9 * rv.double() + 0.1 * unb, 0.9 * rv.double().abs() + 0.1 * unb.abs(), bad, "running_var")
    pick = torch.cat([torch.arange(0, m, 997, device=DEV), torch.arange(m - 600, m, device=DEV)]).unique()
    X = x[pick].double()
    ga, be = gamma.double(), beta.double()
    fig = KB.check_dx16(K.rows(got["y"])[pick], (X - mean) * invstd * ga + be, (X.abs() + mean.abs()) * invstd * ga.abs() + be.abs(),
                        dtype)
    print(f"{shape} {_dt(dtype)}: y {fig['err']:.3e} (excluded {fig['excluded']:.4f}, {pick.numel()} rows)  mean {f_m:.3e}  "
          f"invstd {f_i:.3e}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("eps", [1e-5, 1e-3])
@pytest.mark.parametrize("kind", ["constant_channel", "tiny_sigma", "far_mean", "spread", "outlier", "gamma_sign"])
@pytest.mark.parametrize("shape", [(3, 24, 5, 5), (5, 40, 33, 31)], ids=_ids)
def test_planted_cases(shape, kind, eps, dtype):
    x, gamma, beta, rm, rv = _inputs(shape, dtype, kind, seed=5)
    c, m = shape[1], x.numel() // shape[1]
    got, cf = _check(x, gamma, beta, rm, rv, f"{shape} {kind} eps={eps} {_dt(dtype)}", eps=eps, cap=K.capped(kind, m))
    is0 = float(torch.tensor(eps, dtype=torch.float64).rsqrt().float())
    if kind == "constant_channel":
        for ch, val in ((1, 3.0), (c - 1, 0.0)):
            assert float(got["mean"][ch]) == val                                     # the constant exactly
            assert float(got["invstd"][ch]) == is0                                   # var == 0
            assert torch.equal(_bits(K.rows(got["y"])[:, ch]), _bits(beta[ch].to(dtype).expand(m)))      # R16(beta) bit for bit
            assert float(got["rv"][ch]) == float((0.9 * rv[ch].double()).float())    # ... and adds 0 to the running variance
    if kind == "tiny_sigma":                 # every element rounds to 100: the mean by value, var = 0
        assert bool((got["mean"] == 100.0).all()) and bool((got["invstd"] == is0).all())
        assert torch.equal(_bits(K.rows(got["y"])), _bits(beta.to(dtype).expand(m, c)))
    if kind == "far_mean":                   # one or two 16-bit values per channel: the statistics of exactly those
        X = K.rows(x).float()
        const = (X == X[0]).all(0)
        assert bool((got["mean"][const] == X[0][const]).all()) and bool((got["invstd"][const] == is0).all())
    if kind == "gamma_sign":
        for ch in (0, 2):                    # gamma = 0 and -0
            assert bool((K.rows(got["y"])[:, ch] == beta[ch].to(dtype)).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("f", [0.1, 1.0, 0.0, 1.0 / 3], ids=lambda f: f"f={f:.3g}")
def test_running_statistics_follow_the_factor(f, dtype):
    x, gamma, beta, rm, rv = _inputs((3, 24, 5, 5), dtype, seed=7)
    got, _ = _check(x, gamma, beta, rm, rv, f"f={f} {_dt(dtype)}", f=f)
    if f == 0.0:
        assert torch.equal(got["rm"], rm) and torch.equal(got["rv"], rv)
    # M = 2: the unbiased factor M / (M - 1) = 2
    x, gamma, beta, rm, rv = _inputs((2, 8, 1, 1), dtype, seed=7)
    _check(x, gamma, beta, rm, rv, f"M=2 f={f} {_dt(dtype)}", f=f, cap=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_a_nan_and_an_infinity_poison_their_own_channels_only(dtype):
    x, gamma, beta, rm, rv = _inputs((3, 24, 5, 5), dtype, seed=8)
    clean = _hip_forward(x, gamma, beta, rm, rv)
    # one NaN; then a NaN, an infinity, and an infinity in row 0 (the shift of its channel) in three channels
    for plant in ({(1, 6, 2, 3): float("nan")},
                  {(1, 6, 2, 3): float("nan"), (2, 9, 4, 1): float("inf"), (0, 13, 0, 0): float("-inf")}):
        x2 = x.clone()
        for at, v in plant.items():
            x2[at] = v
        bad = sorted(at[1] for at in plant)
        others = [c for c in range(24) if c not in bad]
        got, cf = _check(x2, gamma, beta, rm, rv, f"non-finite in channels {bad} {_dt(dtype)}")
        assert cf["bad"].nonzero().flatten().tolist() == bad
        for ch in bad:
            assert bool(torch.isnan(got["y"][:, ch]).all()) and not bool(torch.isfinite(got["mean"][ch]))
            assert bool(torch.isnan(got["invstd"][ch])) and not bool(torch.isfinite(got["rv"][ch]))
        for k in ("mean", "invstd", "rm", "rv"):
            assert torch.equal(got[k][others], clean[k][others]), k
        assert torch.equal(_bits(got["y"][:, others]), _bits(clean["y"][:, others]))


def test_fp16_overflow_of_y_gives_infinities():
    x, gamma, beta, rm, rv = _inputs((3, 24, 5, 5), F16, seed=9)
    gamma = torch.where(torch.arange(24, device=DEV) % 2 == 0, 6e4, -6e4) * (1 + torch.rand(24, device=DEV))
    got, cf = _check(x, gamma, beta, rm, rv, "fp16 overflow", cap=False)
    y = K.rows(got["y"]).float()
    over = cf["y"].abs() > 65520
    assert int(over.sum()) > 50 and bool(torch.isinf(y[over]).all()) and bool((torch.sign(y[over]) == torch.sign(cf["y"][over])).all())
    assert bool((y == float("inf")).any()) and bool((y == float("-inf")).any()) and not bool(torch.isnan(y).any())
    assert bool(torch.isfinite(got["mean"]).all()) and bool(torch.isfinite(got["invstd"]).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_argument_errors_leave_the_outputs_untouched(dtype):
    from mhaq_amd import _lib
    L = _lib.lib()
    x, gamma, beta, rm, rv = _inputs((2, 64, 3, 3), dtype)
    m, c = 18, 64
    nb = L.mhaq_fq_bn_fwd_x16_workspace_bytes(m, c)
    sent = 0x5A
    ws = torch.full((nb + 16,), sent, dtype=torch.uint8, device=DEV)
    y = torch.full((x.numel() * 2 + 16,), sent, dtype=torch.uint8, device=DEV)
    outs = torch.full((4, c * 4 + 16), sent, dtype=torch.uint8, device=DEV)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    args = [p(x), p(gamma), p(beta), p(y), p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]), 0.1, EPS, m, c, _code(dtype), p(ws),
            nb, None]
    assert L.mhaq_fq_bn_fwd_x16_workspace_bytes(m, c) > 0
    for k, off in ((0, 8), (3, 4), (13, 8), (1, 2), (4, 2), (7, 1)):
        bad = list(args)
        bad[k] = ctypes.c_void_p(args[k].value + off)
        assert L.mhaq_fq_bn_fwd_x16(*bad) == -3, k
    for k, v, rc in ((14, nb - 1, -2), (10, 1, -4), (11, 60, -4), (7, None, -1), (12, 0, -1), (12, 3, -1), (0, None, -1)):
        bad = list(args)
        bad[k] = v
        assert L.mhaq_fq_bn_fwd_x16(*bad) == rc, (k, v)
    torch.cuda.synchronize()
    assert all(bool((t == sent).all()) for t in (ws, y, outs))


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("shape", [(3, 24, 5, 5), (5, 40, 33, 31), (9, 512, 7, 7)], ids=_ids)
def test_sentinel_guards_around_every_output_and_the_workspace(shape, dtype):
    from mhaq_amd import _lib
    L = _lib.lib()
    x, gamma, beta, rm, rv = _inputs(shape, dtype)
    c = shape[1]
    m = x.numel() // c
    nb = L.mhaq_fq_bn_fwd_x16_workspace_bytes(m, c)
    guard, sent = 4096, 0x5A
    wsbuf = torch.full((nb + 2 * guard,), sent, dtype=torch.uint8, device=DEV)
    ybuf = torch.full((x.numel() * 2 + 2 * guard,), sent, dtype=torch.uint8, device=DEV)
    out = torch.full((4, c * 4 + 128), sent, dtype=torch.uint8, device=DEV)          # 64 guard bytes around each [c] vector
    out[2, 64:64 + c * 4] = rm.view(torch.uint8)
    out[3, 64:64 + c * 4] = rv.view(torch.uint8)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    rc = L.mhaq_fq_bn_fwd_x16(p(x), p(gamma), p(beta), p(ybuf, guard), p(out[0], 64), p(out[1], 64), p(out[2], 64), p(out[3], 64),
                              0.1, EPS, m, c, _code(dtype), p(wsbuf, guard), nb,
                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    for buf, body in ((wsbuf, nb), (ybuf, x.numel() * 2)):
        assert bool((buf[:guard] == sent).all()) and bool((buf[guard + body:] == sent).all())
    assert bool((out[:, :64] == sent).all()) and bool((out[:, 64 + c * 4:] == sent).all())
    ref = _hip_forward(x, gamma, beta, rm, rv)
    assert torch.equal(ybuf[guard:guard + x.numel() * 2], _bits(K.rows(ref["y"])))
    for i, k in enumerate(("mean", "invstd", "rm", "rv")):
        assert torch.equal(out[i, 64:64 + c * 4].contiguous().view(torch.float32), ref[k]), k
    # the workspace of a fresh call starts from zeros, this one from the sentinel: every byte is written
    assert torch.equal(wsbuf[guard:guard + nb], ref["ws"])


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_ops_wrapper_is_the_c_abi_call_and_never_falls_back(dtype):
    from mhaq_amd import _lib, ops
    x, gamma, beta, rm, rv = _inputs((3, 24, 5, 5), dtype, seed=12)
    ref = _hip_forward(x, gamma, beta, rm, rv)
    rm2, rv2 = rm.clone(), rv.clone()
    y, mean, invstd = ops.bn_forward_train_x16(x, gamma, beta, rm2, rv2, 0.1, EPS)
    assert _same(dict(y=y, mean=mean, invstd=invstd, rm=rm2, rv=rv2), ref, keys=("y", "mean", "invstd", "rm", "rv"))
    y, mean, invstd = ops.bn_forward_train_x16(x)
    assert _same(dict(y=y, mean=mean, invstd=invstd), _hip_forward(x, None, None), keys=("y", "mean", "invstd"))
    with pytest.raises(_lib.MhaqFqError):                       # C % 8 != 0: an error, not another implementation
        ops.bn_forward_train_x16(_inputs((2, 12, 4, 4), dtype)[0])
    with pytest.raises(TypeError):
        ops.bn_forward_train_x16(x.float())


# ------------------------------------------------------------------------------------------------ node and module
def _E():
    from mhaq_amd import _ext
    return _ext.ext()


def _counts():
    E = _E()
    return dict(f32=E.bn_hip_forwards(), f16=E.bn_hip_forwards_x16(), b32=E.bn_hip_backwards(), b16=E.bn_hip_backwards_x16())


def _moved(before, **by):
    now = _counts()
    return all(now[k] == before[k] + by.get(k, 0) for k in now)


def _pair(c, x16=True, hip_forward_x16=True, **kw):
    from mhaq_amd import bn_backward
    torch.manual_seed(4)
    stock = nn.BatchNorm2d(c, **kw).to(DEV)
    with torch.no_grad():
        stock.weight.uniform_(-1.5, 1.5)
        stock.bias.uniform_(-1, 1)
        stock.running_mean.uniform_(-1, 1)
        stock.running_var.uniform_(0.5, 1.5)
    mine = copy.deepcopy(stock)
    assert bn_backward.install(mine, x16=x16, hip_forward=True, hip_forward_x16=hip_forward_x16) == 1
    return stock, mine


def _step(bn, x, g):
    x = x.clone().requires_grad_(True)
    for p in bn.parameters():
        p.grad = None
    y = bn(x)
    y.backward(g)
    own = lambda t: None if t is None else t.clone()
    return dict(y=y.detach(), dx=x.grad, dw=own(bn.weight.grad), db=own(bn.bias.grad), rm=bn.running_mean.clone(),
                rv=bn.running_var.clone(), nbt=bn.num_batches_tracked.clone())


def _dy(shape, dtype, seed=11):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(dtype).to(DEV).contiguous(memory_format=torch.channels_last)


def _same_step(a, b):
    for k in a:
        assert (a[k] is None and b[k] is None) or (a[k].dtype == b[k].dtype and torch.equal(_bits(a[k]), _bits(b[k]))), k
    return True


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_module_with_the_three_flags_holds_the_contract_and_feeds_the_16_bit_backward(shape, dtype):
    x = _inputs(shape, dtype, seed=2)[0]
    dy = _dy(shape, dtype)
    stock, mine = _pair(shape[1])
    assert mine.takes_x16() and mine.takes_hip_forward_x16()
    rm, rv = mine.running_mean.clone(), mine.running_var.clone()
    v0 = mine.running_mean._version
    n0 = _counts()
    got = _step(mine, x, dy)
    assert _moved(n0, f16=1, b16=1)                              # the 16-bit routes, never a silent fallback, not the fp32 ones
    assert mine.running_mean._version > v0                       # the in-place update is visible
    assert got["y"].dtype == dtype and got["dx"].dtype == dtype and got["dw"].dtype == torch.float32
    gamma, beta = mine.weight.detach(), mine.bias.detach()
    direct = _hip_forward(x, gamma, beta, rm, rv)
    assert torch.equal(_bits(got["y"]), _bits(direct["y"])) and torch.equal(got["rm"], direct["rm"]) and torch.equal(got["rv"], direct["rv"])
    m = x.numel() // shape[1]
    K.check_all(_rowsed(dict(direct, y=got["y"])), K.closed_form(K.rows(x), gamma, beta, EPS, rm, rv, 0.1), dtype,
                cap=K.capped("plain", m))
    # the backward from the statistics the HIP forward saved, by the 16-bit backward's own checks
    cf = KB.closed_form(x, dy, gamma, direct["mean"], direct["invstd"])
    fig = KB.check_dx16(K.rows(got["dx"]), cf["dx"], cf["dx_abs"], dtype, cap=m >= 9)
    f_g = KB.check_sums(got["dw"], cf["dg"], cf["dg_abs"], "dgamma")
    f_b = KB.check_sums(got["db"], cf["db"], cf["db_abs"], "dbeta")
    print(f"module {shape} {_dt(dtype)}: dx {fig['err']:.3e} (excluded {fig['excluded']:.4f})  dgamma {f_g:.3e}  dbeta {f_b:.3e}")
    # the bookkeeping is the stock module's
    old = _step(stock, x, dy)
    assert torch.equal(got["nbt"], old["nbt"]) and int(got["nbt"]) == 1


@pytest.mark.parametrize("case", ["flag_off", "x16_off", "nchw", "c_not_multiple_of_8", "eval", "fp32_input"])
def test_fallbacks_equal_the_frameworks_forward_bit_for_bit(case):
    shape = (2, 12, 4, 4) if case == "c_not_multiple_of_8" else (3, 24, 5, 5)
    x, dy = _inputs(shape, BF16, seed=3)[0], _dy(shape, BF16)
    if case == "nchw":
        x, dy = x.contiguous(), dy.contiguous()
    stock, mine = _pair(shape[1], x16=case != "x16_off", hip_forward_x16=case != "flag_off")
    if case == "eval":
        stock, mine = stock.eval(), mine.eval()
    n0 = _counts()
    if case == "fp32_input":                                    # the 16-bit flags do not move an fp32 input (hip_forward does)
        from mhaq_amd import bn_backward
        bn_backward.uninstall(mine)
        assert bn_backward.install(mine, x16=True, hip_forward_x16=True) == 1
        x, dy = x.float(), dy.float()
    a, b = _step(stock, x, dy), _step(mine, x, dy)
    for k in ("y", "rm", "rv", "nbt"):
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
    now = _counts()
    assert now["f16"] == n0["f16"] and now["f32"] == n0["f32"]
    if case in ("x16_off", "eval", "nchw", "c_not_multiple_of_8"):      # the framework's backward as well
        assert _same_step(a, b) and now == n0
    # the node itself, called with the flags of the case
    E = _E()
    flags = dict(x16=case != "x16_off", hip_forward=True, hip_forward_x16=case != "flag_off")
    rm, rv = torch.zeros(shape[1], device=DEV), torch.ones(shape[1], device=DEV)
    if case not in ("eval", "fp32_input"):
        y = E.bn_train(x, stock.weight, stock.bias, rm, rv, 0.1, EPS, True, **flags)
        ref = _stock(x, stock.weight.detach(), stock.bias.detach(), torch.zeros_like(rm), torch.ones_like(rv))
        assert torch.equal(_bits(y.detach()), _bits(ref["y"])) and torch.equal(rm, ref["rm"]) and torch.equal(rv, ref["rv"])
        assert E.bn_hip_forwards_x16() == n0["f16"] and E.bn_hip_forwards() == n0["f32"]


def test_one_row_falls_back_to_the_frameworks_forward():
    """N * H * W = 1 has no unbiased variance: the node hands the call to the framework, whatever that does with it."""
    E = _E()
    x = torch.randn(1, 8, 1, 1, device=DEV).to(BF16).contiguous(memory_format=torch.channels_last)
    w, b = torch.rand(8, device=DEV) + 0.5, torch.randn(8, device=DEV)
    outs = []
    n0 = _counts()
    for fn in (lambda rm, rv: torch.ops.aten._batch_norm_impl_index(x, w, b, rm, rv, True, 0.1, EPS, True)[0],
               lambda rm, rv: E.bn_train(x, w, b, rm, rv, 0.1, EPS, True, x16=True, hip_forward=True, hip_forward_x16=True)):
        rm, rv = torch.zeros(8, device=DEV), torch.ones(8, device=DEV)
        try:
            outs.append((fn(rm, rv).detach(), rm, rv))
        except RuntimeError as e:
            outs.append(type(e))
    assert _counts() == n0
    if isinstance(outs[0], tuple):
        assert isinstance(outs[1], tuple) and all(torch.equal(_bits(p), _bits(q)) for p, q in zip(*outs))
    else:
        assert outs[1] is outs[0]


@pytest.mark.parametrize("momentum", [0.1, None])
def test_bookkeeping_equals_the_stock_modules(momentum):
    """num_batches_tracked counts alike, and momentum=None hands the kernels the cumulative factor 1 / n."""
    shape = (3, 24, 5, 5)
    stock, mine = _pair(24, momentum=momentum)
    rm, rv = mine.running_mean.clone(), mine.running_var.clone()
    for i in range(3):
        x, dy = _inputs(shape, BF16, seed=20 + i)[0], _dy(shape, BF16, seed=30 + i)
        a, b = _step(stock, x, dy), _step(mine, x, dy)
        assert torch.equal(a["nbt"], b["nbt"]) and int(b["nbt"]) == i + 1
        f = 1.0 / (i + 1) if momentum is None else momentum
        cf = K.closed_form(K.rows(x), None, None, EPS, rm, rv, f, want_y=False)
        K32.check_running(b["rm"], cf["rm"], cf["rm_abs"], cf["bad"], "running_mean")
        K32.check_running(b["rv"], cf["rv"], cf["rv_abs"], cf["bad"], "running_var")
        rm, rv = b["rm"], b["rv"]
    mine.eval()                                                  # eval mode: the stock forward, from the HIP running statistics
    n0 = _counts()
    ye = mine(x)
    assert _counts() == n0
    assert torch.equal(_bits(ye), _bits(F.batch_norm(x, mine.running_mean, mine.running_var, mine.weight, mine.bias, False, 0.0, EPS)))


def test_a_side_stream_gives_the_default_streams_bits():
    shape = (4, 64, 28, 28)
    x, dy = _inputs(shape, BF16, seed=6)[0], _dy(shape, BF16)
    _, mine = _pair(64)
    other = copy.deepcopy(mine)
    ref = _step(mine, x, dy)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    n0 = _counts()
    with torch.cuda.stream(side):
        got = _step(other, x, dy)
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert _moved(n0, f16=1, b16=1) and _same_step(ref, got)


def test_forward_and_backward_in_a_captured_graph_replay_like_eager():
    shape = (4, 64, 28, 28)
    x, dy = _inputs(shape, BF16, seed=6)[0], _dy(shape, BF16)
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
    assert _moved(n0, f16=1, b16=1)
    mine.load_state_dict(state)
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        e = eager[k]
        assert torch.equal(_bits(ys), _bits(e["y"])) and torch.equal(_bits(xs.grad), _bits(e["dx"]))
        assert torch.equal(mine.weight.grad, e["dw"]) and torch.equal(mine.bias.grad, e["db"])
        assert torch.equal(mine.running_mean, e["rm"]) and torch.equal(mine.running_var, e["rv"])


# ------------------------------------------------------------------------------------------------ the trainer
STEPS = 4


def _trainer(autocast=True, capture=False, more=None, **cfg_kw):
    import mhaq_amd as M
    from mhaq_amd import nets, ops
    from mhaq_amd.qat import QATConfig, QATTrainer
    torch.manual_seed(3)
    ops.manual_seed(3)
    net = nets.resnet18(10).to(memory_format=torch.channels_last)
    g = torch.Generator().manual_seed(2)
    calib = torch.randn(4, 3, 64, 64, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    if autocast:
        cfg_kw = dict(cfg_kw, autocast_dtype=BF16)
    cfg = QATConfig(qscheme=M.QScheme.PER_CHANNEL, qnmethod=M.QNMethod.LSQ, distillation=True, warmup=2,
                    learning_rate=1e-3, **cfg_kw)
    return QATTrainer(net, cfg, DEV, calib_batches=[calib], distributed=False, capture_graph=capture, **(more or {}))


def _batches(n):
    gen = torch.Generator().manual_seed(9)
    return [(torch.randn(4, 3, 64, 64, generator=gen).to(DEV).contiguous(memory_format=torch.channels_last),
             torch.randint(0, 10, (4,), generator=gen).to(DEV)) for _ in range(n)]


def _run(tr, batches):
    losses = [float(tr.train_step(x, y)) for x, y in batches]
    return losses, [p.detach().clone() for p in tr.net.parameters()]


def _flags(tr):
    return [(m.takes_x16(), m.takes_hip_forward_x16()) for m in tr.net.modules() if hasattr(m, "takes_hip_forward_x16")]


_ENVS = ("ENV_SWITCH", "ENV_SWITCH_X16", "ENV_SWITCH_FORWARD", "ENV_SWITCH_FORWARD_X16")
_runs = {}


def _shared(name, monkeypatch, **kw):
    """One run per configuration for the whole module, with the four BatchNorm variables unset: (losses, parameters,
    16-bit HIP forwards during the run, the per-module flags)."""
    from mhaq_amd import bn_backward
    for v in _ENVS:
        monkeypatch.delenv(getattr(bn_backward, v), raising=False)
    if name not in _runs:
        tr = _trainer(**kw)
        n0 = _counts()
        losses, params = _run(tr, _batches(STEPS))
        now = _counts()
        _runs[name] = (losses, params, {k: now[k] - n0[k] for k in now}, _flags(tr))
    return _runs[name]


def test_trainer_runs_every_student_batchnorm_forward_on_the_16_bit_kernels(monkeypatch):
    from mhaq_amd import bn_backward, fused_blocks
    losses, params, moved, flags = _shared("both", monkeypatch, hip_bn_backward_16bit=True, hip_bn_forward_16bit=True)
    assert len(flags) == 20 and all(a and b for a, b in flags)
    # every student BatchNorm, the stem's included (the unpooled node: a 16-bit stem stays maxpool(bn(c))), every step
    assert moved == dict(f32=0, f16=20 * STEPS, b32=0, b16=20 * STEPS)
    assert all(v == v and abs(v) != float("inf") for v in losses), losses
    tr = _trainer(hip_bn_backward_16bit=True, hip_bn_forward_16bit=True, capture=True)
    assert type(tr.net) is fused_blocks.FusedResNet18
    assert not any(hasattr(m, "takes_hip_forward_x16") for m in tr.teacher.modules())
    graphed = _run(tr, _batches(STEPS))
    assert losses == graphed[0] and all(torch.equal(a, b) for a, b in zip(params, graphed[1]))


def test_trainer_switch_off_is_the_trainer_without_the_argument(monkeypatch):
    from mhaq_amd import bn_backward
    from oracle.ref_layers import ORACLE_LAYERS
    base = _shared("x16", monkeypatch, hip_bn_backward_16bit=True)
    assert base[2]["f16"] == 0 and base[2]["b16"] == 20 * STEPS and all(a and not b for a, b in base[3])
    n0 = _counts()
    off = _run(_trainer(hip_bn_backward_16bit=True, hip_bn_forward_16bit=False), _batches(STEPS))
    assert base[0] == off[0] and all(torch.equal(a, b) for a, b in zip(base[1], off[1]))
    # the environment decides when it is set, either way; checker trainers are spared
    monkeypatch.setenv(bn_backward.ENV_SWITCH_FORWARD_X16, "0")
    assert not any(b for _, b in _flags(_trainer(hip_bn_backward_16bit=True, hip_bn_forward_16bit=True)))
    monkeypatch.setenv(bn_backward.ENV_SWITCH_FORWARD_X16, "1")
    assert all(a and b for a, b in _flags(_trainer(hip_bn_backward_16bit=True)))
    assert _counts()["f16"] == n0["f16"]
    tr = _trainer(hip_bn_backward_16bit=True, hip_bn_forward_16bit=True, more=dict(layers=ORACLE_LAYERS))
    assert _flags(tr) == []


def test_trainer_with_only_the_forward_switch_changes_nothing(monkeypatch):
    default = _shared("default", monkeypatch)
    only = _shared("forward_only", monkeypatch, hip_bn_forward_16bit=True)
    assert only[2] == dict(f32=0, f16=0, b32=0, b16=0) and default[2] == only[2]
    assert len(only[3]) == 20 and all(b and not a for a, b in only[3])            # the flag is set; nothing takes it
    assert default[0] == only[0] and all(torch.equal(a, b) for a, b in zip(default[1], only[1]))


def test_trainer_loss_stays_as_near_the_fp32_trainers_as_the_default_bf16_run(monkeypatch):
    """At every step the loss is no farther from the fp32 trainer's on the same batches than twice the largest distance of the
    default bf16 trainer from it, plus 2e-3: both bf16 runs are one-rounding-per-tensor perturbations of the same step, and
    2e-3 is the trajectory tolerance of DESIGN.md section 2."""
    fp32 = _shared("fp32", monkeypatch, autocast=False)[0]
    default = _shared("default", monkeypatch)[0]
    new = _shared("both", monkeypatch, hip_bn_backward_16bit=True, hip_bn_forward_16bit=True)[0]
    d_default = [abs(a - b) for a, b in zip(default, fp32)]
    d_new = [abs(a - b) for a, b in zip(new, fp32)]
    for i in range(STEPS):
        print(f"step {i}: fp32 {fp32[i]:.9g}  default bf16 {default[i]:.9g} (off by {d_default[i]:.3e})  "
              f"16-bit HIP forward + backward {new[i]:.9g} (off by {d_new[i]:.3e})")
    bound = 2 * max(d_default) + 2e-3
    print(f"bound {bound:.3e}")
    assert all(v == v and abs(v) != float("inf") for v in new), new
    assert all(d <= bound for d in d_new), (d_new, bound)
