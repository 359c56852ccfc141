"""GPU (-m gpu): the stem's max pool and the gathering BatchNorm backward on 16-bit tensors (mhaq_fq_maxpool3s2_fwd_x16,
mhaq_fq_bn_pool_bwd_x16, csrc/bn_bwd.hip) through the C ABI.

Every comparison is BIT FOR BIT (int16 / int32 views: signed zeros and NaN payloads count), there are no tolerances.  The
yardsticks are torch's own max_pool2d forward / backward on the 16-bit tensor on the same device, and mhaq_fq_bn_bwd_x16 on the
16-bit dy that backward writes.  The rule by which torch rounds that dy is restated in _dy_from_codes and checked against
torch first (test_gather_restated_...): one covering window passes its g on unchanged (except on a 1 x 1 plane); two or four
are summed in fp32, in ascending oh then ow, from 0.0f, and rounded to 16 bits once by torch's own conversion.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5
BF16, F16 = torch.bfloat16, torch.float16
DTYPES = [BF16, F16]
_dt = lambda d: "bf16" if d is BF16 else "fp16"
ULP1 = {BF16: 2.0 ** -7, F16: 2.0 ** -10}              # the spacing of the format at 1.0

# the smallest shapes at which each part can go wrong (N, C, H, W): one window; even / odd edges; C / 8 = 3 (idle lanes in the
# reduction, a non-zero column step in dx); odd sizes, where some elements have no second window; several column chunks;
# several row chunks with a ragged last one (the stem's row length); and one case just above each size threshold of the
# launcher: 20 Mi elements (the dx kernel's occupancy form: 22.2 M) and 56 Mi (non-temporal loads of x: 59.2 M)
SHAPES = [(1, 8, 1, 1), (2, 8, 2, 3), (1, 8, 3, 3), (3, 24, 5, 7), (2, 64, 9, 9), (2, 8, 17, 15), (2, 512, 7, 7),
          (1, 64, 112, 112), (3, 64, 340, 340), (8, 64, 340, 340)]
_ids = lambda s: "x".join(map(str, s))


@pytest.fixture(autouse=True)
def _deterministic_miopen():
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = det


def _cl(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16) if t.dtype in DTYPES else t.view(torch.int32) if t.dtype == torch.float32 else t


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((_bits(a) == _bits(b)).all())


def _out(n):
    return (n - 1) // 2 + 1


def _code_of(dtype):
    from mhaq_amd import _lib
    return _lib.DT_BF16 if dtype is BF16 else _lib.DT_F16


def _rounding_plants(shape):
    """[(channel, ih, iw, [(oh, ow, value), ..])]: input elements made the strict maximum of every window that covers them (in
    every image), and the gradients of those windows, named relative to the format's ulp at 1.0.
      (odd, odd), four windows {1, e, e, e} with e = ulp / 4: the fp32 sum 1 + 3 e rounds ONCE to 1 + ulp; a 16-bit add
                  per term would give 1.  This is the pair that tells the two rounding rules apart.
      (odd, even), two windows {1, ulp / 2}: the tie, to even: 1.  And {1 + ulp, ulp / 2}: the tie the other way, 1 + 2 ulp.
    Values: "1", "e" = ulp / 4, "h" = ulp / 2, "1+u" = 1 + ulp, "nan" = a quiet NaN with a non-zero payload."""
    n, c, h, w = shape
    plants = []
    if h >= 3 and w >= 3:
        plants.append((4, 1, 1, [(0, 0, "1"), (0, 1, "e"), (1, 0, "e"), (1, 1, "e")]))
        plants.append((3, 1, 1, [(0, 0, "nan"), (1, 0, "1")]))      # a NaN with a payload in a sum: torch's cast decides its bits
        plants.append((6, 1, 2, [(0, 1, "1"), (1, 1, "h")]))
        plants.append((7, 1, 0, [(0, 0, "1+u"), (1, 0, "h")]))
    if h >= 5 and w >= 5:                               # a second (odd, odd) position, the large term LAST in the sum
        plants.append((5, 3, 3, [(1, 1, "e"), (1, 2, "e"), (2, 1, "e"), (2, 2, "1")]))
    if h >= 7 and w >= 7:
        plants.append((4, 5, 5, [(2, 2, "e"), (2, 3, "1"), (3, 2, "e"), (3, 3, "e")]))
    return plants


def _pool_input(shape, dtype, seed=0):
    """Integer-valued data in a small range (exact in both formats; ties in every window), with planted windows: all equal,
    all -inf, one holding +inf, one holding one NaN and one holding several, a whole -inf plane (each in its own channel),
    and the strict maxima of _rounding_plants in channels 4 .. 7 of every image."""
    n, c, h, w = shape
    gen = torch.Generator(device=DEV).manual_seed(seed)
    t = torch.randint(-3, 4, shape, generator=gen, device=DEV).float()
    if h >= 3 and w >= 3:
        a, b = (h - 3) // 2, (w - 3) // 2
        t[0, 0, a:a + 3, b:b + 3] = 2.0
        t[0, 1, a:a + 3, b:b + 3] = float("-inf")
        t[0, 2, a + 1, b + 1] = float("inf")
        t[0, 3, a + 1, b + 2] = float("nan")
        t[n - 1, 0, a, b] = float("nan")
        t[n - 1, 0, a + 2, b + 1] = float("nan")
        t[n - 1, 0, a + 1, b + 2] = float("nan")
        t[n - 1, 1, :, :] = float("-inf")               # a whole plane: no window chooses an element
    else:
        t[0, 1] = float("-inf")
        t[0, 2, 0, 0] = float("nan")
        t[0, 3] = 1.0
    for ch, ih, iw, _ in _rounding_plants(shape):
        t[:, ch, ih, iw] = 9.0
    return _cl(t.to(dtype))


def _pooled_grad(shape, dtype, seed=1):
    """The 16-bit pooled gradient [N, C, OH, OW]: small integers with +-0 among them; NaN and +-inf planted in channels 1 and
    2; the rounding-sensitive values of _rounding_plants."""
    n, c, h, w = shape
    gen = torch.Generator(device=DEV).manual_seed(seed)
    g = torch.randint(-2, 3, (n, c, _out(h), _out(w)), generator=gen, device=DEV).float()
    sign = torch.where(torch.rand(g.shape, generator=gen, device=DEV) < 0.5, -1.0, 1.0)
    g = torch.where(g == 0, g * sign, g)                # +-0
    g[0, 1, 0, 0] = float("nan")
    g[n - 1, 2, -1, -1] = float("inf")
    if _out(w) > 1:
        g[0, 2, 0, 1] = float("-inf")
    u = ULP1[dtype]
    val = {"1": 1.0, "e": u / 4, "h": u / 2, "1+u": 1.0 + u, "nan": float("nan")}
    for ch, _, _, wins in _rounding_plants(shape):
        for oh, ow, v in wins:
            g[:, ch, oh, ow] = val[v]
    out = g.to(dtype)
    assert bool(((out.float() == g) | g.isnan()).all())               # every planted value is exact in the format
    for ch, _, _, wins in _rounding_plants(shape):
        for oh, ow, v in wins:
            if v == "nan":
                out.view(torch.int16)[:, ch, oh, ow] = 0x7FC1 if dtype is BF16 else 0x7E01
    return _cl(out)


def _lib():
    from mhaq_amd import _lib
    return _lib.lib()


_p = lambda t, off=0: None if t is None else ctypes.c_void_p(t.data_ptr() + off)
_stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _hip_pool(t):
    n, c, h, w = t.shape
    p = torch.empty((n, c, _out(h), _out(w)), dtype=t.dtype, device=DEV).contiguous(memory_format=torch.channels_last)
    code = torch.empty((n, c, _out(h), _out(w)), dtype=torch.uint8, device=DEV).contiguous(memory_format=torch.channels_last)
    rc = _lib().mhaq_fq_maxpool3s2_fwd_x16(_p(t), _p(p), _p(code), n, h, w, c, _code_of(t.dtype), _stream())
    assert rc == 0, rc
    return p, code


def _dy_from_codes(g, code, h, w):
    """The test's own statement of the gather on a 16-bit g.  An input element covered by ONE window takes that window's g,
    its 16 bits unchanged, where the code names it and +0.0 where not.  One covered by two or four starts an fp32 sum at 0.0f
    and adds up(g) of every window whose code names it, in ascending oh, then ascending ow -- for a fixed input row that is
    DEscending kh (kh = ih - 2 oh + 1), likewise kw --, and the sum is rounded to the 16-bit type ONCE, by torch's cast.
    A 1 x 1 plane is NCHW and NHWC at once; torch takes its contiguous kernel there, which sums and rounds even the one
    window's g (-0.0 arrives as +0.0)."""
    n, c, oh, ow = g.shape
    acc = torch.zeros((n, c, h, w), device=g.device)                  # fp32
    passed = torch.zeros((n, c, h, w), device=g.device, dtype=g.dtype)
    r, s = torch.arange(oh, device=g.device), torch.arange(ow, device=g.device)
    ihs, iws = torch.arange(h, device=g.device), torch.arange(w, device=g.device)
    one_h = ~((ihs % 2 == 1) & (ihs // 2 + 1 < oh))                   # rows covered by one row of windows
    one_w = ~((iws % 2 == 1) & (iws // 2 + 1 < ow))
    single = one_h[:, None] & one_w[None, :]
    if h == 1 and w == 1:                                             # torch's contiguous kernel: every element is a rounded sum
        single = torch.zeros_like(single)
    for kh in (2, 1, 0):
        ih = 2 * r - 1 + kh
        vh = (ih >= 0) & (ih < h)
        for kw in (2, 1, 0):
            iw = 2 * s - 1 + kw
            vw = (iw >= 0) & (iw < w)
            if not bool(vh.any()) or not bool(vw.any()):
                continue
            rows, cols = ih[vh][:, None], iw[vw][None, :]
            gg = g[:, :, vh][:, :, :, vw]
            hit = code[:, :, vh][:, :, :, vw] == kh * 3 + kw
            old = acc[:, :, rows, cols]
            acc[:, :, rows, cols] = torch.where(hit, old + gg.float(), old)
            passed[:, :, rows, cols] = torch.where(hit, gg, passed[:, :, rows, cols])
    return torch.where(single, passed, acc.to(g.dtype)).contiguous(memory_format=torch.channels_last)


class _Case:
    """Everything the tests of one shape and dtype share, computed once: torch's pool forward and backward on the 16-bit
    tensors on the device, ours, the BatchNorm inputs, and mhaq_fq_bn_bwd_x16 on torch's dy."""

    def __init__(self, shape, dtype):
        n, c, h, w = shape
        self.shape, self.dtype, self.dt = shape, dtype, _code_of(dtype)
        self.t = _pool_input(shape, dtype)
        tt = self.t.clone().requires_grad_(True)
        self.p_torch, self.idx_torch = F.max_pool2d(tt, 3, 2, 1, return_indices=True)
        self.g = _pooled_grad(shape, dtype)
        self.dy_torch, = torch.autograd.grad(self.p_torch, tt, self.g)
        assert self.dy_torch.dtype == dtype and self.dy_torch.is_contiguous(memory_format=torch.channels_last)
        self.p_torch = self.p_torch.detach()
        self.p, self.code = _hip_pool(self.t)
        gen = torch.Generator(device=DEV).manual_seed(7)
        x = torch.randn(shape, generator=gen, device=DEV) * 2 + torch.randn((1, c, 1, 1), generator=gen, device=DEV)
        self.x = _cl(x.to(dtype))
        del x
        xf = self.x.float()
        self.mean = xf.mean((0, 2, 3))
        self.invstd = (xf.var((0, 2, 3), unbiased=False) + EPS).rsqrt() if n * h * w > 1 else torch.full((c,), EPS ** -0.5, device=DEV)
        del xf
        self.gamma = torch.randn(c, generator=gen, device=DEV)
        self.ref = self.bn_bwd()

    def workspace_bytes(self):
        n, c, h, w = self.shape
        L = _lib()
        nb = L.mhaq_fq_bn_pool_bwd_x16_workspace_bytes(n, h, w, c)
        assert nb == L.mhaq_fq_bn_bwd_x16_workspace_bytes(n * h * w, c) and nb > 0
        return nb

    def bn_bwd(self):
        n, c, h, w = self.shape
        nb = self.workspace_bytes()
        ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
        dx, dw, db = torch.empty_like(self.x), torch.empty(c, device=DEV), torch.empty(c, device=DEV)
        rc = _lib().mhaq_fq_bn_bwd_x16(_p(self.x), _p(self.dy_torch), _p(self.mean), _p(self.invstd), _p(self.gamma), _p(dx),
                                       _p(dw), _p(db), n * h * w, c, self.dt, _p(ws), nb, _stream())
        assert rc == 0, rc
        return dx, dw, db, ws

    def bn_pool_bwd(self, want=(True, True, True), gamma=True):
        n, c, h, w = self.shape
        nb = self.workspace_bytes()
        ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
        dx = torch.empty_like(self.x) if want[0] else None
        dw = torch.empty(c, device=DEV) if want[1] else None
        db = torch.empty(c, device=DEV) if want[2] else None
        rc = _lib().mhaq_fq_bn_pool_bwd_x16(_p(self.x), _p(self.g), _p(self.code), _p(self.mean), _p(self.invstd),
                                            _p(self.gamma) if gamma else None, _p(dx), _p(dw), _p(db), n, h, w, c, self.dt,
                                            _p(ws), nb, _stream())
        assert rc == 0, rc
        return dx, dw, db, ws


_cases = {}


def _case(shape, dtype):
    key = (shape, dtype)
    if key not in _cases:
        if len(_cases) and max(s[0] * s[1] * s[2] * s[3] for s, _ in list(_cases) + [key]) > 1 << 24:
            _cases.clear()                              # next to a large case nothing else stays resident
            torch.cuda.empty_cache()
        _cases[key] = _Case(shape, dtype)
    return _cases[key]


# ------------------------------------------------------------------------------------------------ C ABI, forward
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_forward_equals_torch_max_pool2d_values_and_indices(shape, dtype):
    k = _case(shape, dtype)
    n, c, h, w = shape
    assert _same_bits(k.p, k.p_torch)
    code = k.code.long()
    oh = torch.arange(_out(h), device=DEV)[:, None]
    ow = torch.arange(_out(w), device=DEV)[None, :]
    # code 9: the window chose no element (all -inf); torch's channels_last kernel leaves its initial index 0 there
    assert int(code.max()) <= 9 and (h < 3 or w < 3 or bool((code == 9).any()))
    idx = torch.where(code == 9, 0, (2 * oh - 1 + code // 3) * w + (2 * ow - 1 + code % 3))
    assert torch.equal(idx, k.idx_torch)
    chosen = (2 * oh - 1 + code // 3 >= 0) & (2 * oh - 1 + code // 3 < h) & (2 * ow - 1 + code % 3 >= 0) & (2 * ow - 1 + code % 3 < w)
    assert bool((chosen | (code == 9)).all())                      # a chosen element lies inside the tensor
    if h >= 3 and w >= 3:                                          # the all--inf plane: code 4 in window (0, 0), code 9 elsewhere
        assert int(code[n - 1, 1, 0, 0]) == 4 and bool((code[n - 1, 1].flatten()[1:] == 9).all())


def test_forward_keeps_a_nans_payload():
    """The pooled value is the chosen element's ORIGINAL 16 bits: NaNs with payloads (a signalling one among them) arrive
    unchanged, as in torch's kernel."""
    for dtype, pats in ((BF16, (0x7FC1, 0xFFC5, 0x7F81)), (F16, (0x7E01, 0xFE05, 0x7D01))):
        t = torch.zeros((1, 8, 3, 3), dtype=torch.int16, device=DEV)
        for ch, pat in enumerate(pats):
            t[0, ch, 1, 1] = pat - (1 << 16) if pat >= 1 << 15 else pat
        t = _cl(t).view(dtype)
        p, code = _hip_pool(t)
        ref = F.max_pool2d(t, 3, 2, 1)
        assert _same_bits(p, ref)
        for ch, pat in enumerate(pats):
            assert int(p.view(torch.int16)[0, ch, 0, 0]) & 0xFFFF == pat and int(code[0, ch, 0, 0]) == 8


# ------------------------------------------------------------------------------------------------ C ABI, backward
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_gather_restated_in_torch_equals_torch_max_pool2d_backward(shape, dtype):
    """Decides the rounding rule (see the module docstring); the test below means something only where this one passes."""
    k = _case(shape, dtype)
    n, c, h, w = shape
    dy = k.dy_torch
    assert _same_bits(_dy_from_codes(k.g, k.code, h, w), dy)
    u = ULP1[dtype]
    for ch, ih, iw, wins in _rounding_plants(shape):               # the planted sums did discriminate
        kinds = sorted(v for _, _, v in wins)
        if "nan" in kinds:
            assert bool(dy[1:, ch, ih, iw].isnan().all())          # (image 0 holds a NaN next to the planted maximum)
            continue
        want = {("1", "e", "e", "e"): 1.0 + u, ("1", "h"): 1.0, ("1+u", "h"): 1.0 + 2 * u}[tuple(kinds)]
        assert bool((dy[:, ch, ih, iw].float() == want).all()), (ch, ih, iw, dy[:, ch, ih, iw])


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_bn_pool_bwd_equals_bn_bwd_x16_on_torchs_dy_workspace_included(shape, dtype):
    k = _case(shape, dtype)
    dx, dw, db, ws = k.bn_pool_bwd()
    rdx, rdw, rdb, rws = k.ref
    assert dx.dtype == dtype
    assert _same_bits(dx, rdx) and _same_bits(dw, rdw) and _same_bits(db, rdb)
    assert torch.equal(ws, rws)                        # the constants and the fp64 partial rows, byte for byte


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_outputs_are_optional_and_a_null_weight_is_one(dtype):
    k = _case((3, 24, 5, 7), dtype)
    full = k.bn_pool_bwd()
    only = k.bn_pool_bwd(want=(False, True, False))
    assert only[0] is None and only[2] is None and _same_bits(only[1], full[1])
    only = k.bn_pool_bwd(want=(True, False, False))
    assert _same_bits(only[0], full[0])
    only = k.bn_pool_bwd(want=(False, False, True))
    assert _same_bits(only[2], full[2])
    saved = k.gamma
    one = k.bn_pool_bwd(gamma=False)
    k.gamma = torch.ones_like(saved)
    ones = k.bn_pool_bwd()
    k.gamma = saved
    assert all(_same_bits(a, b) for a, b in zip(one[:3], ones[:3]))


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_argument_errors_launch_nothing(dtype):
    """A bad dtype, misaligned base pointers, a short workspace, C % 8 and n * h * w >= 2^31: the error code, and
    sentinel-filled outputs stay untouched."""
    L = _lib()
    k = _case((2, 64, 9, 9), dtype)
    n, c, h, w = k.shape
    sent = 0x5A
    nb = k.workspace_bytes()
    ws = torch.full((nb + 16,), sent, dtype=torch.uint8, device=DEV)
    dx = torch.full((k.x.numel() * 2 + 16,), sent, dtype=torch.uint8, device=DEV)
    dw = torch.full((c * 4,), sent, dtype=torch.uint8, device=DEV)
    db = torch.full((c * 4,), sent, dtype=torch.uint8, device=DEV)
    args = [_p(k.x), _p(k.g), _p(k.code), _p(k.mean), _p(k.invstd), _p(k.gamma), _p(dx), _p(dw), _p(db), n, h, w, c, k.dt,
            _p(ws), nb, _stream()]
    for pos, off in ((0, 8), (1, 8), (2, 4), (6, 8), (14, 8), (3, 2)):
        bad = list(args)
        bad[pos] = ctypes.c_void_p(args[pos].value + off)
        assert L.mhaq_fq_bn_pool_bwd_x16(*bad) == -3, pos
    for dt in (0, 3):
        bad = list(args)
        bad[13] = dt
        assert L.mhaq_fq_bn_pool_bwd_x16(*bad) == -1
    short = list(args)
    short[15] = nb - 1
    assert L.mhaq_fq_bn_pool_bwd_x16(*short) == -2
    odd = list(args)
    odd[12] = 60
    assert L.mhaq_fq_bn_pool_bwd_x16(*odd) == -4
    huge = list(args)
    huge[9], huge[15] = (1 << 31) // (h * w) + 1, 1 << 62
    assert L.mhaq_fq_bn_pool_bwd_x16(*huge) == -4
    # the forward
    p = torch.full((k.p.numel() * 2 + 16,), sent, dtype=torch.uint8, device=DEV)
    code = torch.full((k.p.numel() + 16,), sent, dtype=torch.uint8, device=DEV)
    fargs = [_p(k.t), _p(p), _p(code), n, h, w, c, k.dt, _stream()]
    for pos, off in ((0, 8), (1, 8), (2, 4)):
        bad = list(fargs)
        bad[pos] = ctypes.c_void_p(fargs[pos].value + off)
        assert L.mhaq_fq_maxpool3s2_fwd_x16(*bad) == -3, pos
    bad = list(fargs)
    bad[7] = 0
    assert L.mhaq_fq_maxpool3s2_fwd_x16(*bad) == -1
    bad = list(fargs)
    bad[6] = 60
    assert L.mhaq_fq_maxpool3s2_fwd_x16(*bad) == -4
    bad = list(fargs)
    bad[3] = (1 << 31) // (h * w) + 1
    assert L.mhaq_fq_maxpool3s2_fwd_x16(*bad) == -4
    torch.cuda.synchronize()
    for buf in (ws, dx, dw, db, p, code):
        assert bool((buf == sent).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("shape", [(3, 24, 5, 7), (2, 8, 17, 15), (2, 512, 7, 7)], ids=_ids)
def test_sentinel_guards_around_every_output_and_the_workspace(shape, dtype):
    L = _lib()
    k = _case(shape, dtype)
    n, c, h, w = shape
    guard, sent = 4096, 0x5A
    nb = k.workspace_bytes()
    buf = lambda body: torch.full((body + 2 * guard,), sent, dtype=torch.uint8, device=DEV)
    ws, dx, dw, db = buf(nb), buf(k.x.numel() * 2), buf(c * 4), buf(c * 4)
    p, code = buf(k.p.numel() * 2), buf(k.p.numel())
    assert L.mhaq_fq_maxpool3s2_fwd_x16(_p(k.t), _p(p, guard), _p(code, guard), n, h, w, c, k.dt, _stream()) == 0
    assert L.mhaq_fq_bn_pool_bwd_x16(_p(k.x), _p(k.g), _p(code, guard), _p(k.mean), _p(k.invstd), _p(k.gamma), _p(dx, guard),
                                     _p(dw, guard), _p(db, guard), n, h, w, c, k.dt, _p(ws, guard), nb, _stream()) == 0
    torch.cuda.synchronize()
    for b, body in ((ws, nb), (dx, k.x.numel() * 2), (dw, c * 4), (db, c * 4), (p, k.p.numel() * 2), (code, k.p.numel())):
        assert bool((b[:guard] == sent).all()) and bool((b[guard + body:] == sent).all())
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1)
    assert torch.equal(dx[guard:guard + k.x.numel() * 2].view(torch.int16), rows(k.ref[0]).view(torch.int16))
    assert torch.equal(dw[guard:guard + c * 4].view(torch.int32), k.ref[1].view(torch.int32))
    assert torch.equal(ws[guard:guard + nb], k.ref[3])
    assert torch.equal(code[guard:guard + k.p.numel()], rows(k.code))
    assert torch.equal(p[guard:guard + k.p.numel() * 2].view(torch.int16), rows(k.p).view(torch.int16))
