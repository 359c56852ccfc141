"""GPU (-m gpu): the pooled 16-bit stem forward through the C ABI (mhaq_fq_bn_norm_pool3s2_fwd_x16, csrc/bn_bwd.hip).

The contract is a composition, and so is the yardstick: p and code must be, BIT FOR BIT (int16 / uint8 views: signed zeros and
NaN payloads count, there are no tolerances), what mhaq_fq_maxpool3s2_fwd_x16 writes from the y that mhaq_fq_bn_fwd_x16 writes
from the same x, weight and bias -- with the mean and invstd that call saved.  Both of those are tested against torch in their
own files.  Every output of the kernel under test sits between sentinel guards.

Planted channels (every shape has C >= 8; further channels draw gamma of both signs and beta at random):
  0  gamma = 0: every y equals beta, every window is a tie, the FIRST in-range position must win
  1  gamma < 0: the order of x reverses
  2  gamma = 0.5 with a beta at which the format's spacing is 0.5 (bf16: 96, fp16: 768): about seven distinct y over the
     whole channel, so most windows hold x that are distinct and round to EQUAL y.  The first of them must win; "pool x,
     then normalize the winner" takes the largest x instead.  The windows where that shortcut is wrong are counted.
  3  gamma = +inf: y is +inf above the channel's mean and -inf below it; a block of low x gives windows that are -inf
     throughout (code 9, or code 4 in the window (0, 0)) next to windows that hold +inf
  4  gamma = +inf, beta = -inf: y is NaN (inf - inf) above the mean and -inf below it: NaN windows next to all--inf windows
  5  one NaN in x: the statistics and every y of the channel are NaN; the LAST in-range position wins.  Two NaNs of different
     sign meet in (x - mean) * a here: the kernel must keep the one bn_fwd_norm_kernel keeps
  6  one +inf in x: the mean is +inf and invstd NaN, so y is NaN everywhere -- inf - inf at the planted element, -inf * NaN
     elsewhere
The launcher has ONE kernel per dtype and no size threshold (no cache-policy or occupancy switch), so the shapes of the issue
are all there is: one window; ragged edges; C / 8 = 3; odd and even extents; several blocks; the stem's own plane.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5
BF16, F16 = torch.bfloat16, torch.float16
DTYPES = [BF16, F16]
_dt = lambda d: "bf16" if d is BF16 else "fp16"
SHAPES = [(2, 8, 1, 1), (2, 8, 2, 3), (3, 24, 5, 7), (1, 8, 4, 4), (2, 16, 7, 9), (3, 64, 13, 12), (2, 64, 112, 112)]
_ids = lambda s: "x".join(map(str, s))
GUARD, SENT = 4096, 0x5A
TIE_BETA = {BF16: 96.0, F16: 768.0}                    # the spacing of the format is 0.5 there


def _L():
    from mhaq_amd import _lib
    return _lib.lib()


def _code_of(dtype):
    from mhaq_amd import _lib
    return _lib.DT_BF16 if dtype is BF16 else _lib.DT_F16


_p = lambda t, off=0: None if t is None else ctypes.c_void_p(t.data_ptr() + off)
_stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
_out = lambda n: (n - 1) // 2 + 1
_rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1)   # NHWC memory order of a channels_last tensor


def _cl(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def _inputs(shape, dtype):
    n, c, h, w = shape
    gen = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn(shape, generator=gen, device=DEV) * 2 + torch.randn((1, c, 1, 1), generator=gen, device=DEV)
    if h >= 5 and w >= 5:
        x[:, 3, 0:4, 0:4] = -9.0                       # below the channel's mean: windows (0..1, 0..1) are -inf throughout
        x[:, 4, 0:4, 0:4] = -9.0
    x[n - 1, 5, h // 2, w // 2] = float("nan")
    x[0, 6, 0, 0] = float("inf")
    gamma = torch.randn(c, generator=gen, device=DEV)
    beta = torch.randn(c, generator=gen, device=DEV)
    gamma[:6] = torch.tensor([0.0, -1.5, 0.5, float("inf"), float("inf"), 1.0], device=DEV)
    beta[:6] = torch.tensor([0.25, 0.5, TIE_BETA[dtype], 0.0, float("-inf"), 0.0], device=DEV)
    return _cl(x.to(dtype)), gamma, beta


def _bn_fwd(x, gamma, beta):
    """mhaq_fq_bn_fwd_x16: (y, mean, invstd)."""
    n, c, h, w = x.shape
    L, m = _L(), n * h * w
    nb = L.mhaq_fq_bn_fwd_x16_workspace_bytes(m, c)
    assert nb > 0
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    y, mean, invstd = torch.empty_like(x), torch.empty(c, device=DEV), torch.empty(c, device=DEV)
    rc = L.mhaq_fq_bn_fwd_x16(_p(x), _p(gamma), _p(beta), _p(y), _p(mean), _p(invstd), None, None, 0.1, EPS, m, c,
                              _code_of(x.dtype), _p(ws), nb, _stream())
    assert rc == 0, rc
    return y, mean, invstd


def _pool(t):
    """mhaq_fq_maxpool3s2_fwd_x16: (p, code), channels_last."""
    n, c, h, w = t.shape
    p = torch.empty((n, c, _out(h), _out(w)), dtype=t.dtype, device=DEV).contiguous(memory_format=torch.channels_last)
    code = torch.empty((n, c, _out(h), _out(w)), dtype=torch.uint8, device=DEV).contiguous(memory_format=torch.channels_last)
    rc = _L().mhaq_fq_maxpool3s2_fwd_x16(_p(t), _p(p), _p(code), n, h, w, c, _code_of(t.dtype), _stream())
    assert rc == 0, rc
    return p, code


def _norm_pool(x, mean, invstd, gamma, beta):
    """The kernel under test into guarded buffers: (p bits [N*OH*OW*C] int16, code [N*OH*OW*C] uint8), guards checked."""
    n, c, h, w = x.shape
    nout = n * _out(h) * _out(w) * c
    pb = torch.full((2 * nout + 2 * GUARD,), SENT, dtype=torch.uint8, device=DEV)
    cb = torch.full((nout + 2 * GUARD,), SENT, dtype=torch.uint8, device=DEV)
    rc = _L().mhaq_fq_bn_norm_pool3s2_fwd_x16(_p(x), _p(mean), _p(invstd), _p(gamma), _p(beta), _p(pb, GUARD), _p(cb, GUARD),
                                              n, h, w, c, _code_of(x.dtype), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    for b, body in ((pb, 2 * nout), (cb, nout)):
        assert bool((b[:GUARD] == SENT).all()) and bool((b[GUARD + body:] == SENT).all())
    return pb[GUARD:GUARD + 2 * nout].view(torch.int16), cb[GUARD:GUARD + nout]


class _Case:
    """What the tests of one shape and dtype share, computed once and left unchanged."""

    def __init__(self, shape, dtype):
        self.shape, self.dtype = shape, dtype
        self.x, self.gamma, self.beta = _inputs(shape, dtype)
        self.y, self.mean, self.invstd = _bn_fwd(self.x, self.gamma, self.beta)
        self.p, self.code = _pool(self.y)                # the two-launch composition: the yardstick
        self.got_p, self.got_code = _norm_pool(self.x, self.mean, self.invstd, self.gamma, self.beta)


_cases = {}


def _case(shape, dtype):
    if (shape, dtype) not in _cases:
        _cases[(shape, dtype)] = _Case(shape, dtype)
    return _cases[(shape, dtype)]


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_p_and_code_are_the_bits_of_the_two_launch_composition(shape, dtype):
    k = _case(shape, dtype)
    c = shape[1]
    for what, got, want in (("code", k.got_code, _rows(k.code)), ("p", k.got_p, _rows(k.p).view(torch.int16))):
        bad = (got != want).view(-1, c)
        chans = sorted(set(bad.nonzero()[:, 1].tolist()))
        first = bad.view(-1).nonzero()[:1].view(-1).tolist()
        assert not chans, (what, "channels", chans, "first", [(int(got[i]) & 0xFFFF, int(want[i]) & 0xFFFF) for i in first])


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_the_planted_channels_are_what_they_are_for(shape, dtype):
    """The yardstick itself shows each planted case, so the equality above was tested on it."""
    k = _case(shape, dtype)
    n, c, h, w = shape
    code, p = k.code.long(), k.p
    po = torch.arange(_out(h), device=DEV)[:, None].expand(_out(h), _out(w))
    pw = torch.arange(_out(w), device=DEV)[None, :].expand(_out(h), _out(w))
    # gamma = 0: all ties, the first in-range position: (1, 1) in the corner window, (1, 0) / (0, 1) along the edges, else (0, 0)
    first = torch.where(po == 0, torch.where(pw == 0, 4, 3), torch.where(pw == 0, 1, 0))
    assert bool((code[:, 0] == first).all()) and bool((p[:, 0].float() == 0.25).all())
    # one NaN in x: the whole channel is NaN and the last in-range position wins
    last = torch.clamp(h - 2 * po, max=2) * 3 + torch.clamp(w - 2 * pw, max=2)      # ih = 2 po - 1 + kh <= h - 1
    assert bool(p[:, 5].isnan().all()) and bool((code[:, 5] == last).all())
    assert bool(p[:, 6].isnan().all()) and bool((code[:, 6] == last).all())         # one +inf in x
    assert bool((k.got_code.view(n, _out(h), _out(w), c)[..., 0] == first).all())
    if h >= 5 and w >= 5:
        assert bool((p[:, 3] == float("inf")).any()) and bool((p[:, 3] == float("-inf")).any())
        assert int(code[0, 3, 0, 0]) == 4 and int(code[0, 3, 0, 1]) == 9 and int(code[0, 3, 1, 1]) == 9      # all -inf
        assert bool(p[:, 4].isnan().any()) and bool((p[:, 4] == float("-inf")).any()) and int(code[0, 4, 1, 0]) == 9
    assert bool((p[:, 2].float() - TIE_BETA[dtype]).abs().max() <= 4.0)           # the tie channel sits where the spacing is 0.5


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("shape", [(3, 64, 13, 12), (2, 64, 112, 112)], ids=_ids)
def test_distinct_x_that_round_to_one_y_tie_and_the_shortcut_gets_them_wrong(shape, dtype):
    """Channel 2 (gamma > 0, finite).  "Pool x, then normalize" chooses the first LARGEST x of a window; the contract chooses
    the first largest ROUNDED y.  y is non-decreasing in x, so the largest x has the largest y too: the two codes differ exactly
    where an EARLIER position holds a strictly smaller x whose y rounds to the same bits.  Such windows are counted; there must
    be some, and the kernel must side with the composition in every one of them."""
    k = _case(shape, dtype)
    n, c, h, w = shape
    _, short = _pool(k.x)
    differ = short[:, 2] != k.code[:, 2]
    count = int(differ.sum())
    print(f"{_ids(shape)} {_dt(dtype)}: {count} of {differ.numel()} windows of channel 2 hold distinct x with one rounded y")
    assert count > 0
    got = k.got_code.view(n, _out(h), _out(w), c)[..., 2]
    assert torch.equal(got, k.code[:, 2])
    # gamma < 0 reverses the order: the shortcut's choice is wrong in most windows of channel 1 as well
    assert int((short[:, 1] != k.code[:, 1]).sum()) > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_null_weight_is_one_and_null_bias_is_zero(dtype):
    k = _case((3, 24, 5, 7), dtype)
    c = k.shape[1]
    ones, zeros = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
    for gamma, beta in ((None, None), (None, k.beta), (k.gamma, None)):
        y, mean, invstd = _bn_fwd(k.x, gamma, beta)      # the composition takes NULL likewise ...
        p, code = _pool(y)
        got_p, got_code = _norm_pool(k.x, mean, invstd, gamma, beta)
        assert torch.equal(got_code, _rows(code)) and torch.equal(got_p, _rows(p).view(torch.int16))
        # ... and NULL means 1 and 0
        full_p, full_code = _norm_pool(k.x, mean, invstd, ones if gamma is None else gamma, zeros if beta is None else beta)
        assert torch.equal(got_code, full_code) and torch.equal(got_p, full_p)


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_argument_errors_launch_nothing(dtype):
    L = _L()
    k = _case((2, 16, 7, 9), dtype)
    n, c, h, w = k.shape
    nout = n * _out(h) * _out(w) * c
    pb = torch.full((2 * nout + 16,), SENT, dtype=torch.uint8, device=DEV)
    cb = torch.full((nout + 16,), SENT, dtype=torch.uint8, device=DEV)
    args = [_p(k.x), _p(k.mean), _p(k.invstd), _p(k.gamma), _p(k.beta), _p(pb), _p(cb), n, h, w, c, _code_of(dtype), _stream()]
    fn = L.mhaq_fq_bn_norm_pool3s2_fwd_x16

    def call(pos, val):
        bad = list(args)
        bad[pos] = val
        return fn(*bad)
    for pos, off in ((0, 8), (5, 8), (6, 4), (1, 2), (2, 2), (3, 2), (4, 2)):
        assert call(pos, ctypes.c_void_p(args[pos].value + off)) == -3, pos
    for pos in (0, 1, 2, 5, 6):
        assert call(pos, None) == -1, pos
    assert call(11, 0) == -1 and call(11, 3) == -1
    assert call(10, 12) == -4 and call(7, (1 << 31) // (h * w) + 1) == -4 and call(8, 0) == -1
    torch.cuda.synchronize()
    assert bool((pb == SENT).all()) and bool((cb == SENT).all())
