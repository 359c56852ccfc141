"""CPU: everything about the fused super-resolution metrics (mhaq_fq_sr_metrics, mhaq_amd/sr_metrics.py) that needs no GPU --
the symbols, every argument error (returned before any launch: the pointers here are fake), the workspace query, the pool
factor, the float64 restatement of tests/sr_metrics_ref.py against values derived independently and against direct64 (the
definition written out a second time), the geometry that the shapes of the GPU edge suite reach, the validation meter
and the QATConfig defaults.  The kernels are held to the restatement on the device by tests/test_gpu_sr_metrics.py."""
import ctypes
import dataclasses
import math
import os
import re

import pytest
import torch
from torch import nn

from mhaq_amd import _lib
from mhaq_amd.qat import QATConfig, QATTrainer
from tests import sr_metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mhaq_fq_sr_metrics_workspace_bytes", "mhaq_fq_sr_metrics")
EINVAL, EWORKSPACE, EALIGN, EUNSUPPORTED = -1, -2, -3, -4


def test_symbols_are_declared_exported_and_bound_with_the_headers_arity():
    raw = open(_lib.HEADER_PATH).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = _lib.lib()
    for name in NAMES:
        assert name in _lib.header_functions() and name in _lib.SIGNATURES
        assert hasattr(lib, name)
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1])
    assert lib.mhaq_fq_abi_version() == 4 and re.search(r"#define MHAQ_FQ_ABI_VERSION 4\b", raw)
    mk = open(os.path.join(ROOT, "mhaq_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRC\s*=.*\bsr_metrics\.hip\b", mk, flags=re.M)
    assert "-ffp-contract=off" in mk and "-fno-gpu-approx-transcendentals" in mk


def _call(lib, **kw):
    fake = ctypes.c_void_p(0x1000)
    a = dict(sr=fake, sdt=0, hr=fake, hdt=0, n=2, c=3, h=24, w=37, div=1.0, lum=1, pool=1, psnr=fake, ssim=fake, l1=fake,
             mean=fake, flags=fake, ws=fake, wsb=None)
    a.update(kw)
    if a["wsb"] is None:
        a["wsb"] = lib.mhaq_fq_sr_metrics_workspace_bytes(a["n"], a["c"], a["h"], a["w"], a["lum"], a["pool"])
    return lib.mhaq_fq_sr_metrics(a["sr"], a["sdt"], a["hr"], a["hdt"], a["n"], a["c"], a["h"], a["w"], a["div"], a["lum"],
                                  a["pool"], a["psnr"], a["ssim"], a["l1"], a["mean"], a["flags"], a["ws"], a["wsb"], None)


def test_argument_errors_come_before_any_launch_in_the_librarys_order():
    lib = _lib.lib()
    odd1, odd2, off4 = ctypes.c_void_p(0x1001), ctypes.c_void_p(0x1002), ctypes.c_void_p(0x1004)
    # 1. required pointers
    for k in ("sr", "hr", "psnr", "ssim", "l1", "mean", "flags", "ws"):
        assert _call(lib, **{k: None}) == EINVAL, k
    # 2. known dtypes
    for kw in (dict(sdt=3), dict(sdt=-1), dict(hdt=3), dict(hdt=7)):
        assert _call(lib, **kw) == EINVAL, kw
    # 3. positive sizes, pool >= 1, sr_div finite and non-zero
    for kw in (dict(n=0), dict(n=-1), dict(c=0), dict(h=0), dict(h=-3), dict(w=0), dict(pool=0), dict(pool=-2),
               dict(div=0.0), dict(div=float("inf")), dict(div=float("nan")), dict(div=-float("inf"))):
        assert _call(lib, wsb=1 << 30, **kw) == EINVAL, kw
    # 4. luminance needs three channels
    assert _call(lib, c=1, lum=1, wsb=1 << 30) == EINVAL
    assert _call(lib, c=4, lum=1, wsb=1 << 30) == EINVAL
    # 5. a short workspace
    full = lib.mhaq_fq_sr_metrics_workspace_bytes(2, 3, 24, 37, 1, 1)
    assert _call(lib, wsb=full - 1) == EWORKSPACE and _call(lib, wsb=0) == EWORKSPACE
    # 6. alignment: inputs to their element size, outputs and workspace to 8 bytes
    assert _call(lib, sr=odd2) == EALIGN and _call(lib, hr=odd1) == EALIGN
    assert _call(lib, sr=odd1, sdt=1) == EALIGN and _call(lib, hr=odd1, hdt=2) == EALIGN
    for k in ("psnr", "ssim", "l1", "mean", "flags", "ws"):
        assert _call(lib, **{k: off4}) == EALIGN, k
    # 7. unsupported: no window fits, channels other than 1 or 3, more work than a grid dimension takes
    assert _call(lib, h=10, wsb=1 << 30) == EUNSUPPORTED and _call(lib, w=10, wsb=1 << 30) == EUNSUPPORTED
    assert _call(lib, h=21, w=40, pool=2, wsb=1 << 30) == EUNSUPPORTED         # floor(21 / 2) = 10
    assert _call(lib, c=2, lum=0, wsb=1 << 30) == EUNSUPPORTED
    assert _call(lib, c=4, lum=0, wsb=1 << 30) == EUNSUPPORTED
    assert _call(lib, n=1 << 20, wsb=1 << 40) == EUNSUPPORTED
    # the order: -1 before -2 before -3 before -4
    assert _call(lib, sr=None, wsb=0, ws=off4) == EINVAL
    assert _call(lib, wsb=0, ws=off4) == EWORKSPACE
    assert _call(lib, h=10, ws=off4, wsb=1 << 30) == EALIGN
    # and the sizes the call refuses have no workspace
    assert lib.mhaq_fq_sr_metrics_workspace_bytes(1, 3, 10, 64, 1, 1) == 0
    assert lib.mhaq_fq_sr_metrics_workspace_bytes(0, 3, 64, 64, 1, 1) == 0


def test_workspace_covers_the_pooled_planes_and_the_partials_and_grows_with_every_size():
    ws = _lib.lib().mhaq_fq_sr_metrics_workspace_bytes
    for (n, c, h, w, lum) in ((1, 3, 11, 11, 1), (2, 3, 24, 37, 1), (1, 3, 640, 645, 1), (1, 3, 641, 643, 1),
                              (24, 3, 96, 96, 1), (2, 3, 96, 96, 0), (2, 1, 50, 43, 0), (1, 3, 1356, 2040, 1)):
        f = R.pool_factor(h, w)
        p = 1 if lum else c
        hp, wp = h // f, w // f
        planes = 2 * n * p * hp * wp * 4
        tiles = n * p * math.ceil((hp - 10) / 32) * math.ceil((wp - 10) / 32)      # one fp64 SSIM partial per 32 x 32 tile
        base = ws(n, c, h, w, lum, f)
        assert base >= planes + 8 * tiles + 16 * n, (n, c, h, w)
        assert base < planes + (1 << 20)                                          # and nothing of the inputs' size
        assert ws(n + 1, c, h, w, lum, f) > base
        assert ws(n, c, h + f, w, lum, f) > base and ws(n, c, h, w + f, lum, f) > base
        assert ws(n, c, h + 1, w, lum, f) >= base and ws(n, c, h, w + 1, lum, f) >= base
    assert ws(2, 3, 96, 96, 0, 1) > ws(2, 3, 96, 96, 1, 1)                        # three planes against one


def sr_geometry_replica(n, c, h, w, lum, f):
    """sr_geometry of csrc/sr_metrics.hip in Python: what a shape of the GPU edge suite reaches, and the workspace it needs."""
    p = 1 if lum else c
    unit = 8 * f // math.gcd(8, f)
    cap = 2048 if f == 1 else min(2048, 12288 // (2 * p * f))
    chunk = min(cap // unit, -(-w // unit)) * unit
    nchunk = -(-w // chunk)
    groups = -(-h // f)
    band = max(1, min(groups, -(-2048 // (f * min(chunk, w)))))
    nband = -(-groups // band)
    hp, wp = h // f, w // f
    tx, ty = -(-(wp - 10) // 32), -(-(hp - 10) // 32)
    nblk1, nblk2 = nband * nchunk, p * tx * ty
    plane = (n * p * hp * wp * 4 + 15) & ~15
    total = 2 * plane + n * nblk1 * 16 + n * nblk2 * 8 + n * 24 + ((n * nblk1 * 4 + 7) & ~7)
    return dict(unit=unit, chunk=chunk, nchunk=nchunk, last=w - (nchunk - 1) * chunk, band=band, nband=nband,
                lds=0 if f == 1 else 2 * p * f * chunk * 4, tx=tx, ty=ty, total=total)


def test_the_edge_suites_shapes_reach_the_geometry_they_are_there_for():
    """(unit, chunk, chunks, width of the last chunk, band, bands, bytes of LDS) per shape of tests/test_gpu_sr_metrics_edges.py,
    and the library's workspace query agrees with the replica (it counts the workgroups of both launches)."""
    from tests.test_gpu_sr_metrics_edges import POOLED
    want = {(57, 1257): (40, 1200, 2, 57, 1, 12, 48000), (22, 2071): (8, 2048, 2, 23, 1, 11, 32768),
            (22, 2072): (8, 2048, 2, 24, 1, 11, 32768), (22, 2049): (8, 2048, 2, 1, 1, 11, 32768),
            (22, 2050): (8, 2048, 2, 2, 1, 11, 32768), (35, 707): (24, 672, 2, 35, 2, 6, 48384),
            (44, 556): (8, 512, 2, 44, 1, 11, 49152), (55, 57): (40, 80, 1, 57, 8, 2, 3200),
            (77, 83): (56, 112, 1, 83, 4, 3, 6272), (33, 34): (24, 48, 1, 34, 11, 1, 1152),
            (300, 11): (8, 16, 1, 11, 187, 2, 0)}
    ws = _lib.lib().mhaq_fq_sr_metrics_workspace_bytes
    assert len(POOLED) == len(want)
    for (n, c, h, w, lum, f) in POOLED:
        g = sr_geometry_replica(n, c, h, w, lum, f)
        assert (g["unit"], g["chunk"], g["nchunk"], g["last"], g["band"], g["nband"], g["lds"]) == want[(h, w)], (h, w, g)
        assert ws(n, c, h, w, int(lum), f) == g["total"], (h, w)
        assert g["lds"] <= 49152
    assert sr_geometry_replica(1, 3, 300, 11, True, 1)["ty"] == 10 and sr_geometry_replica(1, 3, 300, 11, True, 1)["tx"] == 1
    # the workload this stands for: a DIV2K validation image on luminance
    g = sr_geometry_replica(1, 3, 1356, 2040, True, 5)
    assert (g["chunk"], g["nchunk"], g["last"]) == (1200, 2, 840) and ws(1, 3, 1356, 2040, 1, 5) == g["total"]


def test_pool_factor_rounds_halves_to_even():
    from mhaq_amd.sr_metrics import ssim_pool_factor
    want = {128: 1, 383: 1, 384: 2, 639: 2, 640: 2, 641: 3, 1356: 5}
    for side, f in want.items():
        assert ssim_pool_factor(side, 4000) == f and ssim_pool_factor(4000, side) == f, side
        assert R.pool_factor(side, 4000) == f
    assert ssim_pool_factor(1356, 2040) == 5 and ssim_pool_factor(16, 16) == 1


def test_restatement_identical_images_and_constant_planes():
    """Values derived independently of the restatement's code: identical images have SSIM 1 and PSNR -10 log10(1e-8) = 80;
    constant planes a, b have zero variances, so cs = 1 and SSIM = (2ab + c1) / (a^2 + b^2 + c1), PSNR from (a - b)^2."""
    sr, hr = R.images(2, 3, 24, 37, seed=3)
    psnr, ssim, l1 = R.restate64(hr, hr)
    assert torch.allclose(ssim, torch.ones(2, dtype=torch.float64), rtol=0, atol=1e-12)
    assert torch.allclose(psnr, torch.full((2,), -10 * math.log10(1e-8), dtype=torch.float64), rtol=1e-12, atol=0)
    assert float(l1) == 0.0
    a, b = 0.625, 0.25
    x, y = torch.full((1, 1, 30, 41), a), torch.full((1, 1, 30, 41), b)
    psnr, ssim, l1 = R.restate64(x, y, luminance=False)
    assert abs(float(ssim) - (2 * a * b + 1e-4) / (a * a + b * b + 1e-4)) < 1e-12
    assert abs(float(psnr) - (-10 * math.log10((a - b) ** 2 + 1e-8))) < 1e-10
    assert abs(float(l1) - (a - b)) < 1e-15
    # the division, the clamp of the prediction alone, and the luminance weights
    x3, y3 = torch.full((1, 3, 12, 12), 1.5 * 255), torch.full((1, 3, 12, 12), 0.5)
    psnr, ssim, l1 = R.restate64(x3, y3, sr_div=255.0)
    k = sum(float(torch.tensor(v, dtype=torch.float32)) for v in R.LUMA) / 256
    assert abs(float(l1) - 1.0) < 1e-12                                            # unclamped: |1.5 - 0.5|
    assert abs(float(psnr) - (-10 * math.log10((k * 0.5) ** 2 + 1e-8))) < 1e-6     # clamped to 1, then luminance
    # f = 2 drops the odd last row and column from SSIM, not from PSNR
    sr, hr = R.images(1, 3, 385, 391, seed=5)
    sr2 = sr.clone()
    sr2[:, :, 384:, :] += 0.25
    p1, s1, _ = R.restate64(sr, hr)
    p2, s2, _ = R.restate64(sr2, hr)
    assert float(s1) == float(s2) and float(p2) < float(p1)


# (n, c, h, w, luminance, pool, noise, flat, sr_div)
DIRECT_CASES = [(1, 3, 11, 11, True, None, 0.05, None, 1.0), (2, 3, 24, 37, False, None, 0.05, None, 1.0),
                (2, 1, 24, 37, False, None, 0.05, None, 1.0), (1, 3, 57, 61, True, 5, 0.05, None, 1.0),
                (1, 3, 35, 38, False, 3, 0.05, None, 1.0), (1, 3, 64, 64, True, None, 0.01, 0.5, 1.0),
                (2, 3, 24, 37, True, None, 0.05, None, 255.0)]


@pytest.mark.parametrize("case", DIRECT_CASES, ids=lambda c: "%dx%dx%dx%d-%s-pool%s-div%g%s" % (
    c[0], c[1], c[2], c[3], "lum" if c[4] else "planes", c[5], c[8], "-flat" if c[7] is not None else ""))
def test_direct64_written_from_the_header_agrees_with_the_restatement(case):
    """Two float64 statements of include/mhaq_fq.h that share no code (conv2d / avg_pool2d in torch against sliding windows,
    block means and an einsum in numpy).  Both are fp64 sums of at most 121 terms of magnitude at most 1, so they differ near
    1e-14; the bounds leave four orders above that and stay three orders below the smallest term of the fp32 bar,
    8 ulp32(1) = 9.5e-7."""
    n, c, h, w, lum, pool, noise, flat, div = case
    sr, hr = R.images(n, c, h, w, noise=noise, seed=7 * h + w + c, flat=flat)
    if div != 1.0:                                        # a de-normalised prediction with values the clamp meets
        sr = sr * div
        sr[0, :, 3, 5] = -0.3 * div
        sr[1, :, 7, 30] = 1.7 * div
        sr[1, 1, 20, 2] = 1.0001 * div
    psnr, ssim, l1 = R.restate64(sr, hr, sr_div=div, luminance=lum, pool=pool)
    dp, ds, dl = R.direct64(sr, hr, sr_div=div, luminance=lum, pool=pool)
    assert dp.shape == (n,) and ds.shape == (n,) and dp.dtype == ds.dtype == "float64"
    print("direct64 - restate64:", [float(abs(dp[i] - float(psnr[i]))) for i in range(n)],
          [float(abs(ds[i] - float(ssim[i]))) for i in range(n)], abs(float(dl) - float(l1)))
    for i in range(n):
        assert abs(dp[i] - float(psnr[i])) <= 1e-9, (i, dp[i], float(psnr[i]))
        assert abs(ds[i] - float(ssim[i])) <= 1e-10, (i, ds[i], float(ssim[i]))
    assert abs(float(dl) - float(l1)) <= 1e-10
    assert 0.0 < float(ds.min()) < 1.0 and float(dp.max()) < 80.0                 # not the degenerate equal-images values


def test_direct64_keeps_a_nan_through_the_clamp_and_takes_the_reference_pool_by_default():
    sr, hr = R.images(2, 3, 24, 37, seed=2)
    bad = sr.clone()
    bad[1, 0, 4, 4] = float("nan")
    dp, ds, dl = R.direct64(bad, hr)
    assert math.isnan(dp[1]) and math.isnan(ds[1]) and math.isnan(dl) and math.isfinite(dp[0]) and math.isfinite(ds[0])
    clean = R.direct64(sr, hr)
    assert dp[0] == clean[0][0] and ds[0] == clean[1][0]
    # pool = None is the factor of the image size; an explicit factor is taken as given
    sr, hr = R.images(1, 3, 384, 390, seed=4)
    assert R.direct64(sr, hr)[1][0] == R.direct64(sr, hr, pool=2)[1][0] != R.direct64(sr, hr, pool=1)[1][0]
    assert float(R.restate64(sr, hr)[1]) == float(R.restate64(sr, hr, pool=2)[1]) != float(R.restate64(sr, hr, pool=1)[1])
    assert float(R.chain32(sr, hr)[1]) == float(R.chain32(sr, hr, pool=2)[1])


def test_chain32_is_the_restatement_in_float32():
    sr, hr = R.images(2, 3, 24, 37, seed=1)
    c, r = R.chain32(sr, hr), R.restate64(sr, hr)
    for a, b in zip(c, r):
        assert a.dtype == torch.float32 and b.dtype == torch.float64
        assert torch.allclose(a.double(), b, rtol=1e-4, atol=1e-5)
    ok, frac = R.within_bar(1.0, 1.0 + 2.0 ** -20, 1.0)
    assert ok and frac == 0.0
    assert not R.within_bar(1.0 + 2.0 ** -17, 1.0 + 2.0 ** -20, 1.0)[0]            # 8 x the chain's error: outside
    assert R.within_bar(1.0 + 7 * 2.0 ** -23, 1.0, 1.0)[0] and not R.within_bar(1.0 + 9 * 2.0 ** -23, 1.0, 1.0)[0]


def test_validation_meter_means_and_the_weighted_mean():
    from mhaq_amd.sr_metrics import SRValidationMeter
    m = SRValidationMeter()
    rec = lambda p, s: {"PSNR": torch.tensor(p), "SSIM": torch.tensor(s)}          # noqa: E731
    m.update("Set5", rec(30.0, 0.9), 2)
    m.update("Set5", rec(33.0, 0.8), 1)
    m.update("B100", rec(27.0, 0.7), 4)
    m.update(None, rec(99.0, 0.1), 3)                                              # unnamed: logged, not weighted
    out = m.compute()
    assert abs(float(out["PSNR/Set5"]) - (30.0 * 2 + 33.0) / 3) < 1e-12
    assert abs(float(out["SSIM/Set5"]) - (0.9 * 2 + 0.8) / 3) < 1e-6
    assert abs(float(out["PSNR/B100"]) - 27.0) < 1e-12
    want = (31.0 / 3 + 27.0 / 4) / (1 / 3 + 1 / 4)                                  # weights 1 / count
    assert abs(float(out["PSNR/Weighted_mean"]) - want) < 1e-9
    assert abs(float(out["PSNR/None"]) - 99.0) < 1e-12
    m.reset()
    assert m.compute() == {}
    m.update("", rec(20.0, 0.5), 1)
    assert "PSNR/Weighted_mean" not in m.compute()


def test_flags_reader_and_cpu_tensors_are_refused():
    from mhaq_amd.sr_metrics import check_sr_flags, sr_metrics
    assert check_sr_flags(torch.tensor([0], dtype=torch.int32)) == 0
    assert check_sr_flags(torch.tensor([1], dtype=torch.int32)) == 1
    with pytest.raises(FloatingPointError):
        check_sr_flags(torch.tensor([1], dtype=torch.int32), nonfinite=True)
    with pytest.raises(AssertionError, match=r"\[0, 1\]"):
        check_sr_flags(torch.tensor([3], dtype=torch.int32))
    with pytest.raises(_lib.MhaqFqError):
        sr_metrics(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16))


def test_config_defaults_are_unchanged_and_sr_needs_a_gpu():
    cfg = QATConfig()
    assert (cfg.task, cfg.sr_to_luminance, cfg.sr_denormalize) == ("cls", True, False)
    assert isinstance(cfg.criterion, nn.CrossEntropyLoss) and cfg.distillation_loss == "Symmetrical KL"
    names = [f.name for f in dataclasses.fields(QATConfig)]
    assert names[-3:] == ["task", "sr_to_luminance", "sr_denormalize"] and names.index("criterion") < names.index("task")
    with pytest.raises(_lib.MhaqFqError):
        QATTrainer(nn.Conv2d(3, 3, 3, padding=1), QATConfig(task="sr", criterion=nn.L1Loss(), distillation=False), "cpu")
    with pytest.raises(ValueError):
        QATTrainer(nn.Conv2d(3, 3, 3, padding=1), QATConfig(task="detect"), "cpu")
