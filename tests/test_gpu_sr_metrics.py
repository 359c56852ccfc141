"""GPU (-m gpu): the fused super-resolution metrics (mhaq_fq_sr_metrics, csrc/sr_metrics.hip) through the C ABI, through
mhaq_amd.sr_metrics and through QATTrainer.validate_step, against the float64 restatement of the definition on the CPU
(tests/sr_metrics_ref.py).  The bar is the framework's own float32 chain on the device, never the kernel:
    |v - v64| <= 4 |v_chain32 - v64| + 8 ulp32(v64)      per image for PSNR and SSIM, and for l1.
Shapes are the smallest that reach each edge: one window (11 x 11), odd width and two images (24 x 37), the 32 x 32 SSIM tile
plus and minus one position (43 x 43, 41 x 41), pool factors 2 and 3 whose floor drops rows and columns (640 x 645,
641 x 643), a pooled image whose rows take the 16-byte loads (384 x 392), two column chunks (11 x 2060)."""
import ctypes
import functools

import pytest
import torch

from tests import sr_metrics_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAND = 64
DT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}

# (n, c, h, w, luminance, noise)
CASES = [(1, 3, 11, 11, True, 0.05), (2, 3, 24, 37, True, 0.02), (1, 3, 43, 43, True, 0.05), (1, 3, 41, 41, True, 0.05),
         (1, 3, 640, 645, True, 0.05), (1, 3, 641, 643, True, 0.05), (1, 3, 384, 392, True, 0.05),
         (1, 3, 11, 2060, True, 0.05), (3, 3, 96, 96, True, 0.3), (1, 3, 96, 96, True, 1e-3),
         (2, 1, 24, 37, False, 0.05), (2, 3, 24, 37, False, 0.05), (1, 3, 384, 392, False, 0.05),
         (1, 3, 64, 64, True, 0.01, 0.5)]                 # the last: a constant 0.5 target, variances at rounding level
ids_case = lambda c: "%dx%dx%dx%d-%s-%g%s" % (c[0], c[1], c[2], c[3], "lum" if c[4] else "planes", c[5],   # noqa: E731
                                              "-flat" if len(c) > 6 else "")


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


class Banded:
    """n elements between two bands of ones (the view starts 256 bytes into the allocation)."""

    def __init__(self, n, dtype, fill=-7):
        self.buf = torch.ones(BAND + n + BAND, dtype=dtype, device=DEV)
        self.n = n
        self.view = self.buf[BAND:BAND + n]
        self.view.fill_(fill)

    def intact(self):
        return bool((self.buf[:BAND] == 1).all()) and bool((self.buf[BAND + self.n:] == 1).all())


def placed(t, off):
    """The values of t, `off` elements into a larger 256-byte-aligned allocation whose other elements are NaN."""
    if not off:
        return t
    buf = torch.full((off + t.numel() + BAND,), float("nan"), dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 256 == 0
    view = buf[off:off + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + off * t.element_size()
    return view


def capi(sr, hr, sr_div=1.0, luminance=True, pool=None, ws_fill=-7, flags_init=0, sr_off=0, hr_off=0):
    """-> (psnr[N], ssim[N], l1[1], mean[2], flags int); asserts that nothing around the outputs and the workspace was written.
    ws_fill: what the workspace holds before the call; flags_init: the flag word before it; sr_off / hr_off: the input starts
    that many elements past a 256-byte boundary."""
    from mhaq_amd import _lib
    lib = _lib.lib()
    assert sr.is_contiguous() and hr.is_contiguous()
    n, c, h, w = sr.shape
    sr, hr = placed(sr, sr_off), placed(hr, hr_off)
    pool = R.pool_factor(h, w) if pool is None else pool
    wsb = lib.mhaq_fq_sr_metrics_workspace_bytes(n, c, h, w, int(luminance), pool)
    assert wsb > 0 and wsb % 8 == 0
    ws = Banded(wsb // 8, torch.float64, fill=ws_fill)
    psnr, ssim = Banded(n + (n & 1), torch.float32), Banded(n + (n & 1), torch.float32)
    l1, mean = Banded(2, torch.float32), Banded(2, torch.float32)
    flags = Banded(2, torch.int32, fill=0)
    flags.view[0] = flags_init
    _lib.check(lib.mhaq_fq_sr_metrics(_ptr(sr), DT[sr.dtype], _ptr(hr), DT[hr.dtype], n, c, h, w, float(sr_div),
                                      int(luminance), pool, _ptr(psnr.view), _ptr(ssim.view), _ptr(l1.view), _ptr(mean.view),
                                      _ptr(flags.view), _ptr(ws.view), wsb, _stream()), "mhaq_fq_sr_metrics")
    torch.cuda.synchronize()
    for b in (ws, psnr, ssim, l1, mean, flags):
        assert b.intact()
    assert float(l1.view[1]) == -7 and int(flags.view[1]) == 0                     # one l1, one flag word
    return psnr.view[:n].clone(), ssim.view[:n].clone(), l1.view[:1].clone(), mean.view.clone(), int(flags.view[0])


@functools.lru_cache(maxsize=None)
def _case(case):
    """Inputs on the device, shared and never modified, with the framework chain there and the float64 restatement."""
    n, c, h, w, lum, noise = case[:6]
    sr, hr = R.images(n, c, h, w, noise=noise, seed=100 * h + w + c, flat=case[6] if len(case) > 6 else None)
    sr, hr = sr.to(DEV), hr.to(DEV)
    return sr, hr, R.chain32(sr, hr, luminance=lum), R.restate64(sr, hr, luminance=lum)


@pytest.mark.parametrize("case", CASES, ids=ids_case)
def test_capi_within_the_bar_of_the_framework_chain(case):
    sr, hr, chain, ref = _case(case)
    psnr, ssim, l1, mean, flags = capi(sr, hr, luminance=case[4])
    R.check_record((psnr, ssim, l1), chain, ref, ids_case(case))
    assert flags == 0
    # the batch means: the fp64 means of the per-image values, rounded once
    assert abs(float(mean[0]) - float(ref[0].mean())) <= 4 * abs(float(chain[0].double().mean()) - float(ref[0].mean())) \
        + 8 * R.ulp32(ref[0].mean())
    assert abs(float(mean[1]) - float(ref[1].mean())) <= 4 * abs(float(chain[1].double().mean()) - float(ref[1].mean())) \
        + 8 * R.ulp32(ref[1].mean())
    # the same inputs give the same bits
    again = capi(sr, hr, luminance=case[4])
    for a, b in zip((psnr, ssim, l1, mean), again[:4]):
        assert torch.equal(_bits(a), _bits(b))


def test_python_entry_gives_the_c_abis_bits_and_takes_strided_inputs():
    from mhaq_amd.sr_metrics import check_sr_flags, sr_metrics
    sr, hr, _, _ = _case(CASES[1])
    psnr, ssim, l1, mean, _ = capi(sr, hr)
    rec = sr_metrics(sr, hr)
    assert set(rec) == {"psnr", "ssim", "l1", "PSNR", "SSIM", "flags"}
    assert rec["l1"].dim() == 0 and rec["PSNR"].dim() == 0 and rec["psnr"].shape == (2,)
    for a, b in ((rec["psnr"], psnr), (rec["ssim"], ssim), (rec["l1"], l1[0]), (rec["PSNR"], mean[0]), (rec["SSIM"], mean[1])):
        assert torch.equal(_bits(a.reshape(-1)), _bits(b.reshape(-1)))
    assert check_sr_flags(rec["flags"], nonfinite=True) == 0
    wide = torch.zeros(2, 3, 24, 50, device=DEV)
    wide[..., :37] = sr
    cl = hr.contiguous(memory_format=torch.channels_last)
    rec2 = sr_metrics(wide[..., :37], cl)
    assert torch.equal(_bits(rec2["ssim"]), _bits(ssim)) and torch.equal(_bits(rec2["psnr"]), _bits(psnr))


def test_rows_and_columns_the_pool_drops_count_for_psnr_and_l1_only():
    sr, hr, _, _ = _case(CASES[5])                        # 641 x 643, f = 3: 213 x 214 pooled, rows 639.. and column 642 dropped
    psnr, ssim, l1, _, _ = capi(sr, hr)
    sr2 = sr.clone()
    sr2[:, :, 639:, :] += 0.25
    sr2[:, :, :, 642:] -= 0.125
    p2, s2, l2, _, _ = capi(sr2, hr)
    assert torch.equal(_bits(s2), _bits(ssim))
    assert float(p2) < float(psnr) and float(l2) > float(l1)
    ref = R.restate64(sr2, hr)
    R.check_record((p2, s2, l2), R.chain32(sr2, hr), ref, "dropped rows")


def test_sr_div_255_on_a_scaled_input():
    sr, hr, _, _ = _case(CASES[1])
    big = (sr * 255).contiguous()
    rec = capi(big, hr, sr_div=255.0)
    R.check_record(rec[:3], R.chain32(big, hr, sr_div=255.0), R.restate64(big, hr, sr_div=255.0), "sr_div 255")
    assert rec[4] == 0


def test_prediction_is_clamped_and_a_target_outside_the_range_sets_bit_1_only():
    sr, hr, _, _ = _case(CASES[1])
    sr2 = sr.clone()
    sr2[0, :, 3, 5] = -0.3
    sr2[1, :, 7, 30] = 1.7
    rec = capi(sr2, hr)
    assert rec[4] == 0
    R.check_record(rec[:3], R.chain32(sr2, hr), R.restate64(sr2, hr), "clamp")
    cl = sr2.clone()
    cl[0, :, 3, 5] = 0.0
    cl[1, :, 7, 30] = 1.0
    rec_cl = capi(cl, hr)
    assert torch.equal(_bits(rec_cl[0]), _bits(rec[0])) and torch.equal(_bits(rec_cl[1]), _bits(rec[1]))   # PSNR, SSIM: clamped
    assert float(rec_cl[2]) < float(rec[2])                                                                 # l1: not
    hr2 = hr.clone()
    hr2[1, :, 2, 2] = 1.2                                 # luminance 1.2 * 0.8588 = 1.03
    assert capi(sr, hr2)[4] == 2
    hr3 = hr.clone()
    hr3[0, 0, 0, 0] = -0.01
    assert capi(sr, hr3, luminance=False)[4] == 2


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", [CASES[1], CASES[6]], ids=ids_case)
def test_16_bit_inputs_give_the_bits_of_the_fp32_entry_on_the_upcast_tensor(case, dtype):
    sr, hr, _, _ = _case(case)
    s16, h16 = sr.to(dtype), hr.to(dtype)
    want = capi(s16.float(), hr, luminance=case[4])
    got = capi(s16, hr, luminance=case[4])
    for a, b in zip(got[:4], want[:4]):
        assert torch.equal(_bits(a), _bits(b))
    want = capi(s16.float(), h16.float(), luminance=case[4])
    got = capi(s16, h16, luminance=case[4])
    for a, b in zip(got[:4], want[:4]):
        assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("case", [CASES[1], CASES[2], CASES[4], CASES[11]], ids=ids_case)
def test_equal_bits_give_ssim_exactly_one(case):
    _, hr, _, _ = _case(case)
    psnr, ssim, l1, mean, flags = capi(hr.clone(), hr, luminance=case[4])
    assert torch.equal(ssim, torch.ones_like(ssim)) and float(mean[1]) == 1.0
    assert float(l1) == 0.0 and flags == 0
    assert torch.allclose(psnr, torch.full_like(psnr, 80.0), rtol=0, atol=8 * R.ulp32(80.0))


def test_a_nan_stays_in_its_own_image():
    sr, hr, _, _ = _case(CASES[1])
    clean = capi(sr, hr)
    bad = sr.clone()
    bad[0, 1, 9, 17] = float("nan")
    psnr, ssim, l1, mean, flags = capi(bad, hr)
    assert flags == 1
    assert torch.isnan(psnr[0]) and torch.isnan(ssim[0]) and torch.isnan(mean).all() and torch.isnan(l1).all()
    assert torch.equal(_bits(psnr[1:]), _bits(clean[0][1:])) and torch.equal(_bits(ssim[1:]), _bits(clean[1][1:]))
    inf = sr.clone()
    inf[1, 0, 0, 0] = float("inf")                        # clamps to 1: no NaN, but bit 0
    r = capi(inf, hr)
    assert r[4] == 1 and not torch.isnan(r[0]).any() and not torch.isnan(r[1]).any()


def test_no_host_synchronisation():
    from mhaq_amd.sr_metrics import sr_metrics
    sr, hr, _, _ = _case(CASES[4])
    sr_metrics(sr, hr)                                    # library load, allocator warm
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        rec = sr_metrics(sr, hr)
        rec16 = sr_metrics(sr.to(torch.bfloat16), hr, to_luminance=False)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert float(rec["SSIM"]) > 0 and float(rec16["SSIM"]) > 0


def _rfdn_trainer(task):
    import mhaq_amd as M
    from mhaq_amd import nets, ops
    from mhaq_amd.qat import QATConfig, QATTrainer
    torch.manual_seed(0)
    ops.manual_seed(1)
    calib = torch.rand(2, 3, 16, 16, generator=torch.Generator().manual_seed(9)).to(DEV) * 255.0
    cfg = QATConfig(qscheme=M.QScheme.PER_CHANNEL, qnmethod=M.QNMethod.LSQ, act_bit=8, weight_bit=8, distillation=False,
                    excluded_layers=("fea_conv", "upsampler.0"), criterion=torch.nn.L1Loss(), task=task,
                    sr_denormalize=(task == "sr"))
    return QATTrainer(nets.rfdn(), cfg, DEV, calib_batches=[calib], distributed=False)


def test_validate_step_records_the_sr_metrics_of_the_trainers_own_eval_output():
    from mhaq_amd.sr_metrics import check_sr_flags
    tr = _rfdn_trainer("sr")
    g = torch.Generator().manual_seed(4)
    x = torch.rand(2, 3, 16, 16, generator=g).to(DEV)
    y = torch.rand(2, 3, 64, 64, generator=g).to(DEV)
    rec = tr.validate_step(x, y)
    assert list(rec) == ["PSNR", "SSIM", "psnr", "ssim", "metric_flags", "val_loss", "mean_weights_bit_width",
                         "actual_weights_bit_width", "actual_weights_max_bit_width", "mean_activations_bit_width",
                         "actual_activations_bit_width", "actual_activations_max_bit_width", "converged"]
    assert check_sr_flags(rec["metric_flags"]) in (0, 1)
    tr.module.eval()
    with torch.no_grad():
        out = tr.net(x * 255)
    tr.module.train()
    chain, ref = R.chain32(out, y, sr_div=255.0), R.restate64(out, y, sr_div=255.0)
    R.check_record((rec["psnr"], rec["ssim"], rec["val_loss"]), chain, ref, "validate_step")
    for key, i in (("PSNR", 0), ("SSIM", 1)):
        ok, frac = R.within_bar(rec[key], chain[i].double().mean(), ref[i].mean())
        assert ok, (key, frac)
    # a criterion that is not the mean L1 runs as the framework's module on the scaled, unclamped prediction
    tr.cfg.criterion = torch.nn.MSELoss()
    rec2 = tr.validate_step(x, y)
    assert torch.allclose(rec2["val_loss"], torch.nn.functional.mse_loss(out / 255, y), rtol=1e-5)
    assert torch.equal(_bits(rec2["psnr"]), _bits(rec["psnr"]))


def test_classification_record_keeps_its_keys():
    import mhaq_amd as M
    from mhaq_amd import nets, ops
    from mhaq_amd.qat import QATConfig, QATTrainer
    torch.manual_seed(3)
    ops.manual_seed(3)
    cfg = QATConfig(qscheme=M.QScheme.PER_CHANNEL, qnmethod=M.QNMethod.LSQ, act_bit=4, weight_bit=4,
                    excluded_layers=("features.init_block.conv", "output"), warmup=2, distillation=False)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(4, 3, 32, 32, generator=g).to(DEV)
    y = torch.randint(0, 10, (4,), generator=g).to(DEV)
    tr = QATTrainer(nets.resnet20_cifar(10), cfg, DEV, calib_batches=[x], distributed=False)
    rec = tr.validate_step(x, y)
    assert list(rec) == ["val_loss", "top1", "mean_weights_bit_width", "actual_weights_bit_width",
                         "actual_weights_max_bit_width", "mean_activations_bit_width", "actual_activations_bit_width",
                         "actual_activations_max_bit_width", "converged"]
