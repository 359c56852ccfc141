"""Checker code for the fused super-resolution metrics (mhaq_fq_sr_metrics, mhaq_amd/sr_metrics.py):

  restate64(sr, hr, ...)   the definition of include/mhaq_fq.h / DESIGN section 16 in float64 on the CPU, from the bits of the
                           inputs: the yardstick.  It restates what `piq.psnr` / `piq.ssim` compute with their default
                           arguments on the reference's validation tensors; it is not a recording of them.
  chain32(sr, hr, ...)     the same statement op for op in float32 torch, where the inputs live (the GPU tests run it on the
                           device): the framework chain whose own error sets the bar
  direct64(sr, hr, ...)    the header's definition written out a second time in numpy float64 (block means, sliding windows and
                           an einsum where the restatement has avg_pool2d and conv2d): the second opinion on the yardstick
  within_bar(v, v32, v64)  |v - v64| <= 4 |v_chain32 - v64| + 8 ulp32(v64)  (the factor of DESIGN section 15, unchanged)

No kernel is involved in any of them."""
import math

import torch
import torch.nn.functional as F

MARGIN = 4.0
C1, C2 = 0.01 ** 2, 0.03 ** 2
LUMA = (65.738, 129.057, 25.064)


def pool_factor(h, w):
    return max(1, round(min(h, w) / 256))


def gaussian_window(dtype, device="cpu"):
    """The 11 x 11 window, sigma 1.5, normalised to sum 1, built in `dtype` as a metrics library builds it."""
    c = torch.arange(11, dtype=dtype, device=device) - 5
    g = c ** 2
    g = (-(g[None] + g[:, None]) / (2 * 1.5 ** 2)).exp()
    return g / g.sum()


def to_luminance(t):
    """transforms.py:389-391: float32 coefficients / 256, mul and sum over the channel dimension."""
    coeffs = (torch.tensor(LUMA, dtype=torch.float32).reshape(1, 3, 1, 1) / 256).to(device=t.device, dtype=t.dtype)
    return t.mul(coeffs).sum(dim=1, keepdim=True)


def _statement(s, h, sr_div, luminance, pool=None):
    """-> (psnr[N], ssim[N], l1) in the dtype of s and h; pool = None: the reference's pool factor of the image size."""
    sp = s / sr_div
    l1 = (sp - h).abs().mean()
    x, y = sp.clamp(0, 1), h
    if luminance:
        x, y = to_luminance(x), to_luminance(y)
    mse = ((x - y) ** 2).mean(dim=[1, 2, 3])
    psnr = -10 * torch.log10(mse + 1e-8)
    f = pool_factor(x.shape[-2], x.shape[-1]) if pool is None else int(pool)
    if f > 1:
        x, y = F.avg_pool2d(x, f), F.avg_pool2d(y, f)
    p = x.shape[1]
    k = gaussian_window(x.dtype, x.device)[None, None].repeat(p, 1, 1, 1)
    mx, my = F.conv2d(x, k, groups=p), F.conv2d(y, k, groups=p)
    mxx, myy, mxy = mx ** 2, my ** 2, mx * my
    sxx = F.conv2d(x ** 2, k, groups=p) - mxx
    syy = F.conv2d(y ** 2, k, groups=p) - myy
    sxy = F.conv2d(x * y, k, groups=p) - mxy
    cs = (2 * sxy + C2) / (sxx + syy + C2)
    ss = (2 * mxy + C1) / (mxx + myy + C1) * cs
    return psnr, ss.mean(dim=(-1, -2)).mean(1), l1


def restate64(sr, hr, sr_div=1.0, luminance=True, pool=None):
    with torch.no_grad():
        return _statement(sr.detach().double().cpu(), hr.detach().double().cpu(), float(sr_div), luminance, pool)


def chain32(sr, hr, sr_div=1.0, luminance=True, pool=None):
    with torch.no_grad():
        return _statement(sr.detach().float(), hr.detach().float(), float(sr_div), luminance, pool)


def direct64(sr, hr, sr_div=1.0, luminance=True, pool=None):
    """The definition of include/mhaq_fq.h once more, in numpy float64 and line by line, sharing no code with `_statement`:
    no convolution, no pooling op, no torch arithmetic.  -> (psnr[N], ssim[N], l1) as float64 numpy."""
    import numpy as np
    from numpy.lib.stride_tricks import sliding_window_view
    s = sr.detach().cpu().double().numpy()
    h = hr.detach().cpu().double().numpy()
    n, c, hh, ww = s.shape
    sp = s / float(sr_div)                                              # s' = s / sr_div
    l1 = np.abs(sp - h).mean()                                          # l1 = mean |s' - h|, unclamped
    x = np.where(sp < 0.0, 0.0, np.where(sp > 1.0, 1.0, sp))            # s'' = clamp(s', 0, 1): a NaN fails both tests
    y = h                                                               # h is not clamped
    if luminance:
        k = (np.array([65.738, 129.057, 25.064], dtype=np.float32) / np.float32(256)).astype(np.float64)
        x = ((x[:, 0] * k[0] + x[:, 1] * k[1]) + x[:, 2] * k[2])[:, None]
        y = ((y[:, 0] * k[0] + y[:, 1] * k[1]) + y[:, 2] * k[2])[:, None]
    p = x.shape[1]
    psnr = -10.0 * np.log10(((x - y) ** 2).reshape(n, -1).mean(axis=1) + 1e-8)     # every pixel of the P planes
    f = max(1, round(min(hh, ww) / 256)) if pool is None else int(pool)
    hp, wp = hh // f, ww // f
    if f > 1:                                                           # floor mode: a crop, then f x f block means
        x = x[:, :, :hp * f, :wp * f].reshape(n, p, hp, f, wp, f).mean(axis=(3, 5))
        y = y[:, :, :hp * f, :wp * f].reshape(n, p, hp, f, wp, f).mean(axis=(3, 5))
    taps = [math.exp(-((i - 5) ** 2) / (2.0 * 1.5 * 1.5)) for i in range(11)]
    total = sum(taps)
    taps = [t / total for t in taps]
    win = np.outer(np.array(taps), np.array(taps))                      # G: sums to 1

    def filt(q):                                                        # G * q without padding: [n][p][hp - 10][wp - 10]
        return np.einsum("npijab,ab->npij", sliding_window_view(q, (11, 11), axis=(2, 3)), win)

    mx, my = filt(x), filt(y)
    sxx = filt(x * x) - mx * mx
    syy = filt(y * y) - my * my
    sxy = filt(x * y) - mx * my
    c1, c2 = 1e-4, 9e-4
    cs = (2.0 * sxy + c2) / (sxx + syy + c2)
    ss = (2.0 * mx * my + c1) / (mx * mx + my * my + c1) * cs
    assert ss.shape == (n, p, hp - 10, wp - 10)
    return psnr, ss.reshape(n, -1).mean(axis=1), l1


def ulp32(v):
    v = abs(float(v))
    if v == 0.0 or not math.isfinite(v):
        return 2.0 ** -149
    return max(2.0 ** (math.floor(math.log2(v)) - 23), 2.0 ** -149)


def within_bar(v, v32, v64, margin=MARGIN):
    """-> (ok, fraction of the bar used) for one scalar."""
    err = abs(float(v) - float(v64))
    bar = margin * abs(float(v32) - float(v64)) + 8 * ulp32(v64)
    return err <= bar, err / bar


def check_record(rec, chain, ref, label=""):
    """rec = (psnr[N], ssim[N], l1) of the code under test; every image's PSNR and SSIM and l1 against the bar.
    -> the largest fraction of the bar used per quantity (printed before anything is asserted)."""
    worst = {}
    bad = []
    for name, v, c, r in zip(("psnr", "ssim", "l1"), rec, chain, ref):
        v, c, r = (t.detach().double().cpu().reshape(-1) for t in (v, c, r))
        fr = []
        for i in range(v.numel()):
            ok, frac = within_bar(v[i], c[i], r[i])
            fr.append(frac)
            if not ok:
                bad.append((name, i, float(v[i]), float(c[i]), float(r[i]), frac))
        worst[name] = max(fr)
    print(f"sr_metrics bar {label}: " + ", ".join(f"{k} {w:.3f}" for k, w in worst.items()))
    assert not bad, f"{label}: outside the bar (name, image, value, chain32, fp64, fraction): {bad}"
    return worst


def images(n, c, h, w, noise=0.05, seed=0, flat=None):
    """Seeded smooth-plus-noise target in [0, 1] and a prediction = target + noise (unclamped), float32 on the CPU."""
    gen = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 6, h), torch.linspace(0, 6, w), indexing="ij")
    base = torch.stack([0.5 + 0.4 * torch.sin(xx * (i + 1)) * torch.cos(yy * (2 - i * 0.5)) for i in range(c)])
    hr = (base[None].repeat(n, 1, 1, 1) + 0.05 * torch.randn(n, c, h, w, generator=gen)).clamp(0, 1)
    if flat is not None:
        hr = torch.full((n, c, h, w), float(flat))
    sr = hr + noise * torch.randn(n, c, h, w, generator=gen)
    return sr, hr
