"""Super-resolution validation: PSNR, SSIM and L1 of a batch in three HIP launches (csrc/sr_metrics.hip).

What the reference's SR validation step logs (vision_sr_module.py:151-167 -- the criterion on the raw prediction, then
`piq.psnr` and `piq.ssim` of the luminance of the clamped prediction and of the target) comes out of one call, with no
host synchronisation; the one host read is `check_sr_flags`.  DESIGN section 16 has the definitions (a restatement of
what those calls compute with their default arguments, not a recording) and the measurements.
"""
from __future__ import annotations

import torch

from . import _lib
from . import ops

FLAG_NONFINITE = 1     # a NaN or an infinity in the scaled prediction or the target
FLAG_TARGET_RANGE = 2  # a target plane value outside [0, 1]


def ssim_pool_factor(h: int, w: int) -> int:
    """The factor by which SSIM average-pools its inputs first: max(1, round(min(h, w) / 256)), python's round (halves
    go to the even neighbour: 640 -> 2, 641 -> 3, 384 -> 2, 383 -> 1)."""
    return max(1, round(min(int(h), int(w)) / 256))


def _input(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise _lib.MhaqFqError(f"{name} is on {t.device}: the SR metrics run only as HIP kernels on an MI355X "
                               "(no CPU fallback by design)")
    if t.dim() != 4:
        raise ValueError(f"{name} must be [N, C, H, W], got {tuple(t.shape)}")
    return t.detach().contiguous()


def sr_metrics(sr: torch.Tensor, hr: torch.Tensor, *, sr_div: float = 1.0, to_luminance: bool = True) -> dict:
    """PSNR, SSIM and L1 of a batch.  `sr` is the model output, `hr` the target, both [N, C, H, W] on the GPU, each
    float32, bfloat16 or float16.  Returns device tensors: `psnr` [N], `ssim` [N], `l1` (0-dim, mean |sr / sr_div - hr|,
    unclamped), `PSNR` and `SSIM` (0-dim batch means) and `flags` (one int32 word for check_sr_flags).  Nothing here
    waits for the device."""
    sr, hr = _input(sr, "sr"), _input(hr, "hr")
    pool = ssim_pool_factor(sr.shape[2], sr.shape[3])
    psnr, ssim, l1, mean, flags = ops.sr_metrics(sr, hr, sr_div, to_luminance, pool)
    return {"psnr": psnr, "ssim": ssim, "l1": l1[0], "PSNR": mean[0], "SSIM": mean[1], "flags": flags}


def check_sr_flags(flags: torch.Tensor, nonfinite: bool = False) -> int:
    """The one host read of a metrics record: raises AssertionError when a target value lay outside [0, 1] (the inputs a
    metrics library refuses) and, only if `nonfinite` is set, FloatingPointError when a NaN or an infinity was seen.
    Returns the flag word."""
    word = int(flags.reshape(-1)[0].item())
    if word & FLAG_TARGET_RANGE:
        raise AssertionError("Expected values to be greater or equal than 0 and lower or equal than 1 in the target "
                             "(data_range 1.0): a target plane value lies outside [0, 1]")
    if nonfinite and word & FLAG_NONFINITE:
        raise FloatingPointError("a NaN or an infinity in the scaled prediction or in the target")
    return word


class SRValidationMeter:
    """Per-dataset sums and counts of PSNR and SSIM over the validation batches, kept as device tensors (`update` never
    waits for the device), and the reference's `PSNR/Weighted_mean` (`_log_weighted_psnr`: the per-dataset means
    weighted by 1 / count; batches without a dataset name do not enter it)."""

    def __init__(self):
        self._sums = {}      # name -> [2] tensor: sum of PSNR * batch_size, of SSIM * batch_size
        self._counts = {}

    def reset(self) -> None:
        self._sums.clear()
        self._counts.clear()

    def update(self, name, rec: dict, batch_size: int) -> None:
        v = torch.stack([rec["PSNR"].detach(), rec["SSIM"].detach()]).double() * float(batch_size)
        if name in self._sums:
            self._sums[name] = self._sums[name] + v
            self._counts[name] += int(batch_size)
        else:
            self._sums[name] = v
            self._counts[name] = int(batch_size)

    def compute(self) -> dict:
        out = {}
        wsum, wtot = None, 0.0
        for name, s in self._sums.items():
            cnt = self._counts[name]
            if cnt == 0:
                continue
            avg = s / float(cnt)
            out[f"PSNR/{name}"] = avg[0]
            out[f"SSIM/{name}"] = avg[1]
            if not name:
                continue
            wgt = 1.0 / cnt
            wsum = avg[0] * wgt if wsum is None else wsum + avg[0] * wgt
            wtot += wgt
        if wtot > 0:
            out["PSNR/Weighted_mean"] = wsum / wtot
        return out
