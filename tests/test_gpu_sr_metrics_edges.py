"""GPU (-m gpu): the paths of csrc/sr_metrics.hip that tests/test_gpu_sr_metrics.py leaves unexecuted, through the C ABI.
  a. a pool factor passed explicitly, so that a pooled image is wider than one column chunk (the DIV2K path: f = 5 on a
     2040-wide image is a chunk of 1200 pixels and two chunks), a last chunk narrower than f, factors whose lcm(8, f) is
     neither 8 nor f, the 49152-byte LDS stage, and an image 11 wide and 300 tall;
  b. batches over 4 images (the finalize's wave takes images w, w + 4, ...; its threads images t, t + 256, ...);
  c. input bases that are not 16-byte aligned, and the pairings of element types that were never passed;
  d. the flag word: OR-ed into a non-zero word, and set from the target, from a dropped row, from a chunk's partial item and
     from an image of a wave's second trip.
The accuracy bar is the one of tests/test_gpu_sr_metrics.py (R.check_record, margin 4), chain32 and restate64 taking the same
pool.  Every call here starts from a workspace full of NaN: a read of a word the call did not write cannot hide in a value."""
import functools

import pytest
import torch

from tests import sr_metrics_ref as R
from tests.test_gpu_sr_metrics import DEV, _bits, capi

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")

# (n, c, h, w, luminance, f): what each reaches is in sr_geometry_replica's table of tests/test_sr_metrics_cpu.py
POOLED = [(1, 3, 57, 1257, True, 5),      # chunk 1200 + 57: two chunks, rows 55.. and columns 1255.. dropped
          (1, 3, 22, 2071, True, 2),      # chunk 2048 + 23
          (1, 3, 22, 2072, True, 2),      # the same with every row base 16-byte aligned
          (1, 3, 22, 2049, True, 2),      # a last chunk of 1 pixel: narrower than f, no pooled column
          (1, 1, 22, 2050, False, 2),     # c == 1 pooled, a last chunk of 2 pixels
          (1, 3, 35, 707, False, 3),      # three planes, chunk 672 + 35, 48384 bytes of LDS
          (1, 3, 44, 556, False, 4),      # chunk 512 + 44, 49152 bytes of LDS: the cap
          (2, 3, 55, 57, True, 5),        # unit 40, a band of 8 groups, the last band short
          (1, 1, 77, 83, False, 7),       # unit 56, a band of 4 groups
          (1, 3, 33, 34, True, 3),        # one workgroup holds all 11 groups
          (1, 3, 300, 11, True, 1)]       # ten tiles tall and one wide; two bands of 187 and 113 rows, two trips of the lanes
ids_pooled = lambda c: "%dx%dx%dx%d-%s-f%d" % (c[0], c[1], c[2], c[3], "lum" if c[4] else "planes", c[5])   # noqa: E731
BY_SIZE = {(c[2], c[3]): c for c in POOLED}


def call(sr, hr, **kw):
    kw.setdefault("ws_fill", NAN)
    return capi(sr, hr, **kw)


def same_bits(a, b, fields=(0, 1, 2, 3)):
    return all(torch.equal(_bits(a[i]), _bits(b[i])) for i in fields)


@functools.lru_cache(maxsize=None)
def _images(n, c, h, w, noise=0.05):
    """Inputs on the device, shared and never modified."""
    sr, hr = R.images(n, c, h, w, noise=noise, seed=100 * h + w + c)
    return sr.to(DEV), hr.to(DEV)


@functools.lru_cache(maxsize=None)
def _refs(n, c, h, w, lum, f):
    """-> (the framework chain on the device, the float64 restatement on the CPU), once per case."""
    sr, hr = _images(n, c, h, w)
    return R.chain32(sr, hr, luminance=lum, pool=f), R.restate64(sr, hr, luminance=lum, pool=f)


def check_means(mean, chain, ref):
    for k in (0, 1):
        ok, frac = R.within_bar(mean[k], chain[k].double().mean(), ref[k].mean())
        assert ok, (k, frac)


# ---------------------------------------------------------------------------------------------- a. explicit pool
@pytest.mark.parametrize("case", POOLED, ids=ids_pooled)
def test_explicit_pool_meets_the_bar_and_reads_nothing_stale(case):
    n, c, h, w, lum, f = case
    sr, hr = _images(n, c, h, w)
    chain, ref = _refs(*case)
    rec = call(sr, hr, luminance=lum, pool=f)
    R.check_record(rec[:3], chain, ref, "edges " + ids_pooled(case))
    check_means(rec[3], chain, ref)
    assert rec[4] == 0
    # a workspace full of NaN gives the bits of one full of -7: no word is read before it is written
    other = capi(sr, hr, luminance=lum, pool=f, ws_fill=-7)
    assert same_bits(rec, other) and other[4] == 0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_two_pooled_chunks_of_16_bit_rows(dtype):
    n, c, h, w, lum, f = BY_SIZE[(22, 2072)]
    sr, hr = _images(n, c, h, w)
    s16, h16 = sr.to(dtype), hr.to(dtype)
    rec = call(s16, h16, pool=f)
    assert same_bits(rec, call(s16.float(), h16.float(), pool=f)) and rec[4] == 0
    R.check_record(rec[:3], R.chain32(s16, h16, pool=f), R.restate64(s16, h16, pool=f), "edges 22x2072 " + str(dtype))


@pytest.mark.parametrize("size", [(22, 2049), (57, 1257)], ids=lambda s: "%dx%d" % s)
def test_what_the_pool_drops_in_the_second_chunk_counts_for_psnr_and_l1_only(size):
    n, c, h, w, lum, f = BY_SIZE[size]
    sr, hr = _images(n, c, h, w)
    psnr, ssim, l1, _, _ = call(sr, hr, pool=f)
    sr2 = sr.clone()
    sr2[:, :, (h // f) * f:, :] += 0.25                    # 57 x 1257: rows 55, 56; 22 x 2049: none
    sr2[:, :, :, (w // f) * f:] += 0.25                    # columns 1255, 1256; column 2048
    assert not torch.equal(sr2, sr)
    p2, s2, l2, _, fl = call(sr2, hr, pool=f)
    assert torch.equal(_bits(s2), _bits(ssim)) and fl == 0
    assert float(p2) < float(psnr) and float(l2) > float(l1)
    R.check_record((p2, s2, l2), R.chain32(sr2, hr, pool=f), R.restate64(sr2, hr, pool=f), "edges dropped %dx%d" % size)


# ---------------------------------------------------------------------------------------------- b. batches
@pytest.mark.parametrize("case", [(5, 3, 11, 11, True), (260, 3, 11, 11, True), (6, 1, 11, 13, False)],
                         ids=lambda c: "%dx%dx%dx%d" % c[:4])
def test_batches_over_four_images(case):
    n, c, h, w, lum = case
    sr, hr = _images(n, c, h, w)
    chain, ref = _refs(n, c, h, w, lum, 1)
    psnr, ssim, l1, mean, flags = call(sr, hr, luminance=lum)
    assert flags == 0
    # image i of the batch has the bits of a call on image i alone: its geometry does not depend on n
    for i in (0, 3, 4, 5, 255, 256, 259):
        if i < n:
            one = call(sr[i:i + 1].clone(), hr[i:i + 1].clone(), luminance=lum)
            assert torch.equal(_bits(one[0]), _bits(psnr[i:i + 1])) and torch.equal(_bits(one[1]), _bits(ssim[i:i + 1])), i
    R.check_record((psnr, ssim, l1), chain, ref, "edges batch %dx%dx%dx%d" % case[:4])
    # the batch means are the fp64 means of the fp64 per-image values, rounded once.  Against the fp64 mean of the RETURNED
    # fp32 values: each addend was rounded once (half an ulp of values of that size), the result once more (half an ulp)
    for k, v in ((0, psnr), (1, ssim)):
        m64 = float(v.double().cpu().mean())
        assert abs(float(mean[k]) - m64) <= 2 * R.ulp32(m64), (k, float(mean[k]), m64)


def test_in_a_batch_of_nine_a_nan_and_a_flag_stay_with_their_image():
    sr, hr = _images(9, 3, 11, 11)
    clean = call(sr, hr)
    assert clean[4] == 0 and bool(torch.isfinite(clean[0]).all()) and bool(torch.isfinite(clean[1]).all())
    bad = sr.clone()
    bad[5, 2, 6, 3] = NAN                                  # image 5: the second image of wave 1
    psnr, ssim, l1, mean, flags = call(bad, hr)
    assert flags == 1
    assert bool(torch.isnan(psnr[5])) and bool(torch.isnan(ssim[5])) and bool(torch.isnan(l1).all())
    assert bool(torch.isnan(mean).all())
    keep = [i for i in range(9) if i != 5]
    assert torch.equal(_bits(psnr[keep]), _bits(clean[0][keep])) and torch.equal(_bits(ssim[keep]), _bits(clean[1][keep]))
    hr2 = hr.clone()
    hr2[7, :, 2, 9] = 1.2                                  # image 7 alone, the second image of wave 3: luminance 1.03
    rec = call(sr, hr2)
    assert rec[4] == 2
    keep = [i for i in range(9) if i != 7]
    assert torch.equal(_bits(rec[0][keep]), _bits(clean[0][keep])) and torch.equal(_bits(rec[1][keep]), _bits(clean[1][keep]))


# ---------------------------------------------------------------------------------------------- c. alignment and types
PAIRS = [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.float32, torch.float16)]


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "-".join(str(d)[6:] for d in p))
@pytest.mark.parametrize("size", [(24, 40), (384, 392)], ids=lambda s: "%dx%d" % s)
def test_a_base_off_the_16_byte_grid_gives_the_bits_of_an_aligned_one(size, pair):
    """Rows of 40 and of 392 elements keep every row base on the 16-byte grid when the tensor starts there, so the aligned
    call takes the 16-byte loads; one element further no row base is on it and every item takes the element loads.  Both do
    the same arithmetic per pixel in the same order."""
    sr, hr = _images(1, 3, *size)
    s, h = sr.to(pair[0]), hr.to(pair[1])
    want = call(s, h)
    assert want[4] == 0 and bool(torch.isfinite(want[1]).all())
    for so, ho in ((1, 0), (0, 1), (1, 1)):
        got = call(s, h, sr_off=so, hr_off=ho)
        assert same_bits(got, want) and got[4] == 0, (so, ho)


@pytest.mark.parametrize("hdt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", [(1, 3, 24, 40), (2, 3, 24, 37)], ids=lambda s: "%dx%dx%dx%d" % s)
def test_fp32_prediction_with_a_16_bit_target(shape, hdt):
    sr, hr = _images(*shape)
    h16 = hr.to(hdt)
    got = call(sr, h16)
    assert same_bits(got, call(sr, h16.float())) and got[4] == 0


@pytest.mark.parametrize("shape", [(1, 1, 24, 40), (2, 1, 24, 37)], ids=lambda s: "%dx%dx%dx%d" % s)
def test_one_channel_of_bf16_elements(shape):
    sr, hr = _images(*shape)
    s16, h16 = sr.to(torch.bfloat16), hr.to(torch.bfloat16)
    got = call(s16, h16, luminance=False)
    assert same_bits(got, call(s16.float(), h16.float(), luminance=False)) and got[4] == 0
    R.check_record(got[:3], R.chain32(s16, h16, luminance=False), R.restate64(s16, h16, luminance=False),
                   "edges bf16 %dx%dx%dx%d" % shape)


# ---------------------------------------------------------------------------------------------- d. flags
def test_the_flag_word_is_ored_into():
    sr, hr = _images(2, 3, 24, 37)
    clean = call(sr, hr, flags_init=4)
    assert clean[4] == 4
    hr2 = hr.clone()
    hr2[1, :, 2, 2] = 1.2                                  # luminance 1.2 * 0.8588 = 1.03
    assert call(sr, hr2, flags_init=4)[4] == 6
    bad = sr.clone()
    bad[0, 1, 9, 17] = NAN
    assert call(bad, hr, flags_init=2)[4] == 3
    assert call(bad, hr, flags_init=1)[4] == 1 and call(sr, hr, flags_init=3)[4] == 3


def test_non_finite_values_in_the_target_and_a_negative_infinity():
    sr, hr = _images(2, 3, 24, 37)
    clean = call(sr, hr)
    hn = hr.clone()
    hn[1, 2, 20, 36] = NAN                                 # a NaN is neither below 0 nor above 1: bit 0 alone
    rec = call(sr, hn)
    assert rec[4] == 1 and bool(torch.isnan(rec[0][1])) and bool(torch.isnan(rec[1][1]))
    assert torch.equal(_bits(rec[0][:1]), _bits(clean[0][:1])) and torch.equal(_bits(rec[1][:1]), _bits(clean[1][:1]))
    hi = hr.clone()
    hi[0, :, 5, 8] = INF                                   # luminance +inf: not finite, and above 1
    assert call(sr, hi)[4] == 3
    sn = sr.clone()
    sn[1, 0, 23, 0] = -INF                                 # clamps to 0
    rec = call(sn, hr)
    assert rec[4] == 1 and bool(torch.isfinite(rec[0]).all()) and bool(torch.isfinite(rec[1]).all())
    assert torch.equal(_bits(rec[0][:1]), _bits(clean[0][:1])) and float(rec[0][1]) < float(clean[0][1])


def test_an_infinity_in_a_dropped_row_and_in_the_last_partial_item_of_the_second_chunk():
    n, c, h, w, lum, f = BY_SIZE[(57, 1257)]
    sr, hr = _images(n, c, h, w)
    clean = call(sr, hr, pool=f)
    for r, col in ((56, 600), (20, 1256)):                 # row 56: no pooled row; column 1256: item 7 of chunk 1, 1 pixel
        bad = sr.clone()
        bad[0, 1, r, col] = INF
        rec = call(bad, hr, pool=f)
        assert rec[4] == 1, (r, col)
        assert torch.equal(_bits(rec[1]), _bits(clean[1])), (r, col)
        assert bool(torch.isfinite(rec[0]).all()) and float(rec[0]) < float(clean[0])
