"""GPU (-m gpu): the library's own sort of the detection candidates (mhaq_fq_od_sorted_keys / mhaq_fq_od_nms_rows,
csrc/od_sort.hip) against the numpy key formula and stable sort of tests/od_ref.py.  Keys and counts are integers: every
comparison is on bits.  T is the sort tile, 256 the anchor tile of the compaction; the shapes sit on their edges."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import od_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("det", "count", "n_candidates", "flags")


@functools.lru_cache(maxsize=None)
def tile():
    from mhaq_amd import ops
    return ops.od_sort_tile()


def planted(n, nc=80, A=100, seed=0, values=None):
    """One image [4 + nc, A] (numpy) with exactly n scores above 0.05, at random pairs; `values`: the scores to draw from."""
    g = np.random.default_rng(seed)
    img = np.zeros((4 + nc, A), np.float32)
    at = g.choice(nc * A, n, replace=False)
    img[4:].reshape(-1)[at] = g.random(n, dtype=np.float32) * 0.9 + 0.1 if values is None else g.choice(values, n)
    return img


def expected(pred, conf_thr, max_nms):
    """pred [B, 4 + nc, A] float32 numpy -> (skeys [B, K], n_cand [B]) of the contract."""
    B, nc, A = pred.shape[0], pred.shape[1] - 4, pred.shape[2]
    K = min(A * nc, max_nms)
    skeys, n_cand = np.full((B, K), R.NO_KEY, np.int64), np.zeros(B, np.int32)
    for b in range(B):
        a, c, s = R.sorted_candidates(pred[b], conf_thr)
        keys = ((np.int64(0x7FFFFFFF) - s.view(np.int32).astype(np.int64)) << np.int64(32)) | (a.astype(np.int64) * nc + c)
        n_cand[b] = keys.size
        skeys[b, :min(keys.size, K)] = keys[:K]
    return skeys, n_cand


def check_keys(pred, conf_thr=0.05, max_nms=30000):
    from mhaq_amd import ops
    pred = torch.as_tensor(pred)
    skeys, n_cand = ops.od_sorted_keys(pred.to(DEV), conf_thr, max_nms)
    want, n = expected(R.to_f32(pred), conf_thr, max_nms)
    assert skeys.dtype == torch.int64 and n_cand.dtype == torch.int32 and tuple(skeys.shape) == want.shape
    assert n_cand.cpu().tolist() == n.tolist()
    got = skeys.cpu().numpy()
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    return n


def raw_bits(nc, A, seed):
    """Scores from raw positive bit patterns (subnormals, every byte random, +inf), some NaNs and negative values."""
    g = np.random.default_rng(seed)
    img = np.zeros((4 + nc, A), np.float32)
    bits = g.integers(1, 0x7F800000, nc * A, dtype=np.int64, endpoint=True).astype(np.int32)
    bits[g.choice(nc * A, 40, replace=False)] = np.float32("nan").view(np.int32)
    bits[g.choice(nc * A, 40, replace=False)] |= np.int32(-2 ** 31)
    bits[:3] = [0x7F800000, 1, 0x007FFFFF]
    img[4:] = bits.view(np.float32).reshape(nc, A)
    return img


CASES = {f"count-{n}": lambda T, n=n: planted(eval(n, {"T": T}), seed=len(n))[None]
         for n in ("0", "1", "T-1", "T", "T+1", "3*T+5")}
CASES.update({f"A{A}-nc{nc}": lambda T, A=A, nc=nc: planted((A * nc + 1) // 2, nc, A, seed=A + nc)[None]
              for A in (1, 255, 256, 257, 600) for nc in (1, 3)})
CASES["mixed-counts"] = lambda T: np.stack([planted(0), planted(T + 1, seed=1), planted(8000, seed=2)])
CASES["ties"] = lambda T: planted(3 * T + 5, seed=3, values=np.float32([0.2, 0.5, 0.5000001, 0.7, 1.0]))[None]
CASES["bf16"] = lambda T: R.random_pred(2, 3, 700, seed=4).to(torch.bfloat16)
CASES["fp16"] = lambda T: R.random_pred(2, 3, 700, seed=5).to(torch.float16)


@pytest.mark.parametrize("case", list(CASES))
def test_sorted_keys_and_counts_equal_the_sorted_rows_of_od_keys(case):
    pred = CASES[case](tile())
    n = check_keys(pred)
    if case == "mixed-counts":
        assert n.tolist() == [0, tile() + 1, 8000]


def test_raw_score_bit_patterns_go_through_all_four_digit_passes():
    pred = raw_bits(3, 1500, seed=6)[None]
    n = check_keys(pred, conf_thr=0.0)
    assert 4 * tile() < int(n[0]) < 3 * 1500 - 30             # the NaNs and the negative values are no candidates


@pytest.mark.parametrize("max_nms", ["1", "T", "n-1", "n", "n+1"])
def test_the_row_is_cut_to_max_nms_and_the_count_is_not(max_nms):
    T = tile()
    n = 2 * T + 7
    n_cand = check_keys(planted(n, seed=7)[None], max_nms=eval(max_nms, {"T": T, "n": n}))
    assert int(n_cand[0]) == n


def _bits(t):
    if t.is_floating_point():
        t = torch.where(torch.isnan(t), torch.full_like(t, float("nan")), t)
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("max_nms,flags", [(30000, 0), (300, 2)])
def test_the_whole_path_equals_the_oracle_and_the_torch_sort_path(max_nms, flags):
    from mhaq_amd.od_metrics import od_nms
    pred = R.random_pred(2, 3, 700, frac=0.5)
    ref = R.nms(R.to_f32(pred), conf_thr=0.05, max_nms=max_nms)
    lib = od_nms(pred.to(DEV), conf_thr=0.05, max_nms=max_nms, sort="lib")
    old = od_nms(pred.to(DEV), conf_thr=0.05, max_nms=max_nms, sort="torch")
    assert ref["flags"] == flags and int(ref["n_cand"].min()) > 300
    assert torch.equal(_bits(lib["det"]).cpu(), _bits(torch.from_numpy(ref["det"])))
    assert lib["count"].cpu().tolist() == ref["count"].tolist() and int(lib["flags"].item()) == flags
    assert lib["n_candidates"].cpu().tolist() == ref["n_cand"].tolist()
    for k in KEYS:
        assert torch.equal(_bits(lib[k]), _bits(old[k])), k


def test_a_captured_lib_sort_chain_replays_the_eager_bits_twice():
    from mhaq_amd.od_metrics import od_nms
    run = lambda p: od_nms(p, conf_thr=0.05, sort="lib")      # noqa: E731
    pred = R.random_pred(2, 3, 700, seed=8, frac=0.5).to(DEV)
    others = [R.random_pred(2, 3, 700, seed=s, frac=0.5).to(DEV) for s in (9, 10)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                # warm-up on the side stream: the workspace is allocated here
        run(pred)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run(pred)
    for other in others:
        pred.copy_(other)
        graph.replay()
        torch.cuda.synchronize()
        eager = run(other)
        for k in KEYS:
            assert torch.equal(_bits(captured[k]), _bits(eager[k])), k
    assert int(captured["count"].min()) > 0


def test_nothing_is_written_outside_the_outputs_and_the_workspace():
    from mhaq_amd import _lib
    L = _lib.lib()
    T = tile()
    B, nc, A, max_nms, band = 2, 3, 700, T + 9, 64
    pred = np.stack([planted(T + 40, nc, A, seed=11), planted(5, nc, A, seed=12)])
    dev = torch.from_numpy(pred).to(DEV)
    nb = L.mhaq_fq_od_sorted_keys_workspace_bytes(B, nc, A, max_nms)
    assert nb >= 2 * B * A * nc * 8 and nb % 8 == 0

    def banded(n, dtype):
        buf = torch.full((band + n + band,), 0x5A5A5A5A, dtype=dtype, device=DEV)
        return buf, buf[band:band + n]

    kbuf, skeys = banded(B * max_nms, torch.int64)
    nbuf, n_cand = banded(B, torch.int32)
    wbuf, ws = banded(nb // 8, torch.int64)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda nbytes: L.mhaq_fq_od_sorted_keys(dev.data_ptr(), 0, B, nc, A, 0.05, max_nms, skeys.data_ptr(),      # noqa: E731
                                                   n_cand.data_ptr(), ws.data_ptr(), nbytes, stream)
    assert call(nb - 8) == -2                                 # MHAQ_FQ_EWORKSPACE, before any launch
    assert call(nb) == 0
    torch.cuda.synchronize()
    for buf, n in ((kbuf, B * max_nms), (nbuf, B), (wbuf, nb // 8)):
        assert bool((buf[:band] == 0x5A5A5A5A).all()) and bool((buf[band + n:] == 0x5A5A5A5A).all())
    want, n = expected(pred, 0.05, max_nms)
    assert np.array_equal(skeys.cpu().numpy().reshape(B, max_nms), want) and n_cand.cpu().tolist() == n.tolist()
