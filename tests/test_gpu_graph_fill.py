"""mhaq_fq_graph_memsets_to_kernels (csrc/graph_fill.hip): the memset nodes of a captured hipGraph become launches of the
fill kernel.  GPU (-m gpu): memsets of every element size, at odd addresses and sizes, one row and pitched, are captured,
replaced BEFORE the graph is instantiated (no memset node is ever replayed), and several replays must leave exactly the bytes
the memsets define -- and no other byte.  CPU: the argument check."""
import ctypes

import pytest
import torch

DEV = "cuda:0"
FILL = 0xA5                      # what the buffer holds before every replay


def test_a_null_graph_is_an_argument_error():
    from mhaq_amd import _lib
    n, left = ctypes.c_int32(7), ctypes.c_int32(7)
    assert _lib.lib().mhaq_fq_graph_memsets_to_kernels(None, ctypes.byref(n), ctypes.byref(left)) == -1
    assert n.value == 0 and left.value == 0           # both words are written in every case
    assert _lib.lib().mhaq_fq_graph_memsets_to_kernels(None, None, None) == -1


def _hip():
    hip = ctypes.CDLL("libamdhip64.so")
    vp, sz, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    for name, args in (("hipMemsetAsync", [vp, i, sz, vp]), ("hipMemsetD16Async", [vp, ctypes.c_ushort, sz, vp]),
                       ("hipMemsetD32Async", [vp, i, sz, vp]), ("hipMemset2DAsync", [vp, sz, i, sz, sz, vp])):
        fn = getattr(hip, name)
        fn.argtypes, fn.restype = args, i
    return hip


# (kind, byte offset of the destination in the buffer, count, value): count is bytes / 16-bit words / 32-bit words
CASES_1D = [
    ("d8", 3, 1, 0x22),                       # one byte at an odd address
    ("d8", 64 + 5, 6, 0x33),                  # head only: ends before the first 16-byte boundary
    ("d8", 128 + 1, 15 + 16 + 7, 0x44),       # head, one vector, tail
    ("d8", 256, 16, 0x55),                    # exactly one aligned vector
    ("d8", 512 + 15, 4099, 0x00),             # many vectors from an odd address: zero, as MIOpen's clears
    ("d16", 8192 + 2, 1, 0xBEEF),             # one 16-bit word, not 4-byte aligned
    ("d16", 8192 + 64 + 6, 1001, 0x1234),     # the pattern's phase at a 2 (mod 4) address
    ("d32", 16384 + 4, 3, 0xDEADBEEF),        # head only
    ("d32", 16384 + 64 + 12, 777, 0x01020304),
    # 9 MiB: more 16-byte vectors than the grid's 2048 blocks x 256 threads hold, so the grid-stride loop goes round again
    ("d8", 32768 + 7, (9 << 20) + 5, 0x7E),
]
# hipMemset2DAsync(dst, pitch, value, width, height): (offset, pitch, width, height, value); the last one has more rows than
# grid.y holds (65535), so the kernel's row loop goes round again
B2 = 10 << 20
CASES_2D = [(B2, 40, 33, 9, 0x66), (B2 + 4096 + 3, 1000, 1000, 3, 0x77), (B2 + 16384 + 1, 64, 17, 300, 0x88),
            (B2 + 65536 + 5, 8, 5, 70000, 0x99)]
NBYTES = 11 << 20


def _expected():
    want = torch.full((NBYTES,), FILL, dtype=torch.uint8)
    for kind, off, count, value in CASES_1D:
        if kind == "d8":
            want[off:off + count] = value
        elif kind == "d16":
            want[off:off + 2 * count] = torch.tensor([value & 0xff, value >> 8], dtype=torch.uint8).repeat(count)
        else:
            want[off:off + 4 * count] = torch.tensor([(value >> (8 * k)) & 0xff for k in range(4)],
                                                     dtype=torch.uint8).repeat(count)
    for off, pitch, width, height, value in CASES_2D:
        want[off:off + height * pitch].view(height, pitch)[:, :width] = value
    return want


@pytest.mark.gpu
def test_replaced_memsets_write_their_bytes_and_no_others_on_every_replay():
    from mhaq_amd import ops
    hip = _hip()
    buf = torch.full((NBYTES,), FILL, dtype=torch.uint8, device=DEV)
    marker = torch.zeros(1, dtype=torch.int64, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, stream=side):
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        base = buf.data_ptr()
        marker.add_(1)                                  # kernel nodes in front of, between and behind the memsets
        for kind, off, count, value in CASES_1D:
            fn = {"d8": hip.hipMemsetAsync, "d16": hip.hipMemsetD16Async, "d32": hip.hipMemsetD32Async}[kind]
            # hipMemsetD32Async takes a C int: the same 32 bits
            v = value - (1 << 32) if kind == "d32" and value >= 1 << 31 else value
            assert fn(ctypes.c_void_p(base + off), v, count, st) == 0, (kind, off, count)
            marker.add_(1)
        for off, pitch, width, height, value in CASES_2D:
            assert hip.hipMemset2DAsync(ctypes.c_void_p(base + off), pitch, value, width, height, st) == 0
        marker.add_(1)
    n_memsets = len(CASES_1D) + len(CASES_2D)
    assert ops.graph_memsets_to_kernels(graph) == (n_memsets, 0)
    assert ops.graph_memsets_to_kernels(graph) == (0, 0)     # the graph that is instantiated holds no memset node
    graph.instantiate()
    want = _expected()
    for k in range(4):
        buf.fill_(FILL)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(buf.cpu(), want), k
        assert int(marker) == (k + 1) * (len(CASES_1D) + 2)       # every other node still runs, once per replay
