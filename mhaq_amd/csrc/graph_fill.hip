// mhaq_fq_graph_memsets_to_kernels (include/mhaq_fq.h): every memset node of a captured hipGraph becomes a kernel node
// that stores the same bytes.
//
// A workaround for the replay of memset nodes in the HIP runtime.  A training step captured under torch.autocast holds
// memset nodes the project never asked for: MIOpen's 16-bit backward-data convolutions clear their output with
// hipMemsetAsync before the kernel that accumulates into it (14 such nodes in the bf16 ResNet-20 step, one linear chain with
// its 724 kernel nodes and 2 copies).  On some MI355X hosts replays of that graph do not repeat the eager step: gradients
// differ at the second replay -- first those of the layers in front of such a convolution, in a few channels -- and are NaN
// at the third.  Established by running the same capture twice in one build: with its memset nodes the trajectory leaves the
// eager one as described, with the nodes replaced all eight steps equal the eager ones bit for bit.  The distillation step
// (teacher on a second stream, so a graph with a fork) has the same memsets and replayed correctly either way; only the
// single-chain graph went wrong.  Why the runtime mishandles the node there has not been found -- nothing in this project
// touches it.  A kernel node in the same place, with the memset's dependencies and dependents, is a launch like every other
// one of the step.
//
// The fill kernel writes the memset's pattern as 16-byte vectors over the aligned body of each row and as bytes over the up
// to 15 bytes in front of and behind it: every byte of [dst + row * pitch, + width * elementSize) and no other.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/mhaq_fq.h"
#include "fq_common.hpp"

namespace mhaq {

constexpr unsigned kFillMaxRows = 65535;      // grid.y

// `word`: the 32-bit word that an ALIGNED 4-byte store of the pattern writes.  Rows start at a multiple of the element size
// (checked on the host), so the byte at address a is byte (a & 3) of that word wherever the row starts.
__device__ __forceinline__ uint8_t fill_byte(uint32_t word, const uint8_t* p) {
  return (uint8_t)(word >> (8u * (unsigned)(reinterpret_cast<uintptr_t>(p) & 3u)));
}

__global__ __launch_bounds__(kBlock) void graph_fill_kernel(uint8_t* __restrict__ dst, size_t pitch, size_t row_bytes,
                                                            size_t height, uint32_t word) {
  for (size_t row = blockIdx.y; row < height; row += gridDim.y) {
    uint8_t* r = dst + row * pitch;
    size_t head = (size_t)((0 - reinterpret_cast<uintptr_t>(r)) & 15u);      // bytes up to the first 16-byte boundary
    if (head > row_bytes) head = row_bytes;
    const size_t nvec = (row_bytes - head) >> 4;
    uint4* body = reinterpret_cast<uint4*>(r + head);
    const uint4 w4 = make_uint4(word, word, word, word);
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < nvec; i += (size_t)gridDim.x * kBlock) body[i] = w4;
    if (blockIdx.x == 0) {
      const size_t tail0 = head + (nvec << 4), t = threadIdx.x;              // row_bytes - tail0 < 16
      if (t < head) r[t] = fill_byte(word, r + t);
      if (t < row_bytes - tail0) r[tail0 + t] = fill_byte(word, r + tail0 + t);
    }
  }
}

inline bool fill_word(unsigned element_size, unsigned value, uint32_t* word) {
  switch (element_size) {
    case 1: *word = (value & 0xffu) * 0x01010101u; return true;
    case 2: *word = (value & 0xffffu) * 0x00010001u; return true;
    case 4: *word = value; return true;
    default: return false;
  }
}

#define MHAQ_HIP_TRY(call)                      \
  do {                                          \
    const hipError_t e_ = (call);               \
    if (e_ != hipSuccess) return (int)e_;       \
  } while (0)

// One memset node -> one kernel node (an empty node for a memset of no bytes) with the same edges; the memset node is
// destroyed and *replaced set.  A node whose parameters the fill kernel does not serve is left as it is.
inline int replace_memset_node(hipGraph_t graph, hipGraphNode_t node, bool* replaced) {
  *replaced = false;
  hipMemsetParams mp;
  MHAQ_HIP_TRY(hipGraphMemsetNodeGetParams(node, &mp));
  uint32_t word = 0;
  if (!fill_word(mp.elementSize, mp.value, &word)) return 0;
  const size_t row_bytes = mp.width * (size_t)mp.elementSize, height = mp.height;
  const bool empty = row_bytes == 0 || height == 0;
  if (!empty) {
    if (!mp.dst || (height > 1 && mp.pitch < row_bytes)) return 0;
    const uintptr_t a = reinterpret_cast<uintptr_t>(mp.dst);
    if (a % mp.elementSize != 0 || (height > 1 && mp.pitch % mp.elementSize != 0)) return 0;
  }
  size_t nin = 0, nout = 0;
  MHAQ_HIP_TRY(hipGraphNodeGetDependencies(node, nullptr, &nin));
  MHAQ_HIP_TRY(hipGraphNodeGetDependentNodes(node, nullptr, &nout));
  std::vector<hipGraphNode_t> in(nin), out(nout);
  if (nin) MHAQ_HIP_TRY(hipGraphNodeGetDependencies(node, in.data(), &nin));
  if (nout) MHAQ_HIP_TRY(hipGraphNodeGetDependentNodes(node, out.data(), &nout));
  hipGraphNode_t fresh = nullptr;
  if (empty) {
    MHAQ_HIP_TRY(hipGraphAddEmptyNode(&fresh, graph, in.data(), nin));
  } else {
    uint8_t* dst = static_cast<uint8_t*>(mp.dst);
    size_t pitch = height > 1 ? mp.pitch : row_bytes, rb = row_bytes, h = height;
    void* args[] = {&dst, &pitch, &rb, &h, &word};
    size_t gx = ((row_bytes >> 4) + kBlock - 1) / kBlock;
    if (gx < 1) gx = 1;
    if (gx > (size_t)kMaxBlocks) gx = kMaxBlocks;
    hipKernelNodeParams kp = {};
    kp.func = reinterpret_cast<void*>(graph_fill_kernel);
    kp.gridDim = dim3((unsigned)gx, (unsigned)(height < kFillMaxRows ? height : kFillMaxRows), 1);
    kp.blockDim = dim3(kBlock, 1, 1);
    kp.sharedMemBytes = 0;
    kp.kernelParams = args;
    kp.extra = nullptr;
    MHAQ_HIP_TRY(hipGraphAddKernelNode(&fresh, graph, in.data(), nin, &kp));
  }
  for (size_t j = 0; j < nout; ++j) MHAQ_HIP_TRY(hipGraphAddDependencies(graph, &fresh, &out[j], 1));
  MHAQ_HIP_TRY(hipGraphDestroyNode(node));
  *replaced = true;
  return 0;
}

}  // namespace mhaq

using namespace mhaq;

extern "C" {

int mhaq_fq_graph_memsets_to_kernels(void* graph, int32_t* replaced_out, int32_t* left_out) {
  if (replaced_out) *replaced_out = 0;
  if (left_out) *left_out = 0;
  if (!graph) return MHAQ_FQ_EINVAL;
  hipGraph_t g = static_cast<hipGraph_t>(graph);
  size_t n = 0;
  MHAQ_HIP_TRY(hipGraphGetNodes(g, nullptr, &n));
  std::vector<hipGraphNode_t> nodes(n);
  if (n) MHAQ_HIP_TRY(hipGraphGetNodes(g, nodes.data(), &n));
  for (size_t i = 0; i < n; ++i) {
    hipGraphNodeType type;
    MHAQ_HIP_TRY(hipGraphNodeGetType(nodes[i], &type));
    if (type != hipGraphNodeTypeMemset) continue;
    bool done = false;
    const int rc = replace_memset_node(g, nodes[i], &done);
    if (rc) return rc;
    if (int32_t* count = done ? replaced_out : left_out) ++*count;
  }
  return 0;
}

}  // extern "C"
