// DART dropout walk: every training row walks a chunk of selected trees of
// the bin-space tree table (csrc/host/gbdt_dart_plan.h) in one launch and
// adds coef[j] * leaf_j(row) to its accumulator, in list order.
//   gbdt_dart_walk  rows of the resident u8 bin matrix B [n, f], 255 = missing
// A block gathers the chunk's trees from their (non-contiguous) ranges of the
// table into LDS once and stays persistent over the row tiles; per tile it
// copies its rows of B into LDS once, coalesced, in dwords; each lane then
// walks every tree for its row from LDS alone. B is read once per chunk
// instead of once per tree. Same decisions as the partition and
// k_leaf_walk_lds (bin <= split bin; missing -> default direction).
// The accumulation is acc = out[i]; acc = acc + coef[j] * leaf for every tree
// in list order, the product and the sum each rounded to fp32 (no FMA
// contraction); one store. That is what adding a forest with leaves
// float32(coef) * float32(leaf) gives, so the result is bit-equal to the
// forest kernels on the same trees.
#include <algorithm>

#include "host/gbdt_dart_plan.h"
#include "wh_common.h"
#include "wh_kernels.h"

// The accumulation must stay a rounded product and a rounded sum. (HIP's
// __fmul_rn / __fadd_rn are inline * and + that carry the header's own
// contraction setting: the compiler fused them into v_fmac_f32. Plain
// operators under this pragma are not fused.)
#pragma clang fp contract(off)

namespace wh {
namespace {

constexpr uint32_t kMissingBin = 255;
constexpr int kDartLdsMax = 160 * 1024;

// LDS: meta [ntree] {table offset, nodes, staging offset, coef bits}, the
// chunk's nodes [nnode], then the tile's rows [blockDim.x * f bytes].
__global__ __launch_bounds__(1024) void k_dart_walk(
    const uint8_t* __restrict__ B, int64_t n, int f, const uint2* __restrict__ table,
    const uint4* __restrict__ meta, int ntree, int nnode, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint32_t dart_lds[];
  uint4* s_meta = reinterpret_cast<uint4*>(dart_lds);
  uint2* s_node = reinterpret_cast<uint2*>(dart_lds + 4 * ntree);
  uint8_t* rows = reinterpret_cast<uint8_t*>(dart_lds + 4 * ntree + 2 * nnode);
  const int R = blockDim.x;
  for (int j = threadIdx.x; j < ntree; j += R) s_meta[j] = meta[j];
  for (int j = 0; j < ntree; ++j) {  // (block-uniform reads: s_meta is not visible yet)
    const uint4 m = meta[j];
    const uint2* src = table + m.x;
    uint2* dst = s_node + m.z;
    for (int k = threadIdx.x; k < (int)m.y; k += R) dst[k] = src[k];
  }
  for (int64_t tile = blockIdx.x; tile * R < n; tile += gridDim.x) {
    const int64_t i0 = tile * R;
    const int nr = (int)min<int64_t>(R, n - i0);
    const int nbytes = nr * f;
    const uint8_t* src = B + i0 * f;  // 4-aligned: R % 4 == 0 and B is
    const int nw = nbytes >> 2;
    __syncthreads();  // (the trees on the first tile; the previous tile's rows after)
    for (int k = threadIdx.x; k < nw; k += R)
      reinterpret_cast<uint32_t*>(rows)[k] = reinterpret_cast<const uint32_t*>(src)[k];
    for (int k = 4 * nw + threadIdx.x; k < nbytes; k += R) rows[k] = src[k];
    __syncthreads();
    if ((int)threadIdx.x < nr) {
      const uint8_t* row = rows + threadIdx.x * f;
      float acc = out[i0 + threadIdx.x];
      for (int j = 0; j < ntree; ++j) {
        const uint4 m = s_meta[j];
        const uint2* tree = s_node + m.z;
        const uint32_t nn = m.y;
        uint2 t = tree[0];
        // bounded: at most kDartMaxDepth steps, no child id past the tree,
        // no feature past the row
        for (int d = 0; d < kDartMaxDepth; ++d) {
          const uint32_t ft = t.x & 0xffffu;
          if (ft >= (uint32_t)f) break;  // (a leaf: 0xffff)
          const uint32_t b = row[ft];
          const bool l = b == kMissingBin ? (t.x >> 24) != 0 : b <= ((t.x >> 16) & 255u);
          const uint32_t nx = l ? (t.y & 0xffffu) : (t.y >> 16);
          if (nx >= nn) break;
          t = tree[nx];
        }
        const float leaf = (t.x & 0xffffu) == kDartLeaf ? __uint_as_float(t.y) : 0.f;
        const float prod = __uint_as_float(m.w) * leaf;  // (rounded: contraction is off)
        acc = acc + prod;
      }
      out[i0 + threadIdx.x] = acc;
    }
  }
}

int dart_cus() {  // of the current device
  int dev = 0, cus = 0;
  WH_HIP_CHECK(hipGetDevice(&dev));
  WH_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  return std::max(cus, 1);
}

}  // namespace

size_t gbdt_dart_lds_bytes(int f, int ntree, int nnode, int rows) {
  return (size_t)ntree * 16 + (size_t)nnode * 8 + (((size_t)rows * f + 15) & ~(size_t)15);
}

int gbdt_dart_grid(int64_t n, int f, int ntree, int nnode, int rows) {
  // persistent blocks: as many per CU as its LDS and its 2048 lanes hold
  const size_t lds = gbdt_dart_lds_bytes(f, ntree, nnode, rows);
  const int per_cu = std::max(1, std::min<int>((int)(kDartLdsMax / std::max<size_t>(lds, 1)),
                                               2048 / rows));
  return grid_for(n, rows, dart_cus() * per_cu);
}

void gbdt_dart_walk(const uint8_t* B, int64_t n, int f, const void* table, const void* meta,
                    int ntree, int nnode, int rows, float* out, hipStream_t s) {
  if (n <= 0 || ntree <= 0) return;
  static bool attr = false;
  if (!attr) {  // dynamic LDS above 64 KB must be opted into per kernel
    WH_HIP_CHECK(hipFuncSetAttribute((const void*)k_dart_walk,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, kDartLdsMax));
    attr = true;
  }
  const size_t lds = gbdt_dart_lds_bytes(f, ntree, nnode, rows);
  hipLaunchKernelGGL(k_dart_walk, dim3(gbdt_dart_grid(n, f, ntree, nnode, rows)), dim3(rows), lds,
                     s, B, n, f, reinterpret_cast<const uint2*>(table),
                     reinterpret_cast<const uint4*>(meta), ntree, nnode, out);
}

}  // namespace wh
