// GBDT forest prediction: every row walks all the trees of a chunk of the
// packed forest (csrc/host/gbdt_forest_plan.h) in one launch.
//   gbdt_predict_forest      dense rows, raw fp32 X [n, f], NaN = missing
//   gbdt_predict_forest_csr  CSR rows, an absent feature = missing
// A block copies the chunk's nodes into LDS once and stays persistent over
// the row tiles, one row per lane; a chunk that is a single tree larger than
// the LDS capacity is walked from global memory. The row itself stays in
// global memory (f is unbounded; a row's few cache lines stay resident across
// the chunk's trees). Output: margins (one fp32 accumulator per lane and
// class, loaded from `out`, added to in tree order and stored back: the same
// additions in the same order as one gbdt_predict per tree) or leaf ids.
// The pack has checked every tree (children beyond their parent and inside
// the tree), so the walk ends at a leaf and needs no depth bound.
#include <algorithm>

#include "host/gbdt_forest_plan.h"
#include "wh_common.h"
#include "wh_kernels.h"

namespace wh {
namespace {

// One row per lane, 256 rows per block: every step of the walk gathers one
// feature value per lane from the lane's own row, so what a CU has in flight
// must stay in its caches across the chunk's trees. Measured on 11M x 28 with
// 16 full depth-8 trees per chunk (profiles/gbdt_forest_predict.txt): 256 to
// 512 rows in flight per CU are the fastest (0.26 ms per tree), 1024 cost
// 1.5x and 2048 3x that time (the rows evict each other), 128 and 64 cost
// 1.7x and 3.3x (too few waves to hide the dependent reads).
constexpr int kForestThreads = 256;
constexpr size_t kForestLdsMax = (size_t)kForestLdsNodes * sizeof(GbdtForestNode);

struct DenseRows {
  const float* __restrict__ X;
  int f;
  struct Row {
    const float* p;
  };
  __device__ Row row(int64_t i) const { return {X + i * f}; }
  __device__ bool go_left(const Row& r, int feat, float thr, bool defl) const {
    const float v = r.p[feat];
    return isnan(v) ? defl : v < thr;
  }
};

struct CsrRows {
  const int64_t* __restrict__ row_off;
  const int32_t* __restrict__ fid;  // ascending within a row
  const float* __restrict__ val;    // null: every stored entry is 1
  struct Row {
    int64_t lo, hi;
  };
  __device__ Row row(int64_t i) const { return {row_off[i], row_off[i + 1]}; }
  // a stored entry goes left iff v < thr, an absent one takes the default
  __device__ bool go_left(const Row& r, int feat, float thr, bool defl) const {
    int64_t lo = r.lo, hi = r.hi;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      const int x = fid[mid];
      if (x == feat) return (val ? val[mid] : 1.f) < thr;
      if (x < feat) lo = mid + 1;
      else hi = mid;
    }
    return defl;
  }
};

// the leaf a row ends in: its id within the tree, its value in *leaf
template <class Rows>
__device__ __forceinline__ int forest_walk(const Rows& rows, const typename Rows::Row& r,
                                           const uint4* tree, float* leaf) {
  int nd = 0;
  uint4 q = tree[0];
  while ((int)q.x >= 0) {
    const bool l = rows.go_left(r, (int)(q.x >> 1), __uint_as_float(q.y), (q.x & 1u) != 0);
    nd = (int)(l ? q.z : q.w);
    q = tree[nd];
  }
  *leaf = __uint_as_float(q.y);
  return nd;
}

// toff: the chunk's slice of tree_off; nodes: the chunk's nnode nodes, the
// first of them node nb of the table. Margins: out [K rows of out_stride],
// tree t adds to class t % K. Leaf ids: leaf_out [n, T].
template <class Rows, bool kLds, bool kLeafIds>
__global__ __launch_bounds__(kForestThreads) void k_forest(
    Rows rows, int64_t n, const uint4* __restrict__ nodes, const int32_t* __restrict__ toff,
    int nb, int nnode, int first_tree, int ntree, int K, float* __restrict__ out,
    int64_t out_stride, int32_t* __restrict__ leaf_out, int T) {
  extern __shared__ __attribute__((aligned(16))) uint4 forest_lds[];
  const uint4* table = nodes;
  if constexpr (kLds) {
    for (int j = threadIdx.x; j < nnode; j += blockDim.x) forest_lds[j] = nodes[j];
    __syncthreads();
    table = forest_lds;
  }
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
    const typename Rows::Row r = rows.row(i);
    float leaf;
    if constexpr (kLeafIds) {
      for (int t = 0; t < ntree; ++t)
        leaf_out[i * T + first_tree + t] = forest_walk(rows, r, table + (toff[t] - nb), &leaf);
    } else {
      // class by class: one accumulator at a time, its trees in tree order
      for (int k = 0; k < K; ++k) {
        const int t0 = (k - first_tree % K + K) % K;  // the chunk's first tree of class k
        if (t0 >= ntree) continue;
        float acc = out[k * out_stride + i];
        for (int t = t0; t < ntree; t += K) {
          forest_walk(rows, r, table + (toff[t] - nb), &leaf);
          acc += leaf;
        }
        out[k * out_stride + i] = acc;
      }
    }
  }
}

int forest_cus() {  // of the current device
  int dev = 0, cus = 0;
  WH_HIP_CHECK(hipGetDevice(&dev));
  WH_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  return std::max(cus, 1);
}

template <class Rows>
void forest_launch(const Rows& rows, int64_t n, const ForestChunk& c, const ForestOut& o,
                   hipStream_t s) {
  if (n <= 0 || c.ntree <= 0) return;
  static bool attr = false;
  if (!attr) {  // dynamic LDS above 64 KB must be opted into per kernel
    const void* ks[2] = {(const void*)k_forest<Rows, true, false>,
                         (const void*)k_forest<Rows, true, true>};
    for (const void* k : ks)
      WH_HIP_CHECK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)kForestLdsMax));
    attr = true;
  }
  const size_t lds = c.in_lds ? (size_t)c.nnode * sizeof(GbdtForestNode) : 0;
  // persistent blocks: two per CU, one when the chunk takes more than half
  // the LDS (more rows in flight per CU only evict each other, see above)
  const int per_cu = lds > 80 * 1024 ? 1 : 2;
  const int grid = grid_for(n, kForestThreads, forest_cus() * per_cu);
  const bool ids = o.leaf != nullptr;
  auto kern = c.in_lds ? (ids ? k_forest<Rows, true, true> : k_forest<Rows, true, false>)
                       : (ids ? k_forest<Rows, false, true> : k_forest<Rows, false, false>);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kForestThreads), lds, s, rows, n,
                     reinterpret_cast<const uint4*>(c.nodes) + c.node_begin,
                     c.tree_off + c.first_tree, c.node_begin, c.nnode, c.first_tree, c.ntree,
                     o.K, o.margin, o.stride, o.leaf, o.T);
}

}  // namespace

void gbdt_predict_forest(const float* X, int64_t n, int f, const ForestChunk& c,
                         const ForestOut& o, hipStream_t s) {
  forest_launch(DenseRows{X, f}, n, c, o, s);
}

void gbdt_predict_forest_csr(const int64_t* row_off, const int32_t* fid, const float* val,
                             int64_t n, const ForestChunk& c, const ForestOut& o, hipStream_t s) {
  forest_launch(CsrRows{row_off, fid, val}, n, c, o, s);
}

}  // namespace wh
