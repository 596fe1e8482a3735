// GBDT per-feature contributions (pred_contribs / approx_contribs) of a packed
// forest, tables and plan from csrc/host/gbdt_shap_plan.h.
//   gbdt_shap, gbdt_shap_csr            exact TreeSHAP over one chunk of paths
//   gbdt_saabas, gbdt_saabas_csr        the Saabas attribution over the forest
// Exact: a lane group of W = 16, 32 or 64 lanes owns a row, one lane per path
// element (lane 0 is the dummy); the wave's groups take different rows and
// step through the chunk's paths together, the path table in LDS; a path's
// element and the row's feature value are fetched one path ahead. EXTEND
// shifts the path weights one lane up per element (a DPP wave shift; the
// element's z is broadcast with o in its sign), UNWOUND-SUM reads them back
// lane by lane; both are the statements of gbdt_shap_path<float> in the same
// order, without FMA contraction, so a row differs from the host fp32
// reference only by the order in which its paths are added. Blocks of 1024
// threads, two per CU while the LDS allows: the kernel is bound by its own
// instructions and wants every wave slot (profiles/gbdt_shap.txt). The lane that
// owns an element adds into the row's accumulator: an LDS tile [rows of the
// block][U + 1], added to `out` once per chunk, or, U + 1 above
// gbdt_shap_lds_cols(), the row's slice of `out` itself. A path's elements
// have distinct columns and a row's paths are taken in plan order by one
// group of one wave, so there are no atomics and a row's bits depend neither
// on n nor on the run.
// Saabas: one row per lane walks the forest with the table of expected
// values beside it and adds m(child) - m(node) into its own output row.
//   gbdt_shap_inter, gbdt_shap_inter_csr   pairwise interactions, one chunk
//   gbdt_shap_inter_out                    triangle and phi -> the matrices
// Interactions (pred_interactions): the exact kernel's structure once more,
// per path one EXTEND and UNWOUND-SUM for every element conditioned on, so
// about path length times its work. The packed triangles of a block's rows,
// U (U - 1) / 2 floats each, stay in LDS beside the path table up to
// gbdt_shap_inter_lds_cols() columns: the block is then as many whole waves,
// 1024 threads down to 704, as the chunk's table leaves room for (the
// arithmetic is in gbdt_shap_plan.h); above that a row accumulates in its own
// slice of the global scratch triangle. The epilogue mirrors the triangle,
// takes the diagonal from the exact kernel's phi and writes the bias row and
// column.
#include <algorithm>

#include "host/gbdt_shap_plan.h"
#include "wh_common.h"
#include "wh_kernels.h"

namespace wh {
namespace {

constexpr int kShapThreads = 1024;
constexpr int kShapBlocksPerCu = 2;
constexpr int kSaabasThreads = 256;

// value(): false for a missing value (NaN, or absent in CSR)
struct DenseRows {
  const float* __restrict__ X;
  int f;
  struct Row {
    const float* p;
  };
  __device__ Row row(int64_t i) const { return {X + i * f}; }
  __device__ bool value(const Row& r, int feat, float* v) const {
    *v = r.p[feat];
    return !isnan(*v);
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
  __device__ bool value(const Row& r, int feat, float* v) const {
    int64_t lo = r.lo, hi = r.hi;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      const int x = fid[mid];
      if (x == feat) {
        *v = val ? val[mid] : 1.f;
        return !isnan(*v);
      }
      if (x < feat) lo = mid + 1;
      else hi = mid;
    }
    return false;
  }
};

// what one wave wrote is read by other lanes of the same wave
__device__ __forceinline__ void wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// LDS: paths [npath] uint4, elements [nelem] uint4, their columns [nelem],
// 1 / k for k <= 64, then the accumulator tile [kShapThreads / W][U1].
__host__ __device__ inline size_t shap_lds_bytes(int npath, int nelem, int rows, int U1,
                                                 bool lds_acc) {
  return (size_t)npath * 16 + (size_t)nelem * 20 + 65 * 4 + (lds_acc ? (size_t)rows * U1 * 4 : 0);
}

// One path for one row, as the lane that owns element `lane` sees it: zo is
// the element's z, negative when the row does not satisfy it (o = 0); lane 0,
// the dummy, holds 1; lanes beyond the path hold 0.
struct ShapLane {
  float zo, leaf;
  int col, d;
};

template <class Rows>
__device__ __forceinline__ ShapLane shap_lane(const Rows& rows, const typename Rows::Row& row,
                                              const uint4* sp, const uint4* se,
                                              const int32_t* sc, int p, int elem_begin,
                                              int lane) {
  const uint4 ph = sp[p];
  ShapLane s{lane == 0 ? 1.f : 0.f, __uint_as_float(ph.z), 0, (int)ph.y};
  if (lane >= 1 && lane <= s.d) {
    const int k = (int)ph.x - elem_begin + lane - 1;
    const uint4 e = se[k];
    s.col = sc[k];
    float v;
    const bool sat = rows.value(row, (int)(e.x >> 1), &v)
                         ? (__uint_as_float(e.y) <= v && v < __uint_as_float(e.z))
                         : (e.x & 1u) != 0;
    s.zo = sat ? __uint_as_float(e.w) : -__uint_as_float(e.w);
  }
  return s;
}

// the value of the lane below (the wave's lane 0 reads 0): a group's lane 0
// never uses it
__device__ __forceinline__ float lane_below(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138 /* wave_shr:1 */,
                                                    0xf, 0xf, true));
}

// paths: the chunk's npath paths; elems / ecol: the whole table (a path's
// first element is an index into it, >= elem_begin); out: the class's
// [n, U1] slice, column U1 - 1 (the bias) is left alone.
template <class Rows, int W, bool kLdsAcc>
__global__ __launch_bounds__(kShapThreads) void k_shap(
    Rows rows, int64_t n, const uint4* __restrict__ paths, const uint4* __restrict__ elems,
    const int32_t* __restrict__ ecol, int elem_begin, int nelem, int npath, int U1,
    float* out) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) uint4 shap_lds[];
  constexpr int R = kShapThreads / W;
  uint4* sp = shap_lds;
  uint4* se = sp + npath;
  int32_t* sc = reinterpret_cast<int32_t*>(se + nelem);
  float* sinv = reinterpret_cast<float*>(sc + nelem);
  float* tile = sinv + 65;
  for (int j = threadIdx.x; j < npath; j += kShapThreads) sp[j] = paths[j];
  for (int j = threadIdx.x; j < nelem; j += kShapThreads) {
    se[j] = elems[elem_begin + j];
    sc[j] = ecol[elem_begin + j];
  }
  if (threadIdx.x < 65) sinv[threadIdx.x] = 1.f / (float)max((int)threadIdx.x, 1);
  __syncthreads();
  const int g = threadIdx.x / W, lane = threadIdx.x % W;
  const int64_t tiles = (n + R - 1) / R;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t r = t * R + g;
    const bool live = r < n;
    const typename Rows::Row row = rows.row(live ? r : n - 1);
    float* acc = kLdsAcc ? tile + (size_t)g * U1 : out + (live ? r : n - 1) * U1;
    if constexpr (kLdsAcc) {
      for (int c = lane; c < U1; c += W) acc[c] = 0.f;
      wave_fence();
    }
    // the next path's element and feature value are fetched while this one
    // is computed
    ShapLane nxt = shap_lane(rows, row, sp, se, sc, 0, elem_begin, lane);
    for (int p = 0; p < npath; ++p) {
      const ShapLane cur = nxt;
      if (p + 1 < npath) nxt = shap_lane(rows, row, sp, se, sc, p + 1, elem_begin, lane);
      const int d = cur.d;
      const float z = fabsf(cur.zo), o = cur.zo > 0.f ? 1.f : 0.f;
      // EXTEND: w[j] of the path's first l elements lives in lane j
      float w = lane == 0 ? 1.f : 0.f;
      for (int l = 1; l <= d; ++l) {
        const float zs = __shfl(cur.zo, l, W);
        const float wp = lane_below(w);
        const float a = fabsf(zs) * w * (float)(l - lane);
        const float bb = lane && zs > 0.f ? wp * (float)lane : 0.f;
        w = (a + bb) * sinv[l + 1];
      }
      // UNWOUND-SUM without the lane's own element
      const float dp1 = (float)(d + 1), rz = 1.f / z;
      float next = __shfl(w, d, W), tot1 = 0.f, tot0 = 0.f;
      for (int j = d - 1; j >= 0; --j) {
        const float wj = __shfl(w, j, W);
        const float tmp = next * (dp1 * sinv[j + 1]);
        tot1 += tmp;
        next = wj - tmp * z * ((float)(d - j) * sinv[d + 1]);
        tot0 += wj * rz * (dp1 * sinv[d - j]);
      }
      if (lane >= 1 && lane <= d && live)
        acc[cur.col] += (o != 0.f ? tot1 : tot0) * (o - z) * cur.leaf;
      wave_fence();
    }
    if constexpr (kLdsAcc) {
      if (live)
        for (int c = lane; c < U1 - 1; c += W) out[r * U1 + c] += acc[c];
      wave_fence();
    }
  }
}

// One row per lane over trees [0, T): tree t adds into class t % K.
template <class Rows>
__global__ __launch_bounds__(kSaabasThreads) void k_saabas(
    Rows rows, int64_t n, const uint4* __restrict__ nodes, const int32_t* __restrict__ tree_off,
    const float* __restrict__ node_m, const int32_t* __restrict__ node_col, int T, int K, int U1,
    float* __restrict__ out) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
    const typename Rows::Row r = rows.row(i);
    for (int t = 0; t < T; ++t) {
      float* phi = out + ((int64_t)(t % K) * n + i) * U1;
      const int o = tree_off[t];
      int nd = o;
      uint4 q = nodes[nd];
      float m = node_m[nd];
      while ((int)q.x >= 0) {
        float v;
        const bool left = rows.value(r, (int)(q.x >> 1), &v) ? v < __uint_as_float(q.y)
                                                             : (q.x & 1u) != 0;
        const int c = o + (int)(left ? q.z : q.w);
        const float mc = node_m[c];
        phi[node_col[nd]] += mc - m;
        nd = c, m = mc, q = nodes[nd];
      }
    }
  }
}

// LDS of the interaction kernel: the path table as in k_shap, then the
// packed triangles [block threads / W][TP] of the block's rows.
__host__ __device__ inline size_t shap_inter_lds_bytes(int npath, int nelem, int rows, int64_t TP,
                                                       bool lds_acc) {
  return (size_t)npath * 16 + (size_t)nelem * 20 + 65 * 4 +
         (lds_acc ? (size_t)rows * (size_t)TP * 4 : 0);
}

// Pairwise interactions of one chunk of paths, the structure of k_shap. For
// each path every element c in turn is conditioned on: EXTEND over the other
// d - 1 elements (lane j holds w[j]), UNWOUND-SUM of the lane's own element,
// and the lane whose column is the larger of the pair adds into the row's
// packed triangle, entry col (col - 1) / 2 + col_c of TP: the statements of
// gbdt_shap_inter_path<float> in its order. A path's pairs are distinct
// cells, so the lanes of a group never meet in one within a path, and the
// paths are fenced from each other. tri: the class's [n, TP] slice of the
// scratch triangle: the LDS tile is added to it once per chunk, or, kLdsAcc
// false, the row's slice of it is the accumulator. The block is whole waves,
// as many as the launch found room for (shap_inter_threads).
template <class Rows, int W, bool kLdsAcc>
__global__ __launch_bounds__(kShapThreads) void k_shap_inter(
    Rows rows, int64_t n, const uint4* __restrict__ paths, const uint4* __restrict__ elems,
    const int32_t* __restrict__ ecol, int elem_begin, int nelem, int npath, int64_t TP,
    float* tri) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) uint4 shap_lds[];
  const int R = blockDim.x / W;
  uint4* sp = shap_lds;
  uint4* se = sp + npath;
  int32_t* sc = reinterpret_cast<int32_t*>(se + nelem);
  float* sinv = reinterpret_cast<float*>(sc + nelem);
  float* tile = sinv + 65;
  for (int j = threadIdx.x; j < npath; j += blockDim.x) sp[j] = paths[j];
  for (int j = threadIdx.x; j < nelem; j += blockDim.x) {
    se[j] = elems[elem_begin + j];
    sc[j] = ecol[elem_begin + j];
  }
  if (threadIdx.x < 65) sinv[threadIdx.x] = 1.f / (float)max((int)threadIdx.x, 1);
  __syncthreads();
  const int g = threadIdx.x / W, lane = threadIdx.x % W;
  const int64_t tiles = (n + R - 1) / R;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t r = t * R + g;
    const bool live = r < n;
    const typename Rows::Row row = rows.row(live ? r : n - 1);
    float* acc = kLdsAcc ? tile + (size_t)g * TP : tri + (live ? r : n - 1) * TP;
    if constexpr (kLdsAcc) {
      for (int c = lane; c < TP; c += W) acc[c] = 0.f;
      wave_fence();
    }
    ShapLane nxt = shap_lane(rows, row, sp, se, sc, 0, elem_begin, lane);
    for (int p = 0; p < npath; ++p) {
      const ShapLane cur = nxt;
      if (p + 1 < npath) nxt = shap_lane(rows, row, sp, se, sc, p + 1, elem_begin, lane);
      const int d = cur.d, m = d - 1;
      if (d < 2) continue;  // (d is the path's: the same in every lane)
      const float z = fabsf(cur.zo), o = cur.zo > 0.f ? 1.f : 0.f;
      const float half = cur.leaf * 0.5f, mp1 = (float)(m + 1), rz = 1.f / z;
      const int64_t base = (int64_t)cur.col * (cur.col - 1) / 2;
      for (int c = 1; c <= d; ++c) {
        const float zc = __shfl(cur.zo, c, W);
        const int colc = __shfl(cur.col, c, W);
        // the element of the path's largest column has no lane above it (the
        // columns are the path's: the same in every group of the wave)
        if (!__any(lane >= 1 && lane <= d && cur.col > colc)) continue;
        const float fc = (zc > 0.f ? 1.f : 0.f) - fabsf(zc);
        // EXTEND by the elements beside c
        float w = lane == 0 ? 1.f : 0.f;
        for (int l = 1; l <= m; ++l) {
          const float zs = __shfl(cur.zo, l < c ? l : l + 1, W);
          const float wp = lane_below(w);
          const float a = fabsf(zs) * w * (float)(l - lane);
          const float bb = lane && zs > 0.f ? wp * (float)lane : 0.f;
          w = (a + bb) * sinv[l + 1];
        }
        // UNWOUND-SUM without the lane's own element
        float next = __shfl(w, m, W), tot1 = 0.f, tot0 = 0.f;
        for (int j = m - 1; j >= 0; --j) {
          const float wj = __shfl(w, j, W);
          const float tmp = next * (mp1 * sinv[j + 1]);
          tot1 += tmp;
          next = wj - tmp * z * ((float)(m - j) * sinv[m + 1]);
          tot0 += wj * rz * (mp1 * sinv[m - j]);
        }
        if (lane >= 1 && lane <= d && cur.col > colc && live)
          acc[base + colc] += (o != 0.f ? tot1 : tot0) * (o - z) * fc * half;
      }
      wave_fence();
    }
    if constexpr (kLdsAcc) {
      if (live)
        for (int c = lane; c < TP; c += W) tri[r * TP + c] += acc[c];
      wave_fence();
    }
  }
}

// out [rows, U1, U1] of tri [rows, TP] and phi [rows, U1] (rows = classes x
// matrix rows), one thread per cell: a pair's two cells are one number of
// the triangle, the diagonal is phi[i] minus the cells of row i one after
// the other by ascending column (gbdt_shap_inter_rows), cell (U, U) is
// phi's bias, the rest of row and column U is zero.
__global__ __launch_bounds__(kSaabasThreads) void k_shap_inter_out(
    const float* __restrict__ tri, const float* __restrict__ phi, int64_t rows, int U1,
    int64_t TP, float* __restrict__ out) {
  const int U = U1 - 1;
  const int64_t cells = rows * U1 * U1, step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < cells; x += step) {
    const int64_t r = x / ((int64_t)U1 * U1);
    const int i = (int)((x / U1) % U1), j = (int)(x % U1);
    const float* t = tri + r * TP;
    float v = 0.f;
    if (i == U || j == U) {
      if (i == j) v = phi[r * U1 + U];
    } else if (i != j) {
      v = i > j ? t[(int64_t)i * (i - 1) / 2 + j] : t[(int64_t)j * (j - 1) / 2 + i];
    } else {
      v = phi[r * U1 + i];
      for (int k = 0; k < U; ++k)
        if (k != i) v -= k < i ? t[(int64_t)i * (i - 1) / 2 + k] : t[(int64_t)k * (k - 1) / 2 + i];
    }
    out[x] = v;
  }
}

int shap_cus() {  // of the current device
  int dev = 0, cus = 0;
  WH_HIP_CHECK(hipGetDevice(&dev));
  WH_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  return std::max(cus, 1);
}

template <class Rows, int W>
void shap_launch_w(const Rows& rows, int64_t n, const ShapChunk& c, hipStream_t s) {
  constexpr int R = kShapThreads / W;
  const bool lds_acc = c.U1 <= kShapLdsCols;
  const size_t lds = shap_lds_bytes(c.npath, c.nelem, R, c.U1, lds_acc);
  static bool attr = false;
  if (!attr) {  // dynamic LDS above 64 KB must be opted into per kernel
    const void* ks[2] = {(const void*)k_shap<Rows, W, true>, (const void*)k_shap<Rows, W, false>};
    for (const void* k : ks)
      WH_HIP_CHECK(hipFuncSetAttribute(
          k, hipFuncAttributeMaxDynamicSharedMemorySize,
          (int)shap_lds_bytes(kShapLdsElems, kShapLdsElems, kShapThreads / 16, kShapLdsCols, true)));
    attr = true;
  }
  const int grid = grid_for(n, R, shap_cus() * kShapBlocksPerCu);
  auto kern = lds_acc ? k_shap<Rows, W, true> : k_shap<Rows, W, false>;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kShapThreads), lds, s, rows, n,
                     reinterpret_cast<const uint4*>(c.paths) + c.path_begin,
                     reinterpret_cast<const uint4*>(c.elems), c.ecol, c.elem_begin, c.nelem,
                     c.npath, c.U1, c.out);
}

template <class Rows>
void shap_launch(const Rows& rows, int64_t n, const ShapChunk& c, hipStream_t s) {
  if (n <= 0 || c.npath <= 0) return;
  if (c.width == 16) shap_launch_w<Rows, 16>(rows, n, c, s);
  else if (c.width == 32) shap_launch_w<Rows, 32>(rows, n, c, s);
  else shap_launch_w<Rows, 64>(rows, n, c, s);
}

// Threads of the block that takes a chunk: kShapThreads, or, with the LDS
// accumulator, the most whole waves whose rows' triangles fit beside the
// chunk's table (at least kShapInterThreads up to kShapInterLdsCols columns,
// whatever the table holds).
inline int shap_inter_threads(int npath, int nelem, int W, int64_t TP, bool lds_acc) {
  int threads = kShapThreads;
  while (threads > 64 && shap_inter_lds_bytes(npath, nelem, threads / W, TP, lds_acc) >
                             (size_t)kShapLdsBytes)
    threads -= 64;
  return threads;
}

template <class Rows, int W>
void shap_inter_launch_w(const Rows& rows, int64_t n, const ShapChunk& c, hipStream_t s) {
  const int U = c.U1 - 1;
  const int64_t TP = gbdt_shap_inter_pairs(U);
  const bool lds_acc = U <= kShapInterLdsCols;
  const int threads = shap_inter_threads(c.npath, c.nelem, W, TP, lds_acc), R = threads / W;
  const size_t lds = shap_inter_lds_bytes(c.npath, c.nelem, R, TP, lds_acc);
  static bool attr = false;
  if (!attr) {  // dynamic LDS above 64 KB must be opted into per kernel
    const void* ks[2] = {(const void*)k_shap_inter<Rows, W, true>,
                         (const void*)k_shap_inter<Rows, W, false>};
    for (const void* k : ks)
      WH_HIP_CHECK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       kShapLdsBytes));
    attr = true;
  }
  const int grid = grid_for(n, R, shap_cus() * kShapBlocksPerCu);
  auto kern = lds_acc ? k_shap_inter<Rows, W, true> : k_shap_inter<Rows, W, false>;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, s, rows, n,
                     reinterpret_cast<const uint4*>(c.paths) + c.path_begin,
                     reinterpret_cast<const uint4*>(c.elems), c.ecol, c.elem_begin, c.nelem,
                     c.npath, TP, c.out);
}

template <class Rows>
void shap_inter_launch(const Rows& rows, int64_t n, const ShapChunk& c, hipStream_t s) {
  if (n <= 0 || c.npath <= 0 || c.U1 < 3) return;  // (one column: no pairs)
  if (c.width == 16) shap_inter_launch_w<Rows, 16>(rows, n, c, s);
  else if (c.width == 32) shap_inter_launch_w<Rows, 32>(rows, n, c, s);
  else shap_inter_launch_w<Rows, 64>(rows, n, c, s);
}

template <class Rows>
void saabas_launch(const Rows& rows, int64_t n, const SaabasForest& f, hipStream_t s) {
  if (n <= 0 || f.T <= 0) return;
  const int grid = grid_for(n, kSaabasThreads, shap_cus() * 8);
  hipLaunchKernelGGL(k_saabas<Rows>, dim3(grid), dim3(kSaabasThreads), 0, s, rows, n,
                     reinterpret_cast<const uint4*>(f.nodes), f.tree_off, f.node_m, f.node_col,
                     f.T, f.K, f.U1, f.out);
}

}  // namespace

int gbdt_shap_max_blocks() { return shap_cus() * kShapBlocksPerCu; }

void gbdt_shap(const float* X, int64_t n, int f, const ShapChunk& c, hipStream_t s) {
  shap_launch(DenseRows{X, f}, n, c, s);
}

void gbdt_shap_csr(const int64_t* row_off, const int32_t* fid, const float* val, int64_t n,
                   const ShapChunk& c, hipStream_t s) {
  shap_launch(CsrRows{row_off, fid, val}, n, c, s);
}

void gbdt_shap_inter(const float* X, int64_t n, int f, const ShapChunk& c, hipStream_t s) {
  shap_inter_launch(DenseRows{X, f}, n, c, s);
}

void gbdt_shap_inter_csr(const int64_t* row_off, const int32_t* fid, const float* val, int64_t n,
                         const ShapChunk& c, hipStream_t s) {
  shap_inter_launch(CsrRows{row_off, fid, val}, n, c, s);
}

void gbdt_shap_inter_out(const float* tri, const float* phi, int64_t rows, int U1, float* out,
                         hipStream_t s) {
  if (rows <= 0) return;
  const int grid = grid_for(rows * U1 * U1, kSaabasThreads, shap_cus() * 8);
  hipLaunchKernelGGL(k_shap_inter_out, dim3(grid), dim3(kSaabasThreads), 0, s, tri, phi, rows, U1,
                     gbdt_shap_inter_pairs(U1 - 1), out);
}

void gbdt_saabas(const float* X, int64_t n, int f, const SaabasForest& fo, hipStream_t s) {
  saabas_launch(DenseRows{X, f}, n, fo, s);
}

void gbdt_saabas_csr(const int64_t* row_off, const int32_t* fid, const float* val, int64_t n,
                     const SaabasForest& fo, hipStream_t s) {
  saabas_launch(CsrRows{row_off, fid, val}, n, fo, s);
}

}  // namespace wh
