// GBDT learning to rank: the gradient pairs of rank:pairwise / rank:ndcg and
// the per-group ndcg / map values, over query groups given as row offsets
// (docs/bsp_apps.md "Ranking"; task lists: csrc/host/gbdt_rank_plan.h).
//
// Everything is counting inside a group, no sort: a row's partner count c,
// its rank by prediction r and by label lr are sums over the group's rows,
// and so are its gradient pair (every pair with a different label, in both
// roles) and the metrics. A row belongs to one thread, which walks ALL the
// group's rows j in ascending order and adds into its own fp64 registers:
// no atomics, one writer per output element, the same bits on every run and
// for any order of the task lists.
//
//   small groups (<= 64 rows)   one wavefront per group, one row per lane;
//                               partner j is read from lane j (v_readlane, j
//                               is wave-uniform), no LDS and no barrier
//   larger groups               one block per 256 rows of a group, in two
//                               launches (counts, then pairs); the group's
//                               rows {m, y, 1/c, discount} (16 B) go through
//                               LDS, in one tile when they fit the launch's
//                               LDS rows; every lane reads the same j (one
//                               broadcast ds_read_b128) while owning a
//                               distinct row i
#include <algorithm>
#include <cmath>

#include "host/gbdt_rank_plan.h"
#include "wh_common.h"
#include "wh_kernels.h"

namespace wh {
namespace {

constexpr int kRankThreads = 256, kRankWaves = kRankThreads / 64;
constexpr int kRankSmallBlocks = 2048;  // grid bound of the wave-per-group kernel
constexpr int kRankKindGrad = 0, kRankKindNdcg = 1, kRankKindMap = 2;

// 1 / log2(2 + r), in fp64 (the fp32 difference of two discounts would else
// carry the logarithm's rounding as well as its own)
__device__ __forceinline__ double rank_discount(int r) { return 1.0 / log2(2.0 + (double)r); }

// What pass 1 counts for row i against partner j (m, y of both; i_after_j:
// j is the earlier row): partners, rank by prediction, rank by label.
struct RankCount {
  int c = 0, r = 0, lr = 0;
  __device__ __forceinline__ void add(float mi, float yi, float mj, float yj, bool j_before_i) {
    c += yj != yi;
    r += (mj > mi) | ((mj == mi) & j_before_i);
    lr += (yj > yi) | ((yj == yi) & j_before_i);
  }
};

// One pair's share of row i's gradient, fp32 terms into fp64 sums. p = {m_j,
// y_j, 1 / c_j, discount_j}. The row with the higher label is "hi": rho =
// sigmoid(m_hi - m_lo), lambda = rho - 1, eta = max(rho (1 - rho), 1e-16);
// hi takes +W lambda, lo -W lambda, both 2 W eta. 1 - rho comes from the
// same exponential as rho (no cancellation at large |m_hi - m_lo|). No
// branch: a partner with the same label weighs 0 and adds +-0, so that the
// partner loops unroll and several pairs' chains of exp, divide and fp64 add
// are in flight per wave (one group of 1024 rows: 294 -> 183 us,
// profiles/gbdt_rank.txt).
template <bool kNdcg>
__device__ __forceinline__ void rank_pair(float mi, float yi, float ci, float di, float gi,
                                          float inv_idcg, const float4& p, double* g, double* h) {
  float w = p.y != yi ? ci + p.z : 0.f;
  if constexpr (kNdcg) {
    const float gj = exp2f(p.y) - 1.f;
    w *= fabsf(gi - gj) * fabsf(di - p.w) * inv_idcg;
  }
  const bool hi = yi > p.y;
  const float d = hi ? mi - p.x : p.x - mi;
  const float t = expf(-fabsf(d));
  const float s = 1.f / (1.f + t);
  const float ts = t * s;
  const float rho = d >= 0.f ? s : ts;
  const float q = d >= 0.f ? ts : s;  // 1 - rho
  const float eta = fmaxf(rho * q, 1e-16f);
  const float wl = w * -q;
  *g += (double)(hi ? wl : -wl);
  *h += (double)(2.f * w * eta);
}

__device__ __forceinline__ float lane_f(float v, int j) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
}

// Reads a task's group: false when the id or its offsets are out of range
// (the lists come from the host plan; a bad one must not reach memory).
__device__ __forceinline__ bool rank_group(const int32_t* __restrict__ tasks, int t,
                                           const int32_t* __restrict__ off, int Q, int64_t n,
                                           int* g, int* beg, int* len) {
  *g = tasks[t];
  if (*g < 0 || *g >= Q) return false;
  *beg = off[*g];
  const int end = off[*g + 1];
  *len = end - *beg;
  return *beg >= 0 && *len > 0 && (int64_t)end <= n;
}

// ------------------------------------------------ small: a wave per group
template <bool kNdcg>
__global__ __launch_bounds__(kRankThreads) void k_rank_grad_wave(
    const float* __restrict__ margin, const float* __restrict__ label,
    const int32_t* __restrict__ off, int Q, int64_t n, const int32_t* __restrict__ tasks,
    int ntask, float2* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * kRankWaves + (threadIdx.x >> 6);
  for (int t = wave; t < ntask; t += gridDim.x * kRankWaves) {
    int g, beg, len;
    if (!rank_group(tasks, t, off, Q, n, &g, &beg, &len) || len > kRankWaveRows) continue;
    len = __builtin_amdgcn_readfirstlane(len);
    const bool on = lane < len;
    const float mi = on ? margin[beg + lane] : 0.f, yi = on ? label[beg + lane] : 0.f;
    RankCount k;
    for (int j = 0; j < len; ++j) k.add(mi, yi, lane_f(mi, j), lane_f(yi, j), j < lane);
    const float ci = k.c > 0 ? 1.f / (float)k.c : 0.f;
    float di = 0.f, gi = 0.f, inv_idcg = 0.f;
    if constexpr (kNdcg) {
      di = (float)rank_discount(k.r);
      gi = exp2f(yi) - 1.f;
      const double idcg = wave_sum_d(on ? (double)gi * rank_discount(k.lr) : 0.0);
      inv_idcg = idcg > 0.0 ? (float)(1.0 / idcg) : 0.f;
    }
    double sg = 0, sh = 0;
#pragma unroll 4
    for (int j = 0; j < len; ++j) {
      const float4 p = make_float4(lane_f(mi, j), lane_f(yi, j), lane_f(ci, j), lane_f(di, j));
      rank_pair<kNdcg>(mi, yi, ci, di, gi, inv_idcg, p, &sg, &sh);
    }
    if (on) out[beg + lane] = make_float2((float)sg, (float)sh);
  }
}

// --------------------------------------- larger: blocks of 256 rows per group
// A group of more than 64 rows is cut into chunks of 256 rows, one block per
// (group, chunk): grid.x walks the task list, grid.y the chunks (a block whose
// chunk lies past its group's end returns at once). One block per group left
// the whole launch waiting for its largest group: 1250 rows took 1.4 ms on
// four waves while the rest of the chip had long finished.
//
// The partners of one pass: the group's rows [0, len) in tiles of `cap` rows
// of LDS (one tile when the group fits). load(j) gives row j's element;
// visit(j, p) is called for every j in ascending order by every thread of a
// wave that owns a row (wave_on, wave-uniform: a group's last chunk is rarely
// full, and its idle waves only keep the barriers, which are inside).
template <class T, class Load, class Visit>
__device__ __forceinline__ void rank_tiles(T* lds, int len, int cap, bool wave_on, Load load,
                                           Visit visit) {
  for (int t0 = 0; t0 < len; t0 += cap) {
    const int tn = min(cap, len - t0);
    if (t0 > 0) __syncthreads();  // the previous tile is read
    for (int j = threadIdx.x; j < tn; j += kRankThreads) lds[j] = load(t0 + j);
    __syncthreads();
    if (!wave_on) continue;
#pragma unroll 4
    for (int j = 0; j < tn; ++j) visit(t0 + j, lds[j]);
  }
}

// Sum over the block, the same value in every thread; sh: kRankWaves doubles.
__device__ __forceinline__ double rank_block_sum(double v, double* sh) {
  v = wave_sum_d(v);
  __syncthreads();  // sh is free
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = 0;
  for (int w = 0; w < kRankWaves; ++w) r += sh[w];
  return r;
}

// Pass 1: aux [n] float2 = every row's {1 / c, discount}; ndcg: idcg [n]
// holds, at a chunk's first row, the chunk's share of its group's IDCG.
template <bool kNdcg>
__global__ __launch_bounds__(kRankThreads) void k_rank_count(
    const float* __restrict__ margin, const float* __restrict__ label,
    const int32_t* __restrict__ off, int Q, int64_t n, const int32_t* __restrict__ tasks,
    int ntask, int cap, float2* __restrict__ aux, double* __restrict__ idcg) {
  extern __shared__ __attribute__((aligned(16))) float2 rank_lds2[];
  __shared__ double red[kRankWaves];
  for (int t = blockIdx.x; t < ntask; t += gridDim.x) {
    int g, beg, len;
    if (!rank_group(tasks, t, off, Q, n, &g, &beg, &len)) continue;  // (block-uniform)
    const float* m = margin + beg;
    const float* y = label + beg;
    for (int i0 = blockIdx.y * kRankThreads; i0 < len; i0 += gridDim.y * kRankThreads) {
      const int i = i0 + threadIdx.x;
      const bool on = i < len;
      const float mi = on ? m[i] : 0.f, yi = on ? y[i] : 0.f;
      RankCount k;
      __syncthreads();  // the previous chunk's LDS is read
      rank_tiles(rank_lds2, len, cap, i0 + (int)(threadIdx.x & ~63u) < len,
                 [&](int j) { return make_float2(m[j], y[j]); },
                 [&](int j, const float2& p) { k.add(mi, yi, p.x, p.y, j < i); });
      if (on) {
        const float ci = k.c > 0 ? 1.f / (float)k.c : 0.f;
        aux[beg + i] = make_float2(ci, kNdcg ? (float)rank_discount(k.r) : 0.f);
      }
      if constexpr (kNdcg) {
        const double part =
            rank_block_sum(on ? (double)(exp2f(yi) - 1.f) * rank_discount(k.lr) : 0.0, red);
        if (threadIdx.x == 0) idcg[beg + i0] = part;
      }
    }
  }
}

// Pass 2 (after pass 1 of every group): every row against all its partners,
// both roles. IDCG is the sum of the group's chunk shares in chunk order.
template <bool kNdcg>
__global__ __launch_bounds__(kRankThreads) void k_rank_pairs(
    const float* __restrict__ margin, const float* __restrict__ label,
    const int32_t* __restrict__ off, int Q, int64_t n, const int32_t* __restrict__ tasks,
    int ntask, int cap, const float2* __restrict__ aux, const double* __restrict__ idcg,
    float2* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float4 rank_lds4[];
  for (int t = blockIdx.x; t < ntask; t += gridDim.x) {
    int g, beg, len;
    if (!rank_group(tasks, t, off, Q, n, &g, &beg, &len)) continue;  // (block-uniform)
    if ((int)(blockIdx.y * kRankThreads) >= len) continue;
    const float* m = margin + beg;
    const float* y = label + beg;
    const float2* ax = aux + beg;
    float inv_idcg = 0.f;
    if constexpr (kNdcg) {
      double sum = 0;  // (every thread the same additions: no broadcast needed)
      for (int c0 = 0; c0 < len; c0 += kRankThreads) sum += idcg[beg + c0];
      inv_idcg = sum > 0.0 ? (float)(1.0 / sum) : 0.f;
    }
    for (int i0 = blockIdx.y * kRankThreads; i0 < len; i0 += gridDim.y * kRankThreads) {
      const int i = i0 + threadIdx.x;
      const bool on = i < len;
      const float mi = on ? m[i] : 0.f, yi = on ? y[i] : 0.f;
      const float2 a = on ? ax[i] : make_float2(0.f, 0.f);
      const float gi = kNdcg ? exp2f(yi) - 1.f : 0.f;
      double sg = 0, sh = 0;
      __syncthreads();  // the previous chunk's LDS is read
      rank_tiles(rank_lds4, len, cap, i0 + (int)(threadIdx.x & ~63u) < len,
                 [&](int j) { return make_float4(m[j], y[j], ax[j].x, ax[j].y); },
                 [&](int j, const float4& p) {
                   rank_pair<kNdcg>(mi, yi, a.x, a.y, gi, inv_idcg, p, &sg, &sh);
                 });
      if (on) out[beg + i] = make_float2((float)sg, (float)sh);
    }
  }
}

// ------------------------------------------------------------ evaluation
// A row's terms of its group's metric {numerator, denominator}, from counts
// against all the group's rows (k: the cut-off, INT32_MAX for none).
struct RankEvalRow {
  int r = 0, lr = 0, hits_le = 0;  // hits_le: hits j with r_j <= r_i
  __device__ __forceinline__ void add(float mi, float yi, float mj, float yj, int i, int j) {
    const bool ahead = (mj > mi) | ((mj == mi) & (j < i));
    r += ahead;
    lr += (yj > yi) | ((yj == yi) & (j < i));
    hits_le += (yj > 0.f) & (ahead | (j == i));
  }
  __device__ __forceinline__ void terms(float yi, int kind, int k, double* num, double* den) const {
    if (kind == kRankKindNdcg) {
      const double gain = exp2((double)yi) - 1.0;
      if (r < k) *num += gain * rank_discount(r);
      if (lr < k) *den += gain * rank_discount(lr);
    } else if (yi > 0.f) {
      if (r < k) *num += (double)hits_le / (double)(r + 1);
      *den += 1.0;
    }
  }
};

__device__ __forceinline__ double rank_eval_value(double num, double den, int minus) {
  return den > 0.0 ? num / den : (minus ? 0.0 : 1.0);
}

__global__ __launch_bounds__(kRankThreads) void k_rank_eval_wave(
    const float* __restrict__ margin, const float* __restrict__ label,
    const int32_t* __restrict__ off, int Q, int64_t n, const int32_t* __restrict__ tasks,
    int ntask, int kind, int k, int minus, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * kRankWaves + (threadIdx.x >> 6);
  for (int t = wave; t < ntask; t += gridDim.x * kRankWaves) {
    int g, beg, len;
    if (!rank_group(tasks, t, off, Q, n, &g, &beg, &len) || len > kRankWaveRows) continue;
    len = __builtin_amdgcn_readfirstlane(len);
    const bool on = lane < len;
    const float mi = on ? margin[beg + lane] : 0.f, yi = on ? label[beg + lane] : 0.f;
    RankEvalRow e;
    for (int j = 0; j < len; ++j) e.add(mi, yi, lane_f(mi, j), lane_f(yi, j), lane, j);
    double num = 0, den = 0;
    if (on) e.terms(yi, kind, k, &num, &den);
    num = wave_sum_d(num);
    den = wave_sum_d(den);
    if (lane == 0) out[g] = rank_eval_value(num, den, minus);
  }
}

// Larger groups, cut as for the gradient: a block per 256 rows leaves its
// rows' {numerator, denominator} in part [n, 2], at its first row ...
__global__ __launch_bounds__(kRankThreads) void k_rank_eval_chunk(
    const float* __restrict__ margin, const float* __restrict__ label,
    const int32_t* __restrict__ off, int Q, int64_t n, const int32_t* __restrict__ tasks,
    int ntask, int cap, int kind, int k, double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float2 rank_lds2[];
  __shared__ double red[kRankWaves];
  for (int t = blockIdx.x; t < ntask; t += gridDim.x) {
    int g, beg, len;
    if (!rank_group(tasks, t, off, Q, n, &g, &beg, &len)) continue;  // (block-uniform)
    const float* m = margin + beg;
    const float* y = label + beg;
    for (int i0 = blockIdx.y * kRankThreads; i0 < len; i0 += gridDim.y * kRankThreads) {
      const int i = i0 + threadIdx.x;
      const bool on = i < len;
      const float mi = on ? m[i] : 0.f, yi = on ? y[i] : 0.f;
      RankEvalRow e;
      __syncthreads();  // the previous chunk's LDS is read
      rank_tiles(rank_lds2, len, cap, i0 + (int)(threadIdx.x & ~63u) < len,
                 [&](int j) { return make_float2(m[j], y[j]); },
                 [&](int j, const float2& p) { e.add(mi, yi, p.x, p.y, i, j); });
      double num = 0, den = 0;
      if (on) e.terms(yi, kind, k, &num, &den);
      num = rank_block_sum(num, red);
      den = rank_block_sum(den, red);
      if (threadIdx.x == 0) {
        part[2 * (int64_t)(beg + i0)] = num;
        part[2 * (int64_t)(beg + i0) + 1] = den;
      }
    }
  }
}

// ... and a thread per group adds them in chunk order.
__global__ __launch_bounds__(kRankThreads) void k_rank_eval_final(
    const int32_t* __restrict__ off, int Q, int64_t n, const int32_t* __restrict__ tasks,
    int ntask, int minus, const double* __restrict__ part, double* __restrict__ out) {
  const int t = blockIdx.x * kRankThreads + threadIdx.x;
  if (t >= ntask) return;
  int g, beg, len;
  if (!rank_group(tasks, t, off, Q, n, &g, &beg, &len)) return;
  double num = 0, den = 0;
  for (int i0 = 0; i0 < len; i0 += kRankThreads)
    num += part[2 * (int64_t)(beg + i0)], den += part[2 * (int64_t)(beg + i0) + 1];
  out[g] = rank_eval_value(num, den, minus);
}

// --------------------------------------------------- root statistics
// {sum g, sum h, max |g|, max |h|} of gpair [n] in two small launches:
// per-block partials in a fixed order, then one block over the partials.
constexpr int kRankStatBlocks = 1024;

__device__ __forceinline__ void rank_stats_reduce(double v[4], double (*sh)[kRankWaves]) {
  v[0] = wave_sum_d(v[0]);
  v[1] = wave_sum_d(v[1]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    v[2] = fmax(v[2], __shfl_xor(v[2], o, 64));
    v[3] = fmax(v[3], __shfl_xor(v[3], o, 64));
  }
  if ((threadIdx.x & 63) == 0)
    for (int q = 0; q < 4; ++q) sh[q][threadIdx.x >> 6] = v[q];
  __syncthreads();
  for (int q = 0; q < 4; ++q) v[q] = 0;
  for (int w = 0; w < kRankWaves; ++w) {
    v[0] += sh[0][w];
    v[1] += sh[1][w];
    v[2] = fmax(v[2], sh[2][w]);
    v[3] = fmax(v[3], sh[3][w]);
  }
}

__global__ __launch_bounds__(kRankThreads) void k_rank_stats_part(int64_t n,
                                                                  const float2* __restrict__ gp,
                                                                  double* __restrict__ part) {
  __shared__ double sh[4][kRankWaves];
  double v[4] = {0, 0, 0, 0};
  for (int64_t i = (int64_t)blockIdx.x * kRankThreads + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kRankThreads) {
    const float2 p = gp[i];
    v[0] += p.x;
    v[1] += p.y;
    v[2] = fmax(v[2], (double)fabsf(p.x));
    v[3] = fmax(v[3], (double)fabsf(p.y));
  }
  rank_stats_reduce(v, sh);
  if (threadIdx.x == 0)
    for (int q = 0; q < 4; ++q) part[blockIdx.x * 4 + q] = v[q];
}

__global__ __launch_bounds__(kRankThreads) void k_rank_stats_final(int nb,
                                                                   const double* __restrict__ part,
                                                                   double* __restrict__ stats) {
  __shared__ double sh[4][kRankWaves];
  double v[4] = {0, 0, 0, 0};
  for (int b = threadIdx.x; b < nb; b += kRankThreads) {
    v[0] += part[b * 4];
    v[1] += part[b * 4 + 1];
    v[2] = fmax(v[2], part[b * 4 + 2]);
    v[3] = fmax(v[3], part[b * 4 + 3]);
  }
  rank_stats_reduce(v, sh);
  if (threadIdx.x == 0)
    for (int q = 0; q < 4; ++q) stats[q] = v[q];
}

// LDS rows of a block launch: what its largest group needs, within the cap.
int rank_cap(int rows) { return std::max(kRankWaveRows, std::min(rows, kRankLdsRows)); }

void rank_lds_opt_in() {  // dynamic LDS of 64 KB must be opted into per kernel
  static bool done = false;
  if (done) return;
  const void* ks[] = {(const void*)k_rank_count<false>, (const void*)k_rank_count<true>,
                      (const void*)k_rank_pairs<false>, (const void*)k_rank_pairs<true>,
                      (const void*)k_rank_eval_chunk};
  for (const void* k : ks)
    WH_HIP_CHECK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     kRankLdsRows * 16));
  done = true;
}

// The grid of a (group, chunk) launch: x over the tasks, y over the chunks of
// 256 rows of the largest group (`rows`; both loop when the grid is smaller).
dim3 rank_chunk_grid(int ntask, int rows) {
  return dim3(std::min(ntask, 1 << 20),
              std::max(1, std::min((rows + kRankThreads - 1) / kRankThreads, 4096)));
}

// One class of larger groups: pass 1 of all its groups, then pass 2.
void rank_grad_chunks(const float* margin, const float* label, const int32_t* off, int Q, int64_t n,
                      const int32_t* tasks, int ntask, int rows, int lds_rows, bool ndcg,
                      float2* aux, double* idcg, float2* out, hipStream_t s) {
  if (ntask <= 0) return;
  rank_lds_opt_in();
  const int cap = rank_cap(lds_rows);
  const dim3 grid = rank_chunk_grid(ntask, rows);
  hipLaunchKernelGGL(ndcg ? k_rank_count<true> : k_rank_count<false>, grid, dim3(kRankThreads),
                     (size_t)cap * 8, s, margin, label, off, Q, n, tasks, ntask, cap, aux, idcg);
  hipLaunchKernelGGL(ndcg ? k_rank_pairs<true> : k_rank_pairs<false>, grid, dim3(kRankThreads),
                     (size_t)cap * 16, s, margin, label, off, Q, n, tasks, ntask, cap, aux, idcg,
                     out);
}

}  // namespace

int64_t gbdt_rank_scratch() { return 4 * (int64_t)kRankStatBlocks; }

void gbdt_gpair_rank(const float* margin, const float* label, const int32_t* group_off, int Q,
                     int64_t n, const RankTasks& tk, bool ndcg, float* aux, double* idcg,
                     float* gpair, double* scratch, double* stats, hipStream_t s) {
  if (n <= 0) return;
  float2* out = reinterpret_cast<float2*>(gpair);
  float2* ax = reinterpret_cast<float2*>(aux);
  if (tk.nsmall > 0) {
    const int grid = std::min(kRankSmallBlocks, (tk.nsmall + kRankWaves - 1) / kRankWaves);
    hipLaunchKernelGGL(ndcg ? k_rank_grad_wave<true> : k_rank_grad_wave<false>, dim3(grid),
                       dim3(kRankThreads), 0, s, margin, label, group_off, Q, n, tk.small,
                       tk.nsmall, out);
  }
  rank_grad_chunks(margin, label, group_off, Q, n, tk.block, tk.nblock, tk.block_rows,
                   tk.block_rows, ndcg, ax, idcg, out, s);
  rank_grad_chunks(margin, label, group_off, Q, n, tk.tiled, tk.ntiled, tk.tiled_rows,
                   tk.tile_rows, ndcg, ax, idcg, out, s);
  const int nb = grid_for(n, kRankThreads, kRankStatBlocks);
  hipLaunchKernelGGL(k_rank_stats_part, dim3(nb), dim3(kRankThreads), 0, s, n, out, scratch);
  hipLaunchKernelGGL(k_rank_stats_final, dim3(1), dim3(kRankThreads), 0, s, nb, scratch, stats);
}

namespace {
// One class of larger groups: the chunks' partial sums, then the groups' values.
void rank_eval_chunks(const float* margin, const float* label, const int32_t* off, int Q,
                      int64_t n, const int32_t* tasks, int ntask, int rows, int lds_rows, int kind,
                      int k, int minus, double* part, double* out, hipStream_t s) {
  if (ntask <= 0) return;
  rank_lds_opt_in();
  const int cap = rank_cap(lds_rows);
  hipLaunchKernelGGL(k_rank_eval_chunk, rank_chunk_grid(ntask, rows), dim3(kRankThreads),
                     (size_t)cap * 8, s, margin, label, off, Q, n, tasks, ntask, cap, kind, k,
                     part);
  hipLaunchKernelGGL(k_rank_eval_final, dim3(grid_for(ntask, kRankThreads)), dim3(kRankThreads), 0,
                     s, off, Q, n, tasks, ntask, minus, part, out);
}

}  // namespace

void gbdt_rank_eval(const float* margin, const float* label, const int32_t* group_off, int Q,
                    int64_t n, const RankTasks& tk, int kind, int k, bool minus, double* part,
                    double* out, hipStream_t s) {
  if (n <= 0) return;
  const int kk = kind == 0 ? kRankKindNdcg : kRankKindMap;
  if (tk.nsmall > 0) {
    const int grid = std::min(kRankSmallBlocks, (tk.nsmall + kRankWaves - 1) / kRankWaves);
    hipLaunchKernelGGL(k_rank_eval_wave, dim3(grid), dim3(kRankThreads), 0, s, margin, label,
                       group_off, Q, n, tk.small, tk.nsmall, kk, k, minus ? 1 : 0, out);
  }
  rank_eval_chunks(margin, label, group_off, Q, n, tk.block, tk.nblock, tk.block_rows,
                   tk.block_rows, kk, k, minus ? 1 : 0, part, out, s);
  rank_eval_chunks(margin, label, group_off, Q, n, tk.tiled, tk.ntiled, tk.tiled_rows,
                   tk.tile_rows, kk, k, minus ? 1 : 0, part, out, s);
}

}  // namespace wh
