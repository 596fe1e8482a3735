// The adaptive objectives' leaf refresh (reg:absoluteerror, reg:quantileerror;
// docs/bsp_apps.md "Absolute and quantile error"): the exact weighted
// alpha-quantile of the residuals of every leaf's rows, for all leaves of a
// tree at once, by an MSD radix select with 8-bit digits -- four passes over
// an order-preserving 32-bit key (csrc/host/gbdt_quantile_plan.h).
//   gbdt_qsel_key    per ridx position: r = y - a, its key, the fixed-point
//                    weight u; both compact in segment order, so the passes
//                    stream them coalesced instead of gathering through ridx
//   gbdt_qsel_hist   one block per task {leaf, begin, end}: a 256-bin int64 LDS
//                    histogram of u over the keys inside the leaf's prefix;
//                    a second launch sums a leaf's chunk partials (no global
//                    atomics: the bins are written once, in a fixed order)
//   gbdt_qsel_pick   one wave per leaf scans its 256 (global) bins against the
//                    remaining threshold, appends the digit, subtracts the
//                    mass below it; no host read between the passes
//   gbdt_qsel_value  prefixes -> fp32 values and the "no weight" flags
// The histograms are exact integer sums, so adding the ranks' histograms
// between hist and pick gives the global quantile for any rank count.
//   gbdt_quantile_eval  the `quantile` metric's sums over K outputs
#include <algorithm>

#include "host/gbdt_quantile_plan.h"
#include "wh_common.h"
#include "wh_kernels.h"

namespace wh {
namespace {

constexpr int kQselThreads = 256;
static_assert(kQselThreads == kQselBins, "k_qsel_hist: one lane per bin");

__global__ __launch_bounds__(kQselThreads) void k_qsel_key(
    const int32_t* __restrict__ ridx, int64_t npos, int64_t nrow, const float* __restrict__ label,
    const float* __restrict__ at, const float* __restrict__ weight,
    const uint8_t* __restrict__ keep, const double* __restrict__ scale,
    uint32_t* __restrict__ key, int64_t* __restrict__ u) {
  const double sc = scale ? scale[0] : 1.0;
  for (int64_t p = (int64_t)blockIdx.x * kQselThreads + threadIdx.x; p < npos;
       p += (int64_t)gridDim.x * kQselThreads) {
    const int64_t row = ridx[p];
    uint32_t k = 0;
    int64_t w = 0;
    if (row >= 0 && row < nrow) {  // (a position outside the matrix weighs nothing)
      k = qsel_key(label[row] - at[row]);
      w = qsel_weight(weight ? weight[row] : 1.f, keep ? keep[row] != 0 : true, sc);
    }
    key[p] = k;
    u[p] = w;
  }
}

// One block per task. A lane keeps the running sum of its current digit in a
// register and goes to the LDS only when the digit changes: residuals crowd
// into a few top digits, where every lane would otherwise hit the same bin.
__global__ __launch_bounds__(kQselThreads) void k_qsel_hist(
    const uint32_t* __restrict__ key, const int64_t* __restrict__ u, int64_t npos,
    const int32_t* __restrict__ tasks, int L, const int64_t* __restrict__ state, int pass,
    int64_t* __restrict__ part) {
  __shared__ unsigned long long bins[kQselBins];
  const int t = blockIdx.x;
  bins[threadIdx.x] = 0;  // (kQselThreads == kQselBins)
  __syncthreads();
  const int leaf = tasks[3 * t];
  const int64_t b_ = tasks[3 * t + 1], e_ = tasks[3 * t + 2];
  const int64_t beg = b_ < 0 ? 0 : b_, end = e_ > npos ? npos : e_;
  if (leaf >= 0 && leaf < L && (pass == 0 || state[kQselState * leaf + 1] > 0)) {
    const uint32_t prefix = (uint32_t)state[kQselState * leaf];
    int cur = -1;
    unsigned long long acc = 0;
    for (int64_t i = beg + threadIdx.x; i < end; i += kQselThreads) {
      const uint32_t k = key[i];
      const int64_t w = u[i];
      if (w == 0 || !qsel_match(k, prefix, pass)) continue;
      const int d = qsel_digit(k, pass);
      if (d != cur) {
        if (acc) atomicAdd(&bins[cur], acc);
        cur = d;
        acc = 0;
      }
      acc += (unsigned long long)w;
    }
    if (acc) atomicAdd(&bins[cur], acc);
  }
  __syncthreads();
  part[(int64_t)t * kQselBins + threadIdx.x] = (int64_t)bins[threadIdx.x];
}

// red {leaf, first task, chunks}: hist[leaf] = the sum of its tasks' partials
__global__ __launch_bounds__(kQselThreads) void k_qsel_reduce(
    const int64_t* __restrict__ part, int64_t ntask, const int32_t* __restrict__ red, int L,
    int64_t* __restrict__ hist) {
  const int leaf = red[3 * blockIdx.x], t0 = red[3 * blockIdx.x + 1];
  const int nch = red[3 * blockIdx.x + 2];
  if (leaf < 0 || leaf >= L || t0 < 0 || nch < 0 || (int64_t)t0 + nch > ntask) return;
  int64_t s = 0;
  for (int c = 0; c < nch; ++c) s += part[(int64_t)(t0 + c) * kQselBins + threadIdx.x];
  hist[(int64_t)leaf * kQselBins + threadIdx.x] = s;
}

// One wave per leaf: lane l owns bins 4l .. 4l + 3. The same decisions as
// qsel_pick of the plan header.
__global__ __launch_bounds__(kQselThreads) void k_qsel_pick(
    const int64_t* __restrict__ hist, int L, int pass, double alpha, int64_t* __restrict__ state) {
  const int lane = threadIdx.x & 63;
  const int leaf = blockIdx.x * (kQselThreads / 64) + (threadIdx.x >> 6);
  if (leaf >= L) return;  // (whole waves leave: the shuffles below stay full)
  const int64_t* h = hist + (int64_t)leaf * kQselBins + 4 * lane;
  const long long b0 = h[0], b1 = h[1], b2 = h[2], b3 = h[3];
  const long long own = b0 + b1 + b2 + b3;
  long long incl = own;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  long long rem = state[kQselState * leaf + 1];
  long long prefix = state[kQselState * leaf];
  if (pass == 0) {
    const long long W = __shfl(incl, 63, 64);
    rem = W > 0 ? qsel_threshold(alpha, W) : 0;
    prefix = 0;
    if (lane == 0 && rem == 0) {
      state[kQselState * leaf] = 0;
      state[kQselState * leaf + 1] = 0;
    }
  }
  if (rem <= 0) return;
  long long below = incl - own;
  if (!(below < rem && rem <= incl)) return;  // exactly one lane holds the crossing
  int d = 4 * lane;
  if (below + b0 < rem) {
    below += b0, ++d;
    if (below + b1 < rem) {
      below += b1, ++d;
      if (below + b2 < rem) below += b2, ++d;
    }
  }
  state[kQselState * leaf] = prefix | ((long long)d << (24 - 8 * pass));
  state[kQselState * leaf + 1] = rem - below;
}

// out [2, L]: the selected residual, then 1 for a leaf without weight
__global__ __launch_bounds__(kQselThreads) void k_qsel_value(const int64_t* __restrict__ state,
                                                             int L, float* __restrict__ out) {
  const int l = blockIdx.x * kQselThreads + threadIdx.x;
  if (l >= L) return;
  const bool empty = state[kQselState * l + 1] <= 0;
  out[l] = empty ? 0.f : qsel_unkey((uint32_t)state[kQselState * l]);
  out[L + l] = empty ? 1.f : 0.f;
}

// ---- the `quantile` metric: {sum_i w_i sum_k pinball_k, sum_i w_i} in fp64
// from the fp32 inputs; per-block partials, then one block sums them in a
// fixed order (the same bits every run).
constexpr int kQevBlocks = 1024;

__device__ __forceinline__ double qev_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ void qev_block_sum(double (&v)[2], double (*sh)[kQselThreads / 64]) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (int q = 0; q < 2; ++q) {
    v[q] = qev_wave_sum(v[q]);
    if (lane == 0) sh[q][wid] = v[q];
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int q = 0; q < 2; ++q) {
      v[q] = 0;
      for (int w = 0; w < kQselThreads / 64; ++w) v[q] += sh[q][w];
    }
}

__global__ __launch_bounds__(kQselThreads) void k_quantile_eval(
    int64_t n, int K, const float* __restrict__ margin, const float* __restrict__ label,
    const float* __restrict__ weight, const double* __restrict__ alphas,
    double* __restrict__ part) {
  __shared__ double sh[2][kQselThreads / 64];
  double v[2] = {0, 0};
  for (int64_t i = (int64_t)blockIdx.x * kQselThreads + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kQselThreads) {
    const double y = (double)label[i], w = weight ? (double)weight[i] : 1.0;
    double s = 0;
    for (int k = 0; k < K; ++k) {
      const double a = alphas[k], d = y - (double)margin[(int64_t)k * n + i];
      s += d >= 0 ? a * d : (a - 1.0) * d;
    }
    v[0] += w * s;
    v[1] += w;
  }
  qev_block_sum(v, sh);
  if (threadIdx.x == 0) part[2 * blockIdx.x] = v[0], part[2 * blockIdx.x + 1] = v[1];
}

__global__ __launch_bounds__(kQselThreads) void k_quantile_eval_sum(
    const double* __restrict__ part, int nb, double* __restrict__ out) {
  __shared__ double sh[2][kQselThreads / 64];
  double v[2] = {0, 0};
  for (int b = threadIdx.x; b < nb; b += kQselThreads) v[0] += part[2 * b], v[1] += part[2 * b + 1];
  qev_block_sum(v, sh);
  if (threadIdx.x == 0) out[0] = v[0], out[1] = v[1];
}

}  // namespace

void gbdt_qsel_key(const int32_t* ridx, int64_t npos, int64_t nrow, const float* label,
                   const float* at, const float* weight, const uint8_t* keep, const double* scale,
                   uint32_t* key, int64_t* u, hipStream_t s) {
  if (npos <= 0) return;
  const int nb = (int)std::min<int64_t>((npos + kQselThreads - 1) / kQselThreads, 4096);
  hipLaunchKernelGGL(k_qsel_key, dim3(nb), dim3(kQselThreads), 0, s, ridx, npos, nrow, label, at,
                     weight, keep, scale, key, u);
}

void gbdt_qsel_hist(const uint32_t* key, const int64_t* u, int64_t npos, const int32_t* tasks,
                    int64_t ntask, const int32_t* red, int64_t nred, int L, const int64_t* state,
                    int pass, int64_t* part, int64_t* hist, hipStream_t s) {
  if (ntask <= 0 || nred <= 0 || L <= 0) return;
  hipLaunchKernelGGL(k_qsel_hist, dim3((unsigned)ntask), dim3(kQselThreads), 0, s, key, u, npos,
                     tasks, L, state, pass, part);
  hipLaunchKernelGGL(k_qsel_reduce, dim3((unsigned)nred), dim3(kQselThreads), 0, s, part, ntask,
                     red, L, hist);
}

void gbdt_qsel_pick(const int64_t* hist, int L, int pass, double alpha, int64_t* state,
                    hipStream_t s) {
  if (L <= 0) return;
  const int per = kQselThreads / 64;
  hipLaunchKernelGGL(k_qsel_pick, dim3((L + per - 1) / per), dim3(kQselThreads), 0, s, hist, L,
                     pass, alpha, state);
}

void gbdt_qsel_value(const int64_t* state, int L, float* out, hipStream_t s) {
  if (L <= 0) return;
  hipLaunchKernelGGL(k_qsel_value, dim3((L + kQselThreads - 1) / kQselThreads),
                     dim3(kQselThreads), 0, s, state, L, out);
}

int64_t gbdt_quantile_eval_scratch() { return 2 * (int64_t)kQevBlocks; }

void gbdt_quantile_eval(int64_t n, int K, const float* margin, const float* label,
                        const float* weight, const double* alphas, double* scratch, double* out,
                        hipStream_t s) {
  if (n <= 0 || K <= 0) return;
  const int nb = (int)std::min<int64_t>((n + kQselThreads - 1) / kQselThreads, kQevBlocks);
  hipLaunchKernelGGL(k_quantile_eval, dim3(nb), dim3(kQselThreads), 0, s, n, K, margin, label,
                     weight, alphas, scratch);
  hipLaunchKernelGGL(k_quantile_eval_sum, dim3(1), dim3(kQselThreads), 0, s, scratch, nb, out);
}

}  // namespace wh
