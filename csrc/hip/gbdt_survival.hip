// Survival objectives of the GBDT trainer.
//
// survival:cox -- the first objective whose gradient is not row-local: a
// row's pair needs sums over every row still at risk at its time. With the
// rows in the plan's ascending order of t (host/gbdt_survival_plan.h), m* the
// largest margin and e = exp(m - m*):
//   S_i = sum_{j >= i} e_j                 (inclusive suffix scan)
//   r_i = sum_{heads k <= i} ev_k / S_k    (inclusive prefix scans, two
//   q_i = sum_{heads k <= i} ev_k / S_k^2   channels; ev_k = the events of
//                                           the tie run that starts at k)
//   g_i = w_i (e_i r_i - delta_i), h_i = w_i max(e_i r_i - e_i^2 q_i, 0)
// e, S, r, q are fp64, the pair is fp32. Four launches per round, one per
// device-wide dependency (m* -> S -> (r, q) -> pair):
//   k_cox_max     m* by per-block partials and the arrival ticket
//   k_cox_exp     e in sorted order (the margins' gather), the tiles' sums;
//                 the block that arrives last scans them into tile offsets
//   k_cox_suffix  S by an in-tile scan plus the tile's offset, the tiles'
//                 sums of the two channels; the last block scans those
//   k_cox_pair    r, q by an in-tile scan plus the offsets, the pair
//                 scattered to row order, the root statistics
// Both scans are reduce-then-scan over fixed tiles of kCoxTile positions,
// counted from the LAST position (tile t holds positions n - 1 - t T down to
// n - (t + 1) T), so the suffix and the prefix scan share one tiling. Every
// combination order is fixed -- a thread's items in order, a wave's shuffle
// scan, the waves in order, the tiles in order: no floating-point atomics, no
// look-back, the same bits on every call. A tile's partial crosses to the
// last block as k_gpair_obj's do (one agent-scope store per value, drained,
// then the arrival ticket; agent-scope loads); everything else a later stage
// reads was written by an earlier launch.
//
// survival:aft is row-local: k_gpair_aft<DIST> evaluates host/gbdt_aft.h
// like k_gpair_obj evaluates host/gbdt_objective.h; k_aft_eval is its metric
// kernel (fp64 from the fp32 inputs).
#include <algorithm>
#include <cmath>

#include "host/gbdt_aft.h"
#include "host/gbdt_survival_plan.h"
#include "wh_common.h"
#include "wh_kernels.h"
#include "wh_lookback.h"

namespace wh {
namespace {

constexpr int kSvWaves = kCoxThreads / 64;
constexpr int kSvSlots = 4;  // doubles of a block's partial

__device__ __forceinline__ double ld_part(const double* p) {
  return __longlong_as_double((long long)lb_load(reinterpret_cast<const unsigned long long*>(p)));
}
__device__ __forceinline__ void st_part(double* p, double v) {
  lb_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v));
}

// Block-wide: the threads' {NS sums, NM maxima} v -> the block's, in v of
// thread 0 (fixed order: butterfly, then the waves in order). max0: what the
// maxima start from. Called by every thread.
template <int NS, int NM>
__device__ __forceinline__ void sv_block_reduce(double (&v)[NS + NM], double (*sh)[kSvWaves],
                                                double max0) {
#pragma unroll
  for (int q = 0; q < NS; ++q) v[q] = wave_sum_d(v[q]);
#pragma unroll
  for (int q = NS; q < NS + NM; ++q)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[q] = fmax(v[q], __shfl_xor(v[q], o, 64));
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  __syncthreads();  // (sh may still be read from its last use)
  if (lane == 0)
    for (int q = 0; q < NS + NM; ++q) sh[q][wid] = v[q];
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 0; q < NS + NM; ++q) {
      double t = q < NS ? 0.0 : max0;
      for (int w = 0; w < kSvWaves; ++w) t = q < NS ? t + sh[q][w] : fmax(t, sh[q][w]);
      v[q] = t;
    }
  }
}

// Thread 0 publishes the block's N values at part[block * N ..] and takes the
// arrival ticket; true (in every thread) in the block that arrives last.
template <int N>
__device__ __forceinline__ bool sv_publish(const double (&v)[N], double* part,
                                           unsigned int* ticket, int* last) {
  if (threadIdx.x == 0) {
    for (int q = 0; q < N; ++q) st_part(part + (int64_t)blockIdx.x * N + q, v[q]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    *last = arrive_last(ticket, blockIdx.x, gridDim.x) ? 1 : 0;
  }
  __syncthreads();
  return *last != 0;
}

// The block's values -> per-block partials -> out[NS + NM] by the block that
// arrives last (thread t takes blocks t, t + 256, ...: the same sums every run).
template <int NS, int NM>
__device__ __forceinline__ void sv_finish(double (&v)[NS + NM], double (*sh)[kSvWaves], int* last,
                                          double max0, double* part, unsigned int* ticket,
                                          double* out) {
  constexpr int N = NS + NM;
  sv_block_reduce<NS, NM>(v, sh, max0);
  if (!sv_publish<N>(v, part, ticket, last)) return;
  for (int q = 0; q < N; ++q) v[q] = q < NS ? 0.0 : max0;
  for (unsigned b = threadIdx.x; b < gridDim.x; b += blockDim.x)
    for (int q = 0; q < N; ++q) {
      const double x = ld_part(part + (int64_t)b * N + q);
      v[q] = q < NS ? v[q] + x : fmax(v[q], x);
    }
  sv_block_reduce<NS, NM>(v, sh, max0);
  if (threadIdx.x == 0)
    for (int q = 0; q < N; ++q) out[q] = v[q];
}

// The wave's inclusive scan of x in lane order, and the exclusive one.
__device__ __forceinline__ void sv_wave_scan(double x, double& inc, double& exc) {
  const int lane = threadIdx.x & 63;
  inc = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  const double p = __shfl_up(inc, 1, 64);
  exc = lane ? p : 0.0;
}

// In-tile inclusive scan of C channels: v[c][k] of thread t is the tile's item
// t * kCoxItems + k. Called by every thread.
template <int C>
__device__ __forceinline__ void cox_tile_scan(double (&v)[C][kCoxItems], double (*sh)[kSvWaves]) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  double inc[C], exc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
#pragma unroll
    for (int k = 1; k < kCoxItems; ++k) v[c][k] += v[c][k - 1];
    sv_wave_scan(v[c][kCoxItems - 1], inc[c], exc[c]);
  }
  __syncthreads();
  if (lane == 63)
    for (int c = 0; c < C; ++c) sh[c][wid] = inc[c];
  __syncthreads();
#pragma unroll
  for (int c = 0; c < C; ++c) {
    double base = 0;
    for (int w = 0; w < kSvWaves; ++w)
      if (w < wid) base += sh[c][w];
    const double add = base + exc[c];
#pragma unroll
    for (int k = 0; k < kCoxItems; ++k) v[c][k] += add;
  }
}

// The last block: exclusive scan of the nt tiles' partials (C per tile) into
// off, over the tiles in ascending or descending order. Thread t takes a
// contiguous chunk, the chunks' sums are scanned across the block.
template <int C>
__device__ __forceinline__ void cox_scan_partials(const double* part, int64_t nt, bool descending,
                                                  double* off, double (*sh)[kSvWaves]) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t len = (nt + kCoxThreads - 1) / kCoxThreads;
  const int64_t a0 = (int64_t)threadIdx.x * len, a = a0 < nt ? a0 : nt;
  const int64_t b = a + len < nt ? a + len : nt;
  double s[C], inc[C], exc[C];
  for (int c = 0; c < C; ++c) s[c] = 0;
  for (int64_t i = a; i < b; ++i) {
    const int64_t t = descending ? nt - 1 - i : i;
    for (int c = 0; c < C; ++c) s[c] += ld_part(part + t * C + c);
  }
  for (int c = 0; c < C; ++c) sv_wave_scan(s[c], inc[c], exc[c]);
  __syncthreads();
  if (lane == 63)
    for (int c = 0; c < C; ++c) sh[c][wid] = inc[c];
  __syncthreads();
  double run[C];
  for (int c = 0; c < C; ++c) {
    double base = 0;
    for (int w = 0; w < kSvWaves; ++w)
      if (w < wid) base += sh[c][w];
    run[c] = base + exc[c];
  }
  for (int64_t i = a; i < b; ++i) {
    const int64_t t = descending ? nt - 1 - i : i;
    for (int c = 0; c < C; ++c) {
      off[t * C + c] = run[c];
      run[c] += ld_part(part + t * C + c);
    }
  }
}

// ---- stage 1: m*
__global__ __launch_bounds__(kCoxThreads) void k_cox_max(int64_t n, const float* __restrict__ margin,
                                                         double* __restrict__ part,
                                                         unsigned int* ticket, double* mstar) {
  __shared__ double sh[kSvSlots][kSvWaves];
  __shared__ int last;
  double v[1] = {-INFINITY};
  for (int64_t i = (int64_t)blockIdx.x * kCoxThreads + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kCoxThreads)
    v[0] = fmax(v[0], (double)margin[i]);
  sv_finish<0, 1>(v, sh, &last, -INFINITY, part, ticket, mstar);
}

// ---- stage 2: e in sorted order, the tiles' sums, their scan. Tile t, item
// j (from the last position down): position n - 1 - (t T + j).
__global__ __launch_bounds__(kCoxThreads) void k_cox_exp(
    int64_t n, const float* __restrict__ margin, const int32_t* __restrict__ order,
    const double* __restrict__ mstar, double* __restrict__ e_out, double* __restrict__ part,
    unsigned int* ticket, double* __restrict__ off) {
  __shared__ double sh[kSvSlots][kSvWaves];
  __shared__ int last;
  const double ms = *mstar;
  const int64_t base = (int64_t)blockIdx.x * kCoxTile + (int64_t)threadIdx.x * kCoxItems;
  double v[1] = {0};
#pragma unroll
  for (int k = 0; k < kCoxItems; ++k) {
    const int64_t rp = base + k;
    if (rp < n) {
      const int64_t pos = n - 1 - rp;
      const double e = exp((double)margin[order[pos]] - ms);
      e_out[pos] = e;
      v[0] += e;
    }
  }
  sv_block_reduce<1, 0>(v, sh, 0.0);
  if (!sv_publish<1>(v, part, ticket, &last)) return;
  cox_scan_partials<1>(part, gridDim.x, false, off, sh);
}

// the two channels' terms at a position: ev / S and ev / S^2. (S == 0: every
// e of the risk set underflowed, margins more than ~745 below m*; the run
// then adds nothing, where 1 / S would put inf and 0 x inf = NaN into pairs.)
__device__ __forceinline__ void cox_terms(int32_t ev, double S, double& c1, double& c2) {
  c1 = c2 = 0;
  if (ev && S > 0) {
    c1 = (double)ev / S;
    c2 = c1 / S;
  }
}

// ---- stage 3: S, the tiles' sums of the two channels, their scan
__global__ __launch_bounds__(kCoxThreads) void k_cox_suffix(
    int64_t n, const double* __restrict__ e, const int32_t* __restrict__ run_events,
    const double* __restrict__ off, double* __restrict__ S_out, double* __restrict__ part,
    unsigned int* ticket, double* __restrict__ off2) {
  __shared__ double sh[kSvSlots][kSvWaves];
  __shared__ int last;
  const int64_t base = (int64_t)blockIdx.x * kCoxTile + (int64_t)threadIdx.x * kCoxItems;
  double v[1][kCoxItems];
#pragma unroll
  for (int k = 0; k < kCoxItems; ++k) v[0][k] = base + k < n ? e[n - 1 - (base + k)] : 0.0;
  cox_tile_scan<1>(v, sh);
  const double o = off[blockIdx.x];
  double s[2] = {0, 0};
#pragma unroll
  for (int k = 0; k < kCoxItems; ++k) {
    const int64_t rp = base + k;
    if (rp < n) {
      const int64_t pos = n - 1 - rp;
      const double S = v[0][k] + o;
      S_out[pos] = S;
      double c1, c2;
      cox_terms(run_events[pos], S, c1, c2);
      s[0] += c1;
      s[1] += c2;
    }
  }
  sv_block_reduce<2, 0>(s, sh, 0.0);
  if (!sv_publish<2>(s, part, ticket, &last)) return;
  cox_scan_partials<2>(part, gridDim.x, true, off2, sh);
}

// ---- stage 4: r, q, the pair in row order, the root statistics. The tile's
// items in ascending position: item j is position n - (t + 1) T + j.
__global__ __launch_bounds__(kCoxThreads) void k_cox_pair(
    int64_t n, const double* __restrict__ e, const double* __restrict__ S,
    const int32_t* __restrict__ run_events, const uint8_t* __restrict__ delta,
    const float* __restrict__ weight, const int32_t* __restrict__ order,
    const double* __restrict__ off2, float2* __restrict__ out, double* __restrict__ part,
    unsigned int* ticket, double* stats) {
  __shared__ double sh[kSvSlots][kSvWaves];
  __shared__ int last;
  const int64_t base =
      n - ((int64_t)blockIdx.x + 1) * kCoxTile + (int64_t)threadIdx.x * kCoxItems;
  double v[2][kCoxItems];
#pragma unroll
  for (int k = 0; k < kCoxItems; ++k) {
    const int64_t pos = base + k;
    v[0][k] = v[1][k] = 0;
    if (pos >= 0) cox_terms(run_events[pos], S[pos], v[0][k], v[1][k]);
  }
  cox_tile_scan<2>(v, sh);
  const double o1 = off2[(int64_t)blockIdx.x * 2], o2 = off2[(int64_t)blockIdx.x * 2 + 1];
  double st[4] = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < kCoxItems; ++k) {
    const int64_t pos = base + k;
    if (pos < 0) continue;
    const double ei = e[pos], er = ei * (v[0][k] + o1);
    float g = (float)(er - (delta[pos] ? 1.0 : 0.0));
    float h = (float)fmax(er - ei * ei * (v[1][k] + o2), 0.0);
    if (weight) {
      const float w = weight[pos];
      g *= w;
      h *= w;
    }
    out[order[pos]] = make_float2(g, h);
    st[0] += g;
    st[1] += h;
    st[2] = fmax(st[2], (double)fabsf(g));
    st[3] = fmax(st[3], (double)fabsf(h));
  }
  sv_finish<2, 2>(st, sh, &last, 0.0, part, ticket, stats);
}

// ---- cox-nloglik: {sum over events of ln D(t_i) - (m_i - m*), E} from the
// plan and the first scan: sum_heads ev ln S - sum_i delta_i (m_i - m*)
__global__ __launch_bounds__(kCoxThreads) void k_cox_eval(
    int64_t n, const float* __restrict__ margin, const int32_t* __restrict__ order,
    const uint8_t* __restrict__ delta, const int32_t* __restrict__ run_events,
    const double* __restrict__ S, const double* __restrict__ mstar, double* __restrict__ part,
    unsigned int* ticket, double* out) {
  __shared__ double sh[kSvSlots][kSvWaves];
  __shared__ int last;
  const double ms = *mstar;
  double v[2] = {0, 0};
  for (int64_t pos = (int64_t)blockIdx.x * kCoxThreads + threadIdx.x; pos < n;
       pos += (int64_t)gridDim.x * kCoxThreads) {
    const int32_t ev = run_events[pos];
    if (ev && S[pos] > 0) v[0] += (double)ev * log(S[pos]);
    if (delta[pos]) {
      v[0] -= (double)margin[order[pos]] - ms;
      v[1] += 1.0;
    }
  }
  sv_finish<2, 0>(v, sh, &last, 0.0, part, ticket, out);
}

// ---- survival:aft
constexpr int kAftBlocks = 1024;

template <int DIST>
__global__ __launch_bounds__(kCoxThreads) void k_gpair_aft(
    int64_t n, const float* __restrict__ margin, const float* __restrict__ lower,
    const float* __restrict__ upper, const float* __restrict__ weight, float sigma,
    float2* __restrict__ out, double* __restrict__ part, unsigned int* ticket, double* stats) {
  __shared__ double sh[kSvSlots][kSvWaves];
  __shared__ int last;
  double v[4] = {0, 0, 0, 0};
  for (int64_t i = (int64_t)blockIdx.x * kCoxThreads + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kCoxThreads) {
    const GbdtPair p = gbdt_aft_pair<DIST>(margin[i], lower[i], upper[i], sigma);
    float g = p.g, h = p.h;
    if (weight) {
      const float w = weight[i];
      g *= w;
      h *= w;
    }
    out[i] = make_float2(g, h);
    v[0] += g;
    v[1] += h;
    v[2] = fmax(v[2], (double)fabsf(g));
    v[3] = fmax(v[3], (double)fabsf(h));
  }
  sv_finish<2, 2>(v, sh, &last, 0.0, part, ticket, stats);
}

// out = {sum w nll, sum w, rows with lower <= exp(m) <= upper, rows}
__global__ __launch_bounds__(kCoxThreads) void k_aft_eval(
    int64_t n, const float* __restrict__ margin, const float* __restrict__ lower,
    const float* __restrict__ upper, const float* __restrict__ weight, int dist, double sigma,
    double* __restrict__ part, unsigned int* ticket, double* out) {
  __shared__ double sh[kSvSlots][kSvWaves];
  __shared__ int last;
  double v[4] = {0, 0, 0, 0};
  for (int64_t i = (int64_t)blockIdx.x * kCoxThreads + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kCoxThreads) {
    const double m = margin[i], yl = lower[i], yu = upper[i];
    const double w = weight ? (double)weight[i] : 1.0;
    v[0] += w * gbdt_aft_loss(dist, m, yl, yu, sigma);
    v[1] += w;
    const double p = exp(m);
    v[2] += yl <= p && p <= yu ? 1.0 : 0.0;
    v[3] += 1.0;
  }
  sv_finish<4, 0>(v, sh, &last, 0.0, part, ticket, out);
}

// AFT scratch (doubles): the block partials, then the (zeroed) ticket words
constexpr int64_t kAftTicketAt = (int64_t)kSvSlots * kAftBlocks;

}  // namespace

// ws: gbdt_cox_ws(n).size doubles; ticket: kArriveWords zeroed words (left
// zeroed). The first `upto` (1..3) stages: m*, e, S -- what the pair and the
// metric share (and the benchmark's split).
void gbdt_cox_scan(int64_t n, const float* margin, const int32_t* order,
                   const int32_t* run_events, double* ws, unsigned int* ticket, int upto,
                   hipStream_t s) {
  if (n <= 0) return;
  const CoxWs w = gbdt_cox_ws(n);
  const int nt = (int)gbdt_cox_tiles(n);
  const dim3 blk(kCoxThreads);
  hipLaunchKernelGGL(k_cox_max, dim3(std::min(nt, 1024)), blk, 0, s, n, margin, ws + w.part, ticket,
                     ws + w.mstar);
  if (upto < 2) return;
  hipLaunchKernelGGL(k_cox_exp, dim3(nt), blk, 0, s, n, margin, order, ws + w.mstar, ws + w.e,
                     ws + w.part, ticket, ws + w.off);
  if (upto < 3) return;
  hipLaunchKernelGGL(k_cox_suffix, dim3(nt), blk, 0, s, n, ws + w.e, run_events, ws + w.off,
                     ws + w.S, ws + w.part, ticket, ws + w.off2);
}

void gbdt_gpair_cox(int64_t n, const float* margin, const int32_t* order, const uint8_t* delta,
                    const float* weight_sorted, const int32_t* run_events, double* ws,
                    unsigned int* ticket, float* gpair, double* stats, hipStream_t s) {
  if (n <= 0) return;
  gbdt_cox_scan(n, margin, order, run_events, ws, ticket, 3, s);
  const CoxWs w = gbdt_cox_ws(n);
  const int nt = (int)gbdt_cox_tiles(n);
  const dim3 blk(kCoxThreads);
  hipLaunchKernelGGL(k_cox_pair, dim3(nt), blk, 0, s, n, ws + w.e, ws + w.S, run_events, delta,
                     weight_sorted, order, ws + w.off2, reinterpret_cast<float2*>(gpair),
                     ws + w.part, ticket, stats);
}

// out [2] = {sum over events of (ln D(t_i) - (m_i - m*)), the events}
void gbdt_cox_eval(int64_t n, const float* margin, const int32_t* order, const uint8_t* delta,
                   const int32_t* run_events, double* ws, unsigned int* ticket, double* out,
                   hipStream_t s) {
  if (n <= 0) return;
  gbdt_cox_scan(n, margin, order, run_events, ws, ticket, 3, s);
  const CoxWs w = gbdt_cox_ws(n);
  const int nb = std::min<int>((int)gbdt_cox_tiles(n), 1024);
  hipLaunchKernelGGL(k_cox_eval, dim3(nb), dim3(kCoxThreads), 0, s, n, margin, order, delta,
                     run_events, ws + w.S, ws + w.mstar, ws + w.part, ticket, out);
}

int64_t gbdt_cox_ticket_words() { return kArriveWords; }

int64_t gbdt_aft_scratch() { return kAftTicketAt + kArriveWords / 2 + 1; }

bool gbdt_gpair_aft(int dist, int64_t n, const float* margin, const float* lower,
                    const float* upper, const float* weight, float sigma, float* gpair,
                    double* scratch, double* stats, hipStream_t s) {
  if (dist < 0 || dist >= kAftDistCount) return false;
  if (n <= 0) return true;
  unsigned int* ticket = reinterpret_cast<unsigned int*>(scratch + kAftTicketAt);
  const dim3 grid(grid_for(n, kCoxThreads, kAftBlocks)), blk(kCoxThreads);
  float2* out = reinterpret_cast<float2*>(gpair);
  switch (dist) {
    case kAftNormal:
      hipLaunchKernelGGL(k_gpair_aft<kAftNormal>, grid, blk, 0, s, n, margin, lower, upper, weight,
                         sigma, out, scratch, ticket, stats);
      break;
    case kAftLogistic:
      hipLaunchKernelGGL(k_gpair_aft<kAftLogistic>, grid, blk, 0, s, n, margin, lower, upper,
                         weight, sigma, out, scratch, ticket, stats);
      break;
    default:
      hipLaunchKernelGGL(k_gpair_aft<kAftExtreme>, grid, blk, 0, s, n, margin, lower, upper, weight,
                         sigma, out, scratch, ticket, stats);
      break;
  }
  return true;
}

void gbdt_aft_eval(int dist, int64_t n, const float* margin, const float* lower,
                   const float* upper, const float* weight, double sigma, double* scratch,
                   double* out, hipStream_t s) {
  if (n <= 0) return;
  unsigned int* ticket = reinterpret_cast<unsigned int*>(scratch + kAftTicketAt);
  hipLaunchKernelGGL(k_aft_eval, dim3(grid_for(n, kCoxThreads, kAftBlocks)), dim3(kCoxThreads), 0,
                     s, n, margin, lower, upper, weight, dist, sigma, scratch, ticket, out);
}

}  // namespace wh
