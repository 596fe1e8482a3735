// Fused factorization-machine / linear forward and backward on a localized
// minibatch (K4-K10 in SURVEY §2.5).
//
// Reference math (learn/difacto/loss.h:53-158, learn/linear/loss.h:92-157):
//   py   = X w + 0.5 * sum_d ((X V)_d^2 - ((X.*X)(V.*V))_d)
//   p    = dual(py)                       (logit: -y / (1 + exp(y py)))
//   gw   = X^T p
//   gV   = X^T diag(p) X V - diag((X.*X)^T p) V
// The reference does this with 2 SpMV + 4 SpMM passes and several
// elementwise loops; here it is ONE forward kernel (a lane group of
// G = vstride/4 lanes per row, float4 per lane: wave64 holds 64/G rows) that
// also emits loss/objective/accuracy sums and the dual, and ONE backward
// kernel that walks each key's occurrence list (the CSC produced by
// localize) so gradients are segmented sums, not scattered atomics. Only
// keys whose occurrence list is longer than one chunk (hot features) use
// float atomics, one per chunk.
//
// Variable-length model layout (the ZVPull/ZVPush value layout of
// learn/difacto/async_sgd.h:234-244, made dense): a pulled minibatch model is
//   hdr[U]  float2 {w, vidx}   vidx = bit-cast int32 row in vc, or -1
//   vc[m]   vstride floats     embedding rows of the keys that have one
// and the gradient mirrors it: gw[U] + gvc[m] (same vidx numbering). Only the
// m keys with an embedding move 256 bytes; the rest move 8 (pull) / 4 (push).
#include "wh_common.h"
#include <string>
#include "kv_device.h"
#include "wh_chunk_plan.h"
#include "wh_kernels.h"
#include "wh_lookback.h"
#include "wh_loss.h"

#include <algorithm>
#include <cstdlib>
#include <type_traits>

namespace wh {
namespace {

constexpr int kThreads = 256;
// cap of the persistent forward grid; resident_blocks sizes it to what fits
// the deep instantiation (k_fm_fwd<16, 10>: 126 VGPRs, 4 waves per SIMD = 4
// blocks per CU; k_fm_fwd<16, 4> needs 94 and runs on the same grid)
constexpr int kFwdBlocks = 2048;

// Memory-level parallelism decides both FM kernels: every V / xv row is a
// dependent gather (index load -> header -> row), and 256-byte rows only
// reach the L2 / Infinity-Cache gather rates with many independent loads in
// flight per wave. tools/microbench/fm_gather_bench.hip measured the forward's
// 1 GB of row gathers per 100k-row minibatch at 189 us with G-lane groups
// issuing 8 rows at a time vs 65 us with ONE WAVE PER ROW issuing all its rows
// at once (15 TB/s), so both kernels use the wave-per-item shape:
//   lanes = SUB sub-groups x G lanes (G = vstride/4, a float4 slice each);
//   one wave-instruction gathers SUB rows; up to TI (backward) / FwdDepth
//   (forward) instructions in flight.
template <int G>
struct Shape {
  static constexpr int SUB = 64 / G;             // rows per wave-instruction
  static constexpr int NI = G;                   // instructions per 64 items
#ifndef WH_FM_TI
#define WH_FM_TI 4
#endif
  // instructions per gather batch: a batch only runs while it covers live
  // slots, so short rows / chunks issue ceil(n / (SUB * TI)) batches instead
  // of all NI instructions (rocprof: the forward was issue-bound at 43 %
  // instruction share with 64 slots per row for 39 non-zeros)
  static constexpr int TI = G < WH_FM_TI ? G : WH_FM_TI;
  static constexpr int VS = 4 * G;               // row stride in floats (= vstride)
};

// Instructions per gather batch of the forward's DEEP schedule
// (WH_FM_FWD_DEPTH=10; the default is Shape::TI, as in k_bwd_v). At G = 16 it
// covers 40 compacted slots, a whole headline row (37 embedded ids on average):
// one wait per row instead of three. What makes it fit 4 waves per SIMD: one
// base pointer with 32-bit element offsets, dead slots gathering the pass's
// first row, the scalars re-read from the LDS stage at accumulate time
// (126 VGPRs; with a per-slot pointer pair and the scalars held in registers
// 8-deep batches took 154 VGPRs and 3 waves). Measured
// (profiles/fm_fwd_rowbatch.txt): alone k_fm_fwd<16> runs 121.6 us deep
// against 136.7 us 4-deep (133.6 us before the register diet); inside the
// headline step, beside the localize and AUC streams, the deep schedule is
// level or behind (587.8-596.5 against 579.9-590.0 us per step), so it is not
// the default. The other widths keep TI: they are not the headline and their
// occupancy must not fall.
template <int G>
struct FwdDepth {
  static constexpr int kDeep = G == 16 ? 10 : Shape<G>::TI;
};

// A backward gather slot without a row reads this zero row instead of
// branching around the load (a predicated load costs an exec-mask branch per
// gather). The forward has one base and zeroes a dead slot's value instead.
__device__ float kZeroRow[256];

// Per-wave LDS staging of the 64 (row index, scalar) pairs of a pass, stored
// transposed ([sub][t]) so that lane (sub, gl) reads the pairs of its
// instructions t = 0.. as consecutive 8-byte entries (ds_read_b128 pairs,
// broadcast across the G lanes of the sub-group) instead of two ds_bpermute
// per gathered row.
template <int G>
__device__ __forceinline__ void stage_pairs(int2* st, int lane, int idx_val, float f) {
  using S = Shape<G>;
  st[(lane % S::SUB) * S::NI + lane / S::SUB] = make_int2(idx_val, __float_as_int(f));
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Forward staging: only the ids that HAVE an embedding row are staged,
// compacted to the front (the others contribute nothing to the
// second-order term). Slots past the returned count hold stale pairs: the
// reader masks them by position.
template <int G>
__device__ __forceinline__ int stage_pairs_compact(int2* st, int lane, int vid, float f) {
  using S = Shape<G>;
  const bool has = vid >= 0;
  const uint64_t m = __ballot(has);
  const int nv = __popcll(m);
  const int pos = __popcll(m & ((1ull << lane) - 1ull));
  if (has) st[(pos % S::SUB) * S::NI + pos / S::SUB] = make_int2(vid, __float_as_int(f));
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  return nv;
}

template <int G, int FI>
__global__ __launch_bounds__(kThreads) void k_fm_fwd(int64_t nrows, const int64_t* __restrict__ off,
                                                     const int32_t* __restrict__ lid,
                                                     const float* __restrict__ val,
                                                     const float2* __restrict__ hdr,
                                                     const float* __restrict__ vc, int vstride,
                                                     const float* __restrict__ label, int loss,
                                                     float* __restrict__ py_out,
                                                     float* __restrict__ dual_out,
                                                     float* __restrict__ xv, double* part,
                                                     double* met, unsigned int* ticket, int acc5) {
  // Persistent waves, one example (row) at a time, software-pipelined over
  // the wave's rows so each row exposes ~one memory round trip instead of
  // four: while row i's embedding rows are gathered, the headers of row i+1,
  // the ids of row i+2 and the CSR bounds of row i+3 are in flight. The
  // gathers are issued first and the prefetches after them, so the in-order
  // vmcnt wait before the accumulation covers the gathers only. A pass of 64
  // ids gathers its compacted slots in batches of SUB x FI (FI: Shape::TI,
  // or FwdDepth::kDeep behind WH_FM_FWD_DEPTH=10), one wait per batch; the
  // per-lane sums run over the slots in ascending order whatever FI is.
  using S = Shape<G>;
  __shared__ double sh[kThreads / 64];
  __shared__ int2 stage[kThreads / 64][64];
  const int lane = threadIdx.x & 63, gl = lane & (G - 1), sub = lane / G;
  const int64_t nw = (int64_t)gridDim.x * (kThreads / 64);
  const int64_t w0 =
      __builtin_amdgcn_readfirstlane((int)(((int64_t)blockIdx.x * kThreads + threadIdx.x) >> 6));
  double m_objv = 0, m_objw = 0, m_corr = 0, m_n = 0;
  auto bounds = [&](int64_t r, int64_t& b, int64_t& e) {
    if (r < nrows) {
      b = off[r];
      e = off[r + 1];
    } else {
      b = e = 0;
    }
  };
  auto load_ids = [&](int64_t b, int64_t e, int& l, float& x) {
    const bool ok = b + lane < e;
    l = ok ? lid[b + lane] : -1;
    x = ok ? (val ? val[b + lane] : 1.f) : 0.f;
  };
  auto load_hdr = [&](int l) {
    return l >= 0 ? hdr[l] : make_float2(0.f, __int_as_float(-1));
  };
  int2* st = stage[threadIdx.x >> 6];
  // gather the embedding rows of one 64-id pass and accumulate them
  auto gather = [&](int vid, float x, float4& s, float4& q2, bool prefetch_first,
                    auto&& prefetch) {
    const int n = stage_pairs_compact<G>(st, lane, vid, x);
    if (n == 0) return;
    // a dead slot gathers the pass's first row (always live, and one base
    // serves every slot); its value is zeroed below, never multiplied: 0 x Inf
    const uint32_t row0 = (uint32_t)st[0].x;
#pragma unroll
    for (int b = 0; b < (S::NI + FI - 1) / FI; ++b) {
      const int t0 = b * FI;
      if (t0 * S::SUB >= n) break;
      float4 v[FI];
#pragma unroll
      for (int t = 0; t < FI; ++t) {
        if (t0 + t >= S::NI) continue;                  // (the last batch of a pass is shorter)
        const bool live = (t0 + t) * S::SUB + sub < n;  // compacted slots only
        const uint32_t row = live ? (uint32_t)st[sub * S::NI + t0 + t].x : row0;
        v[t] = reinterpret_cast<const float4*>(vc + row * (uint32_t)S::VS)[gl];
      }
      if (t0 == 0 && prefetch_first) prefetch();
      // the scalars are read from the stage again here, not held in registers
      // beside the gathers in flight (the barrier keeps the two reads apart)
      asm volatile("" ::: "memory");
#pragma unroll
      for (int t = 0; t < FI; ++t) {
        if (t0 + t >= S::NI) continue;
        const bool live = (t0 + t) * S::SUB + sub < n;
        const float xu = live ? __int_as_float(st[sub * S::NI + t0 + t].y) : 0.f;
        const float xx = xu * xu;
        const float4 u = live ? v[t] : make_float4(0.f, 0.f, 0.f, 0.f);
        s.x += xu * u.x; s.y += xu * u.y; s.z += xu * u.z; s.w += xu * u.w;
        q2.x += xx * u.x * u.x; q2.y += xx * u.y * u.y;
        q2.z += xx * u.z * u.z; q2.w += xx * u.w * u.w;
      }
    }
  };
  int64_t r = w0;
  int64_t bc, ec, bn, en, b2, e2, b3 = 0, e3 = 0;
  bounds(r, bc, ec);
  bounds(r + nw, bn, en);
  bounds(r + 2 * nw, b2, e2);
  int lc, ln, l2 = -1;
  float xc, xn, x2 = 0.f;
  load_ids(bc, ec, lc, xc);
  float2 hc = load_hdr(lc), hn = make_float2(0.f, 0.f);
  load_ids(bn, en, ln, xn);
  for (; r < nrows; r += nw) {
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f), q2 = s;
    float wl = xc * hc.x;
    bool fetched = false;
    auto prefetch = [&]() {
      hn = load_hdr(ln);
      load_ids(b2, e2, l2, x2);
      bounds(r + 3 * nw, b3, e3);
      fetched = true;
    };
    gather(__float_as_int(hc.y), xc, s, q2, true, prefetch);
    if (!fetched) prefetch();  // empty row
    for (int64_t pb = bc + 64; pb < ec; pb += 64) {  // rest of a long row, unpipelined
      int l;
      float x;
      load_ids(pb, ec, l, x);
      const float2 h = load_hdr(l);
      wl += x * h.x;
      gather(__float_as_int(h.y), x, s, q2, false, prefetch);
    }
    // sum the SUB partial rows: lanes gl, gl+G, gl+2G, ... hold the same dims
#pragma unroll
    for (int o = G; o < 64; o <<= 1) {
      s.x += __shfl_xor(s.x, o, 64); s.y += __shfl_xor(s.y, o, 64);
      s.z += __shfl_xor(s.z, o, 64); s.w += __shfl_xor(s.w, o, 64);
      q2.x += __shfl_xor(q2.x, o, 64); q2.y += __shfl_xor(q2.y, o, 64);
      q2.z += __shfl_xor(q2.z, o, 64); q2.w += __shfl_xor(q2.w, o, 64);
    }
    const float wsum = wave_sum(wl);
    float pt = (s.x * s.x - q2.x) + (s.y * s.y - q2.y) + (s.z * s.z - q2.z) + (s.w * s.w - q2.w);
    pt = group_sum<G>(pt);
    if (sub == 0) reinterpret_cast<float4*>(xv + r * vstride)[gl] = s;
    if (lane == 0) {
      const float p = wsum + 0.5f * pt;
      const float y = label[r];
      const LossOut o = eval_loss(loss, y, p);
      const LossOut ow = eval_loss(loss, y, wsum);
      py_out[r] = p;
      dual_out[r] = o.dual;
      m_objv += o.objv;
      m_objw += ow.objv;
      m_corr += ((y > 0.f && p > 0.f) || (y <= 0.f && p <= 0.f)) ? 1.0 : 0.0;
      m_n += 1.0;
    }
    // rotate the pipeline
    bc = bn; ec = en; xc = xn; hc = hn;
    bn = b2; en = e2; ln = l2; xn = x2;
    b2 = b3; e2 = e3;
  }
  block_partials(part, sh, m_objv, m_objw, m_corr, m_n, met, ticket, acc5);
}

// linear model: G lanes stride over one row's non-zeros; persistent over rows
template <int G>
__global__ __launch_bounds__(kThreads) void k_lin_fwd(int64_t nrows, const int64_t* __restrict__ off,
                                                      const int32_t* __restrict__ lid,
                                                      const float* __restrict__ val,
                                                      const float* __restrict__ w, int wstride,
                                                      const float* __restrict__ label, int loss,
                                                      float* __restrict__ py_out,
                                                      float* __restrict__ dual_out, double* part,
                                                      double* met, unsigned int* ticket, int acc5) {
  __shared__ double sh[kThreads / 64];
  const int gl = threadIdx.x & (G - 1);
  const int64_t ngroups = (int64_t)gridDim.x * (kThreads / G);
  double m_objv = 0, m_corr = 0, m_n = 0;
  for (int64_t row = ((int64_t)blockIdx.x * kThreads + threadIdx.x) / G; row < nrows;
       row += ngroups) {
    float acc = 0.f;
    const int64_t b = off[row], e = off[row + 1];
    for (int64_t j = b + gl; j < e; j += G) {
      const int32_t l = lid[j];
      if (wstride == 1) acc += (val ? val[j] : 1.f) * w[l];
      else if (l >= 0) acc += (val ? val[j] : 1.f) * w[(int64_t)l * wstride];  // (table slots)
    }
    acc = group_sum<G>(acc);
    if (gl == 0) {
      const float y = label[row];
      const LossOut o = eval_loss(loss, y, acc);
      py_out[row] = acc;
      dual_out[row] = o.dual;
      m_objv += o.objv;
      m_corr += ((y > 0.f && acc > 0.f) || (y <= 0.f && acc <= 0.f)) ? 1.0 : 0.0;
      m_n += 1.0;
    }
  }
  block_partials(part, sh, m_objv, m_objv, m_corr, m_n, met, ticket, acc5);
}

// ---------------------------------------------------------------- backward
// The two work lists (scalar chunks, V chunks) and their one emitter:
// wh_chunk_plan.h, shared with the open that can emit the plan itself.

// embedding row of key k, -1 without one (hdr == nullptr: the linear model)
__device__ __forceinline__ int32_t key_vidx(const float2* __restrict__ hdr, int64_t k) {
  return hdr ? __float_as_int(hdr[k].y) : -1;
}

// Two-pass plan, for more keys than the look-back scan has tiles:
// k_chunk_count -> one scan per list -> k_chunk_fill.
__global__ __launch_bounds__(kThreads) void k_chunk_count(int64_t nuniq,
                                                          const int64_t* __restrict__ csc_off,
                                                          const float2* __restrict__ hdr,
                                                          int64_t* cnt_s, int64_t* cnt_v) {
  const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (k < nuniq) {
    const bool isv = key_vidx(hdr, k) >= 0;
    const int64_t n = key_chunks(csc_off[k + 1] - csc_off[k], isv);
    cnt_s[k] = isv ? 0 : n;
    cnt_v[k] = isv ? n : 0;
  }
}

__global__ __launch_bounds__(kThreads) void k_chunk_fill(int64_t nuniq,
                                                         const int64_t* __restrict__ csc_off,
                                                         const int64_t* __restrict__ off_s,
                                                         const int64_t* __restrict__ off_v,
                                                         const float2* __restrict__ hdr,
                                                         ChunkOut out) {
  const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  int64_t c0 = 0;
  int32_t nc = 0, b0 = 0, cnt = 0, vid = -1;
  if (k < nuniq) {
    vid = key_vidx(hdr, k);
    const int64_t* off = vid >= 0 ? off_v : off_s;
    c0 = off[k];
    nc = (int32_t)(off[k + 1] - c0);
    b0 = (int32_t)csc_off[k];
    cnt = (int32_t)(csc_off[k + 1] - b0);
  }
  emit_key(out, (int32_t)k, c0, nc, b0, cnt, vid, vid >= 0);
}

// Single-pass version of k_chunk_count -> 2 scans -> k_chunk_fill: each tile
// of 1024 keys (4 per thread) counts its chunks, learns its chunk offsets
// (both lists) by decoupled look-back (wh_lookback.h) and fills its chunks
// in the same launch; the last tile writes the chunk totals to
// off_s[nuniq] / off_v[nuniq].
constexpr int kPlanPer = 4;
constexpr int kPlanTile = kThreads * kPlanPer;

__global__ __launch_bounds__(kThreads) void k_chunk_plan(int64_t nuniq,
                                                         const int64_t* __restrict__ csc_off,
                                                         const float2* __restrict__ hdr,
                                                         Lookback lb, int ntiles,
                                                         int64_t* off_s_tot, int64_t* off_v_tot,
                                                         ChunkOut out) {
  __shared__ uint32_t shs[16];
  __shared__ int sht;
  const int tile = lb_tile(lb, ntiles, &sht);
  const int64_t k0 = (int64_t)tile * kPlanTile + threadIdx.x * kPlanPer;
  int64_t co[kPlanPer + 1];
#pragma unroll
  for (int r = 0; r <= kPlanPer; ++r) co[r] = k0 + r <= nuniq ? csc_off[k0 + r] : 0;
  int32_t vid[kPlanPer];
#pragma unroll
  for (int r = 0; r < kPlanPer; ++r) vid[r] = k0 + r < nuniq ? key_vidx(hdr, k0 + r) : -1;
  uint32_t c[2] = {0u, 0u};
  uint32_t nc[kPlanPer];
#pragma unroll
  for (int r = 0; r < kPlanPer; ++r) {
    nc[r] = k0 + r < nuniq ? (uint32_t)key_chunks(co[r + 1] - co[r], vid[r] >= 0) : 0u;
    c[vid[r] >= 0 ? 1 : 0] += nc[r];
  }
  uint32_t ex[2], tot[2];
  lb_block_scan<2>(lb, tile, c, ex, tot, shs);
  if (tile == ntiles - 1 && threadIdx.x == 0) {
    *off_s_tot = tot[0];
    *off_v_tot = tot[1];
  }
#pragma unroll
  for (int r = 0; r < kPlanPer; ++r) {
    const int isv = vid[r] >= 0;
    emit_key(out, (int32_t)(k0 + r), isv ? ex[1] : ex[0], (int32_t)nc[r], (int32_t)co[r],
             (int32_t)(co[r + 1] - co[r]), vid[r], isv);
    ex[isv ? 1 : 0] += nc[r];
  }
}

// V-chunk order: chunks bucketed by the first row they touch (256 row
// windows of ~400 rows for a 100k minibatch), so the chunks in flight at any
// moment cover a narrow window of rows and their xv gathers hit in L2. A
// key-ordered list had every hot key's chunks sweep all rows concurrently:
// 31% L2 hit rate and 248 us in rocprof, vs 144 us bucketed. A three-kernel
// counting sort (block histograms -> bucket-major scan -> scatter); rocPRIM's
// radix_sort_pairs picks a 10-pass merge sort at this size (124 us).
// The sort digit is row bucket x 2 + class: within each row window the small
// chunks (a single-chunk key of at most `small_n` occurrences, the ones
// k_bwd_v packs SUB to a wave iteration) come first and the rest after, so
// the packed iterations find their SUB small chunks side by side.
constexpr int kBuckets = 256;
constexpr int kDigits = 2 * kBuckets;  // with the class bit (histogram scratch is sized for it)
constexpr int kBucketBlocks = 128;
constexpr int kBucketU = 8;  // chunks per thread with loads in flight together

__device__ __forceinline__ int row_bucket(int row, int shift) {
  const int b = row >> shift;
  return b < kBuckets ? b : kBuckets - 1;
}

// meta.z = n | multi << 8: small means 1 <= n <= small_n and one chunk
__device__ __forceinline__ bool small_chunk(int z, int small_n) { return z >= 1 && z <= small_n; }

// D == kBuckets: the row bucket alone; D == kDigits: row bucket x 2 + class
template <int D>
__device__ __forceinline__ int chunk_digit(int row, int shift, int z, int small_n) {
  const int b = row_bucket(row, shift);
  return D == kBuckets ? b : b * 2 + (small_chunk(z, small_n) ? 0 : 1);
}

template <int D>
__global__ __launch_bounds__(kThreads) void k_vchunk_hist(const int64_t* __restrict__ nchunk_p,
                                                          const int4* __restrict__ meta,
                                                          const int32_t* __restrict__ csc_row,
                                                          int shift, int small_n, int32_t* hist) {
  __shared__ int32_t h[D];
  for (int i = threadIdx.x; i < D; i += kThreads) h[i] = 0;
  __syncthreads();
  const int64_t n = *nchunk_p;
  const int64_t per = (n + gridDim.x - 1) / gridDim.x;
  const int64_t c0 = per * blockIdx.x, c1 = c0 + per < n ? c0 + per : n;
  // kBucketU independent meta -> row load chains in flight per thread (one
  // chain at a time left this kernel waiting on ~17 round trips)
  for (int64_t cb = c0 + threadIdx.x; cb < c1; cb += kThreads * kBucketU) {
    int idx[kBucketU], z[kBucketU], row[kBucketU];
#pragma unroll
    for (int u = 0; u < kBucketU; ++u) {
      const int64_t c = cb + (int64_t)u * kThreads;
      idx[u] = c < c1 ? meta[c].y : -1;
      z[u] = D != kBuckets && c < c1 ? meta[c].z : 0;
    }
#pragma unroll
    for (int u = 0; u < kBucketU; ++u) row[u] = idx[u] >= 0 ? csc_row[idx[u]] : -1;
#pragma unroll
    for (int u = 0; u < kBucketU; ++u)
      if (row[u] >= 0) atomicAdd(&h[chunk_digit<D>(row[u], shift, z[u], small_n)], 1);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < D; i += kThreads) hist[blockIdx.x * D + i] = h[i];
}

// hist[block][digit] -> each count's exclusive offset WITHIN its digit, in
// place, plus the D digit totals in tot[]. kScanBlocks blocks of 1024 own
// D / kScanBlocks digits each; a thread loads kBucketBlocks / kParts counts
// (4 at D = 512, 2 at D = 256: coalesced over the digits, all in flight
// together), and the kParts partial sums of a digit are scanned by shuffles
// in one wave after a transpose through LDS. The scan over the digit totals
// is left to the scatter (digit_bases). One block of 1024 with 64 counts per
// thread spilled at D = 512 (128 VGPRs, 128 bytes of scratch per lane) and
// took 20.0 us where D = 256 took 4.8 (profiles/fm_bwd_packed.txt); this one:
// 21 / 16 VGPRs, no scratch, 2.9 / 2.7 us (profiles/fm_fwd_rowbatch.txt).
constexpr int kScanThreads = 1024;
constexpr int kScanBlocks = 16;

template <int D>
__global__ __launch_bounds__(kScanThreads) void k_vchunk_scan(int32_t* hist, int32_t* tot) {
  constexpr int kOwn = D / kScanBlocks;          // digits of this block: 32 / 16
  constexpr int kParts = kScanThreads / kOwn;    // threads per digit: 32 / 64
  constexpr int kPer = kBucketBlocks / kParts;   // counts per thread: 4 / 2
  static_assert(kParts <= 64 && kPer * kParts == kBucketBlocks, "one wave scans a digit");
  __shared__ int32_t part[kParts][kOwn + 1];
  const int dl = threadIdx.x % kOwn, q = threadIdx.x / kOwn;
  const int d = blockIdx.x * kOwn + dl;
  int32_t v[kPer];
  int32_t sum = 0;
#pragma unroll
  for (int i = 0; i < kPer; ++i) v[i] = hist[(q * kPer + i) * D + d];
#pragma unroll
  for (int i = 0; i < kPer; ++i) sum += v[i];
  part[q][dl] = sum;
  __syncthreads();
  {  // transposed: the kParts lanes of a digit side by side in one wave
    const int tq = threadIdx.x % kParts, td = threadIdx.x / kParts;
    const int32_t t = part[tq][td];
    int32_t x = t;
#pragma unroll
    for (int o = 1; o < kParts; o <<= 1) {
      const int32_t y = __shfl_up(x, o, kParts);
      if (tq >= o) x += y;
    }
    part[tq][td] = x - t;
    if (tq == kParts - 1) tot[blockIdx.x * kOwn + td] = x;
  }
  __syncthreads();
  int32_t base = part[q][dl];
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    hist[(q * kPer + i) * D + d] = base;
    base += v[i];
  }
}

// base[digit] (LDS) = exclusive scan of the D digit totals + this block's
// offset within the digit: every scatter block scans the totals for itself
template <int D>
__device__ __forceinline__ void digit_bases(const int32_t* __restrict__ tot,
                                            const int32_t* __restrict__ within, int32_t* base,
                                            int32_t* wsum) {
  constexpr int kPer = D / kThreads;
  static_assert(kPer * kThreads == D, "digits split evenly over the block");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int32_t t[kPer], w[kPer];
  int32_t sum = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    t[j] = tot[threadIdx.x * kPer + j];
    w[j] = within[threadIdx.x * kPer + j];
    sum += t[j];
  }
  int32_t x = sum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int32_t y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) wsum[wave] = x;
  __syncthreads();
  int32_t off = x - sum;
  for (int k = 0; k < wave; ++k) off += wsum[k];
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    base[threadIdx.x * kPer + j] = off + w[j];
    off += t[j];
  }
  __syncthreads();
}

template <int D>
__global__ __launch_bounds__(kThreads) void k_vchunk_scatter(const int64_t* __restrict__ nchunk_p,
                                                             const int4* __restrict__ meta,
                                                             const int32_t* __restrict__ csc_row,
                                                             int shift, int small_n,
                                                             const int32_t* __restrict__ hist,
                                                             const int32_t* __restrict__ tot,
                                                             int4* out) {
  __shared__ int32_t base[D];
  __shared__ int32_t wsum[kThreads / 64];
  digit_bases<D>(tot, hist + blockIdx.x * D, base, wsum);
  const int64_t n = *nchunk_p;
  const int64_t per = (n + gridDim.x - 1) / gridDim.x;
  const int64_t c0 = per * blockIdx.x, c1 = c0 + per < n ? c0 + per : n;
  for (int64_t cb = c0 + threadIdx.x; cb < c1; cb += kThreads * kBucketU) {
    int4 m[kBucketU];
    int row[kBucketU];
#pragma unroll
    for (int u = 0; u < kBucketU; ++u) {
      const int64_t c = cb + (int64_t)u * kThreads;
      m[u] = c < c1 ? meta[c] : make_int4(0, -1, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < kBucketU; ++u) row[u] = m[u].y >= 0 ? csc_row[m[u].y] : -1;
#pragma unroll
    for (int u = 0; u < kBucketU; ++u)
      if (row[u] >= 0)
        out[atomicAdd(&base[chunk_digit<D>(row[u], shift, m[u].z, small_n)], 1)] = m[u];
  }
}

// scalar chunks: one lane sums dual_i * x_ik over <= kChunkS occurrences
__global__ __launch_bounds__(kThreads) void k_bwd_scalar(const int64_t* __restrict__ nchunk_p,
                                                         const int32_t* __restrict__ chunk_key,
                                                         const int32_t* __restrict__ chunk_beg,
                                                         const int64_t* __restrict__ csc_off,
                                                         const int32_t* __restrict__ csc_row,
                                                         const float* __restrict__ csc_val,
                                                         const float* __restrict__ dual,
                                                         float* __restrict__ gw_out,
                                                         float* __restrict__ part_gw) {
  const int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (c >= *nchunk_p) return;
  const int k = chunk_key[c];
  const int kb = (int)csc_off[k], ke = (int)csc_off[k + 1];
  const int b = chunk_beg[c];
  const int e = b + kChunkS < ke ? b + kChunkS : ke;
  float gw = 0.f;
  int p = b;
  for (; p + 3 < e; p += 4) {  // 4 independent row->dual chains in flight
    int i[4];
    float x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      i[u] = csc_row[p + u];
      x[u] = csc_val ? csc_val[p + u] : 1.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) gw += dual[i[u]] * x[u];
  }
  for (; p < e; ++p) gw += dual[csc_row[p]] * (csc_val ? csc_val[p] : 1.f);
  if (ke - kb <= kChunkS) gw_out[k] = gw;
  else if (part_gw) part_gw[c] = gw;  // deterministic: summed in chunk order later
  else atomicAdd(gw_out + k, gw);
}

// V chunks: one wave per chunk, persistent over the (device-counted) list,
// software-pipelined like the forward: while item i's xv rows are gathered,
// the duals of item i+1, the CSC rows of item i+2 and the list entries after
// them are in flight.
// Packing (fm_bwd_pack): 70 % of the headline's V chunks belong to keys of at
// most 4 occurrences and would use a quarter of a wave or less for a whole
// iteration. A wave therefore takes SUB consecutive list entries: when all
// of them are small (one chunk, n <= TI) they are ONE item, lane group s
// owning key s -- the same gather shape, SUB x TI rows in flight -- else the
// entries are items one by one, as without packing. A packed key's sums
// follow the one-wave tree, so it gets the same bits either way.
// FUSED (FmBwdProblem::fuse_v): the V rows are read from fv, the table's slab
// (vc is null), and a single-chunk key's wave, which holds the key's finished
// gradient row and its V row, applies the AdaGrad step itself (VG row loaded
// beside the V row, behind the gathers) and stores V / VG instead of the gvc
// row. In place is safe: in the backward a V row is read only by its own
// key's chunks, and a single-chunk key has one wave. fv / fvg alias nothing
// declared __restrict__ here. Multi-chunk keys are the same in both variants.
// After the butterfly every one of the 64 / G sub-groups holds the whole row,
// so with 4 or more of them (G <= 16) sub-group s updates component s of each
// float4 -- one element per lane, a quarter of the correctly rounded sqrt /
// divide sequences (~30 VALU instructions per element) that a float4 per
// lane of one sub-group issues. With the float4 form the fused step measured
// level with the unfused one on the headline, with this one 12-20 us per
// step faster (profiles/difacto_open_plan_fused_v.txt).
template <int G, bool FUSED>
__global__ __launch_bounds__(kThreads) void k_bwd_v(const int64_t* __restrict__ nchunk_p,
                                                    const int4* __restrict__ meta,
                                                    const int32_t* __restrict__ csc_row,
                                                    const float* __restrict__ csc_val,
                                                    const float* __restrict__ dual,
                                                    const float* __restrict__ xv,
                                                    const float* __restrict__ vc, int vstride,
                                                    float* __restrict__ gw_out,
                                                    float* __restrict__ gvc,
                                                    float* __restrict__ part_gw,
                                                    float* __restrict__ part_gv, float* fv,
                                                    float* fvg, DifactoHP hp, int pack) {
  using S = Shape<G>;
  constexpr bool kSplit = 64 / G >= 4;  // fused update: one element per lane
  const float* vrows = FUSED ? fv : vc;
  __shared__ int2 stage[kThreads / 64][64];
  int2* st = stage[threadIdx.x >> 6];
  const int lane = threadIdx.x & 63, gl = lane & (G - 1), sub = lane / G;
  const int64_t nch = *nchunk_p, nw = (int64_t)gridDim.x * (kThreads / 64);
  // groups of gs list entries: SUB when packing, else one (a wave's chunks
  // spread over the list as evenly as the waves' one-at-a-time walk)
  const bool can_pack = pack != 0 && S::SUB > 1;
  const int gs = can_pack ? S::SUB : 1;
  const int64_t ngrp = (nch + gs - 1) / gs;
  // Blocks b and b + 8 share an XCD (and its L2): the waves of one XCD take
  // nw / 8 consecutive groups of every round of nw, so a row window's xv rows
  // are fetched into one L2 instead of all eight.
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t w0 = (gridDim.x & 7) == 0
                         ? (int64_t)(blockIdx.x & 7) * (nw / 8) + (blockIdx.x >> 3) * (kThreads / 64) + wv
                         : (int64_t)blockIdx.x * (kThreads / 64) + wv;
  const int4 kNone = make_int4(0, 0, 0, -1);
  // group g of the list: lane group `sub` holds entry g * SUB + sub (gs == 1:
  // every lane holds entry g)
  // (one unconditional load at a clamped index: the list's buffer is never
  // empty, and a lane past the end drops what it read)
  const int64_t e_last = nch > 0 ? nch - 1 : 0;
  auto get_group = [&](int64_t g) {
    const int64_t e = g * gs + (can_pack ? sub : 0);
    const int4 m = meta[e < e_last ? e : e_last];
    return e < nch ? m : kNone;
  };
  // The item generator: walks this wave's groups (gq = w0, w0 + nw, ...) and
  // hands out one packed item for a group of SUB small chunks, or the group's
  // chunks one at a time (entry jq). mg: the group's entries, loaded when the
  // generator moves to it, an iteration before it is read.
  int64_t gq = w0;
  int jq = 0;
  int4 mg = get_group(gq);
  // The next item, in two halves. plan_item, at the top of an iteration
  // (every earlier load has landed there; reading mg behind the gathers
  // would make the wave wait for them): a single chunk's description in im,
  // the same in every lane (read from the owning lane group into scalar
  // registers, like the scalar load of a list walked one entry per wave),
  // occurrence i in lane i; packed, lane group s keeps its key's embedding
  // row in vid, occurrence i of that key in lane (s, i). e: the (first)
  // entry's list index; at: the lane's CSC position, -1 without one. Returns
  // false past the end of the list. issue_item, behind the gathers: the loads.
  bool load_mg = false;
  auto plan_item = [&](int4& im, int& vid, bool& pk, int64_t& e, int& at) {
    const bool ok = gq < ngrp;
    pk = can_pack && __ballot(small_chunk(mg.z, S::TI)) == ~0ull;
    e = gq * gs + jq;
    load_mg = true;
    int beg, n, i;
    if (pk) {
      vid = mg.w;
      beg = mg.y;
      n = mg.z;
      i = gl;
    } else {
      const int src = jq * G;
      im = make_int4(__builtin_amdgcn_readlane(mg.x, src), __builtin_amdgcn_readlane(mg.y, src),
                     __builtin_amdgcn_readlane(mg.z, src), __builtin_amdgcn_readlane(mg.w, src));
      beg = im.y;
      n = im.z & 0xff;
      i = lane;
      ++jq;
      load_mg = jq >= gs || gq * gs + jq >= nch;
    }
    at = i < n ? beg + i : -1;
    if (load_mg) {
      gq += nw;
      jq = 0;
    }
    return ok;
  };
  auto issue_item = [&](int at, int& r, float& x) {
    r = at >= 0 ? csc_row[at] : -1;
    x = at >= 0 ? (csc_val ? csc_val[at] : 1.f) : 0.f;
    if (load_mg) mg = get_group(gq);
  };
  int4 mc = kNone, mn = kNone, m2 = kNone;
  int vic = -1, vin = -1, vi2 = -1;
  bool pc, pn, p2 = false;
  int64_t ec, en, e2 = 0;
  int rc, rn, r2 = -1, at2 = -1;
  float xc, xn, x2 = 0.f;
  bool okc = plan_item(mc, vic, pc, ec, at2);
  issue_item(at2, rc, xc);
  float dc = (rc >= 0 ? dual[rc] : 0.f) * xc;
  bool okn = plan_item(mn, vin, pn, en, at2), ok2 = false;
  issue_item(at2, rn, xn);
  float dn = 0.f;
  // the next stages' loads, issued behind the current item's gathers. dn is
  // the dual alone: its product with x is taken when the pipeline rotates
  // (taken here, beside the load, it made the wave wait for the gathers
  // before it issued the loads that follow)
  auto prefetch = [&]() {
    dn = rn >= 0 ? dual[rn] : 0.f;
    issue_item(at2, r2, x2);
  };
  while (okc) {
    ok2 = plan_item(m2, vi2, p2, e2, at2);
    if (pc) {
      // Packed: lane group `sub` owns the small key of entry ec + sub. Its
      // <= TI pairs (lanes gl < n of the group) are staged as the group's
      // instructions t = 0.., so instruction t gathers row t of all SUB keys.
      if (gl < S::TI) st[sub * S::NI + gl] = make_int2(rc, __float_as_int(dc));
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      float4 a[S::TI];
      float du[S::TI];
#pragma unroll
      for (int t = 0; t < S::TI; ++t) {
        const int2 e = st[sub * S::NI + t];
        du[t] = __int_as_float(e.y);
        const float* src = e.x >= 0 ? xv + (uint32_t)e.x * (uint32_t)S::VS : kZeroRow;
        a[t] = reinterpret_cast<const float4*>(src)[gl];
      }
      const uint32_t vat = (uint32_t)vic * (uint32_t)S::VS;
      float4 v = reinterpret_cast<const float4*>(vrows + vat)[gl];
      float4 vg = make_float4(0.f, 0.f, 0.f, 0.f);
      if (FUSED) vg = reinterpret_cast<const float4*>(fvg + vat)[gl];
      const int key = meta[ec + sub].x;  // (read again, not carried: only the gw store needs it)
      prefetch();
      // The same bits as the one-wave-per-chunk path below gives this key:
      // there occurrence i is accumulated by sub-group i % SUB (in order of
      // i), the sub-groups are summed by the xor butterfly, and the
      // sub-groups without an occurrence add +0 at every level they join.
      constexpr int W = S::SUB < S::TI ? S::SUB : S::TI;
      float4 q[W];
#pragma unroll
      for (int j = 0; j < W; ++j) q[j] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int t = 0; t < S::TI; ++t) {
        float4& p = q[t % S::SUB];
        p.x += du[t] * a[t].x; p.y += du[t] * a[t].y;
        p.z += du[t] * a[t].z; p.w += du[t] * a[t].w;
      }
#pragma unroll
      for (int o = 1; o < W; o <<= 1) {
#pragma unroll
        for (int j = 0; j + o < W; j += 2 * o) {
          q[j].x += q[j + o].x; q[j].y += q[j + o].y;
          q[j].z += q[j + o].z; q[j].w += q[j + o].w;
        }
      }
      float4 acc = q[0];
#pragma unroll
      for (int o = W; o < S::SUB; o <<= 1) {
        acc.x += 0.f; acc.y += 0.f; acc.z += 0.f; acc.w += 0.f;
      }
      // wave_sum over lanes 0..TI-1 and zeros: (d0 + d2) + (d1 + d3), each
      // d first + 0 from the upper lanes
      float gw = dc + 0.f, xx = dc * xc + 0.f;
#pragma unroll
      for (int o = S::TI / 2; o > 0; o >>= 1) {
        gw += __shfl_xor(gw, o, 64);
        xx += __shfl_xor(xx, o, 64);
      }
      const float xxp = __shfl(xx, lane & ~(G - 1), 64);
      if (gl == 0) gw_out[key] = gw;
      acc.x -= xxp * v.x; acc.y -= xxp * v.y; acc.z -= xxp * v.z; acc.w -= xxp * v.w;
      if (FUSED) {
        kvd::adagrad4(v, vg, acc, hp);
        reinterpret_cast<float4*>(fv + vat)[gl] = v;
        reinterpret_cast<float4*>(fvg + vat)[gl] = vg;
      } else {
        *reinterpret_cast<float4*>(gvc + (int64_t)vic * vstride + gl * 4) = acc;
      }
    } else {
    const int n = mc.z & 0xff;
    const bool multi = (mc.z >> 8) != 0;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 vg = make_float4(0.f, 0.f, 0.f, 0.f);
    stage_pairs<G>(st, lane, rc, dc);
    // one gather batch of TB instructions starting at instruction t0
    auto batch = [&](auto tb, int t0) {
      constexpr int TB = decltype(tb)::value;
      float4 a[TB];
      float du[TB];
#pragma unroll
      for (int t = 0; t < TB; ++t) {
        const int2 e = st[sub * S::NI + t0 + t];
        du[t] = __int_as_float(e.y);
        const float* src = e.x >= 0 ? xv + (uint32_t)e.x * (uint32_t)S::VS : kZeroRow;
        a[t] = reinterpret_cast<const float4*>(src)[gl];
      }
      if (t0 == 0) {
        v = reinterpret_cast<const float4*>(vrows + (uint32_t)mc.w * (uint32_t)S::VS)[gl];
        if (FUSED && !multi) {
          if (kSplit) vg.x = fvg[(uint32_t)mc.w * (uint32_t)S::VS + gl * 4 + (sub & 3)];
          else vg = reinterpret_cast<const float4*>(fvg + (uint32_t)mc.w * (uint32_t)S::VS)[gl];
        }
        prefetch();
      }
#pragma unroll
      for (int t = 0; t < TB; ++t) {
        acc.x += du[t] * a[t].x; acc.y += du[t] * a[t].y;
        acc.z += du[t] * a[t].z; acc.w += du[t] * a[t].w;
      }
    };
    // full chunks (hot keys) issue every instruction in one batch for the
    // most loads in flight; short chunks issue only the live instructions
    if (n > S::NI * S::SUB / 2) {
      batch(std::integral_constant<int, S::NI>(), 0);
    } else {
#pragma unroll
      for (int t0 = 0; t0 < S::NI; t0 += S::TI) {
        if (t0 * S::SUB >= n) break;
        batch(std::integral_constant<int, S::TI>(), t0);
      }
    }
    if (n == 0) prefetch();  // (chunks are never empty; keep the pipeline consistent anyway)
    const float gw = wave_sum(dc);
    const float xxp = wave_sum(dc * xc);
#pragma unroll
    for (int o = G; o < 64; o <<= 1) {
      acc.x += __shfl_xor(acc.x, o, 64); acc.y += __shfl_xor(acc.y, o, 64);
      acc.z += __shfl_xor(acc.z, o, 64); acc.w += __shfl_xor(acc.w, o, 64);
    }
    if (lane == 0) {
      if (!multi) gw_out[mc.x] = gw;
      else if (part_gw) part_gw[ec] = gw;
      else atomicAdd(gw_out + mc.x, gw);
    }
    acc.x -= xxp * v.x; acc.y -= xxp * v.y; acc.z -= xxp * v.z; acc.w -= xxp * v.w;
    if (FUSED && !multi) {
      if (kSplit) {
        const int comp = sub & 3;
        const float a = comp == 0 ? acc.x : comp == 1 ? acc.y : comp == 2 ? acc.z : acc.w;
        float v1 = comp == 0 ? v.x : comp == 1 ? v.y : comp == 2 ? v.z : v.w;
        kvd::adagrad1(v1, vg.x, a, hp);
        if (sub < 4) {
          const uint32_t at = (uint32_t)mc.w * (uint32_t)S::VS + gl * 4 + comp;
          fv[at] = v1;
          fvg[at] = vg.x;
        }
      } else {
        kvd::adagrad4(v, vg, acc, hp);
        if (sub == 0) {
          reinterpret_cast<float4*>(fv + (uint32_t)mc.w * (uint32_t)S::VS)[gl] = v;
          reinterpret_cast<float4*>(fvg + (uint32_t)mc.w * (uint32_t)S::VS)[gl] = vg;
        }
      }
    } else if (!multi || part_gv) {
      // single chunk: the row itself; deterministic mode: this chunk's
      // partial row (the list is key-major, unbucketed), summed in order later
      float* dst = multi ? part_gv + ec * (int64_t)vstride : gvc + (int64_t)mc.w * vstride;
      if (sub == 0) *reinterpret_cast<float4*>(dst + gl * 4) = acc;
    } else {
      // every sub-group holds the whole row after the butterfly: lane l adds
      // dim l (+ 64 c), so each atomic wave-instruction covers 256
      // contiguous bytes (4 memory-side requests) instead of 16 lanes at a
      // 16-byte stride (16 requests per row)
      float* gv = gvc + (int64_t)mc.w * vstride;
#pragma unroll
      for (int c = 0; c < (S::VS + 63) / 64; ++c) {
        const int d = c * 64 + lane;
        const int src = (d >> 2) & (G - 1);
        const float ax = __shfl(acc.x, src, 64), ay = __shfl(acc.y, src, 64);
        const float az = __shfl(acc.z, src, 64), aw = __shfl(acc.w, src, 64);
        const int comp = d & 3;
        const float a = comp == 0 ? ax : comp == 1 ? ay : comp == 2 ? az : aw;
        if (d < S::VS) atomicAdd(gv + d, a);
      }
    }
    }
    // rotate the pipeline
    mc = mn; vic = vin; pc = pn; okc = okn; ec = en; rc = rn; xc = xn; dc = dn * xn;
    mn = m2; vin = vi2; pn = p2; okn = ok2; en = e2; rn = r2; xn = x2;
  }
}

// Deterministic mode: the partials of every multi-chunk key, summed in chunk
// order (= occurrence order) by one wave per key, found at its first chunk.
__global__ __launch_bounds__(kThreads) void k_bwd_reduce_s(const int64_t* __restrict__ nchunk_p,
                                                           const int32_t* __restrict__ chunk_key,
                                                           const int32_t* __restrict__ chunk_beg,
                                                           const int64_t* __restrict__ csc_off,
                                                           const float* __restrict__ part_gw,
                                                           float* __restrict__ gw_out) {
  const int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (c >= *nchunk_p) return;
  const int k = chunk_key[c];
  const int64_t kb = csc_off[k], cnt = csc_off[k + 1] - kb;
  if (cnt <= kChunkS || chunk_beg[c] != kb) return;
  const int64_t n = (cnt + kChunkS - 1) / kChunkS;
  float s = 0.f;
  for (int64_t q = 0; q < n; ++q) s += part_gw[c + q];
  gw_out[k] = s;
}

__global__ __launch_bounds__(kThreads) void k_bwd_reduce_v(const int64_t* __restrict__ nchunk_p,
                                                           const int4* __restrict__ meta,
                                                           const int64_t* __restrict__ csc_off,
                                                           const float* __restrict__ part_gw,
                                                           const float* __restrict__ part_gv,
                                                           int vstride, float* __restrict__ gw_out,
                                                           float* __restrict__ gvc) {
  const int lane = threadIdx.x & 63;
  const int64_t c = ((int64_t)blockIdx.x * kThreads + threadIdx.x) >> 6;
  if (c >= *nchunk_p) return;
  const int4 m = meta[c];
  if ((m.z >> 8) == 0 || (int64_t)m.y != csc_off[m.x]) return;  // not a hot key's first chunk
  const int64_t cnt = csc_off[m.x + 1] - m.y;
  const int64_t n = (cnt + kChunkV - 1) / kChunkV;
  float g = 0.f;
  for (int64_t q = 0; q < n; ++q) g += part_gw[c + q];
  for (int d = lane; d < vstride; d += 64) {
    float a = 0.f;
    for (int64_t q = 0; q < n; ++q) a += part_gv[(c + q) * vstride + d];
    gvc[(int64_t)m.w * vstride + d] = a;
  }
  if (lane == 0) gw_out[m.x] = g;
}

// gradient clipping / dropout / normalisation on the m embedding-gradient
// rows (reference learn/difacto/loss.h:131-155); m is a device count
__global__ __launch_bounds__(kThreads) void k_grad_post(const int64_t* __restrict__ m_p,
                                                        float* gvc, int vstride, int dim,
                                                        float clip, float dropout, uint64_t seed,
                                                        double* sumsq) {
  // grid-stride (grid capped at 1024 blocks): one sumsq atomic per block
  __shared__ double sh[kThreads / 64];
  const int64_t total = *m_p * vstride;
  double ss = 0;
  for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * kThreads) {
    const int64_t r = t / vstride;
    const int d = (int)(t % vstride);
    if (d >= dim) continue;
    float v = gvc[t];
    if (clip > 0.f) v = fminf(fmaxf(v, -clip), clip);
    if (dropout > 0.f && uhash01(seed, (uint64_t)r, (uint64_t)d) > 1.f - dropout) v = 0.f;
    gvc[t] = v;
    ss += (double)v * v;
  }
  if (sumsq) {
    const double s = block_sum_d(ss, sh);
    if (threadIdx.x == 0) atomicAdd(sumsq, s);
  }
}

__global__ __launch_bounds__(kThreads) void k_grad_scale(const int64_t* __restrict__ m_p,
                                                         float* gvc, int vstride, int dim,
                                                         const double* sumsq) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const double n2 = *sumsq;
  if (n2 < 1e-10 || t / vstride >= *m_p || (int)(t % vstride) >= dim) return;
  gvc[t] = (float)(gvc[t] / sqrt(n2));
}

}  // namespace

// Calls f(std::integral_constant<int, G>) for the lane-group width G =
// vstride / 4 of an embedding row; the bindings admit no other width.
template <typename F>
static void dispatch_g(int G, F&& f) {
  switch (G) {
    case 1: f(std::integral_constant<int, 1>()); break;
    case 2: f(std::integral_constant<int, 2>()); break;
    case 4: f(std::integral_constant<int, 4>()); break;
    case 8: f(std::integral_constant<int, 8>()); break;
    case 16: f(std::integral_constant<int, 16>()); break;
    case 32: f(std::integral_constant<int, 32>()); break;
    case 64: f(std::integral_constant<int, 64>()); break;
    default:
      fprintf(stderr, "fm.hip: no kernel for vstride %d (4 * 2^k <= 256 only)\n", 4 * G);
      abort();
  }
}

int64_t fm_fwd_partials() { return 4 * kFwdBlocks; }
int64_t fwd_ticket_words() { return kArriveWords; }

// CUs the persistent FM kernels leave free for concurrent collectives. A
// persistent grid that fills every CU's wave slots keeps RCCL's channel
// workgroups (all-to-all over xGMI, issued beside the compute) from being
// dispatched until the whole kernel drains, which serialises the transfer
// behind the compute instead of overlapping it. Set by the multi-rank step
// (kv/psx.py: WH_RCCL_CU_RESERVE); 0 on one GPU.
static int g_cu_reserve = 0;

void fm_set_cu_reserve(int cus) { g_cu_reserve = cus < 0 ? 0 : cus; }
int fm_cu_reserve() { return g_cu_reserve; }

// k_bwd_v packs SUB small single-chunk keys into one wave iteration and the
// bucket sort puts them side by side (default). WH_FM_BWD_PACK=0 /
// fm_set_bwd_pack(false): every chunk gets an iteration of its own, in plain
// row-bucket order -- the same bits for every single-chunk key; kept for A/B
// and the tests (profiles/fm_bwd_packed.txt: alone the kernel runs level
// either way, inside the step the packed one is 10 % of the step faster).
static int g_bwd_pack = -1;

void fm_set_bwd_pack(bool on) { g_bwd_pack = on ? 1 : 0; }
bool fm_bwd_pack() {
  if (g_bwd_pack < 0) {
    const char* e = std::getenv("WH_FM_BWD_PACK");
    g_bwd_pack = !(e && std::string(e) == "0");
  }
  return g_bwd_pack == 1;
}

// k_fm_fwd issues Shape<G>::TI gather instructions per batch, as k_bwd_v does
// (4, the default). WH_FM_FWD_DEPTH=10 / fm_set_fwd_depth(10): batches of
// FwdDepth<G>::kDeep, a headline row's 40 slots at once -- the same bits for
// every input (per-lane sums run over the slots in the same order). Alone the
// deep kernel is 15 us faster, inside the step it is not (FwdDepth, above);
// kept for A/B and the tests.
static int g_fwd_depth = -1;

void fm_set_fwd_depth(int depth) { g_fwd_depth = depth == 10 ? 10 : 4; }
int fm_fwd_depth() {
  if (g_fwd_depth < 0) {
    const char* e = std::getenv("WH_FM_FWD_DEPTH");
    g_fwd_depth = e && std::string(e) == "10" ? 10 : 4;
  }
  return g_fwd_depth;
}

static int device_cus() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0;
    WH_HIP_CHECK(hipGetDevice(&dev));
    WH_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  }
  return std::max(1, cus - std::min(g_cu_reserve, cus / 2));
}

// Persistent grids are sized to what is actually resident: blocks per CU from
// the occupancy API (register-limited kernels fit fewer than 8) x CU count,
// so no block waits for a second round behind a full machine.
template <typename K>
static int resident_blocks(K kernel, int cap) {
  const int cus = device_cus();
  int per_cu = 0;
  WH_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kThreads, 0));
  const int n = std::max(1, per_cu) * cus;
  return n < cap ? n : cap;
}

void fm_forward(int64_t nrows, const int64_t* offset, const int32_t* lid, const float* val,
                const float* w_or_hdr, const float* vc, int vstride, const float* label, int loss,
                float* py, float* dual, float* xv, double* met, double* part,
                unsigned int* ticket, hipStream_t s) {
  if (nrows <= 0) return;
  const int acc5 = (loss >> 8) & 1;  // kLossAcc5: met[4] += flipped accuracy
  loss &= 0xff;
  if (vstride == 0) {
    constexpr int G = 8;
    const int nblk = grid_for(nrows * G, kThreads, kFwdBlocks);
    hipLaunchKernelGGL(k_lin_fwd<G>, dim3(nblk), dim3(kThreads), 0, s, nrows, offset, lid, val,
                       w_or_hdr, 1, label, loss, py, dual, part, met, ticket, acc5);
    return;
  }
  const float2* hdr = reinterpret_cast<const float2*>(w_or_hdr);
  dispatch_g(vstride / 4, [&](auto g) {
    constexpr int G = decltype(g)::value;
    // one grid for both depths (the deep kernel's, the larger register count):
    // the rows of a wave, and with them the order of the metric sums, do not
    // depend on the switch
    const int nblk = grid_for(nrows * 64, kThreads,
                              resident_blocks(k_fm_fwd<G, FwdDepth<G>::kDeep>, kFwdBlocks));
    auto run = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(nblk), dim3(kThreads), 0, s, nrows, offset, lid, val, hdr,
                         vc, vstride, label, loss, py, dual, xv, part, met, ticket, acc5);
    };
    if (fm_fwd_depth() == 10) run(k_fm_fwd<G, FwdDepth<G>::kDeep>);
    else run(k_fm_fwd<G, Shape<G>::TI>);
  });
}

void lin_forward_strided(int64_t nrows, const int64_t* offset, const int32_t* lid,
                         const float* val, const float* w, int wstride, const float* label,
                         int loss, float* py, float* dual, double* met, double* part,
                         unsigned int* ticket, hipStream_t s) {
  if (nrows <= 0) return;
  const int acc5 = (loss >> 8) & 1;
  loss &= 0xff;
  // 8 lanes per row (16: 80.3-81.0, 32: 75.4 vs 82.8 M ex/s at 10k rows)
  constexpr int G = 8;
  const int nblk = grid_for(nrows * G, kThreads, kFwdBlocks);
  hipLaunchKernelGGL(k_lin_fwd<G>, dim3(nblk), dim3(kThreads), 0, s, nrows, offset, lid, val, w,
                     wstride, label, loss, py, dual, part, met, ticket, acc5);
}

static int64_t scalar_cap(int64_t nuniq, int64_t nnz) { return nuniq + nnz / kChunkS + 1; }
static int64_t v_cap(int64_t nuniq, int64_t nnz) { return nuniq + nnz / kChunkV + 1; }

static int bucket_shift(int64_t nrows) {
  int shift = 0;
  while ((((nrows - 1) >> shift) >= kBuckets)) ++shift;
  return shift;
}

int64_t fm_bwd_layout(int64_t nuniq, int64_t nnz, int vstride, bool deterministic,
                      FmBwdLayout* out) {
  int64_t at = 0;
  auto carve = [&](int64_t bytes) {
    const int64_t o = at;
    at += (bytes + 255) / 256 * 256;
    return o;
  };
  const int64_t cap_s = scalar_cap(nuniq, nnz), cap_v = vstride > 0 ? v_cap(nuniq, nnz) : 0;
  FmBwdLayout l;
  l.key_s = carve(cap_s * 4);
  l.beg_s = carve(cap_s * 4);
  l.meta_v = carve(2 * cap_v * 16);
  // block histograms, then the digit totals
  l.hist = carve(vstride > 0 ? (int64_t)kDigits * (kBucketBlocks + 1) * 4 : 0);
  l.det_s = carve(deterministic ? cap_s * 4 : 0);
  l.det_vw = carve(deterministic ? cap_v * 4 : 0);
  l.det_v = carve(deterministic ? cap_v * vstride * 4 : 0);
  l.off = carve(2 * (nuniq + 1) * 8);
  l.cnt = carve(2 * nuniq * 8);
  l.scan_tmp = carve(scan_tmp_elems(nuniq) * 8);
  if (out) *out = l;
  return at;
}

FmBwdPlanDst fm_bwd_plan_dst(const FmBwdProblem& p, void* scratch) {
  FmBwdLayout l;
  fm_bwd_layout(p.nuniq, p.nnz, p.vstride, p.deterministic, &l);
  char* base = static_cast<char*>(scratch);
  int64_t* off_s = reinterpret_cast<int64_t*>(base + l.off);
  return {p.csc_off, reinterpret_cast<int32_t*>(base + l.key_s),
          reinterpret_cast<int32_t*>(base + l.beg_s), base + l.meta_v, p.gw, p.gvc, p.vstride,
          off_s + p.nuniq, off_s + p.nuniq + 1 + p.nuniq};
}

void fm_backward(const FmBwdProblem& p, void* scratch, const Lookback* lb, hipStream_t s,
                 FmBwdPhase phase) {
  const int64_t nuniq = p.nuniq;
  if (nuniq <= 0) return;
  const int vstride = p.vstride;
  const float2* hdr = vstride > 0 ? reinterpret_cast<const float2*>(p.hdr) : nullptr;
  FmBwdLayout l;
  fm_bwd_layout(nuniq, p.nnz, vstride, p.deterministic, &l);
  char* base = static_cast<char*>(scratch);
  int32_t* key_s = reinterpret_cast<int32_t*>(base + l.key_s);
  int32_t* beg_s = reinterpret_cast<int32_t*>(base + l.beg_s);
  int4* meta_v = reinterpret_cast<int4*>(base + l.meta_v);
  int64_t* off_s = reinterpret_cast<int64_t*>(base + l.off);
  int64_t* off_v = off_s + nuniq + 1;
  const int64_t cap_s = scalar_cap(nuniq, p.nnz), cap_v = v_cap(nuniq, p.nnz);
  // V chunks ordered by first-row bucket (the second half of meta_v receives
  // the list); deterministic mode keeps the key-major list (partials by
  // index), and so does a minibatch whose xv rows fit in L2 many times over
  // (the bucketing buys locality there is no need for: three launches of host
  // time in a launch-bound small step)
  const bool bucket =
      hdr && !p.deterministic && p.nrows * (int64_t)vstride * 4 > ((int64_t)2 << 20);
  int4* meta_sorted = bucket ? meta_v + cap_v : meta_v;
  const bool pack = fm_bwd_pack();
  if (phase == FmBwdPhase::kAll || phase == FmBwdPhase::kPlan) {
    const ChunkOut out = {key_s, beg_s, meta_v, p.gw, p.gvc, vstride};
    const int64_t ntiles = (nuniq + kPlanTile - 1) / kPlanTile;
    if (lb && ntiles <= kLbMaxTiles) {  // one launch
      hipLaunchKernelGGL(k_chunk_plan, dim3((unsigned)ntiles), dim3(kThreads), 0, s, nuniq,
                         p.csc_off, hdr, *lb, (int)ntiles, off_s + nuniq, off_v + nuniq, out);
    } else {
      int64_t* cnt_s = reinterpret_cast<int64_t*>(base + l.cnt);
      int64_t* cnt_v = cnt_s + nuniq;
      int64_t* scan_tmp = reinterpret_cast<int64_t*>(base + l.scan_tmp);
      const dim3 grid(grid_for(nuniq, kThreads));
      hipLaunchKernelGGL(k_chunk_count, grid, dim3(kThreads), 0, s, nuniq, p.csc_off, hdr, cnt_s,
                         cnt_v);
      scan_i64(cnt_s, off_s, nuniq, scan_tmp, s);
      if (hdr) scan_i64(cnt_v, off_v, nuniq, scan_tmp, s);
      hipLaunchKernelGGL(k_chunk_fill, grid, dim3(kThreads), 0, s, nuniq, p.csc_off, off_s, off_v,
                         hdr, out);
    }
  }
  if (phase != FmBwdPhase::kRun && bucket) {
    int32_t* hist = reinterpret_cast<int32_t*>(base + l.hist);
    int32_t* tot = hist + kDigits * kBucketBlocks;
    const int shift = bucket_shift(std::max<int64_t>(p.nrows, 1));
    // the chunks k_bwd_v packs: <= TI occurrences, where a wave holds 2+ keys
    const int G = vstride / 4;
    const int small_n = pack && G < 64 ? std::min(G, WH_FM_TI) : 0;
    auto sort = [&](auto d) {
      constexpr int D = decltype(d)::value;
      hipLaunchKernelGGL(k_vchunk_hist<D>, dim3(kBucketBlocks), dim3(kThreads), 0, s,
                         off_v + nuniq, meta_v, p.csc_row, shift, small_n, hist);
      hipLaunchKernelGGL(k_vchunk_scan<D>, dim3(kScanBlocks), dim3(kScanThreads), 0, s, hist,
                         tot);
      hipLaunchKernelGGL(k_vchunk_scatter<D>, dim3(kBucketBlocks), dim3(kThreads), 0, s,
                         off_v + nuniq, meta_v, p.csc_row, shift, small_n, hist, tot,
                         meta_sorted);
    };
    // the class bit only where there are small chunks to put side by side
    if (small_n > 0) sort(std::integral_constant<int, kDigits>());
    else sort(std::integral_constant<int, kBuckets>());
  }
  if (phase == FmBwdPhase::kPlan || phase == FmBwdPhase::kBucket) return;
  // chunk counts are device values (off[nuniq]); the scalar kernel launches
  // over the host-side bound and surplus lanes exit; the V kernel is
  // persistent. No host synchronisation in the step.
  const bool det = p.deterministic;
  float* pgs = det ? reinterpret_cast<float*>(base + l.det_s) : nullptr;
  float* pgv_w = det ? reinterpret_cast<float*>(base + l.det_vw) : nullptr;
  float* pgv = det ? reinterpret_cast<float*>(base + l.det_v) : nullptr;
  hipLaunchKernelGGL(k_bwd_scalar, dim3(grid_for(cap_s, kThreads)), dim3(kThreads), 0, s,
                     off_s + nuniq, key_s, beg_s, p.csc_off, p.csc_row, p.csc_val, p.dual, p.gw,
                     pgs);
  if (det)
    hipLaunchKernelGGL(k_bwd_reduce_s, dim3(grid_for(cap_s, kThreads)), dim3(kThreads), 0, s,
                       off_s + nuniq, key_s, beg_s, p.csc_off, pgs, p.gw);
  if (!hdr) return;
  // (an XCD-aware split of the chunk list -- group b % 8 of the blocks on
  // the b % 8-th eighth -- raised this kernel's L2 hit rate 44.5 -> 54.7 %
  // but cost the step 1.5 %: the groups' uneven ends leave a tail beside the
  // concurrent localize; measured round 4, removed)
  dispatch_g(vstride / 4, [&](auto g) {
    constexpr int G = decltype(g)::value;
    auto run = [&](auto kernel, const float* vc) {
      const int64_t vblk = std::min<int64_t>((cap_v + 3) / 4, resident_blocks(kernel, 2048));
      hipLaunchKernelGGL(kernel, dim3((unsigned)vblk), dim3(kThreads), 0, s, off_v + nuniq,
                         meta_sorted, p.csc_row, p.csc_val, p.dual, p.xv, vc, vstride, p.gw,
                         p.gvc, pgv_w, pgv, p.fuse_v, p.fuse_vg, p.fuse_hp, pack ? 1 : 0);
    };
    if (p.fuse_v && p.fuse_v != p.vc) {
      fprintf(stderr, "fm.hip: the fused update needs vc to be the V slab itself\n");
      abort();
    }
    if (p.fuse_v) run(k_bwd_v<G, true>, nullptr);
    else run(k_bwd_v<G, false>, p.vc);
  });
  if (det)
    hipLaunchKernelGGL(k_bwd_reduce_v, dim3(grid_for(cap_v * 64, kThreads)), dim3(kThreads), 0, s,
                       off_v + nuniq, meta_v, p.csc_off, pgv_w, pgv, vstride, p.gw, p.gvc);
}

void fm_grad_post(const int64_t* m, int64_t m_cap, float* gvc, int vstride, int dim, float clip,
                  float dropout, uint64_t seed, double* sumsq, hipStream_t s) {
  if (m_cap <= 0 || vstride == 0) return;
  hipLaunchKernelGGL(k_grad_post, dim3(grid_for(m_cap * vstride, kThreads, 1024)), dim3(kThreads),
                     0, s, m, gvc, vstride, dim, clip, dropout, seed, sumsq);
}

void fm_grad_scale(const int64_t* m, int64_t m_cap, float* gvc, int vstride, int dim,
                   const double* sumsq, hipStream_t s) {
  if (m_cap <= 0 || vstride == 0) return;
  hipLaunchKernelGGL(k_grad_scale, dim3(grid_for(m_cap * vstride, kThreads)), dim3(kThreads), 0,
                     s, m, gvc, vstride, dim, sumsq);
}

}  // namespace wh
