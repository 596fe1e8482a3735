// The FM backward's chunk planner, as device pieces that kernels embed: the
// planners of fm.hip (k_chunk_plan, k_chunk_fill) and the single-shard open
// (kvstore.hip k_difacto_open_pull, which knows every key's embedding row the
// moment it assigns it and has the same 1024-key tiles and a look-back scan
// already) all count with key_chunks and write with the ONE emit_key.
//
// Two work lists over the CSC: keys WITHOUT an embedding are split into
// "scalar" chunks of <= kChunkS occurrences summed by one lane each (gw
// only); keys WITH an embedding into "V" chunks of <= kChunkV = 64
// occurrences, one WAVE each (gw, xxp and the 64-float gV row). A key with
// more than one chunk accumulates its chunks with float atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wh_kernels.h"  // kChunkV, FmBwdPlanDst

namespace wh {

constexpr int kChunkS = 32;  // occurrences per scalar work item

// chunks of a key with cnt occurrences
__device__ __forceinline__ int64_t key_chunks(int64_t cnt, bool isv) {
  return isv ? (cnt + kChunkV - 1) / kChunkV : (cnt + kChunkS - 1) / kChunkS;
}

// What the chunk planners write: the scalar chunk list {key, CSC begin}, the
// V chunk list, one packed int4 {key, CSC begin, n | multi << 8, vidx} each
// (so the backward wave fetches a chunk's description in one load), and the
// zeroed gradients of multi-chunk keys.
struct ChunkOut {
  int32_t* key_s;
  int32_t* beg_s;
  int4* meta_v;
  float* gw;
  float* gvc;
  int vstride;
};

// The plan as a kernel outside fm.hip emits it (csc_off == nullptr: no plan):
// the CSC offsets to count from, the lists, and the two total words
// off_s[nuniq] / off_v[nuniq] that the last tile writes.
struct ChunkPlanArg {
  const int64_t* csc_off;
  ChunkOut out;
  int64_t* tot_s;
  int64_t* tot_v;
};

inline ChunkPlanArg chunk_plan_arg(const FmBwdPlanDst* d) {
  ChunkPlanArg a = {};
  if (d)
    a = {d->csc_off,
         {d->key_s, d->beg_s, static_cast<int4*>(d->meta_v), d->gw, d->gvc, d->vstride},
         d->tot_s, d->tot_v};
  return a;
}

// The chunks [c0, c0 + nc) of key k (CSC begin b0, cnt occurrences, embedding
// row vid when isv). Called by all 64 lanes, each with its own key (nc == 0:
// none): a single-chunk key is written by its lane; a multi-chunk (hot) key
// is expanded by the whole wave, 64 chunks per round, so the hottest key does
// not serialise.
__device__ __forceinline__ void emit_key(const ChunkOut& o, int32_t k, int64_t c0, int32_t nc,
                                         int32_t b0, int32_t cnt, int32_t vid, int isv) {
  const int lane = threadIdx.x & 63;
  if (nc == 1) {
    if (isv) {
      o.meta_v[c0] = make_int4(k, b0, cnt, vid);
    } else {
      o.key_s[c0] = k;
      o.beg_s[c0] = b0;
    }
  }
  uint64_t m = __ballot(nc > 1);
  while (m) {
    const int src = __ffsll((unsigned long long)m) - 1;
    m &= m - 1;
    const int32_t jk = __shfl(k, src, 64);
    const int64_t jc0 = __shfl(c0, src, 64);
    const int32_t jnc = __shfl(nc, src, 64);
    const int32_t jb0 = __shfl(b0, src, 64);
    const int32_t jcnt = __shfl(cnt, src, 64);
    const int32_t jvid = __shfl(vid, src, 64);
    const int jv = __shfl(isv, src, 64);
    for (int32_t q = lane; q < jnc; q += 64) {
      if (jv) {
        const int32_t cb = q * kChunkV;
        const int32_t n = jcnt - cb < kChunkV ? jcnt - cb : kChunkV;
        o.meta_v[jc0 + q] = make_int4(jk, jb0 + cb, n | (1 << 8), jvid);
      } else {
        o.key_s[jc0 + q] = jk;
        o.beg_s[jc0 + q] = jb0 + q * kChunkS;
      }
    }
    if (lane == 0) o.gw[jk] = 0.f;
    if (jv) {
      for (int d = lane * 4; d < o.vstride; d += 256)
        *reinterpret_cast<float4*>(o.gvc + (int64_t)jvid * o.vstride + d) =
            make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
}

}  // namespace wh
