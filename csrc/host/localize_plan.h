// The localize job's host bookkeeping (csrc/bind/localize_ops.cc): how a
// job's hash table and partition plan are sized from the caller's hint, which
// of the device's two scratch tables a job gets and whether it must be
// refilled first, which heavy-id hints a partitioned job may read, and
// whether a count payload reports an overflow. Free of HIP and torch: the
// binding and the host self-test compile the same code.
#pragma once

#include <algorithm>
#include <cstdint>

namespace wh {

inline int64_t loc_pow2(int64_t x) {
  int64_t p = 1;
  while (p < x) p <<= 1;
  return p;
}

// (non-zeros, unique ids) of the device's last finished localize. A caller's
// hint is the previous minibatch's unique count, scaled here by the non-zero
// ratio when this minibatch is larger (uneven minibatches: CRB records cut
// parts into short and long blocks; an unscaled hint under-sized the plan,
// every partition overflowed LDS and the job fell back to the hash path).
struct LocHintScale {
  int64_t last_nnz = 0, last_u = -1;

  int64_t scaled(int64_t hint, int64_t nnz) const {
    if (hint > 0 && hint == last_u && last_nnz > 0 && nnz > last_nnz)
      return std::min<int64_t>(nnz, hint * nnz / last_nnz + 1);
    return hint;
  }
  void finished(int64_t nnz, int64_t u) {
    last_nnz = nnz;
    last_u = u;
  }
};

// Hash table size: >= 2*nnz can never overflow; with a hint (the previous
// minibatch's unique count) ~2.5x the hint instead, which keeps the scratch
// table small enough to stay cache resident. A job that overflowed the
// hinted size is redone at the safe size.
inline int64_t loc_safe_size(int64_t nnz) { return loc_pow2(std::max<int64_t>(2 * nnz, 1024)); }
inline int64_t loc_hinted_size(int64_t hint, int64_t safe) {
  return hint > 0 ? std::min(safe, loc_pow2(std::max<int64_t>(hint * 5 / 2, 1024))) : safe;
}

// the unique-id estimate the partition plan is sized for
inline int64_t loc_uest(int64_t hint, int64_t nnz) {
  return hint > 0 ? std::min<int64_t>(nnz, hint * 5 / 4 + 1024) : nnz;
}

// occurrences in a minibatch from which an id is elected heavy
inline uint32_t loc_heavy_thr(int64_t nnz) {
  return (uint32_t)std::max<int64_t>(1024, nnz / 1024);
}

// The device's two scratch hash tables (all ~0 between minibatches),
// double-buffered so that minibatch i+1's insert can be enqueued before
// minibatch i's assign has emptied its table. A table is persistent and the
// assign leaves it empty, so a minibatch costs no clearing pass; it is
// refilled only after an overflow retry or an abandoned job (dirty).
struct LocTablePool {
  bool busy[2] = {false, false};
  bool dirty[2] = {false, false};
  int next = 0;

  // the slot of a new hash-path job: `next`, else the other one; -1 when
  // both are held (a third job in flight)
  int acquire() {
    int t = next;
    if (busy[t]) t ^= 1;
    if (busy[t]) return -1;
    busy[t] = true;
    next = t ^ 1;
    return t;
  }

  enum Prep { kReady, kRefill, kRealloc };
  // what slot t (holding `have` entries) needs before an insert of a table
  // of `tsize` entries; the slot counts as dirty from here until assigned()
  Prep prepare(int t, int64_t have, int64_t tsize) {
    const Prep p = have < tsize ? kRealloc : dirty[t] ? kRefill : kReady;
    dirty[t] = true;
    return p;
  }
  // the assign ran: the table is empty again and free
  void assigned(int t) { busy[t] = dirty[t] = false; }
  // the job was dropped before its assign: the table may hold keys
  void abandoned(int t) {
    busy[t] = false;
    dirty[t] = true;
  }
};

// Heavy-id hints of the partitioned path, double-buffered by job parity: a
// job reads the set the previous job elected and elects into the other
// buffer. A job begun while another partitioned job is in flight does
// neither (the set it would read is still being written), and a set elected
// for another layout (shards, heavy owners) is not read.
struct LocHeavyElection {
  int parity = 0;
  int64_t layout = -1;  // nshard * 65536 + nho of the set the last job elected
  int inflight = 0;     // partitioned jobs between begin() and release()

  struct Pick {
    bool elect = false;      // false: no hints at all for this job
    int read = 0, write = 0; // buffer parities
    int nho_read = 0;        // heavy owners of the set read (0: read none)
  };
  // a partitioned job whose plan has nho heavy owners begins; `counted` is
  // the job's own flag, handed back to release()
  Pick begin(int64_t nshard, int nho, bool& counted) {
    Pick p;
    if (nho > 0 && inflight == 0) {
      const int64_t key = nshard * 65536 + nho;
      p.elect = true;
      p.read = parity;
      p.write = parity ^ 1;
      p.nho_read = layout == key ? nho : 0;
      layout = key;
      parity ^= 1;
    }
    ++inflight;
    counted = true;
    return p;
  }
  // exactly one release per counted job, from wherever the job ends first
  // (finish, the fallback to the hash path, destruction)
  void release(bool& counted) {
    if (!counted) return;
    --inflight;
    counted = false;
  }
};

// The overflow flags of a count payload read back on the host: h =
// [owner counts (nshard) | own overflow count | nrecv values of the peers,
// `stride` per peer, a peer's flag second]. Every rank sees every rank's
// flag, so all ranks retry together.
struct LocOverflow {
  bool own = false, any = false;
};
inline LocOverflow loc_overflow(const int64_t* h, int64_t nshard, int64_t nrecv, int64_t stride) {
  LocOverflow o;
  o.own = h[nshard] != 0;
  o.any = o.own;
  for (int64_t q = 1; q < nrecv; q += stride) o.any |= h[nshard + 1 + q] != 0;
  return o;
}

}  // namespace wh
