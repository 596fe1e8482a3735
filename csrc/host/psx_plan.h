// What the multi-shard step puts on the wire, from the host-known counts of a
// minibatch (kv/psx.py is the Python twin: Psx._upload, Psx._c2 / _c3,
// _QFilter.layout, the C0 payload of Psx._counts). Free of HIP and torch: the
// native step (csrc/bind/psx_ops.cc) and the host self-test compile the same
// code.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace wh {

using PsxRows = std::vector<int64_t>;  // one count per peer

inline int64_t psx_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- segment tables of a step: Hw / Ho, the header rows (two floats per
// key in rows of vs floats) this worker gets from / this owner sends to each
// peer, and the device table [4 (P + 1) + P]: exclusive prefix sums of send,
// Hw, recv, Ho, then the previous step's vrecv (zeros without one).
struct PsxSegs {
  PsxRows Hw, Ho, table;
};
inline PsxSegs psx_segs(const PsxRows& send, const PsxRows& recv, int64_t vs, bool linear,
                        const PsxRows* prev_vrecv) {
  const int64_t P = (int64_t)send.size();
  vs = std::max<int64_t>(vs, 1);
  PsxSegs s{PsxRows(P, 0), PsxRows(P, 0), PsxRows(4 * (P + 1) + P, 0)};
  int64_t* a = s.table.data();
  for (int64_t p = 0; p < P; ++p) {
    if (!linear) {
      s.Hw[p] = psx_cdiv(2 * send[p], vs);
      s.Ho[p] = psx_cdiv(2 * recv[p], vs);
    }
    a[p + 1] = a[p] + send[p];
    a[P + 2 + p] = a[P + 1 + p] + s.Hw[p];
    a[2 * P + 3 + p] = a[2 * P + 2 + p] + recv[p];
    a[3 * P + 4 + p] = a[3 * P + 3 + p] + s.Ho[p];
  }
  if (prev_vrecv) std::copy(prev_vrecv->begin(), prev_vrecv->end(), a + 4 * P + 4);
  return s;
}

// ---- rows per peer of the pull / push buffers: the owner side holds, per
// peer, the keys it received (linear) or their header rows and the V rows it
// owns; the worker side the keys it sent, or their header rows and the V rows
// it gets. C2 (pull) sends the owner side and receives the worker side; C3
// (push) is the swap.
struct PsxSides {
  PsxRows owner, worker;
};
inline PsxSides psx_sides(bool linear, const PsxRows& send, const PsxRows& recv, const PsxRows& Hw,
                          const PsxRows& Ho, const PsxRows& vown, const PsxRows& vrecv) {
  if (linear) return {recv, send};
  PsxSides r{Ho, Hw};
  for (size_t p = 0; p < Ho.size(); ++p) {
    r.owner[p] += vown[p];
    r.worker[p] += vrecv[p];
  }
  return r;
}

// ---- fixed_bytes filter: the region table of one side of an exchange. Per
// peer {sf, a, vf, nf, sq, ha}: float offset of the region, exact floats,
// offset and count of the quantised floats, first wire row, raw wire rows;
// rows: wire rows per peer; ext: floats of the whole float layout. n keys, v
// embedding rows, H header rows per peer; W floats per record of R bytes
// (linear: records of W weights; v and H are not read).
struct PsxQLayout {
  PsxRows desc, rows;
  int64_t ext = 0;
};
inline PsxQLayout psx_qlayout(bool linear, int64_t vs, int64_t W, int64_t R, const PsxRows& n,
                              const PsxRows& v, const PsxRows& H) {
  const int64_t P = (int64_t)n.size();
  PsxQLayout L;
  L.desc.assign(6 * P, 0);
  int64_t sf = 0, sq = 0;
  for (int64_t p = 0; p < P; ++p) {
    int64_t a, vf, nf, ha, nr, ext;
    if (linear) {
      a = 0, vf = 0, nf = n[p], ha = 0;
      nr = psx_cdiv(n[p], W);
      ext = n[p];
    } else {
      a = 2 * n[p], vf = H[p] * vs, nf = v[p] * vs;
      ha = psx_cdiv(4 * a, R);
      nr = v[p];
      ext = (H[p] + v[p]) * vs;
    }
    const int64_t d[6] = {sf, a, vf, nf, sq, ha};
    std::copy(d, d + 6, L.desc.begin() + 6 * p);
    L.rows.push_back(ha + nr);
    sf += ext;
    sq += ha + nr;
  }
  L.ext = sf;
  return L;
}

// ---- the 5 P-word tail of a C0 payload: per peer q {keys from q, q's
// table-overflow flag (the localize job's), V rows q sends back for the
// carried step, q has data}, then the V rows this rank owns for q. any: some
// rank has data.
struct PsxCounts {
  PsxRows recv, vrecv, vown;
  bool any = false;
};
inline PsxCounts psx_counts(const int64_t* t, int64_t P) {
  PsxCounts c;
  for (int64_t q = 0; q < P; ++q) {
    c.recv.push_back(t[4 * q]);
    c.vrecv.push_back(t[2 + 4 * q]);
    c.any = c.any || t[3 + 4 * q] != 0;
  }
  c.vown.assign(t + 4 * P, t + 5 * P);
  return c;
}

}  // namespace wh
