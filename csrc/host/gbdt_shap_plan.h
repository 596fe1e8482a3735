// Per-feature contributions of a GBDT forest (pred_contribs: exact TreeSHAP;
// approx_contribs: the Saabas attribution), host side of gbdt_shap.hip. From
// the trees' lists plus the nodes' covers: the expected values (per node m,
// per tree E = m[root]), the merged root-to-leaf paths, the compact column
// list, the launch plan of the kernels, and the reference implementations
// templated on the float type (double: the CPU path and the tests' oracle;
// float: the yardstick of the kernels' rounding error, which they mirror
// operation by operation). The same tables and plan serve the pairwise
// interaction values (pred_interactions; the last section: the accumulator
// limit of their kernel and their references). Free of HIP and torch.
//
// The game (docs/bsp_apps.md "Contributions"): v(S) walks the tree; a node
// whose feature is in S sends the row where it goes (v < cond left, missing
// takes the default), any other node returns cover[left] / cover[node] *
// v_left + cover[right] / cover[node] * v_right. A path's elements are its
// distinct features in order of first occurrence, each with the interval
// [lo, hi) the path allows, missing_ok (every one of its nodes defaults the
// way the path turns) and z, the product of its nodes' cover ratios.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <numeric>
#include <stdexcept>
#include <string>
#include <vector>

#include "host/gbdt_forest_plan.h"

namespace wh {

// What shapes the kernels' plan. A chunk's path elements in LDS (20 B each;
// a full depth-8 tree is 256 paths x 8 elements), the widest accumulator row
// [U + 1] kept in LDS (beside the path table: 64 rows x 256 x 4 B), and the
// longest path a lane group takes (64 lanes: 63 elements and the dummy).
constexpr int kShapLdsElems = 2048;
constexpr int kShapLdsCols = 256;
constexpr int kShapMaxPath = 63;
inline int gbdt_shap_lds_elems() { return kShapLdsElems; }
inline int gbdt_shap_lds_cols() { return kShapLdsCols; }

struct GbdtShapElem {
  int32_t feat, col;  // feature id; compact column: used[col] == feat
  float lo, hi;       // the path allows lo <= v < hi
  double z;
  bool missing_ok;
};

// elements [begin, begin + len) of the model's element list, len >= 1
struct GbdtShapPath {
  int32_t tree, begin, len;
  float leaf;
};

struct GbdtShapModel {
  int K = 1;                          // tree t belongs to class t % K
  std::vector<GbdtForestNode> nodes;  // the packed forest (gbdt_forest_pack)
  std::vector<int32_t> tree_off;      // [T + 1]
  std::vector<double> node_m;         // expected value of the subtree, per node
  std::vector<int32_t> node_col;      // compact column of an inner node's feature, -1 at a leaf
  std::vector<double> node_rl, node_rr;  // cover ratios of the children (0 at a leaf)
  std::vector<double> tree_E;         // [T]
  std::vector<int32_t> used;          // distinct split features, ascending
  std::vector<GbdtShapPath> paths;    // tree order, left before right; no empty path
  std::vector<GbdtShapElem> elems;
  int64_t ntree() const { return (int64_t)tree_off.size() - 1; }
};

// The model of the trees' lists and covers. A malformed tree throws as
// gbdt_forest_pack does; an inner node whose cover, or a child's, is not
// finite and > 0 throws std::invalid_argument("tree t has no usable cover
// statistics").
inline GbdtShapModel gbdt_shap_pack(const GbdtForestTrees& tr,
                                    const std::vector<std::vector<double>>& cover, int K) {
  if (K < 1) throw std::invalid_argument("the number of classes must be positive");
  GbdtShapModel m;
  m.K = K;
  gbdt_forest_pack(tr, &m.nodes, &m.tree_off);
  const int64_t T = m.ntree(), N = (int64_t)m.nodes.size();
  if ((int64_t)cover.size() != T)
    throw std::invalid_argument("forest lists differ in their number of trees");
  for (auto& nd : m.nodes)
    if (nd.fd >= 0) m.used.push_back(nd.fd >> 1);
  std::sort(m.used.begin(), m.used.end());
  m.used.erase(std::unique(m.used.begin(), m.used.end()), m.used.end());
  m.node_m.assign(N, 0.0), m.node_col.assign(N, -1);
  m.node_rl.assign(N, 0.0), m.node_rr.assign(N, 0.0);
  m.tree_E.assign(T, 0.0);
  const auto usable = [](double c) { return std::isfinite(c) && c > 0; };
  struct Frame {
    int32_t node;
    std::vector<GbdtShapElem> path;
  };
  for (int64_t t = 0; t < T; ++t) {
    const GbdtForestNode* nd = m.nodes.data() + m.tree_off[t];
    const int64_t nn = m.tree_off[t + 1] - m.tree_off[t], o = m.tree_off[t];
    if ((int64_t)cover[t].size() != nn)
      throw std::invalid_argument("malformed tree " + std::to_string(t));
    // children lie beyond their parent: one backward pass gives every m
    for (int64_t i = nn - 1; i >= 0; --i) {
      if (nd[i].fd < 0) {
        m.node_m[o + i] = nd[i].v;
        continue;
      }
      const double c = cover[t][i], cl = cover[t][nd[i].left], cr = cover[t][nd[i].right];
      if (!usable(c) || !usable(cl) || !usable(cr) || !usable(cl / c) || !usable(cr / c))
        throw std::invalid_argument("tree " + std::to_string(t) +
                                    " has no usable cover statistics");
      m.node_rl[o + i] = cl / c, m.node_rr[o + i] = cr / c;
      m.node_m[o + i] = cl / c * m.node_m[o + nd[i].left] + cr / c * m.node_m[o + nd[i].right];
      m.node_col[o + i] = (int32_t)(std::lower_bound(m.used.begin(), m.used.end(), nd[i].fd >> 1) -
                                    m.used.begin());
    }
    m.tree_E[t] = m.node_m[o];
    // the merged paths, depth first, left before right
    std::vector<Frame> todo;
    todo.push_back({0, {}});
    while (!todo.empty()) {
      Frame f = std::move(todo.back());
      todo.pop_back();
      const GbdtForestNode& q = nd[f.node];
      if (q.fd < 0) {
        if (f.path.empty()) continue;  // a single leaf: bias only
        if (m.elems.size() + f.path.size() > (size_t)INT32_MAX)
          throw std::invalid_argument("the forest has too many path elements");
        m.paths.push_back({(int32_t)t, (int32_t)m.elems.size(), (int32_t)f.path.size(), q.v});
        m.elems.insert(m.elems.end(), f.path.begin(), f.path.end());
        continue;
      }
      for (int side = 1; side >= 0; --side) {  // (right is pushed first: left comes out first)
        Frame g{side ? q.right : q.left, f.path};
        const int32_t feat = q.fd >> 1;
        auto it = std::find_if(g.path.begin(), g.path.end(),
                               [&](const GbdtShapElem& e) { return e.feat == feat; });
        if (it == g.path.end()) {
          g.path.push_back({feat, m.node_col[o + f.node],
                            -std::numeric_limits<float>::infinity(),
                            std::numeric_limits<float>::infinity(), 1.0, true});
          it = g.path.end() - 1;
        }
        if (side) it->lo = std::max(it->lo, q.v);
        else it->hi = std::min(it->hi, q.v);
        it->missing_ok = it->missing_ok && ((q.fd & 1) != 0) == (side == 0);
        it->z *= side ? m.node_rr[o + f.node] : m.node_rl[o + f.node];
        todo.push_back(std::move(g));
      }
    }
  }
  return m;
}

// ------------------------------------------------------------------ plan
// Lanes of the group that takes a path of len elements and the dummy; 0: the
// path is longer than a group.
inline int gbdt_shap_width(int64_t len) {
  return len + 1 <= 16 ? 16 : len + 1 <= 32 ? 32 : len + 1 <= 64 ? 64 : 0;
}

// Paths order[path_begin, path_begin + npath), whose elements are
// [elem_begin, elem_begin + nelem) of the table laid out in that order.
struct GbdtShapChunk {
  int64_t path_begin, npath, elem_begin, nelem;
  int32_t cls, width;
};

struct GbdtShapPlan {
  std::vector<int32_t> order;  // path ids: by class, then by width, then as given
  std::vector<GbdtShapChunk> chunks;
};

// The launch plan of paths given by length, class and tree: a fixed order of
// the paths and chunks of whole paths, each of one class and one lane-group
// width and of at most lds_elems elements (>= kShapMaxPath, so any path
// fits). A path of more than kShapMaxPath elements throws
// std::invalid_argument that names its tree.
inline GbdtShapPlan gbdt_shap_plan(const std::vector<int32_t>& len, const std::vector<int32_t>& cls,
                                   const std::vector<int32_t>& tree, int64_t lds_elems) {
  const size_t P = len.size();
  if (cls.size() != P || tree.size() != P)
    throw std::invalid_argument("path lists differ in length");
  if (lds_elems < kShapMaxPath)
    throw std::invalid_argument("the element capacity must hold the longest path");
  for (size_t p = 0; p < P; ++p) {
    if (len[p] < 1 || cls[p] < 0) throw std::invalid_argument("an empty path or a negative class");
    if (len[p] > kShapMaxPath)
      throw std::invalid_argument("tree " + std::to_string(tree[p]) + " has a path of " +
                                  std::to_string(len[p]) + " distinct features; the GPU takes " +
                                  std::to_string(kShapMaxPath));
  }
  GbdtShapPlan plan;
  plan.order.resize(P);
  std::iota(plan.order.begin(), plan.order.end(), 0);
  std::stable_sort(plan.order.begin(), plan.order.end(), [&](int32_t a, int32_t b) {
    if (cls[a] != cls[b]) return cls[a] < cls[b];
    return gbdt_shap_width(len[a]) < gbdt_shap_width(len[b]);
  });
  int64_t elem = 0;
  for (size_t k = 0; k < P; ++k) {
    const int32_t p = plan.order[k];
    const int32_t w = gbdt_shap_width(len[p]);
    if (plan.chunks.empty() || plan.chunks.back().cls != cls[p] ||
        plan.chunks.back().width != w || plan.chunks.back().nelem + len[p] > lds_elems)
      plan.chunks.push_back({(int64_t)k, 0, elem, 0, cls[p], w});
    plan.chunks.back().npath += 1;
    plan.chunks.back().nelem += len[p];
    elem += len[p];
  }
  return plan;
}

inline GbdtShapPlan gbdt_shap_plan(const GbdtShapModel& m, int64_t lds_elems = kShapLdsElems) {
  std::vector<int32_t> len, cls, tree;
  for (auto& p : m.paths)
    len.push_back(p.len), cls.push_back(p.tree % m.K), tree.push_back(p.tree);
  return gbdt_shap_plan(len, cls, tree, lds_elems);
}

// The kernels' table in plan order. A path is {first element, len, leaf
// bits, tree}; an element is {feat << 1 | missing_ok, lo, hi, z} (fp32 bits)
// with its compact column beside it.
struct GbdtShapTable {
  std::vector<int32_t> paths;  // [P, 4]
  std::vector<int32_t> elems;  // [E, 4]
  std::vector<int32_t> ecol;   // [E]
};

inline int32_t gbdt_shap_bits(float v) {
  int32_t b;
  static_assert(sizeof(b) == sizeof(v), "fp32 bits");
  std::copy_n(reinterpret_cast<const char*>(&v), 4, reinterpret_cast<char*>(&b));
  return b;
}

inline GbdtShapTable gbdt_shap_table(const GbdtShapModel& m, const GbdtShapPlan& plan) {
  GbdtShapTable t;
  for (int32_t p : plan.order) {
    const GbdtShapPath& q = m.paths[p];
    t.paths.insert(t.paths.end(), {(int32_t)t.ecol.size(), q.len, gbdt_shap_bits(q.leaf), q.tree});
    for (int32_t k = q.begin; k < q.begin + q.len; ++k) {
      const GbdtShapElem& e = m.elems[k];
      t.elems.insert(t.elems.end(), {(int32_t)(e.feat << 1 | (e.missing_ok ? 1 : 0)),
                                     gbdt_shap_bits(e.lo), gbdt_shap_bits(e.hi),
                                     gbdt_shap_bits((float)e.z)});
      t.ecol.push_back(e.col);
    }
  }
  return t;
}

// ------------------------------------------------------------- references
// Rows: value(r, feat, &v) is false for a missing value (NaN, or absent).
struct ShapDenseRows {
  const float* X;
  int64_t f;
  bool value(int64_t r, int32_t feat, float* v) const {
    if (feat >= f) return false;
    *v = X[r * f + feat];
    return !std::isnan(*v);
  }
};

struct ShapCsrRows {
  const int64_t* row_off;
  const int32_t* fid;  // ascending within a row
  const float* val;    // null: every stored entry is 1
  bool value(int64_t r, int32_t feat, float* v) const {
    const int32_t* b = fid + row_off[r];
    const int32_t* e = fid + row_off[r + 1];
    const int32_t* it = std::lower_bound(b, e, feat);
    if (it == e || *it != feat) return false;
    *v = val ? val[it - fid] : 1.f;
    return !std::isnan(*v);
  }
};

// One path of d elements for one row (Lundberg's EXTEND and UNWOUND-SUM over
// the merged elements, a leading dummy with o = z = 1): one[k] says whether
// the row satisfies element k; phi[col] += unwound_sum * (o - z) * leaf. w
// is scratch. Every product is written in the order the kernel takes it.
template <class T>
inline void gbdt_shap_path(const GbdtShapElem* e, int d, T leaf, const uint8_t* one, T* phi,
                           std::vector<T>* scratch) {
  std::vector<T>& w = *scratch;
  w.assign(d + 1, T(0));
  w[0] = T(1);
  for (int l = 1; l <= d; ++l) {  // EXTEND by element l (position 0 is the dummy)
    const T z = (T)e[l - 1].z, o = one[l - 1] ? T(1) : T(0), inv = T(1) / T(l + 1);
    for (int j = l; j >= 0; --j) {
      const T a = z * w[j] * T(l - j);
      const T b = j ? o * w[j - 1] * T(j) : T(0);
      w[j] = (a + b) * inv;
    }
  }
  const T dp1 = T(d + 1);
  for (int i = 1; i <= d; ++i) {  // UNWOUND-SUM without element i
    const T z = (T)e[i - 1].z, rz = T(1) / z;
    T total = T(0), next = w[d];
    for (int j = d - 1; j >= 0; --j) {
      if (one[i - 1]) {
        const T tmp = next * (dp1 * (T(1) / T(j + 1)));
        total += tmp;
        next = w[j] - tmp * z * (T(d - j) * (T(1) / T(d + 1)));
      } else {
        total += w[j] * rz * (dp1 * (T(1) / T(d - j)));
      }
    }
    phi[e[i - 1].col] += total * ((one[i - 1] ? T(1) : T(0)) - z) * leaf;
  }
}

// out [K, n, U + 1] (compact columns, the bias last): exact contributions of
// the model's first `ntree` trees, paths in tree order; or, approx, the
// Saabas attribution along each row's own walk. Everything in T.
template <class T, class Rows>
inline void gbdt_shap_rows(const GbdtShapModel& m, const Rows& rows, int64_t n, double base,
                           bool approx, T* out) {
  const int64_t U1 = (int64_t)m.used.size() + 1, T_ = m.ntree();
  std::fill(out, out + (int64_t)m.K * n * U1, T(0));
  std::vector<T> bias(m.K, (T)base);
  for (int64_t t = 0; t < T_; ++t) bias[t % m.K] += (T)m.tree_E[t];
  for (int k = 0; k < m.K; ++k)
    for (int64_t r = 0; r < n; ++r) out[(k * n + r) * U1 + U1 - 1] = bias[k];
  if (approx) {
    std::vector<T> mT(m.node_m.size());  // the expected values in T, children before parents
    for (int64_t t = 0; t < T_; ++t)
      for (int64_t i = m.tree_off[t + 1] - 1; i >= m.tree_off[t]; --i) {
        const GbdtForestNode& q = m.nodes[i];
        const int64_t o = m.tree_off[t];
        mT[i] = q.fd < 0 ? (T)q.v
                         : (T)m.node_rl[i] * mT[o + q.left] + (T)m.node_rr[i] * mT[o + q.right];
      }
    for (int64_t r = 0; r < n; ++r)
      for (int64_t t = 0; t < T_; ++t) {
        T* phi = out + ((t % m.K) * n + r) * U1;
        const int64_t o = m.tree_off[t];
        int64_t i = o;
        while (m.nodes[i].fd >= 0) {
          const GbdtForestNode& q = m.nodes[i];
          float v;
          const bool left = rows.value(r, q.fd >> 1, &v) ? v < q.v : (q.fd & 1) != 0;
          const int64_t c = o + (left ? q.left : q.right);
          phi[m.node_col[i]] += mT[c] - mT[i];
          i = c;
        }
      }
    return;
  }
  std::vector<uint8_t> one;
  std::vector<T> scratch;
  for (int64_t r = 0; r < n; ++r)
    for (const GbdtShapPath& p : m.paths) {
      const GbdtShapElem* e = m.elems.data() + p.begin;
      one.resize(p.len);
      for (int k = 0; k < p.len; ++k) {
        float v;
        one[k] = rows.value(r, e[k].feat, &v) ? (e[k].lo <= v && v < e[k].hi) : e[k].missing_ok;
      }
      gbdt_shap_path<T>(e, p.len, (T)p.leaf, one.data(), out + ((p.tree % m.K) * n + r) * U1,
                        &scratch);
    }
}

// ----------------------------------------------------------- interactions
// pred_interactions (docs/bsp_apps.md "Interactions"): per row and class the
// matrix [U + 1, U + 1] over the compact columns. The pair accumulator of a
// row is the packed strict lower triangle: cell (a, b), a > b, is entry
// a (a - 1) / 2 + b of U (U - 1) / 2.
//
// What shapes the kernel's plan. It consumes the tables and chunks above
// unchanged, so a block holds up to kShapLdsElems elements and as many paths
// (36 B per one-element path) and the table of 1 / k:
//   2048 * 36 + 65 * 4                = 73 988 B of the CU's 163 840 B (160 KB),
//   163 840 - 73 988                  = 89 852 B for the triangles of its rows.
// A block of 1024 threads (64 rows at 16 lanes a row) would keep only U <= 26
// in LDS beside a full table, less than the 28 columns of the benchmarks'
// matrices, and a group of 64 lanes (a path of 32 elements or more) could
// never meet an LDS accumulator below U = 32. So the block shrinks by whole
// waves while the chunk's own table asks for it, down to 704 threads, 11
// waves, 44 rows at 16 lanes:
//   89 852 / (44 * 4)                 = 510 floats a row,
//   U (U - 1) / 2 <= 510              : U = 32 (496; 33 needs 528),
// and no larger block reaches 32 columns beside a full table. (The table of
// one full depth-8 tree, 256 paths of 8 elements, is 45 KB: with 28 columns
// 1024 threads have room.)
constexpr int kShapLdsBytes = 160 * 1024;
constexpr int kShapInterThreads = 704;
constexpr int kShapInterLdsCols = 32;
static_assert(kShapInterThreads % 64 == 0, "whole waves");
static_assert((size_t)kShapLdsElems * 36 + 65 * 4 +
                      (size_t)(kShapInterThreads / 16) * 4 *
                          (kShapInterLdsCols * (kShapInterLdsCols - 1) / 2) <=
                  kShapLdsBytes,
              "table and triangles fit the CU's LDS");
static_assert((size_t)kShapLdsElems * 36 + 65 * 4 +
                      (size_t)(kShapInterThreads / 16) * 4 *
                          ((kShapInterLdsCols + 1) * kShapInterLdsCols / 2) >
                  kShapLdsBytes,
              "one more column would not");
inline int gbdt_shap_inter_lds_cols() { return kShapInterLdsCols; }
inline int64_t gbdt_shap_inter_pairs(int64_t U) { return U * (U - 1) / 2; }

// One path of d elements for one row: for every conditioning element c,
// EXTEND over the other d - 1 elements in path order, then UNWOUND-SUM of
// every element i whose column is above c's (each unordered pair once):
// tri[(col_i, col_c)] += unwound_sum * (o_i - z_i) * (o_c - z_c) * (leaf / 2).
// A path of one element has no pairs. Every product is written in the order
// the kernel takes it; w is scratch.
template <class T>
inline void gbdt_shap_inter_path(const GbdtShapElem* e, int d, T leaf, const uint8_t* one, T* tri,
                                 std::vector<T>* scratch) {
  if (d < 2) return;
  std::vector<T>& w = *scratch;
  const int m = d - 1;  // the elements beside c
  const T half = leaf * T(0.5), mp1 = T(m + 1);
  for (int c = 1; c <= d; ++c) {
    const T fc = (one[c - 1] ? T(1) : T(0)) - (T)e[c - 1].z;
    w.assign(m + 1, T(0));
    w[0] = T(1);
    for (int l = 1; l <= m; ++l) {  // EXTEND by the l-th element beside c
      const int k = l < c ? l : l + 1;
      const T z = (T)e[k - 1].z, o = one[k - 1] ? T(1) : T(0), inv = T(1) / T(l + 1);
      for (int j = l; j >= 0; --j) {
        const T a = z * w[j] * T(l - j);
        const T b = j ? o * w[j - 1] * T(j) : T(0);
        w[j] = (a + b) * inv;
      }
    }
    for (int i = 1; i <= d; ++i) {  // UNWOUND-SUM without element i
      if (i == c || e[i - 1].col < e[c - 1].col) continue;
      const T z = (T)e[i - 1].z, rz = T(1) / z;
      T total = T(0), next = w[m];
      for (int j = m - 1; j >= 0; --j) {
        if (one[i - 1]) {
          const T tmp = next * (mp1 * (T(1) / T(j + 1)));
          total += tmp;
          next = w[j] - tmp * z * (T(m - j) * (T(1) / T(m + 1)));
        } else {
          total += w[j] * rz * (mp1 * (T(1) / T(m - j)));
        }
      }
      tri[gbdt_shap_inter_pairs(e[i - 1].col) + e[c - 1].col] +=
          total * ((one[i - 1] ? T(1) : T(0)) - z) * fc * half;
    }
  }
}

// out [K, n, U + 1, U + 1] (compact columns, the bias last): the interaction
// values of the model's trees, paths in tree order. Off the diagonal the
// row's pair accumulator, both cells of a pair the same number; on it
// phi[i] (gbdt_shap_rows<T>) minus the off-diagonal cells of row i, one after
// the other by ascending column; cell (U, U) the bias, the rest of row and
// column U zero. Everything in T.
template <class T, class Rows>
inline void gbdt_shap_inter_rows(const GbdtShapModel& m, const Rows& rows, int64_t n, double base,
                                 T* out) {
  const int64_t U = (int64_t)m.used.size(), U1 = U + 1, TP = gbdt_shap_inter_pairs(U);
  std::vector<T> phi((size_t)m.K * n * U1);
  gbdt_shap_rows<T>(m, rows, n, base, false, phi.data());
  std::fill(out, out + (int64_t)m.K * n * U1 * U1, T(0));
  std::vector<uint8_t> one;
  std::vector<T> scratch, tri((size_t)m.K * TP);
  for (int64_t r = 0; r < n; ++r) {
    std::fill(tri.begin(), tri.end(), T(0));
    for (const GbdtShapPath& p : m.paths) {
      const GbdtShapElem* e = m.elems.data() + p.begin;
      one.resize(p.len);
      for (int k = 0; k < p.len; ++k) {
        float v;
        one[k] = rows.value(r, e[k].feat, &v) ? (e[k].lo <= v && v < e[k].hi) : e[k].missing_ok;
      }
      gbdt_shap_inter_path<T>(e, p.len, (T)p.leaf, one.data(), tri.data() + (p.tree % m.K) * TP,
                              &scratch);
    }
    for (int k = 0; k < m.K; ++k) {
      const T* t = tri.data() + k * TP;
      const T* ph = phi.data() + (k * n + r) * U1;
      T* o = out + (k * n + r) * U1 * U1;
      for (int64_t i = 0; i < U; ++i) {
        T diag = ph[i];
        for (int64_t j = 0; j < U; ++j) {
          if (j == i) continue;
          const T v = i > j ? t[gbdt_shap_inter_pairs(i) + j] : t[gbdt_shap_inter_pairs(j) + i];
          o[i * U1 + j] = v;
          diag -= v;
        }
        o[i * U1 + i] = diag;
      }
      o[U * U1 + U] = ph[U];
    }
  }
}

}  // namespace wh
