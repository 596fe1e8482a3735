// The parameter store of one shard (module class _hip.KVStore): the slot
// table, the V slabs and every op on them. Shared by hip_ops.cc, which binds
// it to Python, and the native steps (fm_ops.cc, psx_ops.cc).
#pragma once
#include "bind_common.h"

#include <cstring>
#include <memory>

namespace wh_bind {

// the device's look-back scan workspace (defined in hip_ops.cc)
wh::Lookback lookback(const torch::Device& d);

class KVStore {
 public:
  KVStore(int64_t cap, int64_t vcap, int64_t dim, int64_t device) {
    TORCH_CHECK(cap > 0 && (cap & (cap - 1)) == 0, "cap must be a power of two");
    TORCH_CHECK(dim >= 0 && dim <= 256, "embedding dim must be in [0, 256]");
    dim_ = dim;
    vstride_ = dim == 0 ? 0 : (int)(4 * next_pow2((dim + 3) / 4));
    auto dev = torch::Device(torch::kCUDA, device);
    c10::DeviceGuard g(dev);
    auto f32 = torch::TensorOptions().dtype(torch::kFloat32).device(dev);
    // AoS slot table [cap, 8] x 4 bytes = wh::KVSlot; the per-field tensors
    // below are strided views into it (shared storage, writable)
    auto sl = torch::zeros({cap, 8}, f32.dtype(torch::kInt32));
    sl.view(torch::kInt64).select(1, 0).fill_(-1);  // key: empty
    sl.select(1, 5).fill_(-1);                      // vrow: none
    set_slots(sl);
    if (dim > 0) {
      V_ = torch::zeros({std::max<int64_t>(vcap, 1), vstride_}, f32);
      VG_ = torch::zeros({std::max<int64_t>(vcap, 1), vstride_}, f32);
    }
    vnext_ = torch::zeros({1}, f32.dtype(torch::kInt32));
    stats_ = torch::zeros({wh::kStatShards, wh::kStatStride}, f32.dtype(torch::kInt64));
    cap_ = cap;
    vcap_ = dim > 0 ? vcap : 0;
  }

  wh::KVTable table() const {
    wh::KVTable t;
    t.sl = reinterpret_cast<wh::KVSlot*>(slots_.data_ptr());
    t.V = dim_ > 0 ? ptr<float>(V_) : nullptr;
    t.VG = dim_ > 0 ? ptr<float>(VG_) : nullptr;
    t.vnext = ptr<int32_t>(vnext_);
    t.stats = ptr<int64_t>(stats_);
    t.cap = cap_;
    t.vcap = vcap_;
    t.vstride = vstride_;
    t.dim = (int)dim_;
    return t;
  }

  Tensor find(const Tensor& keys, bool insert) {
    CHECK_IN(keys, torch::kInt64);
    c10::DeviceGuard g(keys.device());
    auto slot = torch::empty({keys.numel()}, keys.options().dtype(torch::kInt32));
    wh::kv_find(table(), reinterpret_cast<const uint64_t*>(keys.data_ptr()), keys.numel(),
                insert ? 1 : 0, ptr<int32_t>(slot), cur_stream(keys));
    return slot;
  }

  Tensor occupied() {
    c10::DeviceGuard g(keys_.device());
    auto out = torch::empty({cap_}, keys_.options().dtype(torch::kInt32));
    auto n = torch::zeros({1}, keys_.options());
    wh::kv_occupied(table(), ptr<int32_t>(out), ptr<int64_t>(n), cur_stream(keys_));
    return out.narrow(0, 0, n.item<int64_t>());
  }

  Tensor linear_pull(const Tensor& slot) {
    CHECK_IN(slot, torch::kInt32);
    c10::DeviceGuard g(slot.device());
    auto out = torch::empty({slot.numel()}, slot.options().dtype(torch::kFloat32));
    wh::linear_pull(table(), ptr<int32_t>(slot), slot.numel(), ptr<float>(out), cur_stream(slot));
    return out;
  }

  void linear_push(const Tensor& slot, const Tensor& grad, int64_t algo, double alpha, double beta,
                   double l1, double l2, double sgd_eta) {
    CHECK_IN(slot, torch::kInt32);
    CHECK_IN(grad, torch::kFloat32);
    TORCH_CHECK(grad.numel() >= slot.numel());
    c10::DeviceGuard g(slot.device());
    wh::LinearHP hp{(int)algo, (float)alpha, (float)beta, (float)l1, (float)l2, (float)sgd_eta};
    wh::linear_push(table(), ptr<int32_t>(slot), ptr<float>(grad), slot.numel(), hp,
                    cur_stream(slot));
  }

  static wh::DifactoHP dhp(const std::vector<double>& h, int64_t threshold, bool l1_shrk,
                           int64_t seed) {
    TORCH_CHECK(h.size() == 8, "difacto hyper-parameter vector must have 8 entries");
    wh::DifactoHP hp;
    hp.alpha = (float)h[0]; hp.beta = (float)h[1]; hp.l1 = (float)h[2]; hp.l2 = (float)h[3];
    hp.v_alpha = (float)h[4]; hp.v_beta = (float)h[5]; hp.v_l2 = (float)h[6];
    hp.v_init = (float)h[7];
    hp.threshold = (uint32_t)threshold;
    hp.l1_shrk = l1_shrk ? 1 : 0;
    hp.seed = (uint64_t)seed;
    return hp;
  }

  void difacto_push_cnt(const Tensor& slot, const Tensor& cnt, const std::vector<double>& h,
                        int64_t threshold, bool l1_shrk, int64_t seed) {
    CHECK_IN(slot, torch::kInt32);
    CHECK_DEV(cnt); CHECK_CONT(cnt);
    TORCH_CHECK(cnt.scalar_type() == torch::kFloat32 || cnt.scalar_type() == torch::kInt32,
                "counts must be float32 or int32");
    TORCH_CHECK(cnt.numel() >= slot.numel());
    c10::DeviceGuard g(slot.device());
    const bool f = cnt.scalar_type() == torch::kFloat32;
    wh::difacto_push_cnt(table(), ptr<int32_t>(slot), f ? ptr<float>(cnt) : nullptr,
                         f ? nullptr : ptr<int32_t>(cnt), slot.numel(),
                         dhp(h, threshold, l1_shrk, seed), cur_stream(slot));
  }

  // Variable-length pull. Returns (hdr [n,2] f32 {w, vidx bits}, vc [mcap, vstride],
  // vpos i64 [n+1]); m = vpos[n] stays on the device (vc is sized by the
  // host-side bound mcap = n so the step needs no host synchronisation).
  std::vector<Tensor> difacto_pull(const Tensor& slot, bool l1_shrk) {
    CHECK_IN(slot, torch::kInt32);
    c10::DeviceGuard g(slot.device());
    auto s = cur_stream(slot);
    const int64_t n = slot.numel();
    auto f32 = slot.options().dtype(torch::kFloat32);
    auto hdr = torch::empty({n, 2}, f32);
    const int64_t mcap = vstride_ > 0 ? n : 0;
    auto vc = torch::empty({mcap, (int64_t)std::max(vstride_, 1)}, f32);
    if (n > 0) {
      auto vpos = torch::empty({n + 1}, slot.options().dtype(torch::kInt64));
      if (wh::difacto_pull_fused(table(), ptr<int32_t>(slot), n, l1_shrk ? 1 : 0,
                                 lookback(slot.device()), ptr<float>(hdr), ptr<int64_t>(vpos),
                                 ptr<float>(vc), s))
        return {hdr, vc, vpos};
    }
    auto vflag = torch::empty({std::max<int64_t>(n, 1)}, slot.options());
    auto vpos = torch::zeros({n + 1}, slot.options().dtype(torch::kInt64));
    wh::difacto_pull_hdr(table(), ptr<int32_t>(slot), n, l1_shrk ? 1 : 0, ptr<float>(hdr),
                         ptr<int32_t>(vflag), s);
    if (vstride_ > 0 && n > 0) {
      auto stmp = torch::empty({wh::scan_tmp_elems(n)}, vpos.options());
      wh::scan_i32(ptr<int32_t>(vflag), ptr<int64_t>(vpos), n, ptr<int64_t>(stmp), s);
      wh::difacto_pull_rows(table(), ptr<int32_t>(slot), n, ptr<int32_t>(vflag),
                            ptr<int64_t>(vpos), ptr<float>(hdr), ptr<float>(vc), s);
    }
    return {hdr, vc, vpos};
  }

  // Single-shard open + pull in one launch. Returns (slot i32 [n], hdr, vc,
  // vpos) like find() followed by difacto_push_cnt() (when cnt is given) and
  // difacto_pull(). Keys must be distinct.
  std::vector<Tensor> difacto_open_pull(const Tensor& keys, bool insert,
                                        const c10::optional<Tensor>& cnt,
                                        const std::vector<double>& h, int64_t threshold,
                                        bool l1_shrk, int64_t seed, bool direct) {
    return difacto_open_pull(keys, insert, cnt, h, threshold, l1_shrk, seed, direct, nullptr,
                             nullptr);
  }

  // The open that also emits the FM backward's chunk plan (DifactoStep): keys
  // are a localize's unique keys, plan names that localize's csc_off and the
  // backward's pre-allocated outputs and scratch (wh::fm_bwd_plan_dst over
  // fm_bwd_alloc's buffers, made on this stream before the call: the emitter
  // zeroes the gw / gvc rows of multi-chunk keys). *planned: the plan was
  // written; false on the fallbacks (more keys than the look-back has tiles,
  // no keys), after which the backward plans for itself (FmBwdPhase::kAll).
  std::vector<Tensor> difacto_open_pull(const Tensor& keys, bool insert,
                                        const c10::optional<Tensor>& cnt,
                                        const std::vector<double>& h, int64_t threshold,
                                        bool l1_shrk, int64_t seed, bool direct,
                                        const wh::FmBwdPlanDst* plan, bool* planned) {
    if (planned) *planned = false;
    CHECK_IN(keys, torch::kInt64);
    const int32_t* cp = nullptr;
    if (cnt.has_value() && cnt->defined()) {
      CHECK_IN((*cnt), torch::kInt32);
      TORCH_CHECK(cnt->numel() >= keys.numel(), "open_pull: count size mismatch");
      cp = ptr<int32_t>(*cnt);
    }
    c10::DeviceGuard g(keys.device());
    auto s = cur_stream(keys);
    const int64_t n = keys.numel();
    auto f32 = keys.options().dtype(torch::kFloat32);
    auto slot = torch::empty({n}, keys.options().dtype(torch::kInt32));
    auto hdr = torch::empty({n, 2}, f32);
    auto vpos = torch::empty({n + 1}, keys.options());
    // direct: no pulled copy -- hdr's vidx column holds the table's V row and
    // the "pulled rows" are the V slab itself (one shard: the forward and
    // backward read the rows in place; the push writes them after both)
    direct = direct && vstride_ > 0;
    auto vc = direct ? V_ : torch::empty({vstride_ > 0 ? n : 0, (int64_t)std::max(vstride_, 1)}, f32);
    if (n == 0) {
      vpos.zero_();
      return {slot, hdr, vc, vpos};
    }
    if (!wh::difacto_open_pull(table(), reinterpret_cast<const uint64_t*>(keys.data_ptr()), n,
                               cp, dhp(h, threshold, l1_shrk, seed), insert ? 1 : 0,
                               lookback(keys.device()), ptr<int32_t>(slot), ptr<float>(hdr),
                               ptr<int64_t>(vpos), direct ? nullptr : ptr<float>(vc), s, plan)) {
      // (too many keys for the one-launch path: the compact pull below)
      slot = find(keys, insert);
      if (cp) difacto_push_cnt(slot, *cnt, h, threshold, l1_shrk, seed);
      auto r = difacto_pull(slot, l1_shrk);
      return {slot, r[0], r[1], r[2]};
    }
    if (planned) *planned = plan != nullptr;
    return {slot, hdr, vc, vpos};
  }

  // hdr: this shard's pull header for the same keys (owner vidx numbering)
  void difacto_push(const Tensor& slot, const Tensor& hdr, const Tensor& gw, const Tensor& gvc,
                    const std::vector<double>& h, int64_t threshold, bool l1_shrk,
                    int64_t seed) {
    difacto_push_after(slot, hdr, gw, gvc, h, threshold, l1_shrk, seed, c10::nullopt);
  }

  // The push behind a fused backward (DifactoStep, wh::FmBwdProblem::fuse_v):
  // with ucnt, the minibatch's occurrence counts, the keys of one V chunk have
  // had their AdaGrad step and get only the FTRL step on w here.
  void difacto_push_after(const Tensor& slot, const Tensor& hdr, const Tensor& gw,
                          const Tensor& gvc, const std::vector<double>& h, int64_t threshold,
                          bool l1_shrk, int64_t seed, const c10::optional<Tensor>& ucnt) {
    CHECK_IN(slot, torch::kInt32);
    CHECK_IN(hdr, torch::kFloat32);
    CHECK_IN(gw, torch::kFloat32);
    CHECK_DEV(gvc); CHECK_CONT(gvc); CHECK_DT(gvc, torch::kFloat32);
    const int64_t n = slot.numel();
    TORCH_CHECK(hdr.numel() == 2 * n && gw.numel() == n, "push: hdr/gw size mismatch");
    TORCH_CHECK(vstride_ == 0 || (gvc.dim() == 2 && gvc.size(1) == vstride_),
                "push: gvc must be [m, vstride]");
    const int32_t* uc = nullptr;
    if (ucnt.has_value()) {
      CHECK_IN((*ucnt), torch::kInt32);
      TORCH_CHECK(ucnt->numel() >= n, "push: count size mismatch");
      uc = ptr<int32_t>(*ucnt);
    }
    c10::DeviceGuard g(slot.device());
    wh::difacto_push(table(), ptr<int32_t>(slot), ptr<float>(hdr), ptr<float>(gw),
                     gvc.numel() ? ptr<float>(gvc) : nullptr, n, dhp(h, threshold, l1_shrk, seed),
                     cur_stream(slot), uc);
  }

  // ---------------------------------------------------- multi-shard (psx.hip)
  // Owner side of a P-shard minibatch. keys: int64 [n] or int32 records
  // [n, 3] {key lo, key hi, count}; segS / segHS: device int64 [P+1]; rows_cap:
  // rows of the reply buffer to allocate (>= segHS[P] + n). Returns (slot,
  // vpos [n+1], chain [n] (int32 view of the chain links), head uint8 [n],
  // rbuf [rows_cap, vstride], vcnt [P]).
  // chain_in: a chain buffer [>= n] the preceding push on this stream
  // zeroed (ps_push prep_chain), with vbase snapshotted there too: the open
  // then skips its own prep launch
  std::vector<Tensor> ps_open(const Tensor& keys, bool use_cnt, const Tensor& segS,
                              const Tensor& segHS, int64_t rows_cap, bool insert, bool chains,
                              const std::vector<double>& h, int64_t threshold, bool l1_shrk,
                              int64_t seed, const c10::optional<Tensor>& chain_in = c10::nullopt) {
    CHECK_DEV(keys); CHECK_CONT(keys);
    CHECK_IN(segS, torch::kInt64);
    CHECK_IN(segHS, torch::kInt64);
    const bool rec = keys.scalar_type() == torch::kInt32;
    TORCH_CHECK(rec ? (keys.dim() == 2 && keys.size(1) == 3) : keys.scalar_type() == torch::kInt64,
                "ps_open: keys must be int64 [n] or int32 records [n, 3]");
    TORCH_CHECK(!use_cnt || rec, "ps_open: counts travel in the records");
    const int64_t n = keys.size(0);
    const int P = (int)segS.numel() - 1;
    TORCH_CHECK(P >= 1 && segHS.numel() == P + 1, "ps_open: bad segment tables");
    TORCH_CHECK(n < (1 << 24), "ps_open: at most 2^24 - 1 keys per minibatch and shard");
    epoch_ = epoch_ % 255 + 1;  // 1..255; a wrap to 1 sweeps the table's tags
    ++opens_;
    TORCH_CHECK(vstride_ == 0 || rows_cap >= n, "ps_open: reply buffer too small");
    c10::DeviceGuard g(keys.device());
    auto s = cur_stream(keys);
    auto i32 = keys.options().dtype(torch::kInt32);
    auto f32 = keys.options().dtype(torch::kFloat32);
    // the open's outputs from ONE allocation
    const int64_t n1 = std::max<int64_t>(n, 1);
    Carve c;
    const int64_t o_s = c.add(n1 * 4), o_w = c.add(n1 * 4), o_p = c.add((n + 1) * 8),
                  o_h = c.add(n1);
    c.alloc(keys.options());
    auto slot = c.view(o_s, n1, torch::kInt32);
    auto wout = c.view(o_w, n1, torch::kFloat32);
    auto vpos = c.view(o_p, n + 1, torch::kInt64);
    const bool prepped = chain_in.has_value() && chain_in->defined() && chain_in->numel() > 0;
    if (prepped) {
      CHECK_IN((*chain_in), torch::kInt32);
      TORCH_CHECK(chain_in->numel() >= std::max<int64_t>(n, 1), "ps_open: prepped chain too small");
      TORCH_CHECK(vbase_.defined(), "ps_open: prepped without a push prep");
    }
    auto chain = prepped ? *chain_in : torch::empty({n1}, i32);
    auto head = c.view(o_h, n1, torch::kUInt8);
    // linear (vstride 0): the reply is w_out itself (returned in rbuf's place)
    auto rbuf = torch::empty({vstride_ > 0 ? rows_cap : 0, (int64_t)std::max(vstride_, 1)}, f32);
    // linear: no V rows, a cached all-zero vcnt (read only; no fill launch per open)
    Tensor vcnt;
    if (vstride_ == 0) {
      if (!vcnt0_.defined() || vcnt0_.numel() != P || vcnt0_.device() != keys.device())
        vcnt0_ = torch::zeros({P}, keys.options().dtype(torch::kInt64));
      vcnt = vcnt0_;
    } else {
      vcnt = torch::empty({P}, keys.options().dtype(torch::kInt64));
    }
    if (!vbase_.defined()) vbase_ = torch::empty({1}, vnext_.options());
    const bool ok = wh::ps_open(
        table(), rec ? nullptr : reinterpret_cast<const uint64_t*>(keys.data_ptr()),
        rec ? ptr<int32_t>(keys) : nullptr, n, use_cnt ? 1 : 0, dhp(h, threshold, l1_shrk, seed),
        insert ? 1 : 0, chains ? 1 : 0, (uint32_t)epoch_, ptr<int32_t>(vbase_),
        ptr<int64_t>(segS), ptr<int64_t>(segHS), P, lookback(keys.device()), ptr<int32_t>(slot),
        ptr<float>(wout), ptr<int64_t>(vpos), reinterpret_cast<uint32_t*>(chain.data_ptr()),
        reinterpret_cast<uint8_t*>(head.data_ptr()), ptr<float>(rbuf), ptr<int64_t>(vcnt), s,
        prepped ? 1 : 0);
    TORCH_CHECK(ok, "ps_open: limits exceeded (P <= 256, n < 2^24)");
    return {slot.narrow(0, 0, n), vpos, chain.narrow(0, 0, n), head.narrow(0, 0, n),
            vstride_ > 0 ? rbuf : wout.narrow(0, 0, n), vcnt};
  }

  // the next open's prep folded into a push (see ps_open chain_in): zero
  // prep_chain's first prep_n entries and snapshot vnext into vbase
  wh::PsPrep push_prep(const c10::optional<Tensor>& prep_chain, int64_t prep_n) {
    wh::PsPrep pr;
    if (!(prep_chain.has_value() && prep_chain->defined() && prep_chain->numel() > 0)) return pr;
    CHECK_IN((*prep_chain), torch::kInt32);
    TORCH_CHECK(prep_n >= 0 && prep_n <= prep_chain->numel(), "push prep: chain too small");
    if (!vbase_.defined()) vbase_ = torch::empty({1}, vnext_.options());
    pr.chain = reinterpret_cast<uint32_t*>(prep_chain->data_ptr());
    pr.n = prep_n;
    pr.vbase = ptr<int32_t>(vbase_);
    return pr;
  }

  // Linear owner push of a P-shard minibatch: g [n] = the gradients pushed
  // for this owner's received keys (segment order); t0 = SGD requests so far.
  void ps_push_linear(const Tensor& slot, const c10::optional<Tensor>& chain,
                      const c10::optional<Tensor>& head, const Tensor& segS, const Tensor& g,
                      int64_t algo, double alpha, double beta, double l1, double l2, double t0,
                      const c10::optional<Tensor>& prep_chain = c10::nullopt,
                      int64_t prep_n = 0) {
    CHECK_IN(slot, torch::kInt32);
    CHECK_IN(segS, torch::kInt64);
    CHECK_IN(g, torch::kFloat32);
    const int64_t n = slot.numel();
    TORCH_CHECK(g.numel() == n, "ps_push_linear: gradient size mismatch");
    TORCH_CHECK(vstride_ == 0, "ps_push_linear needs a linear store");
    const uint32_t* cp = nullptr;
    const uint8_t* hp = nullptr;
    if (chain.has_value() && chain->defined()) {
      CHECK_IN((*chain), torch::kInt32);
      TORCH_CHECK(head.has_value() && head->defined() && chain->numel() == n &&
                      head->numel() == n, "ps_push_linear: chain / head size mismatch");
      cp = reinterpret_cast<const uint32_t*>(chain->data_ptr());
      hp = reinterpret_cast<const uint8_t*>(head->data_ptr());
    }
    c10::DeviceGuard dg(slot.device());
    wh::LinearHP h{(int)algo, (float)alpha, (float)beta, (float)l1, (float)l2, 0.f};
    TORCH_CHECK(wh::ps_push_linear(table(), ptr<int32_t>(slot), cp, hp, n, ptr<int64_t>(segS),
                                   (int)segS.numel() - 1, ptr<float>(g), h, t0, cur_stream(slot),
                                   push_prep(prep_chain, prep_n)),
                "ps_push_linear: limits exceeded (P <= 256)");
  }

  // Owner side push of a P-shard minibatch: gbuf = the received push buffer
  // (rows in the reply layout of the matching ps_open).
  void ps_push(const Tensor& slot, const Tensor& vpos, const c10::optional<Tensor>& chain,
               const c10::optional<Tensor>& head, const Tensor& segS, const Tensor& segHS,
               const Tensor& gbuf, const std::vector<double>& h, int64_t threshold, bool l1_shrk,
               int64_t seed, const c10::optional<Tensor>& prep_chain = c10::nullopt,
               int64_t prep_n = 0) {
    CHECK_IN(slot, torch::kInt32);
    CHECK_IN(vpos, torch::kInt64);
    CHECK_IN(segS, torch::kInt64);
    CHECK_IN(segHS, torch::kInt64);
    CHECK_IN(gbuf, torch::kFloat32);
    const int64_t n = slot.numel();
    TORCH_CHECK(vpos.numel() == n + 1, "ps_push: vpos size mismatch");
    const uint32_t* cp = nullptr;
    const uint8_t* hp = nullptr;
    if (chain.has_value() && chain->defined()) {
      CHECK_IN((*chain), torch::kInt32);
      TORCH_CHECK(head.has_value() && head->defined(), "ps_push: chain without head flags");
      CHECK_IN((*head), torch::kUInt8);
      TORCH_CHECK(chain->numel() == n && head->numel() == n, "ps_push: chain size mismatch");
      cp = reinterpret_cast<const uint32_t*>(chain->data_ptr());
      hp = reinterpret_cast<const uint8_t*>(head->data_ptr());
    }
    const int P = (int)segS.numel() - 1;
    c10::DeviceGuard g(slot.device());
    TORCH_CHECK(wh::ps_push(table(), ptr<int32_t>(slot), ptr<int64_t>(vpos), cp, hp, n,
                            ptr<int64_t>(segS), ptr<int64_t>(segHS), P, ptr<float>(gbuf),
                            dhp(h, threshold, l1_shrk, seed), cur_stream(slot),
                            push_prep(prep_chain, prep_n)),
                "ps_push: limits exceeded");
  }

  // ------------------------------------------------------- growth / health
  // Re-hash into a table of newcap (power of two) slots; returns the old ->
  // new slot map (int32 [old cap]) for the slot ids of in-flight sessions.
  Tensor grow(int64_t newcap) {
    TORCH_CHECK(newcap > cap_ && (newcap & (newcap - 1)) == 0,
                "grow: new capacity must be a larger power of two");
    c10::DeviceGuard g(slots_.device());
    auto s = cur_stream(slots_);
    auto ns = torch::zeros({newcap, 8}, slots_.options());
    ns.view(torch::kInt64).select(1, 0).fill_(-1);
    ns.select(1, 5).fill_(-1);
    auto remap = torch::empty({cap_}, slots_.options());
    wh::kv_rehash(reinterpret_cast<const wh::KVSlot*>(slots_.data_ptr()), cap_,
                  reinterpret_cast<wh::KVSlot*>(ns.data_ptr()), newcap, ptr<int32_t>(remap),
                  ptr<int64_t>(stats_), s);
    set_slots(ns);
    cap_ = newcap;
    return remap;
  }

  // enlarge the V slab to newvcap rows (rows keep their ids)
  void grow_v(int64_t newvcap) {
    TORCH_CHECK(dim_ > 0 && newvcap > vcap_, "grow_v: new capacity must be larger");
    c10::DeviceGuard g(slots_.device());
    auto f32 = V_.options();
    auto nv = torch::empty({newvcap, vstride_}, f32);
    auto ng = torch::empty({newvcap, vstride_}, f32);
    nv.narrow(0, 0, V_.size(0)).copy_(V_);
    ng.narrow(0, 0, VG_.size(0)).copy_(VG_);
    nv.narrow(0, V_.size(0), newvcap - V_.size(0)).zero_();
    ng.narrow(0, VG_.size(0), newvcap - VG_.size(0)).zero_();
    V_ = nv;
    VG_ = ng;
    vcap_ = newvcap;
  }

  // device int64 [4] {keys, failed inserts, V-slab overflows, V rows used}
  Tensor summary() {
    c10::DeviceGuard g(slots_.device());
    auto out = torch::empty({4}, stats_.options());
    wh::kv_summary(table(), ptr<int64_t>(out), cur_stream(slots_));
    return out;
  }

  // The summary written by its kernel straight into coherent host memory
  // (slot 0..3; the store guard alternates two), on the current stream; read
  // with summary_read once an event recorded after it has completed. A
  // 32-byte copy into pinned memory instead cost ~40 us of host time.
  void summary_async(int64_t slot) {
    TORCH_CHECK(slot >= 0 && slot < 4, "summary slot out of range");
    c10::DeviceGuard g(slots_.device());
    if (!sum_host_) {
      void* p = nullptr;
      WH_HIP_CHECK_HOST(hipHostMalloc(&p, 4 * 64, hipHostMallocMapped | hipHostMallocCoherent));
      std::memset(p, 0, 4 * 64);
      sum_host_.reset(static_cast<int64_t*>(p));
    }
    wh::kv_summary(table(), sum_host_.get() + 8 * slot, cur_stream(slots_));
  }
  std::vector<int64_t> summary_read(int64_t slot) const {
    TORCH_CHECK(sum_host_ && slot >= 0 && slot < 4, "no summary in that slot");
    const volatile int64_t* h = sum_host_.get() + 8 * slot;
    return {h[0], h[1], h[2], h[3]};
  }
  struct HostFree {
    void operator()(int64_t* p) const { (void)hipHostFree(p); }
  };
  std::unique_ptr<int64_t, HostFree> sum_host_;

  int64_t dim() const { return dim_; }
  int64_t vstride() const { return vstride_; }
  int64_t cap() const { return cap_; }
  int64_t vcap() const { return vcap_; }

  Tensor slots_, keys_, w_, z_, sq_, cnt_, vrow_, V_, VG_, vnext_, stats_, vbase_, vcnt0_;
  int64_t epoch_ = 0;  // ps_open chain-tag epoch (1..255)
  int64_t opens_ = 0;  // ps_open calls so far (tests: the epoch wrapped)

 private:
  void set_slots(const Tensor& sl) {
    slots_ = sl;
    auto as_i64 = slots_.view(torch::kInt64);   // [cap, 4]
    auto as_f32 = slots_.view(torch::kFloat32); // [cap, 8]
    keys_ = as_i64.select(1, 0);
    w_ = as_f32.select(1, 2);
    z_ = as_f32.select(1, 3);
    sq_ = as_f32.select(1, 4);
    vrow_ = slots_.select(1, 5);
    cnt_ = slots_.select(1, 6);
  }

  int64_t cap_ = 0, vcap_ = 0, dim_ = 0;
  int vstride_ = 0;
};

}  // namespace wh_bind
