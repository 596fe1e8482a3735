// torch / pybind11 binding layer for the gfx950 HIP kernels (module
// wormhole_amd._hip): the module itself and everything that shares the
// parameter-server state -- the device workspaces, KVStore's bindings (the
// class is kv_store.h), the ps_* ops of the multi-shard exchange,
// quantisation, and a few stateless ops (scan, key_mod, synth, gather). FM and
// the single-shard native steps (fm_ops.cc), the multi-shard step and RCCL
// (psx_ops.cc), localize (localize_ops.cc), the AUC family (auc_ops.cc) and
// the stateless BSP families (gbdt_ops.cc, kmeans_ops.cc, bsp_ops.cc,
// ingest_ops.cc) have translation units of their own, registered from
// PYBIND11_MODULE below; what those call here is declared in ps_ops.h. The
// steps' streams and host timers are step_rt.cc. Host-only: validates
// tensors, sizes outputs and launches on the current PyTorch HIP stream.
#include "bind_common.h"
#include "kv_store.h"
#include "ps_ops.h"
#include "step_rt.h"

#include <algorithm>
#include <vector>

using namespace wh_bind;

// (in wh_bind, not an anonymous namespace: fm_ops.cc, psx_ops.cc and
// auc_ops.cc call some of these)
namespace wh_bind {

DevWs& dev_ws(const torch::Device& d) {
  static std::vector<DevWs*> ws(64, nullptr);
  const int i = d.index() < 0 ? 0 : d.index();
  TORCH_CHECK(i < 64, "device index out of range");
  if (!ws[i]) {
    auto o = torch::TensorOptions().device(d);
    auto* w = new DevWs();
    w->lb = torch::zeros({wh::lookback_ws_words()}, o.dtype(torch::kInt64));
    w->auc = torch::zeros({wh::auc_ws_persistent_bytes() / 8}, o.dtype(torch::kInt64));
    w->auc.select(0, wh::auc_ws_lohi_offset() / 8).fill_(-1);
    w->fwd_ticket = torch::zeros({wh::fwd_ticket_words()}, o.dtype(torch::kInt32));
    ws[i] = w;
  }
  return *ws[i];
}

wh::Lookback lookback(const torch::Device& d) {
  return wh::lookback_bind(dev_ws(d).lb.data_ptr());
}

// ------------------------------------------------------------------ scan
Tensor scan_excl(const Tensor& in) {
  CHECK_DEV(in); CHECK_CONT(in);
  c10::DeviceGuard g(in.device());
  const int64_t n = in.numel();
  auto o = torch::empty({n + 1}, in.options().dtype(torch::kInt64));
  auto tmp = torch::empty({wh::scan_tmp_elems(n)}, in.options().dtype(torch::kInt64));
  if (in.scalar_type() == torch::kInt32)
    wh::scan_i32(ptr<int32_t>(in), ptr<int64_t>(o), n, ptr<int64_t>(tmp), cur_stream(in));
  else {
    CHECK_DT(in, torch::kInt64);
    wh::scan_i64(ptr<int64_t>(in), ptr<int64_t>(o), n, ptr<int64_t>(tmp), cur_stream(in));
  }
  return o;
}

// worker side of the multi-shard exchange (psx.hip). rbuf: the received pull
// reply [R, vstride]; segS/segHS: int64 [P+1] over the keys sent per owner;
// vrecv: int64 [P] V rows received per owner. Returns (hdr [U, 2], rows
// int64 [1] = R actually used).
std::vector<Tensor> ps_unpack(const Tensor& rbuf, int64_t U, const Tensor& segS,
                              const Tensor& segHS, const Tensor& vrecv) {
  CHECK_IN(rbuf, torch::kFloat32);
  CHECK_IN(segS, torch::kInt64);
  CHECK_IN(segHS, torch::kInt64);
  CHECK_IN(vrecv, torch::kInt64);
  TORCH_CHECK(rbuf.dim() == 2, "ps_unpack: rbuf must be [R, vstride]");
  const int P = (int)segS.numel() - 1;
  TORCH_CHECK(segHS.numel() == P + 1 && vrecv.numel() == P, "ps_unpack: bad segment tables");
  c10::DeviceGuard g(rbuf.device());
  auto hdr = torch::empty({U, 2}, rbuf.options());
  auto rows = torch::empty({1}, segS.options());
  TORCH_CHECK(wh::ps_unpack(ptr<float>(rbuf), U, (int)rbuf.size(1), ptr<int64_t>(segS),
                            ptr<int64_t>(segHS), ptr<int64_t>(vrecv), P, ptr<float>(hdr),
                            ptr<int64_t>(rows), cur_stream(rbuf)),
              "ps_unpack: limits exceeded");
  return {hdr, rows};
}

// 12-byte key records {lo, hi, count} int32 [U, 3] (ucnt optional)
Tensor ps_records(const Tensor& uniq, const c10::optional<Tensor>& ucnt) {
  CHECK_IN(uniq, torch::kInt64);
  const int32_t* cp = nullptr;
  if (ucnt.has_value() && ucnt->defined()) {
    CHECK_IN((*ucnt), torch::kInt32);
    TORCH_CHECK(ucnt->numel() == uniq.numel(), "ps_records: count size mismatch");
    cp = ptr<int32_t>(*ucnt);
  }
  c10::DeviceGuard g(uniq.device());
  auto rec = torch::empty({uniq.numel(), 3}, uniq.options().dtype(torch::kInt32));
  wh::ps_records(reinterpret_cast<const uint64_t*>(uniq.data_ptr()), cp, uniq.numel(),
                 ptr<int32_t>(rec), cur_stream(uniq));
  return rec;
}

// C0 buffers from the owner counts [S+1] (S shards + the overflow flag), the
// V row counts [P] (optional) and this rank's has-data flag: (send int64
// [4P], payload int64 [S+1+5P]; payload[S+1 : S+1+4P] is the exchange's
// receive slot)
std::vector<Tensor> ps_c0(const Tensor& owner_cnt, const c10::optional<Tensor>& vcnt, int64_t P,
                          int64_t flag, bool loopback) {
  CHECK_IN(owner_cnt, torch::kInt64);
  const int S = (int)owner_cnt.numel() - 1;
  TORCH_CHECK(S >= 1 && S <= P, "ps_c0: owner counts must cover 1..P shards");
  const int64_t* vp = nullptr;
  if (vcnt.has_value() && vcnt->defined()) {
    CHECK_IN((*vcnt), torch::kInt64);
    TORCH_CHECK(vcnt->numel() == P, "ps_c0: vcnt size mismatch");
    vp = ptr<int64_t>(*vcnt);
  }
  c10::DeviceGuard g(owner_cnt.device());
  auto send = torch::empty({4 * P}, owner_cnt.options());
  auto payload = torch::empty({S + 1 + 5 * P}, owner_cnt.options());
  TORCH_CHECK(wh::ps_c0(ptr<int64_t>(owner_cnt), vp, S, (int)P, flag, ptr<int64_t>(send),
                        ptr<int64_t>(payload), cur_stream(owner_cnt), loopback ? 1 : 0),
              "ps_c0: too many peers");
  return {send, payload};
}

// gw [U] into the header rows of the push buffer gbuf [R, vstride] (in place)
void ps_pack_gw(const Tensor& gw, const Tensor& gbuf, const Tensor& segS, const Tensor& segHS,
                const Tensor& vrecv) {
  CHECK_IN(gw, torch::kFloat32);
  CHECK_IN(gbuf, torch::kFloat32);
  CHECK_IN(segS, torch::kInt64);
  CHECK_IN(segHS, torch::kInt64);
  CHECK_IN(vrecv, torch::kInt64);
  TORCH_CHECK(gbuf.dim() == 2, "ps_pack_gw: gbuf must be [R, vstride]");
  const int P = (int)segS.numel() - 1;
  c10::DeviceGuard g(gw.device());
  TORCH_CHECK(wh::ps_pack_gw(ptr<float>(gw), gw.numel(), (int)gbuf.size(1), ptr<int64_t>(segS),
                             ptr<int64_t>(segHS), ptr<int64_t>(vrecv), P, ptr<float>(gbuf),
                             cur_stream(gw)),
              "ps_pack_gw: limits exceeded");
}

// worker side of a multi-shard pull: renumber hdr vidx into local compact
// order; returns m as a device int64 [1] tensor
Tensor vidx_renumber(const Tensor& hdr) {
  CHECK_IN(hdr, torch::kFloat32);
  c10::DeviceGuard g(hdr.device());
  const int64_t n = hdr.numel() / 2;
  if (n > 0) {
    auto cnt = torch::empty({1}, hdr.options().dtype(torch::kInt64));
    if (wh::vidx_renumber_fused(ptr<float>(hdr), n, lookback(hdr.device()), ptr<int64_t>(cnt),
                                cur_stream(hdr)))
      return cnt;
  }
  auto flag = torch::empty({std::max<int64_t>(n, 1)}, hdr.options().dtype(torch::kInt32));
  auto pos = torch::zeros({n + 1}, hdr.options().dtype(torch::kInt64));
  auto stmp = torch::empty({wh::scan_tmp_elems(n)}, pos.options());
  wh::vidx_renumber(ptr<float>(hdr), n, ptr<int32_t>(flag), ptr<int64_t>(pos), ptr<int64_t>(stmp),
                    cur_stream(hdr));
  return pos.narrow(0, n, 1);
}

// keys % m (uint64 semantics), returned as a new tensor
Tensor key_mod(const Tensor& keys, int64_t m) {
  CHECK_IN(keys, torch::kInt64);
  TORCH_CHECK(m > 0, "max_key must be positive");
  c10::DeviceGuard g(keys.device());
  auto out = keys.clone();
  wh::key_mod(reinterpret_cast<uint64_t*>(out.data_ptr()), out.numel(), (uint64_t)m,
              cur_stream(keys));
  return out;
}

// ------------------------------------------------------- payload filter
// x [rows, w] f32 -> uint8 [rows, record_bytes]
Tensor quant_rows(const Tensor& x, int64_t nb, int64_t seed) {
  CHECK_IN(x, torch::kFloat32);
  TORCH_CHECK(nb >= 1 && nb <= 3, "fixed_bytes must be 1, 2 or 3");
  TORCH_CHECK(x.dim() == 2, "quant_rows: x must be [rows, w]");
  c10::DeviceGuard g(x.device());
  const int w = (int)x.size(1);
  auto out = torch::empty({x.size(0), wh::quant_record_bytes(w, (int)nb)},
                          x.options().dtype(torch::kUInt8));
  wh::quant_rows(ptr<float>(x), x.size(0), w, (int)nb, (uint64_t)seed, ptr<uint8_t>(out),
                 cur_stream(x));
  return out;
}

Tensor dequant_rows(const Tensor& q, int64_t w, int64_t nb) {
  CHECK_IN(q, torch::kUInt8);
  TORCH_CHECK(nb >= 1 && nb <= 3, "fixed_bytes must be 1, 2 or 3");
  TORCH_CHECK(q.dim() == 2 && q.size(1) == wh::quant_record_bytes((int)w, (int)nb),
              "dequant_rows: bad record size");
  c10::DeviceGuard g(q.device());
  auto x = torch::empty({q.size(0), w}, q.options().dtype(torch::kFloat32));
  wh::dequant_rows(ptr<uint8_t>(q), q.size(0), (int)w, (int)nb, ptr<float>(x), cur_stream(q));
  return x;
}

// region filter of the multi-shard exchange (quant.hip qregion_*): x the
// float layout (flat view), desc int64 [P, 6] on the device, built and
// bounds-checked on the host (kv/psx.py _QFilter) against x / out sizes.
Tensor ps_qpack(const Tensor& x, const Tensor& desc, int64_t rows, int64_t W, int64_t nb,
                int64_t seed) {
  CHECK_IN(x, torch::kFloat32);
  CHECK_IN(desc, torch::kInt64);
  TORCH_CHECK(nb >= 1 && nb <= 3 && W >= 1 && W <= 1024, "ps_qpack: bad record shape");
  TORCH_CHECK(desc.dim() == 2 && desc.size(1) == 6 && desc.size(0) >= 1, "ps_qpack: desc [P, 6]");
  c10::DeviceGuard g(x.device());
  auto out = torch::empty({rows, wh::quant_record_bytes((int)W, (int)nb)},
                          x.options().dtype(torch::kUInt8));
  wh::qregion_pack(ptr<float>(x), ptr<int64_t>(desc), (int)desc.size(0), rows, (int)W, (int)nb,
                   (uint64_t)seed, ptr<uint8_t>(out), cur_stream(x));
  return out;
}

void ps_qunpack(const Tensor& q, const Tensor& desc, int64_t W, int64_t nb, const Tensor& out) {
  CHECK_IN(q, torch::kUInt8);
  CHECK_IN(desc, torch::kInt64);
  CHECK_IN(out, torch::kFloat32);
  TORCH_CHECK(nb >= 1 && nb <= 3 && q.dim() == 2 &&
                  q.size(1) == wh::quant_record_bytes((int)W, (int)nb),
              "ps_qunpack: bad record size");
  TORCH_CHECK(desc.dim() == 2 && desc.size(1) == 6 && desc.size(0) >= 1, "ps_qunpack: desc [P, 6]");
  c10::DeviceGuard g(q.device());
  wh::qregion_unpack(ptr<uint8_t>(q), ptr<int64_t>(desc), (int)desc.size(0), q.size(0), (int)W,
                     (int)nb, ptr<float>(out), cur_stream(q));
}

Tensor trunc_u8(const Tensor& c) {
  CHECK_IN(c, torch::kInt32);
  c10::DeviceGuard g(c.device());
  auto out = torch::empty({c.numel()}, c.options().dtype(torch::kUInt8));
  wh::trunc_u8(ptr<int32_t>(c), c.numel(), ptr<uint8_t>(out), cur_stream(c));
  return out;
}

// ---------------------------------------------------------------- synth
std::vector<Tensor> synth_criteo(int64_t nrows, int64_t seed, int64_t step, const Tensor& card) {
  CHECK_IN(card, torch::kInt64);
  c10::DeviceGuard g(card.device());
  const int nfield = (int)card.numel();
  auto keys = torch::empty({nrows * nfield}, card.options());
  auto label = torch::empty({nrows}, card.options().dtype(torch::kFloat32));
  auto offset = torch::empty({nrows + 1}, card.options());
  wh::synth_criteo(nrows, (uint64_t)seed, (uint64_t)step, ptr<int64_t>(card), nfield,
                   reinterpret_cast<uint64_t*>(keys.data_ptr()), ptr<float>(label),
                   ptr<int64_t>(offset), cur_stream(card));
  return {keys, label, offset};
}

Tensor gather_rows(const Tensor& in, const Tensor& idx) {
  CHECK_IN(in, torch::kFloat32);
  CHECK_IN(idx, torch::kInt32);
  c10::DeviceGuard g(in.device());
  const int64_t width = in.dim() > 1 ? in.numel() / in.size(0) : 1;
  auto out = torch::empty({idx.numel(), width}, in.options());
  wh::gather_rows(ptr<float>(in), ptr<int32_t>(idx), idx.numel(), (int)width, ptr<float>(out),
                  cur_stream(in));
  return in.dim() > 1 ? out : out.view({idx.numel()});
}

}  // namespace wh_bind

PYBIND11_MODULE(_hip, m) {
  m.doc() = "wormhole_amd gfx950 HIP kernels";
  m.def("scan_excl", &scan_excl);
  bind_localize(m);
  bind_fm(m);  // LinearStep, DifactoStep, fm_*, spmv_t (before KVStore: their signatures)
  bind_psx(m);  // RcclComm, PSX_TX_*, PsxStep, a2a_plan, c10d_a2a_rows
  m.def("vidx_renumber", &vidx_renumber);
  m.def("ps_unpack", &ps_unpack);
  m.def("ps_pack_gw", &ps_pack_gw);
  m.def("ps_records", &ps_records);
  m.def("ps_c0", &ps_c0, py::arg("owner_cnt"), py::arg("vcnt"), py::arg("P"), py::arg("flag"),
        py::arg("loopback") = false);
  m.def("quant_rows", &quant_rows);
  m.def("key_mod", &key_mod);
  m.def("dequant_rows", &dequant_rows);
  m.def("trunc_u8", &trunc_u8);
  m.def("ps_qpack", &ps_qpack, py::arg("x"), py::arg("desc"), py::arg("rows"), py::arg("W"),
        py::arg("nb"), py::arg("seed"));
  m.def("ps_qunpack", &ps_qunpack, py::arg("q"), py::arg("desc"), py::arg("W"), py::arg("nb"),
        py::arg("out"));
  bind_auc(m);  // auc, auc_acc, auc_acc_side, auc_join, auc_host_threads, auc_sorted
  m.def("timing_flush", &timing_flush);
  m.def("synth_criteo", &synth_criteo);
  m.def("gather_rows", &gather_rows);
  // the stateless families, each from its own translation unit
  bind_bsp(m);
  bind_gbdt(m);
  bind_kmeans(m);
  bind_ingest(m);
  py::class_<KVStore>(m, "KVStore")
      .def(py::init<int64_t, int64_t, int64_t, int64_t>(), py::arg("cap"), py::arg("vcap"),
           py::arg("dim"), py::arg("device"))
      .def("find", &KVStore::find)
      .def("occupied", &KVStore::occupied)
      .def("linear_pull", &KVStore::linear_pull)
      .def("linear_push", &KVStore::linear_push)
      .def("difacto_push_cnt", &KVStore::difacto_push_cnt)
      .def("difacto_pull", &KVStore::difacto_pull)
      .def("difacto_open_pull",
           py::overload_cast<const Tensor&, bool, const c10::optional<Tensor>&,
                             const std::vector<double>&, int64_t, bool, int64_t, bool>(
               &KVStore::difacto_open_pull),
           py::arg("keys"), py::arg("insert"),
           py::arg("cnt"), py::arg("h"), py::arg("threshold"), py::arg("l1_shrk"), py::arg("seed"),
           py::arg("direct") = false)
      .def("difacto_push", &KVStore::difacto_push)
      .def("ps_open", &KVStore::ps_open, py::arg("keys"), py::arg("use_cnt"), py::arg("segS"),
           py::arg("segHS"), py::arg("rows_cap"), py::arg("insert"), py::arg("chains"), py::arg("h"),
           py::arg("threshold"), py::arg("l1_shrk"), py::arg("seed"),
           py::arg("chain_in") = py::none())
      .def("ps_push", &KVStore::ps_push, py::arg("slot"), py::arg("vpos"), py::arg("chain"),
           py::arg("head"), py::arg("segS"), py::arg("segHS"), py::arg("gbuf"), py::arg("h"),
           py::arg("threshold"), py::arg("l1_shrk"), py::arg("seed"),
           py::arg("prep_chain") = py::none(), py::arg("prep_n") = 0)
      .def("ps_push_linear", &KVStore::ps_push_linear, py::arg("slot"), py::arg("chain"),
           py::arg("head"), py::arg("segS"), py::arg("g"), py::arg("algo"), py::arg("alpha"),
           py::arg("beta"), py::arg("l1"), py::arg("l2"), py::arg("t0"),
           py::arg("prep_chain") = py::none(), py::arg("prep_n") = 0)
      .def("grow", &KVStore::grow)
      .def("grow_v", &KVStore::grow_v)
      .def("summary", &KVStore::summary)
      .def("summary_async", &KVStore::summary_async)
      .def("summary_read", &KVStore::summary_read)
      .def_property_readonly("dim", &KVStore::dim)
      .def_property_readonly("vstride", &KVStore::vstride)
      .def_property_readonly("cap", &KVStore::cap)
      .def_property_readonly("vcap", &KVStore::vcap)
      .def_readonly("ps_opens", &KVStore::opens_)
      .def_readonly("slots", &KVStore::slots_)
      .def_readonly("keys", &KVStore::keys_)
      .def_readonly("w", &KVStore::w_)
      .def_readonly("z", &KVStore::z_)
      .def_readonly("sq", &KVStore::sq_)
      .def_readonly("cnt", &KVStore::cnt_)
      .def_readonly("vrow", &KVStore::vrow_)
      .def_readonly("V", &KVStore::V_)
      .def_readonly("VG", &KVStore::VG_)
      .def_readonly("vnext", &KVStore::vnext_)
      .def_property_readonly("stats", [](const KVStore& k) {
        // counters summed over their shards: [8] int64 (a copy)
        return k.stats_.narrow(1, 0, wh::kStatCount).sum(0);
      })
      .def("reset_stats", [](KVStore& k, int64_t i0, int64_t i1) {
        k.stats_.narrow(1, i0, i1 - i0).zero_();
      })
      .def("add_stat", [](KVStore& k, int64_t i, int64_t v) {
        k.stats_.select(1, i).narrow(0, 0, 1).add_(v);
      });
}
