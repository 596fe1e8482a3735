// localize for module wormhole_amd._hip: LocalizeJob, the per-device
// workspace its jobs share, and their bindings. The sizing rules and the
// workspace's bookkeeping are host/localize_plan.h (also compiled into the
// host self-test); this file allocates, launches and reads.
#include "localize_job.h"

#include <memory>

#include "host/localize_plan.h"

namespace wh_bind {

// pinned count buffer + event of a localize job's one host read, reused (a
// pinned allocation, an event create and destroy per job were host time of
// the launch-bound small-minibatch step)
struct LocPinnedRead {
  int64_t* host = nullptr;
  int64_t cap = 0;
  hipEvent_t ev = nullptr;
  bool busy = false;
};

namespace {

// Per-device persistent localize workspace (allocated once; the kernels
// that use it leave it in its initial state). Intentionally leaked: it must
// outlive every stream-ordered use and the process exit order.
struct LocalizeWs {
  // hash tables (all ~0 between minibatches) and overflow counters (0
  // between minibatches), one per slot of `tables`
  Tensor tab[2], ovf[2];
  wh::LocTablePool tables;
  // partitioned localize: its own look-back workspace (a localize may be
  // begun on a side stream, concurrently with other look-back users) and
  // {per-partition publish words, arrival counter}
  Tensor lb, part_ws;
  // heavy-id hints, double-buffered by job parity: keys [2][kPartMaxHeavy]
  // u64, then counts [2][kPartMaxOwners] u32
  Tensor heavy_ws;
  wh::LocHeavyElection heavy;
  wh::LocHintScale hint;
  std::vector<std::unique_ptr<LocPinnedRead>> reads;

  LocPinnedRead* acquire_read(int64_t n) {
    for (auto& r : reads)
      if (!r->busy && r->cap >= n) {
        r->busy = true;
        return r.get();
      }
    auto r = std::make_unique<LocPinnedRead>();
    r->cap = std::max<int64_t>(n, 64);
    void* p = nullptr;
    WH_HIP_CHECK_HOST(hipHostMalloc(&p, r->cap * sizeof(int64_t), hipHostMallocDefault));
    r->host = static_cast<int64_t*>(p);
    WH_HIP_CHECK_HOST(hipEventCreateWithFlags(&r->ev, hipEventDisableTiming));
    r->busy = true;
    reads.push_back(std::move(r));
    return reads.back().get();
  }
};

LocalizeWs& loc_ws(const torch::Device& d) {
  static std::vector<LocalizeWs*> ws(64, nullptr);
  const int i = d.index() < 0 ? 0 : d.index();
  TORCH_CHECK(i < 64, "device index out of range");
  if (!ws[i]) {
    auto o = torch::TensorOptions().device(d).dtype(torch::kInt64);
    auto* w = new LocalizeWs();
    w->lb = torch::zeros({wh::lookback_ws_words()}, o);
    w->part_ws = torch::zeros({wh::kPartMaxDigits + 2}, o);
    w->heavy_ws = torch::zeros({2 * wh::kPartMaxHeavy + wh::kPartMaxOwners}, o);
    for (int b = 0; b < 2; ++b) {
      w->tab[b] = torch::full({1024}, -1, o);
      w->ovf[b] = torch::zeros({1}, o);
    }
    ws[i] = w;
  }
  return *ws[i];
}

// WH_TIMING=loc: the partitioned dedup stores per-partition phase
// timestamps (100 MHz) into a device buffer (loc_timing_read)
bool loc_timing() {
  static int on = -1;
  if (on < 0) on = timing_on("loc") ? 1 : 0;
  return on == 1;
}
Tensor& loc_timing_buf() {
  static Tensor t;
  if (!t.defined())
    t = torch::zeros({4 * wh::kPartMaxDigits},
                     torch::TensorOptions().dtype(torch::kInt64).device(torch::kCUDA));
  return t;
}

// localize retries after a partition overflowed its LDS table (diagnostics)
int64_t& loc_retries() {
  static int64_t n = 0;
  return n;
}

std::vector<Tensor> localize(const Tensor& keys, const Tensor& offset,
                             const c10::optional<Tensor>& val, int64_t nshard, int64_t hint,
                             py::object exchange) {
  LocalizeJob job(keys, offset, val, nshard, hint, exchange);
  return job.finish();
}

}  // namespace

LocalizeJob::LocalizeJob(const Tensor& keys, const Tensor& offset,
                         const c10::optional<Tensor>& val, int64_t nshard, int64_t hint,
                         NativeExchange nex, bool defer_exchange, const char* form)
    : keys_(keys), offset_(offset), nshard_(nshard), nex_(std::move(nex)), form_(form),
      defer_(defer_exchange) {
  CHECK_IN(keys, torch::kInt64);
  CHECK_IN(offset, torch::kInt64);
  TORCH_CHECK(nshard >= 1 && nshard <= 1024, "nshard out of range");
  nnz_ = keys.numel();
  TORCH_CHECK(nnz_ < (int64_t)INT32_MAX, "minibatch too large for int32 local ids");
  if (val.has_value() && val->defined() && val->numel() > 0) {
    CHECK_IN((*val), torch::kFloat32);
    TORCH_CHECK(val->numel() == nnz_);
    val_ = *val;
  }
  hint = loc_ws(keys.device()).hint.scaled(hint, nnz_);
  safe_ = wh::loc_safe_size(nnz_);
  tsize_ = wh::loc_hinted_size(hint, safe_);
  c10::DeviceGuard g(keys.device());
  // the partitioned path unless a deterministic localize is asked for (the
  // hash path is the deterministic one, WH_DETERMINISTIC=1) or the minibatch
  // does not fit its plan; the hash path is the fallback
  plan_ = wh::loc_part_plan(nnz_, offset.numel() - 1, (int)nshard, wh::loc_uest(hint, nnz_), true);
  part_ = plan_.ok && !deterministic();
  enqueue();
}

LocalizeJob::~LocalizeJob() {
  // abandoned before its read: the copy may still be in flight
  if (rd_) (void)hipEventSynchronize(rd_->ev);
  release(kAll);
}

// The one place a job gives back what it holds in the device's workspace;
// giving back what it does not hold (any more) does nothing.
void LocalizeJob::release(unsigned what) {
  LocalizeWs& ws = loc_ws(keys_.device());
  if ((what & kRead) && rd_) {
    rd_->busy = false;
    rd_ = nullptr;
  }
  if (what & kInflight) ws.heavy.release(counted_);
  if ((what & kTable) && tab_ >= 0) {
    // after finish() the assign has emptied the table; before, it may hold keys
    done_ ? ws.tables.assigned(tab_) : ws.tables.abandoned(tab_);
    tab_ = -1;
  }
}

void LocalizeJob::exchange() {
  TORCH_CHECK(!done_, "localize job already finished");
  if (!defer_ || exchanged_) return;
  c10::DeviceGuard g(keys_.device());
  exchanged_ = true;
  exchange_and_read();
}

std::vector<Tensor> LocalizeJob::counts() {
  TORCH_CHECK(!done_, "localize job already finished");
  if (owner_cnt_h_.defined()) return {owner_cnt_h_, recv_h_};
  TORCH_CHECK(!defer_ || exchanged_, "localize: counts() before the deferred exchange()");
  c10::DeviceGuard g(keys_.device());
  while (true) {
    wait_event(rd_->ev);
    const auto over = wh::loc_overflow(rd_->host, nshard_, nrecv_, stride_);
    if (!over.any) break;
    if (part_) {  // a partition overflowed its LDS table (here or on a peer)
      ++loc_retries();
      part_ = false;
      release(kInflight);
    } else {
      TORCH_CHECK(!(over.own && tsize_ >= safe_), "localize: table overflow");
    }
    // every rank saw the same flags: all retry at the safe size together
    tsize_ = safe_;
    enqueue();
  }
  const int64_t* h = rd_->host;
  owner_cnt_h_ = torch::empty({nshard_}, torch::kInt64);
  std::copy(h, h + nshard_, owner_cnt_h_.data_ptr<int64_t>());
  // everything after the owner counts (the peers' values and any extra)
  const int64_t ntail = nrecv_ ? dev_counts_.numel() - nshard_ - 1 : 0;
  recv_h_ = torch::empty({ntail}, torch::kInt64);
  std::copy(h + nshard_ + 1, h + nshard_ + 1 + ntail, recv_h_.data_ptr<int64_t>());
  release(kRead);  // read and copied out: back to the pool
  return {owner_cnt_h_, recv_h_};
}

std::vector<Tensor> LocalizeJob::finish() {
  counts();
  c10::DeviceGuard g(keys_.device());
  auto s = cur_stream(keys_);
  auto i32 = keys_.options().dtype(torch::kInt32);
  auto i64 = keys_.options().dtype(torch::kInt64);
  int64_t U = 0;
  for (int64_t p = 0; p < nshard_; ++p) U += owner_cnt_h_.data_ptr<int64_t>()[p];
  loc_ws(keys_.device()).hint.finished(nnz_, U);
  if (part_) {  // everything was computed before the host read
    done_ = true;
    release(kInflight);
    return {uniq_.narrow(0, 0, U), ucnt_.narrow(0, 0, U), owner_cnt_h_, lid_,
            csc_off_.narrow(0, 0, U + 1), csc_row_, csc_val_, recv_h_};
  }
  const int64_t nnz = nnz_, nrows = offset_.numel() - 1;
  const float* vp = val_.defined() ? ptr<float>(val_) : nullptr;
  auto tlid = torch::empty({tsize_}, i32);
  auto uniq = torch::empty({U}, i64);
  wh::loc_assign(reinterpret_cast<uint64_t*>(tkeys_.data_ptr()), tsize_, (int)nshard_,
                 ptr<int64_t>(blkoff_), ptr<int32_t>(tlid),
                 reinterpret_cast<uint64_t*>(uniq.data_ptr()), s);
  done_ = true;
  release(kTable);  // loc_assign empties the table again
  auto row_of = torch::empty({std::max<int64_t>(nnz, 1)}, i32);
  const int64_t n1 = std::max<int64_t>(nnz, 1);
  auto lid = torch::empty({nnz}, i32);
  auto work = torch::empty({3 * n1}, i32);  // pos | sorted lid | sorted pos
  wh::loc_rows_lid(ptr<int64_t>(offset_), nrows, ptr<int32_t>(slot_of_), ptr<int32_t>(tlid),
                   ptr<int32_t>(row_of), ptr<int32_t>(lid), vp ? ptr<int32_t>(work) : nullptr, s);
  const size_t sbytes = wh::loc_sort_tmp_bytes(nnz, U);
  auto stmp = torch::empty({(int64_t)sbytes + 16}, keys_.options().dtype(torch::kUInt8));
  auto csc_off = torch::empty({U + 1}, i64);
  auto ucnt = torch::empty({U}, i32);
  auto csc_row = torch::empty({nnz}, i32);
  auto csc_val = vp ? torch::empty({nnz}, keys_.options().dtype(torch::kFloat32))
                    : torch::empty({0}, keys_.options().dtype(torch::kFloat32));
  int32_t* wp = ptr<int32_t>(work);
  wh::loc_csc(ptr<int32_t>(row_of), vp, nnz, U, ptr<int32_t>(lid), wp, wp + n1, wp + 2 * n1,
              stmp.data_ptr(), sbytes, ptr<int64_t>(csc_off), ptr<int32_t>(ucnt),
              ptr<int32_t>(csc_row), vp ? ptr<float>(csc_val) : nullptr, s);
  return {uniq, ucnt, owner_cnt_h_, lid, csc_off, csc_row, csc_val, recv_h_};
}

// One begin (the constructor's, or a retry's) on the current stream. An
// overflow retry from counts() exchanges at once, deferred or not: every
// rank retries there together.
void LocalizeJob::enqueue() {
  owner_cnt_ = part_ ? enqueue_part() : enqueue_hash();
  if (!defer_ || exchanged_) exchange_and_read();
}

// partitioned path: every output is produced before the count read
Tensor LocalizeJob::enqueue_part() {
  auto s = cur_stream(keys_);
  LocalizeWs& ws = loc_ws(keys_.device());
  const int64_t nnz = nnz_, nrows = offset_.numel() - 1;
  const int nsh = (int)nshard_;
  const float* vp = val_.defined() ? ptr<float>(val_) : nullptr;
  const int64_t nv = vp ? nnz : 0;
  auto owner_cnt = torch::empty({nshard_ + 1}, keys_.options().dtype(torch::kInt64));
  {
    // the job's outputs carved from ONE allocation (six separate tensors
    // were six trips through the allocator per minibatch)
    Carve c;
    const int64_t o_u = c.add(nnz * 8), o_c = c.add(nnz * 4), o_o = c.add((nnz + 1) * 8),
                  o_r = c.add(nnz * 4), o_v = c.add(nv * 4), o_l = c.add(nnz * 4);
    c.alloc(keys_.options());
    uniq_ = c.view(o_u, nnz, torch::kInt64);
    ucnt_ = c.view(o_c, nnz, torch::kInt32);
    csc_off_ = c.view(o_o, nnz + 1, torch::kInt64);
    csc_row_ = c.view(o_r, nnz, torch::kInt32);
    csc_val_ = c.view(o_v, nv, torch::kFloat32);
    lid_ = c.view(o_l, nnz, torch::kInt32);
  }
  // heavy-id hints: read the set the previous job elected, elect into the
  // other buffer; a job begun while another is in flight uses none
  wh::PartHeavy hv{};
  const auto pick = ws.heavy.begin(nshard_, plan_.nho, counted_);
  if (pick.elect) {
    auto* hk = reinterpret_cast<uint64_t*>(ws.heavy_ws.data_ptr());
    auto* hc = reinterpret_cast<uint32_t*>(hk + 2 * wh::kPartMaxHeavy);
    hv.keys = hk + pick.read * wh::kPartMaxHeavy;
    hv.cnt = hc + pick.read * wh::kPartMaxOwners;
    hv.nho = pick.nho_read;
    hv.next_keys = hk + pick.write * wh::kPartMaxHeavy;
    hv.next_cnt = hc + pick.write * wh::kPartMaxOwners;
    hv.nho_next = plan_.nho;
    hv.thr = wh::loc_heavy_thr(nnz);
  }
  // the job's temporaries in ONE allocation (eight separate tensors were
  // eight trips through the allocator and dispatcher per minibatch: host
  // time is the bound of the multi-shard step at 10k rows); the stream-
  // ordered allocator keeps it safe to drop at the end of this call
  const int64_t nh = (int64_t)plan_.ndig * plan_.ntiles;
  const int64_t ng = wh::loc_part_groups(plan_) * plan_.ndig;
  Carve c;
  const int64_t o_hist = c.add(nh * 4), o_gsum = c.add(ng * 4),
                o_base = c.add((plan_.ndig + 1) * 8), o_pk = c.add(nnz * 8), o_pr = c.add(nnz * 4),
                o_pv = c.add(nv * 4), o_pos = c.add(nnz * 4), o_plid = c.add(nnz * 4);
  c.alloc(keys_.options());
  auto* hist = c.at<uint32_t>(o_hist);
  auto* gsum = c.at<uint32_t>(o_gsum);
  auto* base = c.at<int64_t>(o_base);
  auto* pk = c.at<uint64_t>(o_pk);
  auto* pr = c.at<int32_t>(o_pr);
  auto* pv = vp ? c.at<float>(o_pv) : nullptr;
  auto* pos_of = c.at<int32_t>(o_pos);
  auto* plid = c.at<int32_t>(o_plid);
  const auto* kp = reinterpret_cast<const uint64_t*>(keys_.data_ptr());
  wh::loc_part_hist(kp, ptr<int64_t>(offset_), nrows, nsh, plan_, hv, hist, s);
  wh::loc_part_offsets(plan_, hist, gsum, base, s);
  wh::loc_part_scatter(kp, vp, ptr<int64_t>(offset_), nrows, nsh, plan_, hv, base, gsum, hist, pk,
                       pr, pv, pos_of, s);
  auto* pw = reinterpret_cast<unsigned long long*>(ws.part_ws.data_ptr());
  wh::loc_part_dedup(pk, pr, pv, nnz, nsh, plan_, hv, base, wh::lookback_bind(ws.lb.data_ptr()),
                     reinterpret_cast<uint64_t*>(uniq_.data_ptr()), ptr<int32_t>(ucnt_),
                     ptr<int64_t>(csc_off_), ptr<int32_t>(csc_row_),
                     vp ? ptr<float>(csc_val_) : nullptr, plid, pw,
                     reinterpret_cast<unsigned int*>(pw + wh::kPartMaxDigits),
                     ptr<int64_t>(owner_cnt), s,
                     loc_timing() ? ptr<int64_t>(loc_timing_buf()) : nullptr);
  wh::loc_part_lid(pos_of, plid, nnz, ptr<int32_t>(lid_), s);
  return owner_cnt;
}

// hash path: insert + owner counts now, the rest in finish()
Tensor LocalizeJob::enqueue_hash() {
  auto s = cur_stream(keys_);
  LocalizeWs& ws = loc_ws(keys_.device());
  auto i32 = keys_.options().dtype(torch::kInt32);
  auto i64 = keys_.options().dtype(torch::kInt64);
  if (tab_ < 0) {  // (a retry at the safe size keeps its slot)
    tab_ = ws.tables.acquire();
    TORCH_CHECK(tab_ >= 0, "localize: at most two minibatches in flight per device");
  }
  Tensor& tab = ws.tab[tab_];
  Tensor& ovf = ws.ovf[tab_];
  const auto prep = ws.tables.prepare(tab_, tab.numel(), tsize_);
  if (prep == wh::LocTablePool::kRealloc) tab = torch::full({safe_}, -1, i64);
  else if (prep == wh::LocTablePool::kRefill) tab.fill_(-1);
  if (prep != wh::LocTablePool::kReady) ovf.zero_();
  tkeys_ = tab.narrow(0, 0, tsize_);
  slot_of_ = torch::empty({std::max<int64_t>(nnz_, 1)}, i32);
  auto owner_cnt = torch::empty({nshard_ + 1}, i64);  // [nshard] = overflow count
  wh::loc_insert(reinterpret_cast<const uint64_t*>(keys_.data_ptr()), nnz_,
                 reinterpret_cast<uint64_t*>(tkeys_.data_ptr()), tsize_, ptr<int32_t>(slot_of_),
                 ptr<int64_t>(ovf), s);
  blkoff_ = torch::empty({nshard_ * wh::loc_owner_blocks(tsize_)}, i64);
  wh::loc_owner_count(reinterpret_cast<const uint64_t*>(tkeys_.data_ptr()), tsize_, (int)nshard_,
                      ptr<int64_t>(blkoff_), ptr<int64_t>(owner_cnt), ptr<int64_t>(ovf), s);
  return owner_cnt;
}

// A Python exchange as a NativeExchange (None: no exchange). The callable
// gets the device owner counts and returns either
//  - the extended protocol (kv/psx.py): (payload, stream handle, stride,
//    world), payload = [owner_cnt (nshard+1) | stride values per peer,
//    {count, overflow flag, ...} | extra], already on that stream; the read
//    goes on that stream so the compute stream never waits for the exchange;
//  - or the device i64 [2W] of a count all-to-all on the current stream.
NativeExchange LocalizeJob::from_python(py::object exchange) {
  if (exchange.is_none()) return NativeExchange();
  return [exchange](const Tensor& owner_cnt) {
    py::object r = exchange(owner_cnt);
    if (py::isinstance<py::tuple>(r)) {
      auto t = r.cast<py::tuple>();
      TORCH_CHECK(t.size() == 4, "localize: extended exchange returns 4 items");
      return std::make_tuple(t[0].cast<Tensor>(),
                             reinterpret_cast<hipStream_t>(t[1].cast<intptr_t>()),
                             t[2].cast<int64_t>(), t[3].cast<int64_t>());
    }
    Tensor recv = r.cast<Tensor>();
    TORCH_CHECK(recv.scalar_type() == torch::kInt64 && recv.numel() % 2 == 0,
                "localize: exchange must return int64 [2 * world]");
    return std::make_tuple(torch::cat({owner_cnt, recv.reshape({-1}).to(owner_cnt.device())}),
                           cur_stream(owner_cnt), (int64_t)2, recv.numel() / 2);
  };
}

// The count exchange and the ASYNC copy of its payload into pinned host
// memory (+ an event): nothing blocks here.
void LocalizeJob::exchange_and_read() {
  Tensor payload = owner_cnt_;  // (no exchange: the owner counts alone)
  hipStream_t cs = cur_stream(keys_);  // stream of the count read
  int64_t stride = 2, world = 0;
  if (nex_) {
    std::tie(payload, cs, stride, world) = nex_(owner_cnt_);
    TORCH_CHECK(payload.scalar_type() == torch::kInt64 && stride >= 2 &&
                    payload.numel() >= nshard_ + 1 + stride * world,
                "localize: bad ", form_, " exchange payload");
  }
  stride_ = stride;
  nrecv_ = stride * world;
  dev_counts_ = payload.contiguous();
  // (a retry: the last copy was waited for) keep the pinned buffer if it fits
  if (rd_ && rd_->cap < dev_counts_.numel()) release(kRead);
  if (!rd_) rd_ = loc_ws(keys_.device()).acquire_read(dev_counts_.numel());
  WH_HIP_CHECK_HOST(hipMemcpyAsync(rd_->host, dev_counts_.data_ptr(),
                                   dev_counts_.numel() * sizeof(int64_t), hipMemcpyDeviceToHost,
                                   cs));
  WH_HIP_CHECK_HOST(hipEventRecord(rd_->ev, cs));
}

void bind_localize(py::module_& m) {
  py::class_<LocalizeJob>(m, "LocalizeJob")
      .def(py::init<const Tensor&, const Tensor&, const c10::optional<Tensor>&, int64_t, int64_t,
                    py::object, bool>(),
           py::arg("keys"), py::arg("offset"), py::arg("val") = py::none(), py::arg("nshard") = 1,
           py::arg("hint") = 0, py::arg("exchange") = py::none(),
           py::arg("defer_exchange") = false)
      .def("exchange", &LocalizeJob::exchange)
      .def("counts", &LocalizeJob::counts)
      .def("finish", &LocalizeJob::finish);
  m.def("loc_timing_read", []() { return loc_timing_buf().clone(); });
  m.def("loc_retries", []() { return loc_retries(); },
        "localize jobs redone on the hash path after a partition overflow (count)");
  m.def("localize", &localize, py::arg("keys"), py::arg("offset"), py::arg("val") = py::none(),
        py::arg("nshard") = 1, py::arg("hint") = 0, py::arg("exchange") = py::none());
}

}  // namespace wh_bind
