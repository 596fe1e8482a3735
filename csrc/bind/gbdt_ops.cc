// Bindings of the GBDT family (module wormhole_amd._hip): binning, histograms,
// split search, partition, objectives, prediction (dense and CSR; per tree,
// and the packed forest in one pass per chunk) and the two tree growers.
// Stateless: tensors are validated, outputs sized and kernels
// launched on the current PyTorch HIP stream.
#include "bind_common.h"

#include <array>
#include <cstring>
#include <limits>
#include <map>
#include <tuple>
#include <utility>

#include "host/gbdt_aft.h"
#include "host/gbdt_dart_plan.h"
#include "host/gbdt_leaf_plan.h"
#include "host/gbdt_forest_plan.h"
#include "host/gbdt_hist_plan.h"
#include "host/gbdt_level_plan.h"
#include "host/gbdt_node_rule.h"
#include "host/gbdt_objective.h"
#include "host/gbdt_quantile_plan.h"
#include "host/gbdt_rank_plan.h"
#include "host/gbdt_shap_plan.h"
#include "host/gbdt_survival_plan.h"

namespace wh_bind {
namespace {

// ------------------------------------------------------------------ gbdt
Tensor gbdt_bin(const Tensor& X, const Tensor& cuts, const Tensor& cut_off) {
  CHECK_IN(X, torch::kFloat32);
  CHECK_IN(cuts, torch::kFloat32);
  CHECK_IN(cut_off, torch::kInt32);
  TORCH_CHECK(X.dim() == 2 && cut_off.numel() == X.size(1) + 1);
  c10::DeviceGuard g(X.device());
  auto B = torch::empty({X.size(0), X.size(1)}, X.options().dtype(torch::kUInt8));
  wh::gbdt_bin(ptr<float>(X), X.size(0), (int)X.size(1), ptr<float>(cuts), ptr<int32_t>(cut_off),
               ptr<uint8_t>(B), cur_stream(X));
  return B;
}

// The arguments of wh::gbdt_hist that stay the same for every histogram of a
// tree (and of the stand-alone binding): the checked bin matrix, gradients
// and fixed-point scales, the sizes, the stream. A call site passes only
// what differs.
struct HistCtx {
  const Tensor &B, &gpair, &qscale;
  const int nbin, max_fcnt;
  const int chunk;  // rows per task of lists addressed by chunk index (0: row ranges)
  int F;
  bool dw;
  hipStream_t s;

  HistCtx(const Tensor& B, const Tensor& gpair, const Tensor& qscale, int64_t nbin,
          int64_t max_fcnt, int chunk)
      : B(B), gpair(gpair), qscale(qscale), nbin((int)nbin), max_fcnt((int)max_fcnt),
        chunk(chunk) {
    CHECK_IN(B, torch::kUInt8);
    CHECK_IN(gpair, torch::kFloat32);
    CHECK_IN(qscale, torch::kFloat32);
    F = (int)B.size(1);
    // dword row loads need every group 4-aligned; the caller guarantees equal
    // multiple-of-4 groups when F % 4 == 0 (checked again here on the host copy)
    dw = F % 4 == 0 && max_fcnt % 4 == 0;
    s = cur_stream(B);
  }

  // the fixed-point partial sums of ntask tasks
  Tensor part(int64_t ntask) const {
    return torch::empty({ntask * wh::gbdt_hist_pstride(max_fcnt, nbin)},
                        gpair.options().dtype(torch::kInt64));
  }

  // dseg: the device {begin, end} pairs the tasks' chunks index (or null);
  // ntask_dev: the device task count when ntask is only its bound; sib_*:
  // the reduce also derives the sibling histograms (wh_kernels.h)
  void run(const Tensor& ridx, const int32_t* tasks, int64_t ntask, const int32_t* red,
           int64_t nred, const Tensor& part, const Tensor& hist, const int32_t* dseg,
           const int32_t* ntask_dev = nullptr, const double* sib_hf = nullptr,
           const int32_t* sib_sp = nullptr, const int32_t* sib_par = nullptr) const {
    wh::gbdt_hist(ptr<uint8_t>(B), F, nbin, ptr<int32_t>(ridx), ptr<float>(gpair),
                  ptr<float>(qscale), tasks, (int)ntask, red, (int)nred, max_fcnt, dw,
                  ptr<int64_t>(part), ptr<double>(hist), s, dseg, chunk, ntask_dev,
                  qscale.numel() == 3, sib_hf, sib_sp, sib_par);
  }
};

// tasks [T, 5] (slot, fbeg, fcnt, rbeg, rend); red [R, 6] (slot, fbeg, fcnt,
// t0, nt, tstride) sums the fp32 partials of tasks t0 + k * tstride into hist
// qscale [2] float32 = {2^eg, 2^eh}: fixed-point scales of g and h (see gbdt.hip);
// [3] = {2^eg, 2^eh, R}: int32 LDS sums over <= R rows (k_hist W32)
void gbdt_hist(const Tensor& B, int64_t nbin, const Tensor& ridx, const Tensor& gpair,
               const Tensor& qscale, const Tensor& tasks, const Tensor& red, int64_t max_fcnt,
               const Tensor& hist) {
  const HistCtx cx(B, gpair, qscale, nbin, max_fcnt, /*chunk=*/0);
  CHECK_IN(ridx, torch::kInt32);
  CHECK_IN(tasks, torch::kInt32);
  CHECK_IN(red, torch::kInt32);
  CHECK_IN(hist, torch::kFloat64);
  TORCH_CHECK(nbin >= 1 && nbin <= 255, "nbin must be in [1, 255]");
  TORCH_CHECK(qscale.numel() == 2 || qscale.numel() == 3,
              "qscale must hold {scale_g, scale_h} or {scale_g, scale_h, int32 rows}");
  TORCH_CHECK(wh::gbdt_hist_lds((int)max_fcnt, (int)nbin) <= 160 * 1024, "feature group too wide");
  TORCH_CHECK(tasks.dim() == 2 && tasks.size(1) == 5);
  TORCH_CHECK(red.dim() == 2 && red.size(1) == 6);
  TORCH_CHECK(hist.numel() % ((int64_t)cx.F * nbin * 2) == 0, "hist must be [S, F, nbin, 2]");
  c10::DeviceGuard g(B.device());
  cx.run(ridx, ptr<int32_t>(tasks), tasks.size(0), ptr<int32_t>(red), red.size(0),
         cx.part(tasks.size(0)), hist, nullptr);
}

// The best split of each of S slots into out [S, 6] {gain, feature, bin, dir,
// GL, HL}: hist [S, F, nbin, 2], totals [S x 2] and the [F x nbin] candidate
// mask on hist's device. False: the kernel refused (nbin > 1024 or no input).
// c: the constraints over hist's features and these slots (wh_kernels.h).
bool split_search(const Tensor& hist, const double* totals, const uint8_t* valid, int S,
                  double alpha, double lambda, double mcw, const Tensor& out, hipStream_t s,
                  const wh::GbdtCons& c) {
  auto cand = torch::empty({std::max<int64_t>(S * hist.size(1) * 4, 1)}, hist.options());
  return wh::gbdt_split(ptr<double>(hist), totals, valid, S, (int)hist.size(1), (int)hist.size(2),
                        alpha, lambda, mcw, ptr<double>(cand), ptr<double>(out), s, c);
}

// An array of a constraint, when `given`: `name` must be a contiguous GPU
// tensor of dtype dt (CHECK_IN's texts, under the tensor's and the caller's
// names) with n elements on like's device. Null when it is not given.
template <typename T>
const T* cons_array(bool given, const c10::optional<Tensor>& t, c10::ScalarType dt, int64_t n,
                    const Tensor& like, const char* who, const char* name, const char* shape) {
  if (!given) return nullptr;
  TORCH_CHECK(t->is_cuda(), who, ": ", name, " must be a GPU tensor");
  TORCH_CHECK(t->is_contiguous(), who, ": ", name, " must be contiguous");
  TORCH_CHECK(t->scalar_type() == dt, who, ": ", name, " has wrong dtype ", t->scalar_type());
  TORCH_CHECK(t->device() == like.device(), who, ": ", name, " on another device");
  TORCH_CHECK(t->numel() == n, who, ": ", name, " must be ", shape);
  return reinterpret_cast<const T*>(t->data_ptr());
}

// The constraints of a stand-alone split search (`who`): the optional pairs
// (mono [F] int8, bounds [S, 2] float64) and (fmask [F], state [S], int64 bit
// patterns), each both or neither
wh::GbdtCons split_cons(const c10::optional<Tensor>& mono, const c10::optional<Tensor>& bounds,
                        const c10::optional<Tensor>& fmask, const c10::optional<Tensor>& state,
                        const Tensor& like, int64_t S, int64_t F, const char* who) {
  const bool m = mono.has_value(), i = fmask.has_value();
  TORCH_CHECK(m == bounds.has_value(), who, ": mono and bounds go together");
  TORCH_CHECK(i == state.has_value(), who, ": fmask and state go together");
  wh::GbdtCons c;
  c.mono = cons_array<int8_t>(m, mono, torch::kInt8, F, like, who, "mono", "[F]");
  c.bnd = cons_array<double>(m, bounds, torch::kFloat64, 2 * S, like, who, "bounds", "[S, 2]");
  c.fmask = cons_array<uint64_t>(i, fmask, torch::kInt64, F, like, who, "fmask", "[F]");
  c.state = cons_array<uint64_t>(i, state, torch::kInt64, S, like, who, "state", "[S]");
  return c;
}

// The constraints of a grower, checked once: mono [F] int8
// (monotone_constraints) and fmask [F] int64 (interaction_constraints) on B's
// device, each optional and over ALL features, and max_delta_step, which
// bounds the root's interval and therefore needs mono (all zero for no signs).
struct GrowCons {
  const int8_t* mono;
  const uint64_t* fmask;
  bool mono_on, inter_on;
  double top;  // the root's interval is (-top, top)

  GrowCons(const c10::optional<Tensor>& mono_, const c10::optional<Tensor>& fmask_,
           double max_delta_step, const Tensor& B, int F, const char* who)
      : mono(cons_array<int8_t>(present(mono_), mono_, torch::kInt8, F, B, who, "mono", "[F]")),
        fmask(cons_array<uint64_t>(present(fmask_), fmask_, torch::kInt64, F, B, who, "fmask",
                                   "[F]")),
        mono_on(mono != nullptr), inter_on(fmask != nullptr),
        top(max_delta_step > 0 ? max_delta_step : std::numeric_limits<double>::infinity()) {
    TORCH_CHECK(max_delta_step >= 0 && (max_delta_step == 0 || mono_on), who,
                ": max_delta_step >= 0, and it needs mono (all zero for no signs)");
  }

  // a split search over the slots whose intervals start at bnd [. x 2] and
  // whose group sets start at state [.] (neither is read when its constraint
  // is off) and over the features from f_lo on
  wh::GbdtCons at(const double* bnd, const uint64_t* state, int64_t f_lo = 0) const {
    wh::GbdtCons c;
    if (mono_on) c.mono = mono + f_lo, c.bnd = bnd;
    if (inter_on) c.fmask = fmask + f_lo, c.state = state;
    return c;
  }
  // (the same from slot0 of two tables, undefined when their constraint is off)
  wh::GbdtCons at(const Tensor& bnd, const Tensor& state, int64_t slot0 = 0,
                  int64_t f_lo = 0) const {
    return at(mono_on ? ptr<double>(bnd) + 2 * slot0 : nullptr,
              inter_on ? ptr<uint64_t>(state) + slot0 : nullptr, f_lo);
  }

  // a bookkeeping step, which also writes: the children's tables (undefined
  // when there are none), or the leaf loop's own in place
  wh::GbdtCons step(const Tensor& bnd, const Tensor& state, const Tensor& bnd_out,
                    const Tensor& state_out) const {
    wh::GbdtCons c = at(bnd, state);
    if (mono_on && bnd_out.defined()) c.bnd_out = ptr<double>(bnd_out);
    if (inter_on && state_out.defined()) c.state_out = ptr<uint64_t>(state_out);
    return c;
  }
};

Tensor gbdt_split(const Tensor& hist, const Tensor& totals, const Tensor& valid, double alpha,
                  double lambda, double min_child_weight, const c10::optional<Tensor>& mono,
                  const c10::optional<Tensor>& bounds, const c10::optional<Tensor>& fmask,
                  const c10::optional<Tensor>& state) {
  CHECK_IN(hist, torch::kFloat64);
  CHECK_IN(totals, torch::kFloat64);
  CHECK_IN(valid, torch::kBool);
  c10::DeviceGuard g(hist.device());
  TORCH_CHECK(hist.dim() == 4 && hist.size(3) == 2, "hist must be [S, F, nbin, 2]");
  const int S = (int)hist.size(0), F = (int)hist.size(1), nbin = (int)hist.size(2);
  TORCH_CHECK(totals.numel() == 2 * (int64_t)S, "totals must be [S, 2]");
  TORCH_CHECK(valid.numel() == (int64_t)F * nbin, "valid must be [F, nbin]");
  auto out = torch::empty({S, 6}, hist.options());
  TORCH_CHECK(split_search(hist, ptr<double>(totals), ptr<uint8_t>(valid), S, alpha, lambda,
                           min_child_weight, out, cur_stream(hist),
                           split_cons(mono, bounds, fmask, state, hist, S, F, "gbdt_split")),
              "gbdt_split: nbin > 1024 or empty input");
  return out;
}

Tensor gbdt_seg_fill(const Tensor& beg, const Tensor& node, int64_t n) {
  CHECK_IN(beg, torch::kInt32);
  CHECK_IN(node, torch::kInt32);
  TORCH_CHECK(beg.numel() == node.numel() && beg.numel() > 0, "segment arrays mismatch");
  c10::DeviceGuard g(beg.device());
  auto out = torch::empty({n}, beg.options());
  wh::gbdt_seg_fill(ptr<int32_t>(beg), ptr<int32_t>(node), (int)beg.numel(), n, ptr<int32_t>(out),
                    cur_stream(beg));
  return out;
}

// The stable partition of the split nodes' rows from their go-left flags
// (left [n], one per ridx position): scan of the flags, per-node left counts
// nleft[node] = lscan[seg_end] - lscan[seg_beg], scatter. The counts are
// copied into *nleft when it is defined, else *nleft becomes them; the new
// ridx is written to out (allocated here unless the caller did) and returned.
Tensor partition_by_flags(const Tensor& ridx, const Tensor& pos_node, const Tensor& left,
                          const int32_t* node_feat, const Tensor& seg_beg, const Tensor& seg_end,
                          Tensor* nleft, Tensor out, hipStream_t s) {
  const int64_t n = ridx.numel();
  auto lscan = torch::empty({n + 1}, ridx.options().dtype(torch::kInt64));
  auto tmp = torch::empty({wh::scan_tmp_elems(n)}, lscan.options());
  wh::scan_i32(ptr<int32_t>(left), ptr<int64_t>(lscan), n, ptr<int64_t>(tmp), s);
  auto nl = (lscan.index_select(0, seg_end.to(torch::kInt64)) -
             lscan.index_select(0, seg_beg.to(torch::kInt64))).to(torch::kInt32);
  *nleft = nleft->defined() ? nleft->copy_(nl) : nl;
  if (!out.defined()) out = torch::empty_like(ridx);
  wh::gbdt_scatter(ptr<int32_t>(ridx), n, ptr<int32_t>(pos_node), node_feat,
                   ptr<int32_t>(seg_beg), ptr<int32_t>(*nleft), ptr<int32_t>(left),
                   ptr<int64_t>(lscan), ptr<int32_t>(out), s);
  return out;
}

// partition the positions of the split nodes; returns the new ridx
Tensor gbdt_partition(const Tensor& B, const Tensor& ridx, const Tensor& pos_node,
                      const Tensor& node_feat, const Tensor& node_bin, const Tensor& node_defl,
                      const Tensor& seg_beg, const Tensor& seg_end, Tensor nleft_out,
                      const c10::optional<Tensor>& Bc) {
  CHECK_IN(B, torch::kUInt8);
  const uint8_t* bc = nullptr;
  if (Bc.has_value() && Bc->defined()) {
    CHECK_IN((*Bc), torch::kUInt8);
    TORCH_CHECK(Bc->dim() == 2 && Bc->size(0) == B.size(1) && Bc->size(1) == B.size(0),
                "Bc must be B transposed ([f, nrows])");
    bc = ptr<uint8_t>(*Bc);
  }
  CHECK_IN(ridx, torch::kInt32);
  CHECK_IN(pos_node, torch::kInt32);
  c10::DeviceGuard g(B.device());
  auto s = cur_stream(B);
  const int64_t n = ridx.numel();
  auto left = torch::empty({n}, ridx.options());
  wh::gbdt_goleft(ptr<uint8_t>(B), bc, B.size(0), (int)B.size(1), ptr<int32_t>(ridx), n,
                  ptr<int32_t>(pos_node), ptr<int32_t>(node_feat), ptr<int32_t>(node_bin),
                  ptr<uint8_t>(node_defl), ptr<int32_t>(left), s);
  return partition_by_flags(ridx, pos_node, left, ptr<int32_t>(node_feat), seg_beg, seg_end,
                            &nleft_out, Tensor(), s);
}

void gbdt_leaf_add(const Tensor& ridx, const Tensor& pos_node, const Tensor& leaf,
                   const Tensor& margin) {
  CHECK_IN(ridx, torch::kInt32);
  CHECK_IN(leaf, torch::kFloat32);
  CHECK_IN(margin, torch::kFloat32);
  c10::DeviceGuard g(ridx.device());
  wh::gbdt_leaf_add(ptr<int32_t>(ridx), ridx.numel(), ptr<int32_t>(pos_node), ptr<float>(leaf),
                    ptr<float>(margin), cur_stream(ridx));
}

// tree arrays: int32 feat / bin / left / right, uint8 defl, float val [nodes]
// (gpair f32 [n, 2], stats f64 [4] = {sum g, sum h, max|g|, max|h|})
std::vector<Tensor> gbdt_gpair(const Tensor& margin, const Tensor& label,
                               const c10::optional<Tensor>& weight, bool logistic) {
  CHECK_IN(margin, torch::kFloat32);
  CHECK_IN(label, torch::kFloat32);
  const int64_t n = margin.numel();
  TORCH_CHECK(label.numel() == n, "gbdt_gpair: label size mismatch");
  const float* wp = nullptr;
  if (weight.has_value() && weight->defined()) {
    CHECK_IN((*weight), torch::kFloat32);
    TORCH_CHECK(weight->numel() == n, "gbdt_gpair: weight size mismatch");
    wp = ptr<float>(*weight);
  }
  c10::DeviceGuard g(margin.device());
  static std::vector<Tensor> scratch(64);  // per device, the ticket tail stays zeroed
  const int dev = margin.device().index();
  if (!scratch[dev].defined())
    scratch[dev] = torch::zeros({wh::gbdt_gpair_scratch()}, margin.options().dtype(torch::kFloat64));
  auto gp = torch::empty({n, 2}, margin.options());
  auto st = n > 0 ? torch::empty({4}, margin.options().dtype(torch::kFloat64))  // k_gpair writes all 4
                  : torch::zeros({4}, margin.options().dtype(torch::kFloat64));
  if (n > 0)
    wh::gbdt_gpair(n, ptr<float>(margin), ptr<float>(label), wp, logistic, ptr<float>(gp),
                   ptr<double>(scratch[dev]), ptr<double>(st), cur_stream(margin));
  return {gp, st};
}

// ---- the objectives of host/gbdt_objective.h
namespace {
const float* obj_args(const char* op, const Tensor& margin, const Tensor& label,
                      const c10::optional<Tensor>& weight) {
  CHECK_IN(margin, torch::kFloat32);
  CHECK_IN(label, torch::kFloat32);
  TORCH_CHECK(label.numel() == margin.numel(), op, ": label size mismatch");
  if (!(weight.has_value() && weight->defined())) return nullptr;
  CHECK_IN((*weight), torch::kFloat32);
  TORCH_CHECK(weight->numel() == margin.numel(), op, ": weight size mismatch");
  return ptr<float>(*weight);
}

// per device and per op (slot), zeroed once: the ticket words stay zeroed
double* obj_scratch(const Tensor& like, int slot, int64_t need) {
  static std::vector<Tensor> scratch(2 * 64);
  Tensor& t = scratch[2 * like.device().index() + slot];
  if (!t.defined()) t = torch::zeros({need}, like.options().dtype(torch::kFloat64));
  return ptr<double>(t);
}
}  // namespace

// (gpair f32 [n, 2], stats f64 [4]) as gbdt_gpair; objective: a wh::GbdtObj id
std::vector<Tensor> gbdt_gpair_obj(const Tensor& margin, const Tensor& label,
                                   const c10::optional<Tensor>& weight, int64_t objective,
                                   double max_delta_step, double tweedie_variance_power,
                                   double huber_slope, double scale_pos_weight,
                                   double quantile_alpha) {
  const float* wp = obj_args("gbdt_gpair_obj", margin, label, weight);
  TORCH_CHECK(objective >= 0 && objective < wh::kObjCount && objective != 7,
              "gbdt_gpair_obj: unknown objective id ", objective);
  TORCH_CHECK(quantile_alpha > 0 && quantile_alpha < 1,
              "gbdt_gpair_obj: quantile_alpha in (0, 1)");
  TORCH_CHECK(max_delta_step >= 0 && huber_slope > 0 && scale_pos_weight > 0 &&
                  tweedie_variance_power > 1 && tweedie_variance_power < 2,
              "gbdt_gpair_obj: max_delta_step >= 0, tweedie_variance_power in (1, 2), "
              "huber_slope > 0 and scale_pos_weight > 0");
  const int64_t n = margin.numel();
  c10::DeviceGuard g(margin.device());
  auto gp = torch::empty({n, 2}, margin.options());
  auto st = n > 0 ? torch::empty({4}, margin.options().dtype(torch::kFloat64))  // all 4 written
                  : torch::zeros({4}, margin.options().dtype(torch::kFloat64));
  if (n > 0) {
    const auto a = wh::gbdt_obj_scalars(max_delta_step, tweedie_variance_power, huber_slope,
                                        scale_pos_weight, quantile_alpha);
    const bool ok = wh::gbdt_gpair_obj(
        (int)objective, n, ptr<float>(margin), ptr<float>(label), wp, a, ptr<float>(gp),
        obj_scratch(margin, 0, wh::gbdt_gpair_scratch()), ptr<double>(st), cur_stream(margin));
    TORCH_CHECK(ok, "gbdt_gpair_obj: no kernel for objective id ", objective);
  }
  return {gp, st};
}

// f64 [8] = {sum w loss_j for the wh::GbdtMetric ids j of mask (else 0), sum w}
Tensor gbdt_obj_eval(const Tensor& margin, const Tensor& label,
                     const c10::optional<Tensor>& weight, int64_t link, int64_t mask,
                     double tweedie_variance_power, double huber_slope) {
  const float* wp = obj_args("gbdt_obj_eval", margin, label, weight);
  TORCH_CHECK(link >= 0 && link <= wh::kLinkStep, "gbdt_obj_eval: unknown link ", link);
  TORCH_CHECK(mask >= 0 && mask < (1 << wh::kMetCount), "gbdt_obj_eval: unknown metric bits");
  const int64_t n = margin.numel();
  c10::DeviceGuard g(margin.device());
  auto out = torch::zeros({wh::gbdt_obj_eval_out()}, margin.options().dtype(torch::kFloat64));
  if (n > 0)
    wh::gbdt_obj_eval(n, ptr<float>(margin), ptr<float>(label), wp, (int)link, (int)mask,
                      tweedie_variance_power, huber_slope,
                      obj_scratch(margin, 1, wh::gbdt_obj_eval_scratch()), ptr<double>(out),
                      cur_stream(margin));
  return out;
}

// ---- survival:cox. The plan of a matrix' labels (y > 0: an event at y, else
// censored at |y|) and weights, on the labels' device (CPU tensors too: the
// torch path shares it): the stable ascending order of t = |y| (int32), t,
// delta (uint8) and the weights (or an empty tensor) in that order, the tie
// runs (wh::gbdt_cox_runs, on the host: once per matrix) and the kernels'
// zeroed workspace and ticket words.
py::dict gbdt_cox_plan(const Tensor& label, const c10::optional<Tensor>& weight) {
  CHECK_CONT(label);
  CHECK_DT(label, torch::kFloat32);
  const int64_t n = label.numel();
  TORCH_CHECK(label.dim() == 1 && n < (int64_t)1 << 31, "gbdt_cox_plan: label must be [n], n < 2^31");
  TORCH_CHECK(n == 0 || label.isfinite().all().item<bool>(),
              "gbdt_cox_plan: label must be finite");
  const bool weighted = weight.has_value() && weight->defined();
  if (weighted)
    TORCH_CHECK(weight->numel() == n && weight->scalar_type() == torch::kFloat32 &&
                    weight->device() == label.device(),
                "gbdt_cox_plan: weight must be float32 [n] on the labels' device");
  c10::DeviceGuard g(label.device());
  auto sorted = torch::sort(label.abs(), /*stable=*/true, /*dim=*/0, /*descending=*/false);
  const Tensor ts = std::get<0>(sorted).contiguous(), order = std::get<1>(sorted);
  const Tensor delta = (label > 0).to(torch::kUInt8).index_select(0, order).contiguous();
  const auto i32 = torch::TensorOptions().dtype(torch::kInt32);
  Tensor head = torch::empty({n}, i32), tail = torch::empty({n}, i32), ev = torch::empty({n}, i32);
  const Tensor ts_h = ts.cpu(), delta_h = delta.cpu();
  const int64_t events =
      wh::gbdt_cox_runs(ts_h.data_ptr<float>(), delta_h.data_ptr<uint8_t>(), n,
                        head.data_ptr<int32_t>(), tail.data_ptr<int32_t>(), ev.data_ptr<int32_t>());
  py::dict p;
  p["n"] = n;
  p["events"] = events;
  p["order"] = order.to(torch::kInt32).contiguous();
  p["t"] = ts;
  p["delta"] = delta;
  p["weight"] = weighted ? weight->index_select(0, order).contiguous()
                         : torch::empty({0}, label.options());
  p["head"] = head.to(label.device());
  p["tail"] = tail.to(label.device());
  p["run_events"] = ev.to(label.device());
  p["ws"] = torch::zeros({wh::gbdt_cox_ws(n).size}, label.options().dtype(torch::kFloat64));
  p["ticket"] = torch::zeros({label.is_cuda() ? wh::gbdt_cox_ticket_words() : 0},
                             label.options().dtype(torch::kInt32));
  return p;
}

namespace {
struct CoxArgs {
  int64_t n;
  const float* weight = nullptr;
};
CoxArgs cox_args(const char* op, const Tensor& margin, const Tensor& order, const Tensor& delta,
                 const c10::optional<Tensor>& weight, const Tensor& run_events, const Tensor& ws,
                 const Tensor& ticket) {
  CHECK_IN(margin, torch::kFloat32);
  CHECK_IN(order, torch::kInt32);
  CHECK_IN(delta, torch::kUInt8);
  CHECK_IN(run_events, torch::kInt32);
  CHECK_IN(ws, torch::kFloat64);
  CHECK_IN(ticket, torch::kInt32);
  CoxArgs a;
  a.n = margin.numel();
  TORCH_CHECK(a.n < (int64_t)1 << 31 && order.numel() == a.n && delta.numel() == a.n &&
                  run_events.numel() == a.n && ws.numel() == wh::gbdt_cox_ws(a.n).size &&
                  ticket.numel() == wh::gbdt_cox_ticket_words(),
              op, ": the plan does not fit the ", a.n, " margins");
  if (weight.has_value() && weight->defined() && weight->numel() > 0) {
    CHECK_IN((*weight), torch::kFloat32);
    TORCH_CHECK(weight->numel() == a.n, op, ": weight size mismatch");
    a.weight = ptr<float>(*weight);
  }
  return a;
}
}  // namespace

// (gpair f32 [n, 2] in row order, stats f64 [4]) as gbdt_gpair; the other
// arguments are a gbdt_cox_plan's.
std::vector<Tensor> gbdt_gpair_cox(const Tensor& margin, const Tensor& order, const Tensor& delta,
                                   const c10::optional<Tensor>& weight, const Tensor& run_events,
                                   const Tensor& ws, const Tensor& ticket) {
  const CoxArgs a = cox_args("gbdt_gpair_cox", margin, order, delta, weight, run_events, ws, ticket);
  c10::DeviceGuard g(margin.device());
  auto gp = torch::empty({a.n, 2}, margin.options());
  auto st = torch::zeros({4}, margin.options().dtype(torch::kFloat64));
  wh::gbdt_gpair_cox(a.n, ptr<float>(margin), ptr<int32_t>(order), ptr<uint8_t>(delta), a.weight,
                     ptr<int32_t>(run_events), ptr<double>(ws), ptr<unsigned int>(ticket),
                     ptr<float>(gp), ptr<double>(st), cur_stream(margin));
  return {gp, st};
}

// For benchmarks/bench_gbdt_survival.py only: the first `stages` (1..3) of the
// launches the pair and the metric share (m*, e, S), into the plan's
// workspace; returns nothing.
void gbdt_cox_scan_stages(const Tensor& margin, const Tensor& order, const Tensor& delta,
                          const Tensor& run_events, const Tensor& ws, const Tensor& ticket,
                          int64_t stages) {
  const CoxArgs a =
      cox_args("gbdt_cox_scan_stages", margin, order, delta, c10::nullopt, run_events, ws, ticket);
  TORCH_CHECK(stages >= 1 && stages <= 3, "gbdt_cox_scan_stages: stages in [1, 3]");
  c10::DeviceGuard g(margin.device());
  wh::gbdt_cox_scan(a.n, ptr<float>(margin), ptr<int32_t>(order), ptr<int32_t>(run_events),
                    ptr<double>(ws), ptr<unsigned int>(ticket), (int)stages, cur_stream(margin));
}

// f64 [2] = {sum over the events of ln D(t_i) - (m_i - m*), the events}
Tensor gbdt_cox_eval(const Tensor& margin, const Tensor& order, const Tensor& delta,
                     const Tensor& run_events, const Tensor& ws, const Tensor& ticket) {
  const CoxArgs a =
      cox_args("gbdt_cox_eval", margin, order, delta, c10::nullopt, run_events, ws, ticket);
  c10::DeviceGuard g(margin.device());
  auto out = torch::zeros({2}, margin.options().dtype(torch::kFloat64));
  wh::gbdt_cox_eval(a.n, ptr<float>(margin), ptr<int32_t>(order), ptr<uint8_t>(delta),
                    ptr<int32_t>(run_events), ptr<double>(ws), ptr<unsigned int>(ticket),
                    ptr<double>(out), cur_stream(margin));
  return out;
}

// ---- survival:aft (host/gbdt_aft.h): the rows' intervals [lower, upper]
namespace {
const float* aft_args(const char* op, const Tensor& margin, const Tensor& lower,
                      const Tensor& upper, const c10::optional<Tensor>& weight, int64_t dist,
                      double sigma) {
  CHECK_IN(lower, torch::kFloat32);
  CHECK_IN(upper, torch::kFloat32);
  TORCH_CHECK(upper.numel() == lower.numel(), op, ": bound size mismatch");
  TORCH_CHECK(dist >= 0 && dist < wh::kAftDistCount, op, ": unknown distribution id ", dist);
  TORCH_CHECK(sigma > 0, op, ": aft_loss_distribution_scale > 0");
  return obj_args(op, margin, lower, weight);
}

double* aft_scratch(const Tensor& like, int slot) {
  static std::vector<Tensor> scratch(2 * 64);
  Tensor& t = scratch[2 * like.device().index() + slot];
  if (!t.defined())
    t = torch::zeros({wh::gbdt_aft_scratch()}, like.options().dtype(torch::kFloat64));
  return ptr<double>(t);
}
}  // namespace

// (gpair f32 [n, 2], stats f64 [4]) as gbdt_gpair; dist: a wh::GbdtAftDist id
std::vector<Tensor> gbdt_gpair_aft(const Tensor& margin, const Tensor& lower, const Tensor& upper,
                                   const c10::optional<Tensor>& weight, int64_t dist,
                                   double sigma) {
  const float* wp = aft_args("gbdt_gpair_aft", margin, lower, upper, weight, dist, sigma);
  const int64_t n = margin.numel();
  c10::DeviceGuard g(margin.device());
  auto gp = torch::empty({n, 2}, margin.options());
  auto st = torch::zeros({4}, margin.options().dtype(torch::kFloat64));
  const bool ok = wh::gbdt_gpair_aft((int)dist, n, ptr<float>(margin), ptr<float>(lower),
                                     ptr<float>(upper), wp, (float)sigma, ptr<float>(gp),
                                     aft_scratch(margin, 0), ptr<double>(st), cur_stream(margin));
  TORCH_CHECK(ok, "gbdt_gpair_aft: no kernel for distribution id ", dist);
  return {gp, st};
}

// f64 [4] = {sum w nll, sum w, rows with lower <= exp(m) <= upper, rows}
Tensor gbdt_aft_eval(const Tensor& margin, const Tensor& lower, const Tensor& upper,
                     const c10::optional<Tensor>& weight, int64_t dist, double sigma) {
  const float* wp = aft_args("gbdt_aft_eval", margin, lower, upper, weight, dist, sigma);
  c10::DeviceGuard g(margin.device());
  auto out = torch::zeros({4}, margin.options().dtype(torch::kFloat64));
  wh::gbdt_aft_eval((int)dist, margin.numel(), ptr<float>(margin), ptr<float>(lower),
                    ptr<float>(upper), wp, sigma, aft_scratch(margin, 1), ptr<double>(out),
                    cur_stream(margin));
  return out;
}

// ---- the `quantile` metric: margin f32 [K, n] (or [n]: K = 1), alphas f64 [K]
// on the margins' device -> f64 [2] = {sum w sum_k pinball_k, sum w}
Tensor gbdt_quantile_eval(const Tensor& margin, const Tensor& label,
                          const c10::optional<Tensor>& weight, const Tensor& alphas) {
  CHECK_IN(margin, torch::kFloat32);
  CHECK_IN(label, torch::kFloat32);
  CHECK_IN(alphas, torch::kFloat64);
  const int64_t n = label.numel(), K = alphas.numel();
  TORCH_CHECK(K >= 1 && K <= 64 && margin.numel() == K * n,
              "gbdt_quantile_eval: margin must be [K, n] for 1 <= K <= 64 alphas");
  const float* wp = nullptr;
  if (weight.has_value() && weight->defined()) {
    CHECK_IN((*weight), torch::kFloat32);
    TORCH_CHECK(weight->numel() == n, "gbdt_quantile_eval: weight size mismatch");
    wp = ptr<float>(*weight);
  }
  c10::DeviceGuard g(margin.device());
  auto out = torch::zeros({2}, margin.options().dtype(torch::kFloat64));
  if (n > 0) {
    auto scratch = torch::empty({wh::gbdt_quantile_eval_scratch()}, out.options());
    wh::gbdt_quantile_eval(n, (int)K, ptr<float>(margin), ptr<float>(label), wp,
                           ptr<double>(alphas), ptr<double>(scratch), ptr<double>(out),
                           cur_stream(margin));
  }
  return out;
}

// ---- the adaptive objectives' leaf refresh: the radix select of
// host/gbdt_quantile_plan.h, pass by pass (models/gbdt_quantile.py drives it
// and adds the ranks' histograms between hist and pick)
// (key i32 [npos] holding the uint32 keys, u i64 [npos]) of the ridx positions
std::vector<Tensor> gbdt_qsel_key(const Tensor& ridx, const Tensor& label, const Tensor& at,
                                  const c10::optional<Tensor>& weight,
                                  const c10::optional<Tensor>& keep,
                                  const c10::optional<Tensor>& scale) {
  CHECK_IN(ridx, torch::kInt32);
  CHECK_IN(label, torch::kFloat32);
  CHECK_IN(at, torch::kFloat32);
  const int64_t npos = ridx.numel(), nrow = label.numel();
  TORCH_CHECK(at.numel() == nrow, "gbdt_qsel_key: label and margin sizes differ");
  const float* wp = nullptr;
  const uint8_t* kp = nullptr;
  const double* sp = nullptr;
  if (weight.has_value() && weight->defined()) {
    CHECK_IN((*weight), torch::kFloat32);
    TORCH_CHECK(weight->numel() == nrow, "gbdt_qsel_key: weight size mismatch");
    wp = ptr<float>(*weight);
  }
  if (keep.has_value() && keep->defined()) {
    TORCH_CHECK(keep->is_cuda() && keep->is_contiguous() && keep->numel() == nrow &&
                    (keep->scalar_type() == torch::kUInt8 || keep->scalar_type() == torch::kBool),
                "gbdt_qsel_key: keep must be a contiguous bool / uint8 [n] on the device");
    kp = ptr<uint8_t>(*keep);
  }
  if (scale.has_value() && scale->defined()) {
    CHECK_IN((*scale), torch::kFloat64);
    TORCH_CHECK(scale->numel() == 1, "gbdt_qsel_key: scale is one double");
    sp = ptr<double>(*scale);
  }
  c10::DeviceGuard g(ridx.device());
  auto key = torch::empty({npos}, ridx.options());
  auto u = torch::empty({npos}, ridx.options().dtype(torch::kInt64));
  wh::gbdt_qsel_key(ptr<int32_t>(ridx), npos, nrow, ptr<float>(label), ptr<float>(at), wp, kp, sp,
                    ptr<uint32_t>(key), ptr<int64_t>(u), cur_stream(ridx));
  return {key, u};
}

// hist i64 [L, 256]: this rank's bins of pass `radix_pass` for the L segments
// [seg_beg[l], seg_end[l]) of the key positions, each cut into tasks of
// `chunk` positions (qsel_plan; the task lists go down in one pinned copy);
// zero for an empty segment
Tensor gbdt_qsel_hist(const Tensor& key, const Tensor& u, const std::vector<int64_t>& seg_beg,
                      const std::vector<int64_t>& seg_end, int64_t chunk, const Tensor& state,
                      int64_t radix_pass) {
  CHECK_IN(key, torch::kInt32);
  CHECK_IN(u, torch::kInt64);
  CHECK_IN(state, torch::kInt64);
  TORCH_CHECK(u.numel() == key.numel(), "gbdt_qsel_hist: key and u sizes differ");
  TORCH_CHECK(state.dim() == 2 && state.size(1) == wh::kQselState && state.size(0) <= INT32_MAX &&
                  state.size(0) == (int64_t)seg_beg.size(),
              "gbdt_qsel_hist: state must be [L, 2] for L segments");
  TORCH_CHECK(radix_pass >= 0 && radix_pass < wh::kQselPasses, "gbdt_qsel_hist: pass in [0, 4)");
  std::vector<int32_t> plan, red;
  TORCH_CHECK(wh::qsel_plan(seg_beg, seg_end, key.numel(), chunk, &plan, &red),
              "gbdt_qsel_hist: segments must lie within the keys with begin <= end, chunk >= 1");
  c10::DeviceGuard g(key.device());
  const int64_t L = state.size(0), T = (int64_t)plan.size() / 3, R = (int64_t)red.size() / 3;
  auto hist = torch::zeros({L, wh::kQselBins}, u.options());
  if (T > 0 && L > 0) {
    plan.insert(plan.end(), red.begin(), red.end());
    auto host = torch::empty({(int64_t)plan.size()},
                             torch::TensorOptions().dtype(torch::kInt32).pinned_memory(true));
    std::memcpy(host.data_ptr(), plan.data(), plan.size() * 4);
    auto dev = host.to(key.device(), /*non_blocking=*/true);
    auto part = torch::empty({T, wh::kQselBins}, u.options());
    wh::gbdt_qsel_hist(ptr<uint32_t>(key), ptr<int64_t>(u), key.numel(), ptr<int32_t>(dev), T,
                       ptr<int32_t>(dev) + 3 * T, R, (int)L, ptr<int64_t>(state), (int)radix_pass,
                       ptr<int64_t>(part), ptr<int64_t>(hist), cur_stream(key));
  }
  return hist;
}

void gbdt_qsel_pick(const Tensor& hist, const Tensor& state, int64_t pass, double alpha) {
  CHECK_IN(hist, torch::kInt64);
  CHECK_IN(state, torch::kInt64);
  TORCH_CHECK(state.dim() == 2 && state.size(1) == wh::kQselState && state.size(0) <= INT32_MAX &&
                  hist.dim() == 2 && hist.size(0) == state.size(0) &&
                  hist.size(1) == wh::kQselBins,
              "gbdt_qsel_pick: hist [L, 256] and state [L, 2]");
  TORCH_CHECK(pass >= 0 && pass < wh::kQselPasses, "gbdt_qsel_pick: pass in [0, 4)");
  TORCH_CHECK(alpha > 0 && alpha < 1, "gbdt_qsel_pick: alpha in (0, 1)");
  c10::DeviceGuard g(hist.device());
  wh::gbdt_qsel_pick(ptr<int64_t>(hist), (int)state.size(0), (int)pass, alpha,
                     ptr<int64_t>(state), cur_stream(hist));
}

// f32 [2, L]: the selected residuals, then 1 where the leaf has no weight
Tensor gbdt_qsel_value(const Tensor& state) {
  CHECK_IN(state, torch::kInt64);
  TORCH_CHECK(state.dim() == 2 && state.size(1) == wh::kQselState && state.size(0) <= INT32_MAX,
              "gbdt_qsel_value: state must be [L, 2]");
  c10::DeviceGuard g(state.device());
  auto out = torch::zeros({2, state.size(0)}, state.options().dtype(torch::kFloat32));
  wh::gbdt_qsel_value(ptr<int64_t>(state), (int)state.size(0), ptr<float>(out), cur_stream(state));
  return out;
}

// ---- multi-class softmax: margin f32 [K, n] class-major, label f32 [n]
namespace {
// per device, grown with K; the ticket words at its head stay zeroed
double* softmax_scratch(const Tensor& like, int64_t K) {
  static std::vector<Tensor> scratch(64);
  Tensor& t = scratch[like.device().index()];
  const int64_t need = wh::gbdt_softmax_scratch((int)K);
  if (!t.defined() || t.numel() < need)
    t = torch::zeros({need}, like.options().dtype(torch::kFloat64));
  return ptr<double>(t);
}

const float* softmax_args(const char* op, const Tensor& margin, const Tensor* label,
                          const c10::optional<Tensor>& weight, int64_t* K, int64_t* n) {
  CHECK_IN(margin, torch::kFloat32);
  TORCH_CHECK(margin.dim() == 2 && margin.size(0) >= 1 && margin.size(0) < (1 << 23), op,
              ": margin must be [num_class, n]");
  *K = margin.size(0);
  *n = margin.size(1);
  if (label) {
    CHECK_IN((*label), torch::kFloat32);
    TORCH_CHECK(label->numel() == *n, op, ": label size mismatch");
  }
  if (weight.has_value() && weight->defined()) {
    CHECK_IN((*weight), torch::kFloat32);
    TORCH_CHECK(weight->numel() == *n, op, ": weight size mismatch");
    return ptr<float>(*weight);
  }
  return nullptr;
}
}  // namespace

// (gpair f32 [K, n, 2], stats f64 [K, 4] = per class {sum g, sum h, max|g|, max|h|})
std::vector<Tensor> gbdt_gpair_softmax(const Tensor& margin, const Tensor& label,
                                       const c10::optional<Tensor>& weight) {
  int64_t K, n;
  const float* wp = softmax_args("gbdt_gpair_softmax", margin, &label, weight, &K, &n);
  c10::DeviceGuard g(margin.device());
  auto gp = torch::empty({K, n, 2}, margin.options());
  auto st = torch::zeros({K, 4}, margin.options().dtype(torch::kFloat64));
  if (n > 0)
    wh::gbdt_gpair_softmax(n, (int)K, ptr<float>(margin), ptr<float>(label), wp, ptr<float>(gp),
                           softmax_scratch(margin, K), ptr<double>(st), cur_stream(margin));
  return {gp, st};
}

// prob: probabilities f32 [n, K]; else arg-max class ids f32 [n]
Tensor gbdt_softmax_out(const Tensor& margin, bool prob) {
  int64_t K, n;
  softmax_args("gbdt_softmax_out", margin, nullptr, c10::nullopt, &K, &n);
  c10::DeviceGuard g(margin.device());
  auto out = prob ? torch::empty({n, K}, margin.options()) : torch::empty({n}, margin.options());
  wh::gbdt_softmax_out(n, (int)K, ptr<float>(margin), prob, ptr<float>(out), cur_stream(margin));
  return out;
}

// f64 [3] = {sum w [arg-max != y], sum w (-log max(p_y, 1e-16)), sum w}
Tensor gbdt_multi_eval(const Tensor& margin, const Tensor& label,
                       const c10::optional<Tensor>& weight) {
  int64_t K, n;
  const float* wp = softmax_args("gbdt_multi_eval", margin, &label, weight, &K, &n);
  c10::DeviceGuard g(margin.device());
  auto out = torch::zeros({3}, margin.options().dtype(torch::kFloat64));
  if (n > 0)
    wh::gbdt_multi_eval(n, (int)K, ptr<float>(margin), ptr<float>(label), wp,
                        softmax_scratch(margin, 1), ptr<double>(out), cur_stream(margin));
  return out;
}

// {2^eg, 2^eh[, R]} (f32) from m = {max|g|, max|h|} (f32 [2], on the device)
Tensor gbdt_qscale(const Tensor& m, double nglobal, int64_t R) {
  CHECK_IN(m, torch::kFloat32);
  TORCH_CHECK(m.numel() == 2 && nglobal >= 1 && R >= 0, "gbdt_qscale: bad arguments");
  c10::DeviceGuard g(m.device());
  auto out = torch::empty({R > 0 ? 3 : 2}, m.options());
  wh::gbdt_qscale(ptr<float>(m), nglobal, (int)R, ptr<float>(out), cur_stream(m));
  return out;
}

void gbdt_leaf_walk(const Tensor& B, const Tensor& feat, const Tensor& bin, const Tensor& defl,
                    const Tensor& left, const Tensor& right, const Tensor& val,
                    const Tensor& margin, bool lds) {
  CHECK_IN(B, torch::kUInt8);
  CHECK_IN(feat, torch::kInt32);
  CHECK_IN(bin, torch::kInt32);
  CHECK_IN(defl, torch::kUInt8);
  CHECK_IN(left, torch::kInt32);
  CHECK_IN(right, torch::kInt32);
  CHECK_IN(val, torch::kFloat32);
  CHECK_IN(margin, torch::kFloat32);
  TORCH_CHECK(B.dim() == 2 && margin.numel() == B.size(0), "leaf_walk: B must be [n, f]");
  const int64_t nn = feat.numel();
  TORCH_CHECK(bin.numel() == nn && defl.numel() == nn && left.numel() == nn &&
                  right.numel() == nn && val.numel() == nn && nn > 0,
              "leaf_walk: tree array sizes differ");
  c10::DeviceGuard g(B.device());
  TORCH_CHECK(nn <= INT32_MAX, "leaf_walk: too many nodes");
  wh::gbdt_leaf_walk(ptr<uint8_t>(B), B.size(0), (int)B.size(1), (int)nn, ptr<int32_t>(feat),
                     ptr<int32_t>(bin), ptr<uint8_t>(defl), ptr<int32_t>(left),
                     ptr<int32_t>(right), ptr<float>(val), ptr<float>(margin), cur_stream(B), lds);
}

void gbdt_predict(const Tensor& X, const Tensor& feat, const Tensor& thr, const Tensor& left,
                  const Tensor& right, const Tensor& defl, const Tensor& leaf, const Tensor& margin) {
  CHECK_IN(X, torch::kFloat32);
  CHECK_IN(margin, torch::kFloat32);
  c10::DeviceGuard g(X.device());
  wh::gbdt_predict(ptr<float>(X), X.size(0), (int)X.size(1), ptr<int32_t>(feat), ptr<float>(thr),
                   ptr<int32_t>(left), ptr<int32_t>(right), ptr<uint8_t>(defl), ptr<float>(leaf),
                   ptr<float>(margin), cur_stream(X));
}

// ------------------------------------------------------------- gbdt (CSR)
Tensor gbdt_bin_csr(const Tensor& fid, const c10::optional<Tensor>& val, int64_t ncol,
                    const Tensor& cuts, const Tensor& cut_off) {
  CHECK_IN(fid, torch::kInt32);
  CHECK_IN(cuts, torch::kFloat32);
  CHECK_IN(cut_off, torch::kInt32);
  TORCH_CHECK(cut_off.numel() == ncol + 1, "cut_off must be [ncol + 1]");
  c10::DeviceGuard g(fid.device());
  auto gbin = torch::empty_like(fid);
  wh::gbdt_bin_csr(ptr<int32_t>(fid), optptr<float>(val), fid.numel(), (int)ncol, ptr<float>(cuts),
                   ptr<int32_t>(cut_off), ptr<int32_t>(gbin), cur_stream(fid));
  return gbin;
}

// tasks [T, 3] {slot, rbeg, rend} (device int32) -> hist double [nslot, tb, 2]
Tensor gbdt_hist_csr(const Tensor& row_off, const Tensor& gbin, const Tensor& ridx,
                     const Tensor& gpair, const Tensor& qscale, const Tensor& tasks,
                     int64_t max_rows, int64_t tb, int64_t nslot) {
  CHECK_IN(row_off, torch::kInt64);
  CHECK_IN(gbin, torch::kInt32);
  CHECK_IN(ridx, torch::kInt32);
  CHECK_IN(gpair, torch::kFloat32);
  CHECK_IN(qscale, torch::kFloat32);
  CHECK_IN(tasks, torch::kInt32);
  c10::DeviceGuard g(gbin.device());
  auto hist = torch::empty({nslot, tb, 2}, gpair.options().dtype(torch::kFloat64));
  auto hq = torch::empty({std::max<int64_t>(nslot * tb * 2, 1)}, gpair.options().dtype(torch::kInt64));
  wh::gbdt_hist_csr(ptr<int64_t>(row_off), ptr<int32_t>(gbin), ptr<int32_t>(ridx),
                    ptr<float>(gpair), ptr<float>(qscale), ptr<int32_t>(tasks),
                    (int)(tasks.numel() / 3), (int)max_rows, tb, (int)nslot, ptr<int64_t>(hq),
                    ptr<double>(hist), cur_stream(gbin));
  return hist;
}

Tensor gbdt_split_csr(const Tensor& hist, const Tensor& totals, const Tensor& cut_off,
                      const c10::optional<Tensor>& fvalid, double alpha, double lambda, double mcw,
                      const c10::optional<Tensor>& mono, const c10::optional<Tensor>& bounds,
                      const c10::optional<Tensor>& fmask, const c10::optional<Tensor>& state) {
  CHECK_IN(hist, torch::kFloat64);
  CHECK_IN(totals, torch::kFloat64);
  CHECK_IN(cut_off, torch::kInt32);
  c10::DeviceGuard g(hist.device());
  const int S = (int)hist.size(0);
  const int F = (int)cut_off.numel() - 1;
  auto out = torch::empty({S, 6}, hist.options());
  auto cand = torch::empty({std::max<int64_t>((int64_t)S * F * 5, 1)}, hist.options());
  wh::gbdt_split_csr(ptr<double>(hist), hist.size(1), ptr<double>(totals), ptr<int32_t>(cut_off),
                     optptr<uint8_t>(fvalid), S, F, alpha, lambda, mcw, ptr<double>(cand),
                     ptr<double>(out), cur_stream(hist),
                     split_cons(mono, bounds, fmask, state, hist, S, F, "gbdt_split_csr"));
  return out;
}

Tensor gbdt_partition_csr(const Tensor& row_off, const Tensor& fid, const Tensor& gbin,
                          const Tensor& cut_off, const Tensor& ridx, const Tensor& pos_node,
                          const Tensor& node_feat, const Tensor& node_bin, const Tensor& node_defl,
                          const Tensor& seg_beg, const Tensor& seg_end, Tensor nleft_out) {
  CHECK_IN(row_off, torch::kInt64);
  CHECK_IN(fid, torch::kInt32);
  CHECK_IN(gbin, torch::kInt32);
  CHECK_IN(ridx, torch::kInt32);
  CHECK_IN(pos_node, torch::kInt32);
  c10::DeviceGuard g(ridx.device());
  auto s = cur_stream(ridx);
  const int64_t n = ridx.numel();
  auto left = torch::empty({n}, ridx.options());
  wh::gbdt_goleft_csr(ptr<int64_t>(row_off), ptr<int32_t>(fid), ptr<int32_t>(gbin),
                      ptr<int32_t>(cut_off), ptr<int32_t>(ridx), n, ptr<int32_t>(pos_node),
                      ptr<int32_t>(node_feat), ptr<int32_t>(node_bin), ptr<uint8_t>(node_defl),
                      ptr<int32_t>(left), s);
  return partition_by_flags(ridx, pos_node, left, ptr<int32_t>(node_feat), seg_beg, seg_end,
                            &nleft_out, Tensor(), s);
}

void gbdt_predict_csr(const Tensor& row_off, const Tensor& fid, const c10::optional<Tensor>& val,
                      const Tensor& feat, const Tensor& thr, const Tensor& left,
                      const Tensor& right, const Tensor& defl, const Tensor& leaf,
                      const Tensor& margin) {
  CHECK_IN(row_off, torch::kInt64);
  CHECK_IN(fid, torch::kInt32);
  CHECK_IN(margin, torch::kFloat32);
  c10::DeviceGuard g(fid.device());
  wh::gbdt_predict_csr(ptr<int64_t>(row_off), ptr<int32_t>(fid), optptr<float>(val),
                       row_off.numel() - 1, ptr<int32_t>(feat), ptr<float>(thr),
                       ptr<int32_t>(left), ptr<int32_t>(right), ptr<uint8_t>(defl),
                       ptr<float>(leaf), ptr<float>(margin), cur_stream(fid));
}

// ------------------------------------------------------ forest prediction
// The packed forest of the trees' lists (host/gbdt_forest_plan.h): (nodes
// int32 [N, 4], tree_off int32 [T + 1], largest feature id or -1), on the
// host. A tree a walk could leave or spin in raises ValueError.
py::tuple gbdt_forest_pack(std::vector<std::vector<int64_t>> feat,
                           std::vector<std::vector<double>> cond,
                           std::vector<std::vector<int64_t>> left,
                           std::vector<std::vector<int64_t>> right,
                           std::vector<std::vector<int64_t>> defl,
                           std::vector<std::vector<double>> leaf) {
  wh::GbdtForestTrees tr{std::move(feat), std::move(left), std::move(right), std::move(defl),
                         std::move(cond), std::move(leaf)};
  std::vector<wh::GbdtForestNode> nodes;
  std::vector<int32_t> off;
  wh::gbdt_forest_pack(tr, &nodes, &off);  // (std::invalid_argument -> ValueError)
  int64_t max_feat = -1;
  for (auto& nd : nodes)
    if (nd.fd >= 0) max_feat = std::max<int64_t>(max_feat, nd.fd >> 1);
  auto tn = torch::empty({(int64_t)nodes.size(), 4}, torch::kInt32);
  if (!nodes.empty()) std::memcpy(tn.data_ptr(), nodes.data(), nodes.size() * sizeof(nodes[0]));
  auto to = torch::empty({(int64_t)off.size()}, torch::kInt32);
  std::memcpy(to.data_ptr(), off.data(), off.size() * 4);
  return py::make_tuple(tn, to, max_feat);
}

// (first_tree, ntree, node_begin, nnode, in_lds) per chunk
using ForestChunks = std::vector<std::tuple<int64_t, int64_t, int64_t, int64_t, bool>>;

ForestChunks gbdt_forest_plan(const std::vector<int64_t>& tree_sizes, int64_t lds_nodes) {
  TORCH_CHECK(lds_nodes >= 1, "gbdt_forest_plan: lds_nodes must be positive");
  for (int64_t sz : tree_sizes) TORCH_CHECK(sz >= 1, "gbdt_forest_plan: an empty tree");
  ForestChunks out;
  for (auto& c : wh::gbdt_forest_plan(tree_sizes, lds_nodes))
    out.emplace_back(c.first_tree, c.ntree, c.node_begin, c.nnode, c.in_lds);
  return out;
}

// The checks both forest predictions share, then one launch per chunk.
// out: float32 margins [n] or [K, n] (rows may be views into a larger
// buffer), or, leaf, int32 leaf ids [n, T].
template <class Launch>
void forest_run(const Tensor& nodes, const Tensor& tree_off, const ForestChunks& chunks,
                const Tensor& out, bool leaf, int64_t n, Launch launch) {
  CHECK_IN(nodes, torch::kInt32);
  CHECK_IN(tree_off, torch::kInt32);
  CHECK_DEV(out);
  TORCH_CHECK(nodes.dim() == 2 && nodes.size(1) == 4, "forest nodes must be int32 [N, 4]");
  const int64_t T = tree_off.numel() - 1;
  TORCH_CHECK(T >= 0 && T <= INT32_MAX, "forest tree_off must be [T + 1]");
  wh::ForestOut o{nullptr, 0, 1, nullptr, (int)T};
  if (leaf) {
    CHECK_CONT(out);
    CHECK_DT(out, torch::kInt32);
    TORCH_CHECK(out.dim() == 2 && out.size(0) == n && out.size(1) == T, "leaf ids must be [n, T]");
    o.leaf = ptr<int32_t>(out);
  } else {
    CHECK_DT(out, torch::kFloat32);
    TORCH_CHECK((out.dim() == 1 || out.dim() == 2) && out.size(-1) == n &&
                    (n <= 1 || out.stride(-1) == 1) && (out.dim() == 1 || out.size(0) >= 1),
                "margins must be [n] or [K, n] with unit stride along n");
    o.margin = ptr<float>(out);
    if (out.dim() == 2) o.K = (int)out.size(0), o.stride = out.stride(0);
  }
  if (n == 0 || T == 0) return;
  int64_t tree = 0, node = 0;
  for (auto& [first_tree, ntree, node_begin, nnode, in_lds] : chunks) {
    TORCH_CHECK(first_tree == tree && node_begin == node && ntree >= 1 && nnode >= ntree &&
                    (!in_lds || nnode <= wh::gbdt_forest_lds_nodes()),
                "forest chunks must be consecutive whole trees that fit the LDS");
    tree += ntree, node += nnode;
  }
  TORCH_CHECK(tree == T && node == nodes.size(0), "forest chunks must cover the forest");
  for (auto& [first_tree, ntree, node_begin, nnode, in_lds] : chunks)
    launch(wh::ForestChunk{nodes.data_ptr(), ptr<int32_t>(tree_off), (int)first_tree, (int)ntree,
                           (int)node_begin, (int)nnode, in_lds},
           o);
}

void gbdt_predict_forest(const Tensor& X, const Tensor& nodes, const Tensor& tree_off,
                         const ForestChunks& chunks, int64_t max_feat, const Tensor& out,
                         bool leaf) {
  CHECK_IN(X, torch::kFloat32);
  TORCH_CHECK(X.dim() == 2 && max_feat < X.size(1), "forest splits on a feature X does not have");
  c10::DeviceGuard g(X.device());
  auto s = cur_stream(X);
  forest_run(nodes, tree_off, chunks, out, leaf, X.size(0),
             [&](const wh::ForestChunk& c, const wh::ForestOut& o) {
               wh::gbdt_predict_forest(ptr<float>(X), X.size(0), (int)X.size(1), c, o, s);
             });
}

void gbdt_predict_forest_csr(const Tensor& row_off, const Tensor& fid,
                             const c10::optional<Tensor>& val, const Tensor& nodes,
                             const Tensor& tree_off, const ForestChunks& chunks, const Tensor& out,
                             bool leaf) {
  CHECK_IN(row_off, torch::kInt64);
  CHECK_IN(fid, torch::kInt32);
  TORCH_CHECK(row_off.numel() >= 1, "row_off must be [n + 1]");
  if (present(val)) {
    CHECK_IN((*val), torch::kFloat32);
    TORCH_CHECK(val->numel() == fid.numel(), "val and fid sizes differ");
  }
  c10::DeviceGuard g(row_off.device());
  auto s = cur_stream(row_off);
  const int64_t n = row_off.numel() - 1;
  forest_run(nodes, tree_off, chunks, out, leaf, n,
             [&](const wh::ForestChunk& c, const wh::ForestOut& o) {
               wh::gbdt_predict_forest_csr(ptr<int64_t>(row_off), ptr<int32_t>(fid),
                                           optptr<float>(val), n, c, o, s);
             });
}

// ------------------------------------------------------ DART dropout walk
// booster=dart (host/gbdt_dart_plan.h, gbdt_dart.hip). A tree's 8-byte nodes
// int32 [nn, 2] on the host, or None when the table does not admit it. bin:
// the split bins where known, else None (recovered from cond and the cuts).
py::object gbdt_dart_pack(std::vector<int64_t> feat, c10::optional<std::vector<int64_t>> bin,
                          std::vector<double> cond, std::vector<int64_t> left,
                          std::vector<int64_t> right, std::vector<int64_t> defl,
                          std::vector<double> leaf, const std::vector<double>& cut_vals,
                          const std::vector<int64_t>& cut_off) {
  TORCH_CHECK(!cut_off.empty(), "gbdt_dart_pack: cut_off must be [F + 1]");
  wh::GbdtDartTree t{std::move(feat), bin ? std::move(*bin) : std::vector<int64_t>(),
                     std::move(left), std::move(right), std::move(defl), std::move(cond),
                     std::move(leaf)};
  std::vector<wh::GbdtDartNode> nodes;
  if (!wh::gbdt_dart_pack(t, cut_vals, cut_off, &nodes)) return py::none();
  auto tn = torch::empty({(int64_t)nodes.size(), 2}, torch::kInt32);
  std::memcpy(tn.data_ptr(), nodes.data(), nodes.size() * sizeof(nodes[0]));
  return py::cast(tn);
}

// (first, count, nnode, staged, stage_off) per chunk of the selection
using DartChunks = std::vector<std::tuple<int64_t, int64_t, int64_t, bool, std::vector<int64_t>>>;

DartChunks gbdt_dart_plan(const std::vector<int64_t>& tree_sizes, const std::vector<int64_t>& sel,
                          int64_t lds_nodes) {
  DartChunks out;  // (std::invalid_argument -> ValueError)
  for (auto& c : wh::gbdt_dart_plan(tree_sizes, sel, lds_nodes))
    out.emplace_back(c.first, c.count, c.nnode, c.staged, c.stage_off);
  return out;
}

// grow_policy=lossguide (host/gbdt_leaf_plan.h): the (leaves, depth) limits in
// effect, ValueError with the reason when the pair is refused
std::pair<int64_t, int64_t> gbdt_leaf_limits(int64_t max_leaves, int64_t max_depth) {
  const auto l = wh::gbdt_leaf_limits(max_leaves, max_depth);
  if (l.error) throw std::invalid_argument(l.error);
  return {l.leaves, l.depth};
}

// The open leaf to split next: its index in the three lists, or -1
int64_t gbdt_leaf_pick(const std::vector<int64_t>& node, const std::vector<int64_t>& depth,
                       const std::vector<double>& gain, double rt_eps, int64_t depth_cap) {
  TORCH_CHECK(node.size() == depth.size() && node.size() == gain.size(),
              "gbdt_leaf_pick: node, depth and gain must be of one length");
  std::vector<wh::GbdtOpenLeaf> open(node.size());
  for (size_t i = 0; i < node.size(); ++i) open[i] = {node[i], depth[i], gain[i]};
  return wh::gbdt_leaf_pick(open, rt_eps, depth_cap);
}

int64_t dart_rows(int64_t rows) {
  TORCH_CHECK(rows >= 64 && rows <= 1024 && rows % 64 == 0,
              "gbdt_dart: rows per tile must be a multiple of 64, at most 1024");
  return rows;
}

int64_t gbdt_dart_grid(int64_t n, int64_t f, int64_t ntree, int64_t nnode, int64_t rows) {
  return wh::gbdt_dart_grid(n, (int)f, (int)ntree, (int)nnode, (int)dart_rows(rows));
}

// One staged chunk: tree j is nodes [tree_off[j], tree_off[j] + tree_nn[j]) of
// `table` (int32 [N, 2], device), staged at stage_off[j], weighted coef[j];
// out float32 [n] (may be a view) is added to.
void gbdt_dart_walk(const Tensor& B, const Tensor& table, const std::vector<int64_t>& tree_off,
                    const std::vector<int64_t>& tree_nn, const std::vector<int64_t>& stage_off,
                    const std::vector<double>& coef, const Tensor& out, int64_t rows) {
  CHECK_IN(B, torch::kUInt8);
  CHECK_IN(table, torch::kInt32);
  CHECK_DEV(out);
  CHECK_DT(out, torch::kFloat32);
  dart_rows(rows);
  TORCH_CHECK(B.dim() == 2 && B.size(1) >= 1 && B.size(1) <= wh::kDartMaxF &&
                  reinterpret_cast<uintptr_t>(B.data_ptr()) % 4 == 0,
              "gbdt_dart_walk: B must be a 4-byte aligned [n, f] with f <= ", wh::kDartMaxF);
  const int64_t n = B.size(0), f = B.size(1);
  TORCH_CHECK(out.dim() == 1 && out.size(0) == n && (n <= 1 || out.stride(0) == 1) &&
                  out.device() == B.device() && table.device() == B.device(),
              "gbdt_dart_walk: out must be [n] with unit stride on B's device");
  TORCH_CHECK(table.dim() == 2 && table.size(1) == 2, "gbdt_dart_walk: table must be int32 [N, 2]");
  const int64_t T = (int64_t)tree_off.size();
  TORCH_CHECK((int64_t)tree_nn.size() == T && (int64_t)stage_off.size() == T &&
                  (int64_t)coef.size() == T && T <= wh::kDartMaxTrees,
              "gbdt_dart_walk: the chunk's lists differ or it has too many trees");
  if (n == 0 || T == 0) return;
  // the staging ranges tile [0, nnode) in list order, each tree inside the table
  int64_t nnode = 0;
  auto mh = torch::empty({T, 4}, torch::TensorOptions().dtype(torch::kInt32).pinned_memory(true));
  int32_t* m = mh.data_ptr<int32_t>();
  for (int64_t j = 0; j < T; ++j) {
    TORCH_CHECK(tree_nn[j] >= 1 && tree_nn[j] <= 65535 && tree_off[j] >= 0 &&
                    tree_off[j] + tree_nn[j] <= table.size(0) && stage_off[j] == nnode,
                "gbdt_dart_walk: tree ", j, " lies outside the table or its staging range");
    nnode += tree_nn[j];
    const float c = (float)coef[j];
    m[4 * j] = (int32_t)tree_off[j], m[4 * j + 1] = (int32_t)tree_nn[j];
    m[4 * j + 2] = (int32_t)stage_off[j];
    std::memcpy(&m[4 * j + 3], &c, 4);
  }
  TORCH_CHECK(nnode <= wh::kDartLdsNodesMax &&
                  wh::gbdt_dart_lds_bytes((int)f, (int)T, (int)nnode, (int)rows) <= 160 * 1024,
              "gbdt_dart_walk: the chunk does not fit the LDS");
  c10::DeviceGuard g(B.device());
  auto md = mh.to(B.device(), /*non_blocking=*/true);
  wh::gbdt_dart_walk(ptr<uint8_t>(B), n, (int)f, table.data_ptr(), md.data_ptr(), (int)T,
                     (int)nnode, (int)rows, ptr<float>(out), cur_stream(B));
}

// ------------------------------------------------- feature contributions
// pred_contribs / approx_contribs (host/gbdt_shap_plan.h, gbdt_shap.hip).
// Pack, plan and the host references need no GPU.
using TreeInts = std::vector<std::vector<int64_t>>;
using TreeReals = std::vector<std::vector<double>>;

Tensor int32_tensor(const std::vector<int32_t>& v, std::vector<int64_t> shape) {
  auto t = torch::empty(shape, torch::kInt32);
  TORCH_CHECK(t.numel() == (int64_t)v.size());
  if (!v.empty()) std::memcpy(t.data_ptr(), v.data(), v.size() * 4);
  return t;
}

// (path_begin, npath, elem_begin, nelem, class, width) per chunk
using ShapChunks = std::vector<std::tuple<int64_t, int64_t, int64_t, int64_t, int64_t, int64_t>>;

ShapChunks shap_chunks(const wh::GbdtShapPlan& plan) {
  ShapChunks out;
  for (auto& c : plan.chunks)
    out.emplace_back(c.path_begin, c.npath, c.elem_begin, c.nelem, c.cls, c.width);
  return out;
}

// The kernels' tables of the trees' lists and covers, on the host: (used
// int32 [U], tree_E float64 [T], paths int32 [P, 4], elems int32 [E, 4], ecol
// int32 [E], chunks, nodes int32 [N, 4], tree_off int32 [T + 1], node_m
// float32 [N], node_col int32 [N]). ValueError: a malformed tree, a tree
// without usable covers, a path of more than 63 distinct features.
py::tuple gbdt_shap_pack(TreeInts feat, TreeReals cond, TreeInts left, TreeInts right,
                         TreeInts defl, TreeReals leaf, const TreeReals& cover, int64_t num_class,
                         int64_t lds_elems) {
  wh::GbdtForestTrees tr{std::move(feat), std::move(left), std::move(right), std::move(defl),
                         std::move(cond), std::move(leaf)};
  const wh::GbdtShapModel m = wh::gbdt_shap_pack(tr, cover, (int)num_class);
  const wh::GbdtShapPlan plan = wh::gbdt_shap_plan(m, lds_elems);
  const wh::GbdtShapTable tab = wh::gbdt_shap_table(m, plan);
  const int64_t N = (int64_t)m.nodes.size();
  auto nodes = torch::empty({N, 4}, torch::kInt32);
  if (N) std::memcpy(nodes.data_ptr(), m.nodes.data(), N * sizeof(m.nodes[0]));
  auto E = torch::empty({m.ntree()}, torch::kFloat64);
  if (m.ntree()) std::memcpy(E.data_ptr(), m.tree_E.data(), m.ntree() * 8);
  auto nm = torch::empty({N}, torch::kFloat32);
  for (int64_t i = 0; i < N; ++i) nm.data_ptr<float>()[i] = (float)m.node_m[i];
  return py::make_tuple(int32_tensor(m.used, {(int64_t)m.used.size()}), E,
                        int32_tensor(tab.paths, {(int64_t)tab.paths.size() / 4, 4}),
                        int32_tensor(tab.elems, {(int64_t)tab.elems.size() / 4, 4}),
                        int32_tensor(tab.ecol, {(int64_t)tab.ecol.size()}), shap_chunks(plan), nodes,
                        int32_tensor(m.tree_off, {(int64_t)m.tree_off.size()}), nm,
                        int32_tensor(m.node_col, {N}));
}

// (order, chunks) of paths given by length, class and tree
py::tuple gbdt_shap_plan(const std::vector<int32_t>& path_len, const std::vector<int32_t>& path_class,
                         const std::vector<int32_t>& path_tree, int64_t lds_elems) {
  const wh::GbdtShapPlan plan = wh::gbdt_shap_plan(path_len, path_class, path_tree, lds_elems);
  return py::make_tuple(plan.order, shap_chunks(plan));
}

// The host references: (phi float64 [K, n, U + 1] in compact columns, the
// bias last; used int32 [U]); f32: computed in fp32 throughout.
template <class Rows>
py::tuple shap_rows_host(wh::GbdtForestTrees tr, const TreeReals& cover, int64_t num_class,
                         double base, const Rows& rows, int64_t n, bool approx, bool f32) {
  const wh::GbdtShapModel m = wh::gbdt_shap_pack(tr, cover, (int)num_class);
  const int64_t U1 = (int64_t)m.used.size() + 1;
  auto phi = torch::empty({num_class, n, U1}, torch::kFloat64);
  if (f32) {
    auto p32 = torch::empty({num_class, n, U1}, torch::kFloat32);
    wh::gbdt_shap_rows<float>(m, rows, n, base, approx, p32.data_ptr<float>());
    phi.copy_(p32);
  } else {
    wh::gbdt_shap_rows<double>(m, rows, n, base, approx, phi.data_ptr<double>());
  }
  return py::make_tuple(phi, int32_tensor(m.used, {U1 - 1}));
}

py::tuple gbdt_shap_rows(TreeInts feat, TreeReals cond, TreeInts left, TreeInts right,
                         TreeInts defl, TreeReals leaf, const TreeReals& cover, int64_t num_class,
                         double base, const Tensor& X, bool approx, bool f32) {
  TORCH_CHECK(!X.is_cuda() && X.dim() == 2 && X.scalar_type() == torch::kFloat32 &&
                  X.is_contiguous(),
              "gbdt_shap_rows: X must be a contiguous CPU float32 matrix");
  return shap_rows_host(wh::GbdtForestTrees{std::move(feat), std::move(left), std::move(right),
                                            std::move(defl), std::move(cond), std::move(leaf)},
                        cover, num_class, base, wh::ShapDenseRows{X.data_ptr<float>(), X.size(1)},
                        X.size(0), approx, f32);
}

// the CSR rows of a host reference, checked: (rows, n)
std::pair<wh::ShapCsrRows, int64_t> shap_host_csr(const char* who, const Tensor& row_off,
                                                  const Tensor& fid,
                                                  const c10::optional<Tensor>& val) {
  TORCH_CHECK(!row_off.is_cuda() && row_off.scalar_type() == torch::kInt64 &&
                  row_off.is_contiguous() && row_off.numel() >= 1 && !fid.is_cuda() &&
                  fid.scalar_type() == torch::kInt32 && fid.is_contiguous(),
              who, ": row_off int64 [n + 1] and fid int32 on the CPU");
  const int64_t n = row_off.numel() - 1;
  const int64_t* off = row_off.data_ptr<int64_t>();
  TORCH_CHECK(off[0] >= 0 && off[n] <= fid.numel(), who, ": row_off leaves fid");
  for (int64_t r = 0; r < n; ++r)
    TORCH_CHECK(off[r] <= off[r + 1], who, ": row_off must not decrease");
  const float* v = nullptr;
  if (present(val)) {
    TORCH_CHECK(!val->is_cuda() && val->scalar_type() == torch::kFloat32 && val->is_contiguous() &&
                    val->numel() == fid.numel(),
                who, ": val must be float32 of fid's size");
    v = val->data_ptr<float>();
  }
  return {wh::ShapCsrRows{off, fid.data_ptr<int32_t>(), v}, n};
}

py::tuple gbdt_shap_rows_csr(TreeInts feat, TreeReals cond, TreeInts left, TreeInts right,
                             TreeInts defl, TreeReals leaf, const TreeReals& cover,
                             int64_t num_class, double base, const Tensor& row_off,
                             const Tensor& fid, const c10::optional<Tensor>& val, bool approx,
                             bool f32) {
  const auto [rows, n] = shap_host_csr("gbdt_shap_rows_csr", row_off, fid, val);
  return shap_rows_host(wh::GbdtForestTrees{std::move(feat), std::move(left), std::move(right),
                                            std::move(defl), std::move(cond), std::move(leaf)},
                        cover, num_class, base, rows, n, approx, f32);
}

// The interactions' host references: (Phi float64 [K, n, U + 1, U + 1] in
// compact columns, the bias last; used int32 [U]); f32: computed in fp32
// throughout.
template <class Rows>
py::tuple shap_inter_rows_host(wh::GbdtForestTrees tr, const TreeReals& cover, int64_t num_class,
                               double base, const Rows& rows, int64_t n, bool f32) {
  const wh::GbdtShapModel m = wh::gbdt_shap_pack(tr, cover, (int)num_class);
  const int64_t U1 = (int64_t)m.used.size() + 1;
  auto phi = torch::empty({num_class, n, U1, U1}, torch::kFloat64);
  if (f32) {
    auto p32 = torch::empty({num_class, n, U1, U1}, torch::kFloat32);
    wh::gbdt_shap_inter_rows<float>(m, rows, n, base, p32.data_ptr<float>());
    phi.copy_(p32);
  } else {
    wh::gbdt_shap_inter_rows<double>(m, rows, n, base, phi.data_ptr<double>());
  }
  return py::make_tuple(phi, int32_tensor(m.used, {U1 - 1}));
}

py::tuple gbdt_shap_inter_rows(TreeInts feat, TreeReals cond, TreeInts left, TreeInts right,
                               TreeInts defl, TreeReals leaf, const TreeReals& cover,
                               int64_t num_class, double base, const Tensor& X, bool f32) {
  TORCH_CHECK(!X.is_cuda() && X.dim() == 2 && X.scalar_type() == torch::kFloat32 &&
                  X.is_contiguous(),
              "gbdt_shap_inter_rows: X must be a contiguous CPU float32 matrix");
  return shap_inter_rows_host(
      wh::GbdtForestTrees{std::move(feat), std::move(left), std::move(right), std::move(defl),
                          std::move(cond), std::move(leaf)},
      cover, num_class, base, wh::ShapDenseRows{X.data_ptr<float>(), X.size(1)}, X.size(0), f32);
}

py::tuple gbdt_shap_inter_rows_csr(TreeInts feat, TreeReals cond, TreeInts left, TreeInts right,
                                   TreeInts defl, TreeReals leaf, const TreeReals& cover,
                                   int64_t num_class, double base, const Tensor& row_off,
                                   const Tensor& fid, const c10::optional<Tensor>& val, bool f32) {
  const auto [rows, n] = shap_host_csr("gbdt_shap_inter_rows_csr", row_off, fid, val);
  return shap_inter_rows_host(
      wh::GbdtForestTrees{std::move(feat), std::move(left), std::move(right), std::move(defl),
                          std::move(cond), std::move(leaf)},
      cover, num_class, base, rows, n, f32);
}

// out: float32 [K, n, U + 1], contiguous, the bias column set by the caller.
void shap_out_check(const Tensor& out, int64_t n, int64_t ncol) {
  CHECK_IN(out, torch::kFloat32);
  TORCH_CHECK(out.dim() == 3 && out.size(0) >= 1 && out.size(1) == n && out.size(2) == ncol + 1 &&
                  out.size(2) <= INT32_MAX,
              "contributions must be [K, n, U + 1]");
}

// The checks both exact kernels share, then one launch per chunk.
template <class Launch>
void shap_run(const Tensor& paths, const Tensor& elems, const Tensor& ecol,
              const ShapChunks& chunks, int64_t ncol, const Tensor& out, int64_t n,
              Launch launch) {
  CHECK_IN(paths, torch::kInt32);
  CHECK_IN(elems, torch::kInt32);
  CHECK_IN(ecol, torch::kInt32);
  TORCH_CHECK(paths.dim() == 2 && paths.size(1) == 4 && elems.dim() == 2 && elems.size(1) == 4 &&
                  ecol.dim() == 1 && ecol.numel() == elems.size(0) &&
                  elems.size(0) <= INT32_MAX,
              "the path table must be paths [P, 4], elems [E, 4], ecol [E]");
  shap_out_check(out, n, ncol);
  const int64_t K = out.size(0), U1 = out.size(2);
  int64_t path = 0, elem = 0;
  for (auto& [path_begin, npath, elem_begin, nelem, cls, width] : chunks) {
    TORCH_CHECK(path_begin == path && elem_begin == elem && npath >= 1 && nelem >= npath &&
                    nelem <= wh::gbdt_shap_lds_elems() && cls >= 0 && cls < K &&
                    (width == 16 || width == 32 || width == 64),
                "contribution chunks must be consecutive whole paths that fit the LDS");
    path += npath, elem += nelem;
  }
  TORCH_CHECK(path == paths.size(0) && elem == elems.size(0),
              "contribution chunks must cover the path table");
  if (n == 0) return;
  for (auto& [path_begin, npath, elem_begin, nelem, cls, width] : chunks)
    launch(wh::ShapChunk{paths.data_ptr(), elems.data_ptr(), ptr<int32_t>(ecol), (int)path_begin,
                         (int)npath, (int)elem_begin, (int)nelem, (int)width, (int)U1,
                         ptr<float>(out) + cls * n * U1});
}

void gbdt_shap(const Tensor& X, const Tensor& paths, const Tensor& elems, const Tensor& ecol,
               const ShapChunks& chunks, int64_t ncol, int64_t max_feat, const Tensor& out) {
  CHECK_IN(X, torch::kFloat32);
  TORCH_CHECK(X.dim() == 2 && max_feat < X.size(1), "forest splits on a feature X does not have");
  c10::DeviceGuard g(X.device());
  auto s = cur_stream(X);
  shap_run(paths, elems, ecol, chunks, ncol, out, X.size(0), [&](const wh::ShapChunk& c) {
    wh::gbdt_shap(ptr<float>(X), X.size(0), (int)X.size(1), c, s);
  });
}

// the CSR arguments the contribution kernels share; returns n
int64_t shap_csr_check(const Tensor& row_off, const Tensor& fid, const c10::optional<Tensor>& val) {
  CHECK_IN(row_off, torch::kInt64);
  CHECK_IN(fid, torch::kInt32);
  TORCH_CHECK(row_off.numel() >= 1, "row_off must be [n + 1]");
  if (present(val)) {
    CHECK_IN((*val), torch::kFloat32);
    TORCH_CHECK(val->numel() == fid.numel(), "val and fid sizes differ");
  }
  return row_off.numel() - 1;
}

void gbdt_shap_csr(const Tensor& row_off, const Tensor& fid, const c10::optional<Tensor>& val,
                   const Tensor& paths, const Tensor& elems, const Tensor& ecol,
                   const ShapChunks& chunks, int64_t ncol, const Tensor& out) {
  const int64_t n = shap_csr_check(row_off, fid, val);
  c10::DeviceGuard g(row_off.device());
  auto s = cur_stream(row_off);
  shap_run(paths, elems, ecol, chunks, ncol, out, n, [&](const wh::ShapChunk& c) {
    wh::gbdt_shap_csr(ptr<int64_t>(row_off), ptr<int32_t>(fid), optptr<float>(val), n, c, s);
  });
}

// Interactions: out float32 [K, n, U + 1, U + 1], contiguous, cell (U, U) of
// every matrix (the bias) set by the caller; every other cell is written. The
// exact contributions of the same rows (launch_phi: the unchanged kernels)
// give the diagonal; the pairs are gathered in a scratch triangle
// [K, n, U (U - 1) / 2].
template <class LaunchPhi, class LaunchInter>
void shap_inter_run(const Tensor& paths, const Tensor& elems, const Tensor& ecol,
                    const ShapChunks& chunks, int64_t ncol, const Tensor& out, int64_t n,
                    hipStream_t s, LaunchPhi launch_phi, LaunchInter launch_inter) {
  CHECK_IN(out, torch::kFloat32);
  TORCH_CHECK(out.dim() == 4 && out.size(0) >= 1 && out.size(1) == n && out.size(2) == ncol + 1 &&
                  out.size(3) == ncol + 1 && ncol < INT32_MAX,
              "interactions must be [K, n, U + 1, U + 1]");
  const int64_t K = out.size(0), U1 = ncol + 1, TP = wh::gbdt_shap_inter_pairs(ncol);
  auto phi = torch::zeros({K, n, U1}, out.options());
  phi.select(2, ncol).copy_(out.select(2, ncol).select(2, ncol));
  shap_run(paths, elems, ecol, chunks, ncol, phi, n, launch_phi);  // (checks the table)
  auto tri = torch::zeros({K, n, TP}, out.options());
  if (n == 0) return;
  for (auto& [path_begin, npath, elem_begin, nelem, cls, width] : chunks)
    launch_inter(wh::ShapChunk{paths.data_ptr(), elems.data_ptr(), ptr<int32_t>(ecol),
                               (int)path_begin, (int)npath, (int)elem_begin, (int)nelem,
                               (int)width, (int)U1, ptr<float>(tri) + cls * n * TP});
  wh::gbdt_shap_inter_out(ptr<float>(tri), ptr<float>(phi), K * n, (int)U1, ptr<float>(out), s);
}

void gbdt_shap_inter(const Tensor& X, const Tensor& paths, const Tensor& elems,
                     const Tensor& ecol, const ShapChunks& chunks, int64_t ncol, int64_t max_feat,
                     const Tensor& out) {
  CHECK_IN(X, torch::kFloat32);
  TORCH_CHECK(X.dim() == 2 && max_feat < X.size(1), "forest splits on a feature X does not have");
  c10::DeviceGuard g(X.device());
  auto s = cur_stream(X);
  shap_inter_run(
      paths, elems, ecol, chunks, ncol, out, X.size(0), s,
      [&](const wh::ShapChunk& c) {
        wh::gbdt_shap(ptr<float>(X), X.size(0), (int)X.size(1), c, s);
      },
      [&](const wh::ShapChunk& c) {
        wh::gbdt_shap_inter(ptr<float>(X), X.size(0), (int)X.size(1), c, s);
      });
}

void gbdt_shap_inter_csr(const Tensor& row_off, const Tensor& fid,
                         const c10::optional<Tensor>& val, const Tensor& paths,
                         const Tensor& elems, const Tensor& ecol, const ShapChunks& chunks,
                         int64_t ncol, const Tensor& out) {
  const int64_t n = shap_csr_check(row_off, fid, val);
  c10::DeviceGuard g(row_off.device());
  auto s = cur_stream(row_off);
  shap_inter_run(
      paths, elems, ecol, chunks, ncol, out, n, s,
      [&](const wh::ShapChunk& c) {
        wh::gbdt_shap_csr(ptr<int64_t>(row_off), ptr<int32_t>(fid), optptr<float>(val), n, c, s);
      },
      [&](const wh::ShapChunk& c) {
        wh::gbdt_shap_inter_csr(ptr<int64_t>(row_off), ptr<int32_t>(fid), optptr<float>(val), n, c,
                                s);
      });
}

wh::SaabasForest saabas_forest(const Tensor& nodes, const Tensor& tree_off, const Tensor& node_m,
                               const Tensor& node_col, int64_t ncol, const Tensor& out, int64_t n) {
  CHECK_IN(nodes, torch::kInt32);
  CHECK_IN(tree_off, torch::kInt32);
  CHECK_IN(node_m, torch::kFloat32);
  CHECK_IN(node_col, torch::kInt32);
  const int64_t T = tree_off.numel() - 1;
  TORCH_CHECK(nodes.dim() == 2 && nodes.size(1) == 4 && node_m.numel() == nodes.size(0) &&
                  node_col.numel() == nodes.size(0) && T >= 0 && T <= INT32_MAX,
              "the forest must be nodes [N, 4], tree_off [T + 1], node_m [N], node_col [N]");
  shap_out_check(out, n, ncol);
  return wh::SaabasForest{nodes.data_ptr(), ptr<int32_t>(tree_off), ptr<float>(node_m),
                          ptr<int32_t>(node_col), (int)T, (int)out.size(0), (int)out.size(2),
                          ptr<float>(out)};
}

void gbdt_saabas(const Tensor& X, const Tensor& nodes, const Tensor& tree_off,
                 const Tensor& node_m, const Tensor& node_col, int64_t ncol, int64_t max_feat,
                 const Tensor& out) {
  CHECK_IN(X, torch::kFloat32);
  TORCH_CHECK(X.dim() == 2 && max_feat < X.size(1), "forest splits on a feature X does not have");
  c10::DeviceGuard g(X.device());
  const auto f = saabas_forest(nodes, tree_off, node_m, node_col, ncol, out, X.size(0));
  wh::gbdt_saabas(ptr<float>(X), X.size(0), (int)X.size(1), f, cur_stream(X));
}

void gbdt_saabas_csr(const Tensor& row_off, const Tensor& fid, const c10::optional<Tensor>& val,
                     const Tensor& nodes, const Tensor& tree_off, const Tensor& node_m,
                     const Tensor& node_col, int64_t ncol, const Tensor& out) {
  const int64_t n = shap_csr_check(row_off, fid, val);
  c10::DeviceGuard g(row_off.device());
  const auto f = saabas_forest(nodes, tree_off, node_m, node_col, ncol, out, n);
  wh::gbdt_saabas_csr(ptr<int64_t>(row_off), ptr<int32_t>(fid), optptr<float>(val), n, f,
                      cur_stream(row_off));
}

int64_t gbdt_shap_max_blocks() { return wh::gbdt_shap_max_blocks(); }

// ----------------------------------------------------- learning to rank
// The task plan of a matrix's query groups (host/gbdt_rank_plan.h), on the
// host: group_off, a CPU integer tensor [Q + 1] -> (small, block, tiled: int32
// group ids, larger groups first; the rows of the largest block group and of
// the largest tiled group). Malformed offsets raise ValueError.
py::tuple gbdt_rank_plan(const Tensor& group_off, int64_t n, int64_t lds_rows) {
  TORCH_CHECK(!group_off.is_cuda() && group_off.dim() == 1 &&
                  at::isIntegralType(group_off.scalar_type(), false),
              "gbdt_rank_plan: group_off must be a CPU integer vector");
  const auto off = group_off.to(torch::kInt64).contiguous();
  // (std::invalid_argument -> ValueError)
  const auto p = wh::gbdt_rank_plan(off.data_ptr<int64_t>(), (size_t)off.numel(), n, lds_rows);
  const auto ids = [](const std::vector<int32_t>& v) {
    auto t = torch::empty({(int64_t)v.size()}, torch::kInt32);
    if (!v.empty()) std::memcpy(t.data_ptr(), v.data(), v.size() * 4);
    return t;
  };
  return py::make_tuple(ids(p.small), ids(p.block), ids(p.tiled), p.max_block_rows,
                        p.max_tiled_rows);
}

namespace {
// The checked inputs both ranking ops share -> the kernels' task lists.
wh::RankTasks rank_args(const char* op, const Tensor& margin, const Tensor& label,
                        const Tensor& group_off, const Tensor& small, const Tensor& block,
                        const Tensor& tiled, int64_t block_rows, int64_t tiled_rows,
                        int64_t tile_rows) {
  CHECK_IN(margin, torch::kFloat32);
  CHECK_IN(label, torch::kFloat32);
  CHECK_IN(group_off, torch::kInt32);
  CHECK_IN(small, torch::kInt32);
  CHECK_IN(block, torch::kInt32);
  CHECK_IN(tiled, torch::kInt32);
  const int64_t n = margin.numel();
  TORCH_CHECK(label.numel() == n && n <= INT32_MAX, op, ": label size mismatch");
  TORCH_CHECK(group_off.numel() >= 1 && group_off.numel() - 1 <= INT32_MAX, op,
              ": group_off must be [Q + 1]");
  const int64_t cap = wh::gbdt_rank_lds_rows();
  if (tile_rows <= 0) tile_rows = cap;
  TORCH_CHECK(block_rows >= 0 && block_rows <= cap && tile_rows <= cap, op,
              ": at most gbdt_rank_lds_rows() rows fit the LDS");
  TORCH_CHECK(tiled_rows >= 0 && tiled_rows <= INT32_MAX, op, ": tiled_rows out of range");
  TORCH_CHECK(std::max({small.numel(), block.numel(), tiled.numel()}) <= INT32_MAX, op,
              ": too many tasks");
  return {ptr<int32_t>(small), ptr<int32_t>(block), ptr<int32_t>(tiled),
          (int)small.numel(), (int)block.numel(), (int)tiled.numel(),
          (int)block_rows, (int)tiled_rows, (int)tile_rows};
}
}  // namespace

// (gpair f32 [n, 2], stats f64 [4] = {sum g, sum h, max|g|, max|h|}) of
// rank:pairwise, or, ndcg, rank:ndcg
std::vector<Tensor> gbdt_gpair_rank(const Tensor& margin, const Tensor& label,
                                    const Tensor& group_off, const Tensor& small,
                                    const Tensor& block, const Tensor& tiled, int64_t block_rows,
                                    int64_t tiled_rows, bool ndcg, int64_t tile_rows) {
  const auto tk = rank_args("gbdt_gpair_rank", margin, label, group_off, small, block, tiled,
                            block_rows, tiled_rows, tile_rows);
  const int64_t n = margin.numel();
  c10::DeviceGuard g(margin.device());
  const auto f64 = margin.options().dtype(torch::kFloat64);
  auto gp = torch::zeros({n, 2}, margin.options());
  auto st = torch::zeros({4}, f64);
  if (n > 0) {
    const bool chunks = tk.ntiled > 0 || tk.nblock > 0;
    auto aux = torch::empty({chunks ? 2 * n : 2}, margin.options());
    auto idcg = torch::empty({chunks && ndcg ? n : 1}, f64);
    auto scratch = torch::empty({wh::gbdt_rank_scratch()}, f64);
    wh::gbdt_gpair_rank(ptr<float>(margin), ptr<float>(label), ptr<int32_t>(group_off),
                        (int)group_off.numel() - 1, n, tk, ndcg, ptr<float>(aux), ptr<double>(idcg),
                        ptr<float>(gp),
                        ptr<double>(scratch), ptr<double>(st), cur_stream(margin));
  }
  return {gp, st};
}

// f64 [Q]: every group's ndcg@k (kind 0) or map@k (kind 1), NaN for an empty
// group; k <= 0: no cut-off
Tensor gbdt_rank_eval(const Tensor& margin, const Tensor& label, const Tensor& group_off,
                      const Tensor& small, const Tensor& block, const Tensor& tiled,
                      int64_t block_rows, int64_t tiled_rows, int64_t kind, int64_t k, bool minus,
                      int64_t tile_rows) {
  const auto tk = rank_args("gbdt_rank_eval", margin, label, group_off, small, block, tiled,
                            block_rows, tiled_rows, tile_rows);
  TORCH_CHECK(kind == 0 || kind == 1, "gbdt_rank_eval: kind is 0 (ndcg) or 1 (map)");
  c10::DeviceGuard g(margin.device());
  const int64_t Q = group_off.numel() - 1;
  auto out = torch::full({Q}, std::numeric_limits<double>::quiet_NaN(),
                         margin.options().dtype(torch::kFloat64));
  const int kk = k <= 0 || k > INT32_MAX ? INT32_MAX : (int)k;
  auto part = torch::empty({tk.nblock > 0 || tk.ntiled > 0 ? 2 * margin.numel() : 2}, out.options());
  wh::gbdt_rank_eval(ptr<float>(margin), ptr<float>(label), ptr<int32_t>(group_off), (int)Q,
                     margin.numel(), tk, (int)kind, kk, minus, ptr<double>(part), ptr<double>(out),
                     cur_stream(margin));
  return out;
}

// ------------------------------------------------------------ gbdt grower
// Depth-wise histogram tree growth with the level loop in C++ (reference:
// xgboost hist updater driven by bin/xgboost.dmlc). Per level
// ONE host synchronisation: the split results of this level and the
// partition counts of the previous one come back in a single pinned copy;
// the child row segments the histograms need are derived on the device
// (k_child_segs), histogram tasks address them by chunk index, and the
// sibling histograms are parent - built child in one kernel. Host tables go
// down as one pinned upload per level. (The Python level loop it replaces
// left the GPU idle ~60% of each tree on per-node Python work and two syncs
// per level.)
// What the two growers share: the checked inputs, the row and feature-group
// counts, the rows per histogram task and the dtype options of B's device.
struct GrowCtx : HistCtx {
  const int64_t n;
  const int G;
  const torch::TensorOptions f64, i32, u8;

  GrowCtx(const Tensor& B, const Tensor& Bc, const Tensor& ridx0, const Tensor& gpair,
          const Tensor& qscale, const Tensor& valid, int64_t nbin,
          const std::vector<std::pair<int64_t, int64_t>>& fgroups, int64_t max_fcnt)
      : HistCtx(B, gpair, qscale, nbin, max_fcnt,
                (int)std::max<int64_t>(8192, (ridx0.numel() + 1023) / 1024)),
        n(ridx0.numel()), G((int)fgroups.size()), f64(B.options().dtype(torch::kFloat64)),
        i32(B.options().dtype(torch::kInt32)), u8(B.options().dtype(torch::kUInt8)) {
    CHECK_IN(Bc, torch::kUInt8);
    CHECK_IN(ridx0, torch::kInt32);
    CHECK_DEV(valid);
    TORCH_CHECK(n < (int64_t)INT32_MAX, "rows must fit int32");
  }
};

// A grown tree on the host, nodes in breadth-first creation order, and the
// tuple both growers hand to Python (models/gbdt_tree.py RegTree.from_lists):
// (feat, bin, cond, defl, left, right, parent, gain, cover, base weight, leaf,
// [(leaf id, begin, end)])
struct TreeLists {
  std::vector<int> feat, bin, defl, left, right, parent;
  std::vector<double> gain, cover, bw, leaf;

  int add(int par) {  // a new leaf
    feat.push_back(-1), bin.push_back(0), defl.push_back(0), left.push_back(-1),
        right.push_back(-1), parent.push_back(par), gain.push_back(0), cover.push_back(0),
        bw.push_back(0), leaf.push_back(0);
    return (int)feat.size() - 1;
  }

  py::tuple pack(const std::vector<float>& cut_vals, const std::vector<int64_t>& cut_off,
                 const py::list& segs) const {
    std::vector<float> cond(feat.size(), 0.f);
    for (size_t i = 0; i < feat.size(); ++i)
      if (feat[i] >= 0) cond[i] = cut_vals[cut_off[feat[i]] + bin[i]];
    return py::make_tuple(feat, bin, cond, defl, left, right, parent, gain, cover, bw, leaf, segs);
  }
};

py::tuple gbdt_grow(const Tensor& B, const Tensor& Bc, const Tensor& ridx0, const Tensor& gpair,
                    const Tensor& qscale, const Tensor& valid, int64_t nbin,
                    std::vector<std::pair<int64_t, int64_t>> fgroups, int64_t max_fcnt,
                    std::vector<double> root_tot, std::vector<float> cut_vals,
                    std::vector<int64_t> cut_off, double eta, double alpha, double lambda,
                    double mcw, int64_t max_depth, double rt_eps, py::object allreduce,
                    const c10::optional<Tensor>& mono, const c10::optional<Tensor>& fmask,
                    double max_delta_step) {
  const GrowCtx cx(B, Bc, ridx0, gpair, qscale, valid, nbin, fgroups, max_fcnt);
  c10::DeviceGuard g(B.device());
  const auto s = cx.s;
  const int64_t n = cx.n;
  const int F = cx.F;
  const auto &f64 = cx.f64, &i32 = cx.i32;
  const int64_t per = (int64_t)F * nbin * 2;
  const bool reduce = !allreduce.is_none();
  // monotone_constraints: the signs on the device (the split search) and on
  // the host (the children's intervals), and every node's weight interval
  const GrowCons cons(mono, fmask, max_delta_step, B, F, "gbdt_grow");
  const bool mono_on = cons.mono_on, inter_on = cons.inter_on;
  std::vector<int8_t> mono_h;
  if (mono_on) {
    auto mh = mono->cpu();
    mono_h.assign(mh.data_ptr<int8_t>(), mh.data_ptr<int8_t>() + F);
  }
  // interaction_constraints: the features' group bit sets on the device (the
  // split search) and on the host (the children's states), and every node's
  std::vector<uint64_t> fmask_h;
  if (inter_on) {
    auto fh = fmask->cpu();
    const auto* q = reinterpret_cast<const uint64_t*>(fh.data_ptr<int64_t>());
    fmask_h.assign(q, q + F);
  }
  // host tree
  TreeLists t;
  std::vector<std::array<double, 2>> tot;
  std::vector<wh::GbdtBounds> bnd;
  std::vector<uint64_t> state;
  // (max_delta_step: the root's interval; the children's are cut inside it)
  auto add = [&](int par) {
    return tot.push_back({0, 0}), bnd.push_back({-cons.top, cons.top}),
           state.push_back(wh::kGbdtInterRoot), t.add(par);
  };
  // a node's weight inside an interval ((-inf, inf) without constraints)
  auto weight = [&](int nd, const wh::GbdtBounds& b) {
    return wh::gbdt_weight(tot[nd][0], tot[nd][1], alpha, lambda, mcw, b);
  };
  const int root = add(-1);
  tot[root] = {root_tot[0], root_tot[1]};
  std::map<int, std::pair<int, int>> seg;  // live frontier segments (node -> [b, e))
  seg[root] = {0, (int)n};
  py::list segs;  // finished leaves: (node, b, e)
  // staging rings for the uploads (node tables, task lists), a plain buffer
  // for the one download per level (read right after its synchronisation)
  PinnedRing<4> up, up_tasks;
  PinnedBuf down;
  Tensor ridx = ridx0;
  // histogram of the given (slot -> [b, e) device segments); tasks by chunk.
  // Prepared (task lists built and uploaded, outputs allocated) before the
  // level's partition is enqueued, so the histogram launch follows the
  // child segments without host work in between.
  struct HistPlan {
    Tensor d, hist, part;
    int64_t nt = 0, nr = 0;
  };
  auto plan_hist = [&](const std::vector<int64_t>& seglen) -> HistPlan {
    const int S = (int)seglen.size();
    std::vector<int32_t> tasks, red;
    wh::gbdt_hist_plan(seglen, fgroups, cx.chunk, &tasks, &red);
    HistPlan hp;
    hp.nt = (int64_t)tasks.size() / 5;
    hp.nr = (int64_t)red.size() / 6;
    int32_t* h = up_tasks.get<int32_t>(tasks.size() + red.size());
    std::memcpy(h, tasks.data(), tasks.size() * 4);
    std::memcpy(h + tasks.size(), red.data(), red.size() * 4);
    hp.d = up_tasks.tensor().narrow(0, 0, (int64_t)(tasks.size() + red.size()) * 4)
               .to(B.device(), /*non_blocking=*/true).view(torch::kInt32);
    up_tasks.mark(s);
    hp.hist = torch::empty({S, F, nbin, 2}, f64);
    hp.part = cx.part(hp.nt);
    return hp;
  };
  auto run_hist = [&](const HistPlan& hp, const Tensor& dseg) -> Tensor {
    cx.run(ridx, ptr<int32_t>(hp.d), hp.nt, ptr<int32_t>(hp.d) + hp.nt * 5, hp.nr, hp.part,
           hp.hist, ptr<int32_t>(dseg));
    // (no drain here: the staging ring waits for this copy only when its slot
    // comes round again; the histogram allreduce is stream-ordered)
    if (reduce) allreduce(hp.hist);
    return hp.hist;
  };
  Tensor dseg_root = torch::tensor({0, (int)n}, torch::TensorOptions().dtype(torch::kInt32))
                         .to(B.device());
  Tensor H_front = run_hist(plan_hist({n}), dseg_root);
  std::vector<int> frontier{root};
  // splits whose children's segments wait for the partition counts
  std::vector<std::array<int, 5>> pending;  // nd, l, r, b, e
  // (resolved once the host holds that partition's left counts nleft [node])
  auto resolve_pending = [&](const int32_t* nleft) {
    for (auto& pd : pending) {
      const int m = pd[3] + nleft[pd[0]];
      seg[pd[1]] = {pd[3], m};
      seg[pd[2]] = {m, pd[4]};
    }
    pending.clear();
  };
  Tensor nleft_dev;
  for (int depth = 0; depth <= max_depth && !frontier.empty(); ++depth) {
    const int S = (int)frontier.size();
    const bool last = depth == max_depth;
    Tensor split_out;
    if (!last) {
      // 8-byte words: totals [S x 2], then (constraints) the weight intervals
      // [S x 2], then the group sets [S]
      const int w_bnd = 2 * S, w_state = w_bnd + (mono_on ? 2 * S : 0);
      const int nw = w_state + (inter_on ? S : 0);
      double* th = up.get<double>(nw);
      for (int k = 0; k < S; ++k) th[2 * k] = tot[frontier[k]][0], th[2 * k + 1] = tot[frontier[k]][1];
      if (mono_on)
        for (int k = 0; k < S; ++k)
          th[w_bnd + 2 * k] = bnd[frontier[k]].lo, th[w_bnd + 2 * k + 1] = bnd[frontier[k]].hi;
      if (inter_on)
        for (int k = 0; k < S; ++k) std::memcpy(th + w_state + k, &state[frontier[k]], 8);
      auto T = up.tensor().narrow(0, 0, 8 * (int64_t)nw).to(B.device(), true).view(torch::kFloat64);
      up.mark(s);
      split_out = torch::empty({S, 6}, f64);
      TORCH_CHECK(split_search(H_front, ptr<double>(T), ptr<uint8_t>(valid), S, alpha, lambda, mcw,
                               split_out, s,
                               cons.at(ptr<double>(T) + w_bnd,
                                       reinterpret_cast<const uint64_t*>(ptr<double>(T) + w_state))),
                  "gbdt_split failed");
    }
    // the level's one synchronisation: split results + previous partition counts
    const int64_t nl_n = nleft_dev.defined() ? nleft_dev.numel() : 0;
    double* hdown = down.get<double>(6 * (last ? 0 : S) + nl_n / 2 + 2);
    if (!last)
      WH_HIP_CHECK_HOST(hipMemcpyAsync(hdown, split_out.data_ptr(), 48 * S, hipMemcpyDeviceToHost, s));
    int32_t* nl_h = reinterpret_cast<int32_t*>(hdown + 6 * (last ? 0 : S));
    if (nl_n)
      WH_HIP_CHECK_HOST(hipMemcpyAsync(nl_h, nleft_dev.data_ptr(), 4 * nl_n, hipMemcpyDeviceToHost, s));
    WH_HIP_CHECK_HOST(hipStreamSynchronize(s));
    resolve_pending(nl_h);
    for (int nd : frontier) {
      t.cover[nd] = tot[nd][1];
      t.bw[nd] = weight(nd, bnd[nd]);
      t.leaf[nd] = eta * t.bw[nd];
    }
    if (last) break;
    std::vector<int> split_k;
    for (int k = 0; k < S; ++k) {
      const double* o = hdown + 6 * k;
      if (!(o[0] > rt_eps)) continue;
      const int nd = frontier[k];
      const int f = (int)o[1], b = (int)o[2];
      t.feat[nd] = f, t.bin[nd] = b, t.defl[nd] = (int)o[3], t.gain[nd] = o[0];
      const int l = add(nd), r = add(nd);
      t.left[nd] = l, t.right[nd] = r;
      tot[l] = {o[4], o[5]};
      tot[r] = {tot[nd][0] - o[4], tot[nd][1] - o[5]};
      if (mono_on) {
        const wh::GbdtBounds pb = bnd[nd];  // (bnd grew: no reference into it)
        const auto cb = wh::gbdt_child_bounds(mono_h[f], pb, weight(l, pb), weight(r, pb));
        bnd[l] = cb.left, bnd[r] = cb.right;
      }
      if (inter_on) state[l] = state[r] = wh::gbdt_child_state(state[nd], fmask_h[f]);
      split_k.push_back(k);
    }
    if (split_k.empty()) break;
    const int nnode = (int)t.feat.size();
    const int nsplit = (int)split_k.size();
    // segment tiling of [0, n) for the position -> node map (gaps: -1)
    std::vector<std::array<int, 3>> live;
    for (auto& kv : seg) live.push_back({kv.second.first, kv.second.second, kv.first});
    const auto tiles = wh::gbdt_level_tiles(live, n);  // (begin, node)
    const int nt = (int)tiles.size();
    // one pinned upload of the level's tables
    const wh::GbdtNodeTables at(nnode, nt, nsplit);
    int32_t* hw = up.get<int32_t>(at.nwords);
    std::memset(hw, 0, at.nwords * 4);
    uint8_t* h_defl = reinterpret_cast<uint8_t*>(hw + at.defl);
    for (int i = 0; i < nnode; ++i) hw[at.feat + i] = -1;
    std::vector<int64_t> small_len(nsplit);
    for (int q = 0; q < nsplit; ++q) {
      const int k = split_k[q], nd = frontier[k];
      hw[at.feat + nd] = t.feat[nd], hw[at.bin + nd] = t.bin[nd], h_defl[nd] = (uint8_t)t.defl[nd];
      const auto sg = seg[nd];
      hw[at.sb + nd] = sg.first, hw[at.se + nd] = sg.second;
      hw[at.lc + nd] = sg.first, hw[at.rc + nd] = sg.second;
      // build the child with the smaller GLOBAL hessian, derive the other
      const int l = t.left[nd], r = t.right[nd];
      const int build_left = tot[l][1] <= tot[r][1] ? 1 : 0;
      int32_t* h_sp = hw + at.sp + 4 * q;
      h_sp[0] = nd, h_sp[1] = sg.first, h_sp[2] = sg.second, h_sp[3] = build_left;
      hw[at.par + q] = k;
      small_len[q] = sg.second - sg.first;  // upper bound of the built child's rows
    }
    for (int i = 0; i < nt; ++i) hw[at.tb + i] = tiles[i][0], hw[at.tn + i] = tiles[i][1];
    auto dw32 = up.tensor().narrow(0, 0, at.nwords * 4).to(B.device(), true).view(torch::kInt32);
    up.mark(s);
    int32_t* d = ptr<int32_t>(dw32);
    const int32_t *d_feat = d + at.feat, *d_bin = d + at.bin, *d_sb = d + at.sb;
    const uint8_t* d_defl = reinterpret_cast<const uint8_t*>(d + at.defl);
    const int32_t *d_tb = d + at.tb, *d_tn = d + at.tn, *d_sp = d + at.sp;
    // the built children's histogram tasks, sized by the host-side bounds
    const HistPlan hplan = plan_hist(small_len);
    auto ridx_new = torch::empty_like(ridx);
    nleft_dev = torch::empty({nnode}, i32);
    if (!wh::gbdt_partition_cursor(ptr<uint8_t>(B), ptr<uint8_t>(Bc), B.size(0), F,
                                   ptr<int32_t>(ridx), n, d_tb, 1, d_tn, nt, d_feat, d_bin, d_defl,
                                   d + at.lc, d + at.rc, d_sb, nnode, ptr<int32_t>(nleft_dev),
                                   ptr<int32_t>(ridx_new), s)) {
      // position -> node map, flags, scan, per-node left counts, stable scatter
      auto pos_node = torch::empty({n}, i32);
      wh::gbdt_seg_fill(d_tb, d_tn, nt, n, ptr<int32_t>(pos_node), s);
      auto leftf = torch::empty({n}, i32);
      wh::gbdt_goleft(ptr<uint8_t>(B), ptr<uint8_t>(Bc), B.size(0), F, ptr<int32_t>(ridx), n,
                      ptr<int32_t>(pos_node), d_feat, d_bin, d_defl, ptr<int32_t>(leftf), s);
      nleft_dev = Tensor();  // (the counts themselves: no copy)
      partition_by_flags(ridx, pos_node, leftf, d_feat, dw32.narrow(0, at.sb, nnode),
                         dw32.narrow(0, at.se, nnode), &nleft_dev, ridx_new, s);
    }
    ridx = ridx_new;
    // built children's rows, from the device counts
    auto dseg = torch::empty({2 * nsplit}, i32);
    wh::gbdt_child_segs(d_sp, nsplit, ptr<int32_t>(nleft_dev), ptr<int32_t>(dseg), s);
    Tensor hs = run_hist(hplan, dseg);
    auto H_next = torch::empty({2 * nsplit, F, nbin, 2}, f64);
    wh::gbdt_sibling(ptr<double>(H_front), ptr<double>(hs), d_sp, d + at.par, nsplit, per,
                     ptr<double>(H_next), s);
    // next frontier [l, r] per split; unsplit frontier nodes are final leaves
    std::vector<int> nf;
    std::vector<bool> was_split(S, false);
    for (int q = 0; q < nsplit; ++q) {
      const int k = split_k[q], nd = frontier[k];
      was_split[k] = true;
      const auto sg = seg[nd];
      pending.push_back({nd, t.left[nd], t.right[nd], sg.first, sg.second});
      seg.erase(nd);
      nf.push_back(t.left[nd]), nf.push_back(t.right[nd]);
    }
    for (int k = 0; k < S; ++k)
      if (!was_split[k]) {
        const int nd = frontier[k];
        auto it = seg.find(nd);
        if (it != seg.end()) {
          segs.append(py::make_tuple(nd, it->second.first, it->second.second));
          seg.erase(it);
        }
      }
    frontier = nf;
    H_front = H_next;
  }
  if (!pending.empty())  // (a loop that ended right after a partition)
    resolve_pending(nleft_dev.cpu().data_ptr<int32_t>());
  for (auto& kv : seg) segs.append(py::make_tuple(kv.first, kv.second.first, kv.second.second));
  return py::make_tuple(t.pack(cut_vals, cut_off, segs), ridx);
}

// The same tree as gbdt_grow with the level loop on the device: heap-numbered
// nodes, the split decisions, partition set-up, child segments and the
// histogram task lists are written by kernels (gbdt.hip k_gd_apply /
// k_gd_children), so the host enqueues every level without waiting and reads
// the finished tree ONCE (gbdt_grow syncs once per level: ~1.5 ms of idle
// GPU per depth-8 tree of 11M rows). Every max_depth level is enqueued; the
// levels below a tree's last split find no live node and do no row work but
// the partition's pass.
// A device grower's heap node table (host copy, float64 [2^(D+1) - 1, REC])
// -> the tree lists, renumbered breadth-first: (feat, bin, cond, defl, left,
// right, parent, gain, cover, base weight, leaf, [(leaf id, begin, end)])
py::tuple gbdt_tree_from_nodes(const Tensor& hn, const std::vector<float>& cut_vals,
                               const std::vector<int64_t>& cut_off) {
  const int REC = wh::gbdt_node_rec();
  TORCH_CHECK(!hn.is_cuda() && hn.scalar_type() == torch::kFloat64 && hn.is_contiguous() &&
                  hn.dim() == 2 && hn.size(1) == REC,
              "gbdt_tree_from_nodes: a host float64 node table");
  const int NN = (int)hn.size(0);
  const double* r = hn.data_ptr<double>();
  std::vector<int> id_of(NN, -1), order;
  for (int h = 0; h < NN; ++h)
    if (r[(int64_t)h * REC] != 0.0) {
      id_of[h] = (int)order.size();
      order.push_back(h);
    }
  TreeLists t;
  py::list segs;
  for (size_t i = 0; i < order.size(); ++i) t.add(-1);
  for (size_t i = 0; i < order.size(); ++i) {
    const int h = order[i];
    const double* q = r + (int64_t)h * REC;
    t.feat[i] = (int)q[1], t.bin[i] = (int)q[2], t.defl[i] = (int)q[3];
    t.gain[i] = q[4], t.cover[i] = q[5], t.bw[i] = q[6], t.leaf[i] = q[7];
    if (t.feat[i] >= 0) {
      TORCH_CHECK(2 * h + 2 < NN, "gbdt_tree_from_nodes: a split at the last depth");
      const int l = t.left[i] = id_of[2 * h + 1], rt = t.right[i] = id_of[2 * h + 2];
      TORCH_CHECK(l >= 0 && rt >= 0, "gbdt_tree_from_nodes: a split node lost a child");
      t.parent[l] = (int)i, t.parent[rt] = (int)i;
    } else {
      segs.append(py::make_tuple((int)i, (int)q[8], (int)q[9]));
    }
  }
  return t.pack(cut_vals, cut_off, segs);
}

// margin += the leaf value each row reaches in a device grower's node table
// (device float64 [NN, REC]): the table becomes the walk's compact arrays on
// the device (one small kernel, to_arrays: wh::gbdt_heap_tree for the level
// loop's heap table, wh::gbdt_leaf_tree for the leaf loop's), then the usual
// row walk
void walk_nodes(decltype(&wh::gbdt_heap_tree) to_arrays, const Tensor& B, const Tensor& nodes,
                const Tensor& margin, bool lds) {
  const int64_t NN = nodes.size(0);
  auto buf = torch::empty({6 * NN}, B.options().dtype(torch::kInt32));
  int32_t* b = ptr<int32_t>(buf);
  int32_t *feat = b, *bin = b + NN, *left = b + 2 * NN, *right = b + 3 * NN;
  float* leaf = reinterpret_cast<float*>(b + 4 * NN);
  uint8_t* defl = reinterpret_cast<uint8_t*>(b + 5 * NN);
  auto s = cur_stream(B);
  to_arrays(ptr<double>(nodes), (int)NN, feat, bin, defl, left, right, leaf, s);
  wh::gbdt_leaf_walk(ptr<uint8_t>(B), B.size(0), (int)B.size(1), (int)NN, feat, bin, defl, left,
                     right, leaf, ptr<float>(margin), s, lds);
}

void gbdt_walk_heap(const Tensor& B, const Tensor& nodes, const Tensor& margin, bool lds) {
  CHECK_IN(B, torch::kUInt8);
  CHECK_IN(nodes, torch::kFloat64);
  CHECK_IN(margin, torch::kFloat32);
  const int REC = wh::gbdt_node_rec();
  TORCH_CHECK(nodes.dim() == 2 && nodes.size(1) == REC && nodes.size(0) > 0 &&
                  nodes.size(0) <= 65535,
              "gbdt_walk_heap: a heap node table");
  TORCH_CHECK(B.dim() == 2 && margin.numel() == B.size(0), "gbdt_walk_heap: B must be [n, f]");
  c10::DeviceGuard g(B.device());
  walk_nodes(wh::gbdt_heap_tree, B, nodes, margin, lds);
}

py::tuple gbdt_grow_dev(const Tensor& B, const Tensor& Bc, const Tensor& ridx0, const Tensor& gpair,
                        const Tensor& qscale, const Tensor& valid, int64_t nbin,
                        std::vector<std::pair<int64_t, int64_t>> fgroups, int64_t max_fcnt,
                        const Tensor& root_tot, std::vector<float> cut_vals,
                        std::vector<int64_t> cut_off, double eta, double alpha, double lambda,
                        double mcw, int64_t max_depth, double rt_eps, py::object allreduce,
                        py::object reduce_scatter, py::object pick, int64_t f_lo, bool walk,
                        bool defer, const c10::optional<Tensor>& mono,
                        const c10::optional<Tensor>& fmask, double max_delta_step) {
  // Multi-rank: either every level's built histograms are allreduced (all
  // features on every rank), or -- reduce_scatter / pick given
  // (models/gbdt.py HistExchange) -- each rank receives the global sums of
  // its feature slice [f_lo, f_lo + Fl) only, keeps the node histograms of
  // that slice, searches its features, and the per-slot best candidates are
  // reduced over the ranks by `pick`.
  CHECK_IN(root_tot, torch::kFloat64);  // {sum g, sum h} stays on the device: no host wait
  TORCH_CHECK(root_tot.numel() == 2, "gbdt_grow_dev: root totals are {sum g, sum h}");
  const GrowCtx cx(B, Bc, ridx0, gpair, qscale, valid, nbin, fgroups, max_fcnt);
  TORCH_CHECK(max_depth >= 0 && max_depth <= 10, "gbdt_grow_dev: max_depth in [0, 10]");
  c10::DeviceGuard g(B.device());
  const auto s = cx.s;
  const int64_t n = cx.n;
  const int F = cx.F, G = cx.G, chunk = cx.chunk;
  const auto &f64 = cx.f64, &i32 = cx.i32, &u8 = cx.u8;
  const bool shard = !reduce_scatter.is_none();
  TORCH_CHECK(!shard || !pick.is_none(), "gbdt_grow_dev: reduce_scatter needs pick");
  // monotone_constraints: mono [F] int8 (all features: the split search reads
  // this rank's slice, the apply kernel the picked, global feature) and the
  // slots' weight intervals, ping-ponged level by level like the totals
  const GrowCons cons(mono, fmask, max_delta_step, B, F, "gbdt_grow_dev");
  const bool mono_on = cons.mono_on, inter_on = cons.inter_on;
  Tensor bounds_cur;
  if (mono_on) {
    // the root's interval: max_delta_step on either side of 0, else unbounded
    bounds_cur = torch::empty({1, 2}, f64);
    bounds_cur.select(1, 0).fill_(-cons.top);
    bounds_cur.select(1, 1).fill_(cons.top);
  }
  // interaction_constraints: fmask [F] int64 (all features, as mono) and the
  // slots' group sets, ping-ponged like the weight intervals
  const auto i64 = f64.dtype(torch::kInt64);
  Tensor state_cur;
  if (inter_on) state_cur = torch::full({1}, (int64_t)wh::kGbdtInterRoot, i64);
  const bool reduce = shard || !allreduce.is_none();
  // rank partials -> global sums: all features, or this rank's slice
  auto reduce_hist = [&](Tensor h) -> Tensor {
    if (!reduce) return h;
    if (!shard) {
      allreduce(h);
      return h;
    }
    Tensor r = reduce_scatter(h).cast<Tensor>();
    TORCH_CHECK(r.scalar_type() == torch::kFloat64 && r.is_contiguous() &&
                    r.device() == h.device() && r.dim() == 4 && r.size(0) == h.size(0) &&
                    r.size(1) <= F && f_lo + r.size(1) <= F,
                "gbdt_grow_dev: reduce_scatter returned a bad slice");
    return r;
  };
  const int D = (int)max_depth, NN = (2 << D) - 1, Smax = 1 << D, REC = wh::gbdt_node_rec();
  // one small upload: root segment, feature groups, slot iota, then the root
  // histogram's task list -- the same for every tree of a model, so kept
  // per (device, rows, depth, groups) instead of uploaded per tree
  std::vector<int32_t> hw;
  hw.reserve(3 + 2 * G + Smax);
  hw.push_back(0), hw.push_back((int32_t)n), hw.push_back(1);
  for (auto& fg : fgroups) hw.push_back((int32_t)fg.first), hw.push_back((int32_t)fg.second);
  for (int i = 0; i < Smax; ++i) hw.push_back(i);
  std::vector<int32_t> root_tasks, root_red;
  wh::gbdt_hist_plan({n}, fgroups, chunk, &root_tasks, &root_red);
  const int64_t nt_root = (int64_t)root_tasks.size() / 5;
  root_tasks.insert(root_tasks.end(), root_red.begin(), root_red.end());
  // (never destroyed: device tensors must not be freed by static teardown)
  static auto& upload_cache = *new std::map<std::vector<int32_t>, std::pair<Tensor, Tensor>>();
  std::vector<int32_t> ukey = hw;
  ukey.push_back((int32_t)B.device().index());
  ukey.push_back(D);
  auto uit = upload_cache.find(ukey);
  if (uit == upload_cache.end()) {
    if (upload_cache.size() > 16) upload_cache.clear();
    auto a = torch::from_blob(hw.data(), {(int64_t)hw.size()}, torch::kInt32).to(B.device());
    auto b = torch::from_blob(root_tasks.data(), {(int64_t)root_tasks.size()}, torch::kInt32)
                 .to(B.device());
    uit = upload_cache.emplace(ukey, std::make_pair(a, b)).first;
  }
  auto hdev = uit->second.first;
  const int32_t* d_root_seg = ptr<int32_t>(hdev);
  const int32_t* d_fg = d_root_seg + 3;
  const int32_t* d_iota = d_fg + 2 * G;
  Tensor tot_cur = root_tot;
  Tensor seg_cur = hdev.narrow(0, 0, 2);
  Tensor alive_cur = hdev.narrow(0, 2, 1).view(torch::kUInt8).narrow(0, 0, 1);  // (= 1: the root)
  auto nodes = torch::empty({NN, REC}, f64);  // every depth's apply writes all its slots' records
  const uint8_t* vp = reinterpret_cast<const uint8_t*>(valid.data_ptr());
  Tensor ridx = ridx0;
  // root histogram: the host's task list over [0, n)
  Tensor H_front;
  {
    const Tensor& d = uit->second.second;
    H_front = torch::empty({1, F, nbin, 2}, f64);
    cx.run(ridx, ptr<int32_t>(d), nt_root, ptr<int32_t>(d) + nt_root * 5, G, cx.part(nt_root),
           H_front, ptr<int32_t>(seg_cur));
    H_front = reduce_hist(H_front);
  }
  const int Fl = (int)H_front.size(1);  // features of the node histograms kept here
  const int64_t per = (int64_t)Fl * nbin * 2;
  for (int d = 0; d <= D; ++d) {
    const int S = 1 << d;
    const bool last = d == D;
    Tensor so;
    if (!last) {
      so = torch::empty({S, 6}, f64);
      if (Fl > 0) {
        TORCH_CHECK(split_search(H_front, ptr<double>(tot_cur), vp + (int64_t)f_lo * nbin, S, alpha,
                                 lambda, mcw, so, s, cons.at(bounds_cur, state_cur, 0, f_lo)),
                    "gbdt_split failed");
      } else {  // (more ranks than features: this rank owns none)
        so.zero_();
        so.select(1, 0).fill_(-std::numeric_limits<double>::infinity());
      }
      if (shard) {
        so.select(1, 1).add_((double)f_lo);  // global feature ids
        so = pick(so).cast<Tensor>().contiguous();
        TORCH_CHECK(so.scalar_type() == torch::kFloat64 && so.size(0) == S && so.size(1) == 6,
                    "gbdt_grow_dev: pick returned a bad candidate table");
      }
    }
    auto pi = torch::empty({4 * S}, i32);  // pfeat | pbin | lcur | rcur
    auto pb = torch::empty({3 * S}, u8);   // pdefl | split | build_left
    Tensor tot_next = last ? Tensor() : torch::empty({2 * S, 2}, f64);
    Tensor bounds_next = last || !mono_on ? Tensor() : torch::empty({2 * S, 2}, f64);
    Tensor state_next = last || !inter_on ? Tensor() : torch::empty({2 * S}, i64);
    int32_t* pfeat = ptr<int32_t>(pi);
    uint8_t* pdefl = ptr<uint8_t>(pb);
    wh::gbdt_dev_apply(S, S - 1, last, last ? nullptr : ptr<double>(so), ptr<double>(tot_cur),
                       ptr<int32_t>(seg_cur), ptr<uint8_t>(alive_cur), eta, alpha, lambda, mcw,
                       rt_eps, ptr<double>(nodes), pfeat, pfeat + S, pdefl, pfeat + 2 * S,
                       pfeat + 3 * S, pdefl + S, pdefl + 2 * S,
                       last ? nullptr : ptr<double>(tot_next), nullptr, s,
                       cons.step(bounds_cur, state_cur, bounds_next, state_next));
    if (last) break;
    // walk: the caller adds the leaf values by walking the tree over each
    // row's bins (models/gbdt.py _finish), so the level whose children are
    // the max-depth leaves needs neither their rows partitioned nor their
    // histograms (never split): only the children's totals (from the split
    // search, above) and the node table (~9 % of a depth-8 tree)
    const bool leaves_next = walk && d + 1 == D;
    // partition of the split slots' rows on the device segment table (the
    // segment begins read in place from seg_cur's {begin, end} pairs; the
    // children read the left cursors: no copy, no count kernel)
    auto ridx_new = leaves_next ? ridx : torch::empty_like(ridx);
    if (n > 0 && !leaves_next)
      TORCH_CHECK(wh::gbdt_partition_cursor(ptr<uint8_t>(B), ptr<uint8_t>(Bc), B.size(0), F,
                                            ptr<int32_t>(ridx), n, ptr<int32_t>(seg_cur), 2, d_iota,
                                            S, pfeat, pfeat + S, pdefl, pfeat + 2 * S, pfeat + 3 * S,
                                            nullptr, S, nullptr, ptr<int32_t>(ridx_new), s),
                  "gbdt_grow_dev: partition refused the segment table");
    ridx = ridx_new;
    // next level's segments, the built children, their histogram tasks
    const int64_t ub = ((n + chunk - 1) / chunk + S) * G;  // >= the tasks of the built children
    auto seg_next = torch::empty({4 * S}, i32);
    auto alive_next = torch::empty({2 * S}, u8);
    auto dseg = torch::empty({2 * S}, i32);
    auto sp = torch::empty({5 * S + 1}, i32);  // sp [S x 4] | par [S] | ntask
    auto tasks = torch::empty({std::max<int64_t>(ub, 1) * 5}, i32);
    auto red = torch::empty({(int64_t)S * G * 6}, i32);
    TORCH_CHECK(wh::gbdt_dev_children(S, ptr<int32_t>(seg_cur), pdefl + S, pdefl + 2 * S,
                                      pfeat + 2 * S, d_fg, G, chunk, ptr<int32_t>(seg_next),
                                      ptr<uint8_t>(alive_next), ptr<int32_t>(dseg),
                                      ptr<int32_t>(sp), ptr<int32_t>(sp) + 4 * S, ptr<int32_t>(tasks),
                                      ptr<int32_t>(sp) + 5 * S, ptr<int32_t>(red), s),
                "gbdt_grow_dev: too many slots");
    if (leaves_next) {  // (leaf segments: left child empty -- unused by the walk)
      tot_cur = tot_next;
      bounds_cur = bounds_next;
      state_cur = state_next;
      seg_cur = seg_next;
      alive_cur = alive_next;
      continue;
    }
    const int64_t ntask = std::max<int64_t>(ub, 1);  // (the count itself: sp's last word)
    auto part = cx.part(ntask);
    auto H_next = torch::empty({2 * S, Fl, nbin, 2}, f64);
    if (!reduce) {  // one rank: the reduce writes both children (no hs, no sibling launch)
      cx.run(ridx, ptr<int32_t>(tasks), ntask, ptr<int32_t>(red), S * G, part, H_next,
             ptr<int32_t>(dseg), ptr<int32_t>(sp) + 5 * S, ptr<double>(H_front),
             ptr<int32_t>(sp), ptr<int32_t>(sp) + 4 * S);
    } else {
      auto hs = torch::empty({S, F, nbin, 2}, f64);
      cx.run(ridx, ptr<int32_t>(tasks), ntask, ptr<int32_t>(red), S * G, part, hs,
             ptr<int32_t>(dseg), ptr<int32_t>(sp) + 5 * S);
      hs = reduce_hist(hs);
      wh::gbdt_sibling(ptr<double>(H_front), ptr<double>(hs), ptr<int32_t>(sp),
                       ptr<int32_t>(sp) + 4 * S, S, per, ptr<double>(H_next), s);
    }
    H_front = H_next;
    tot_cur = tot_next;
    bounds_cur = bounds_next;
    state_cur = state_next;
    seg_cur = seg_next;
    alive_cur = alive_next;
  }
  // the finished tree: ONE host read, renumbered breadth-first (the host
  // grower's creation order) -- or, defer: the device node table itself, for
  // a heap walk on the device (gbdt_walk_heap) and a host read one tree later
  // (gbdt_tree_from_nodes), so the host's tree bookkeeping overlaps the next
  // tree instead of idling the GPU between trees
  if (defer) return py::make_tuple(nodes, ridx);
  return py::make_tuple(gbdt_tree_from_nodes(nodes.cpu(), cut_vals, cut_off), ridx);
}

// A leaf loop's node table (host float64 [NN, REC], explicit child ids) as
// the growers' tuple, renumbered breadth-first (host/gbdt_leaf_plan.h)
py::tuple gbdt_leaf_tree_from_nodes(const Tensor& hn, const std::vector<float>& cut_vals,
                                    const std::vector<int64_t>& cut_off) {
  const int REC = wh::gbdt_node_rec();
  TORCH_CHECK(!hn.is_cuda() && hn.scalar_type() == torch::kFloat64 && hn.is_contiguous() &&
                  hn.dim() == 2 && hn.size(1) == REC && hn.size(0) >= 1,
              "gbdt_leaf_tree_from_nodes: a host float64 node table");
  wh::GbdtLeafTree lt;
  TORCH_CHECK(wh::gbdt_leaf_tree_lists(hn.data_ptr<double>(), hn.size(0), REC, &lt),
              "gbdt_leaf_tree_from_nodes: the node table is no tree");
  const int64_t F = (int64_t)cut_off.size() - 1;
  for (size_t i = 0; i < lt.feat.size(); ++i)
    TORCH_CHECK(lt.feat[i] < 0 || (lt.feat[i] < F && lt.bin[i] >= 0 &&
                                   cut_off[lt.feat[i]] + lt.bin[i] < cut_off[lt.feat[i] + 1]),
                "gbdt_leaf_tree_from_nodes: a split outside the cuts");
  TreeLists t;
  t.feat = lt.feat, t.bin = lt.bin, t.defl = lt.defl, t.left = lt.left, t.right = lt.right;
  t.parent = lt.parent, t.gain = lt.gain, t.cover = lt.cover, t.bw = lt.bw, t.leaf = lt.leaf;
  py::list segs;
  for (auto& sg : lt.segs) segs.append(py::make_tuple(sg[0], sg[1], sg[2]));
  return t.pack(cut_vals, cut_off, segs);
}

// grow_policy=lossguide on the device (gbdt.hip "the best-first leaf loop"):
// max_leaves - 1 steps of pick-and-apply, segment partition, children,
// smaller-child histogram with the fused sibling step and a two-slot split
// search, all enqueued without a host wait; the node table is read once. One
// rank, the dense matrix. walk_margin: when given, the leaf values are added
// to it by a row walk from the device table before that read (the caller
// neither prunes nor refreshes). Returns (the tree's lists, the final ridx:
// every leaf's rows contiguous).
py::tuple gbdt_grow_leaf(const Tensor& B, const Tensor& Bc, const Tensor& ridx0, const Tensor& gpair,
                         const Tensor& qscale, const Tensor& valid, int64_t nbin,
                         std::vector<std::pair<int64_t, int64_t>> fgroups, int64_t max_fcnt,
                         const Tensor& root_tot, std::vector<float> cut_vals,
                         std::vector<int64_t> cut_off, double eta, double alpha, double lambda,
                         double mcw, int64_t max_leaves, int64_t depth_cap, double rt_eps,
                         const c10::optional<Tensor>& mono, const c10::optional<Tensor>& fmask,
                         double max_delta_step, const c10::optional<Tensor>& walk_margin,
                         bool lds) {
  CHECK_IN(root_tot, torch::kFloat64);
  TORCH_CHECK(root_tot.numel() == 2, "gbdt_grow_leaf: root totals are {sum g, sum h}");
  const GrowCtx cx(B, Bc, ridx0, gpair, qscale, valid, nbin, fgroups, max_fcnt);
  TORCH_CHECK(max_leaves >= 1 && max_leaves <= wh::kLeafMaxLeaves && depth_cap >= 1 &&
                  depth_cap <= wh::kLeafDepthCap,
              "gbdt_grow_leaf: max_leaves in [1, 32768], depth_cap in [1, ", wh::kLeafDepthCap, "]");
  c10::DeviceGuard g(B.device());
  const auto s = cx.s;
  const int64_t n = cx.n;
  const int F = cx.F, G = cx.G, chunk = cx.chunk;
  const auto &f64 = cx.f64, &i32 = cx.i32;
  TORCH_CHECK(n > 0 && B.size(0) == n && G >= 1, "gbdt_grow_leaf: B must be [n, f], n > 0");
  const GrowCons cons(mono, fmask, max_delta_step, B, F, "gbdt_grow_leaf");
  const int L = (int)max_leaves, NN = (int)wh::gbdt_leaf_pool_slots(L), REC = wh::gbdt_node_rec();
  const int WS = wh::gbdt_leaf_ws();
  const int64_t per = (int64_t)F * nbin * 2;
  // feature groups and the root histogram's task list: the same for every
  // tree of a model, uploaded once per (device, rows, groups)
  std::vector<int32_t> hw;
  for (auto& fg : fgroups) hw.push_back((int32_t)fg.first), hw.push_back((int32_t)fg.second);
  std::vector<int32_t> root_tasks, root_red;
  wh::gbdt_hist_plan({n}, fgroups, chunk, &root_tasks, &root_red);
  const int64_t nt_root = (int64_t)root_tasks.size() / 5;
  hw.insert(hw.end(), root_tasks.begin(), root_tasks.end());
  hw.insert(hw.end(), root_red.begin(), root_red.end());
  static auto& upload_cache = *new std::map<std::vector<int32_t>, Tensor>();
  std::vector<int32_t> ukey = hw;
  ukey.push_back((int32_t)B.device().index());
  ukey.push_back((int32_t)n);
  auto uit = upload_cache.find(ukey);
  if (uit == upload_cache.end()) {
    if (upload_cache.size() > 16) upload_cache.clear();
    uit = upload_cache
              .emplace(ukey, torch::from_blob(hw.data(), {(int64_t)hw.size()}, torch::kInt32)
                                 .to(B.device()))
              .first;
  }
  const int32_t* d_fg = ptr<int32_t>(uit->second);
  const int32_t* d_root_tasks = d_fg + 2 * G;
  const int32_t* d_root_red = d_root_tasks + nt_root * 5;
  // the tables, indexed by node id; so starts at -inf so that a node nobody
  // searched can never be picked
  auto nodes = torch::zeros({NN, REC}, f64);
  auto so = torch::full({NN, 6}, -std::numeric_limits<double>::infinity(), f64);
  auto tot = torch::zeros({NN, 2}, f64);
  auto meta = torch::zeros({NN, 4}, i32);
  auto ws = torch::zeros({WS}, i32);
  Tensor bnd = cons.mono_on ? torch::zeros({NN, 2}, f64) : Tensor();
  Tensor state = cons.inter_on ? torch::zeros({NN}, f64.dtype(torch::kInt64)) : Tensor();
  auto pool = torch::empty({NN, F, nbin, 2}, f64);  // a node's histogram: slot = node id
  const wh::GbdtCons tables = cons.step(bnd, state, bnd, state);  // in place
  wh::gbdt_leaf_root(ptr<double>(root_tot), (int)n, cons.top, (uint64_t)wh::kGbdtInterRoot, eta,
                     alpha, lambda, mcw, ptr<double>(tot), ptr<int32_t>(meta), ptr<double>(nodes), s,
                     tables);
  const uint8_t* vp = reinterpret_cast<const uint8_t*>(valid.data_ptr());
  Tensor ridx = ridx0.clone();  // partitioned in place, segment by segment
  auto search = [&](int node0, int S) {
    TORCH_CHECK(split_search(pool.narrow(0, node0, S), ptr<double>(tot) + 2 * node0, vp, S, alpha,
                             lambda, mcw, so.narrow(0, node0, S), s, cons.at(bnd, state, node0)),
                "gbdt_split failed");
  };
  if (L > 1) {
    // (the root's {begin, end} = {0, n}: its meta entry, written by gbdt_leaf_root)
    cx.run(ridx, d_root_tasks, nt_root, d_root_red, G, cx.part(nt_root), pool.narrow(0, 0, 1),
           ptr<int32_t>(meta) + 2);
    search(0, 1);
  }
  // a step's built child has at most ceil(n / chunk) + 1 chunks
  const int64_t ub = ((n + chunk - 1) / chunk + 1) * G;
  auto scratch = torch::empty_like(ridx);
  auto tasks = torch::empty({ub * 5}, i32);
  auto red = torch::empty({(int64_t)G * 6}, i32);
  auto part = L > 1 ? cx.part(ub) : Tensor();
  int32_t* d_ws = ptr<int32_t>(ws);
  for (int k = 0; k + 1 < L; ++k) {
    const bool last = k + 2 == L;  // the tree is full after this step
    wh::gbdt_leaf_pick(k, (int)depth_cap, last, ptr<double>(so), ptr<double>(tot),
                       ptr<int32_t>(meta), eta, alpha, lambda, mcw, rt_eps, ptr<double>(nodes),
                       d_ws, s, tables);
    wh::gbdt_leaf_partition(ptr<uint8_t>(B), ptr<uint8_t>(Bc), B.size(0), F, ptr<int32_t>(ridx), n,
                            d_ws, ptr<int32_t>(scratch), s);
    wh::gbdt_leaf_children(d_ws, ptr<int32_t>(meta), ptr<double>(nodes), d_fg, G, chunk,
                           ptr<int32_t>(tasks), ptr<int32_t>(red), s);
    if (last) break;  // nothing reads the children's histograms or splits
    const int l = (int)wh::gbdt_leaf_left(k);
    cx.run(ridx, ptr<int32_t>(tasks), ub, ptr<int32_t>(red), G, part, pool.narrow(0, l, 2),
           d_ws + 18, d_ws + 17, ptr<double>(pool), d_ws + 12, d_ws + 16);
    search(l, 2);
  }
  if (present(walk_margin)) {
    const Tensor& margin = *walk_margin;
    CHECK_IN(margin, torch::kFloat32);
    TORCH_CHECK(margin.numel() == n, "gbdt_grow_leaf: walk_margin must be [n]");
    walk_nodes(wh::gbdt_leaf_tree, B, nodes, margin, lds);
  }
  return py::make_tuple(gbdt_leaf_tree_from_nodes(nodes.cpu(), cut_vals, cut_off), ridx);
}

}  // namespace

void bind_gbdt(py::module_& m) {
  m.def("gbdt_bin", &gbdt_bin);
  m.def("gbdt_hist", &gbdt_hist, py::arg("B"), py::arg("nbin"), py::arg("ridx"), py::arg("gpair"),
        py::arg("qscale"), py::arg("tasks"), py::arg("red"), py::arg("max_fcnt"), py::arg("hist"));
  m.def("gbdt_partition", &gbdt_partition, py::arg("B"), py::arg("ridx"), py::arg("pos_node"),
        py::arg("node_feat"), py::arg("node_bin"), py::arg("node_defl"), py::arg("seg_beg"),
        py::arg("seg_end"), py::arg("nleft"), py::arg("Bc") = py::none());
  m.def("gbdt_seg_fill", &gbdt_seg_fill);
  m.def("gbdt_split", &gbdt_split, py::arg("hist"), py::arg("totals"), py::arg("valid"),
        py::arg("alpha"), py::arg("reg_lambda"), py::arg("min_child_weight"),
        py::arg("mono") = py::none(), py::arg("bounds") = py::none(),
        py::arg("fmask") = py::none(), py::arg("state") = py::none());
  m.def("gbdt_leaf_add", &gbdt_leaf_add);
  m.def("gbdt_leaf_walk", &gbdt_leaf_walk, py::arg("B"), py::arg("feat"), py::arg("bin"),
        py::arg("defl"), py::arg("left"), py::arg("right"), py::arg("val"), py::arg("margin"),
        py::arg("lds") = true, "margins += the tree's leaf per row (lds: the LDS-resident walk "
        "when the tree and row tile fit; else the global-memory walk)");
  m.def("gbdt_predict", &gbdt_predict);
  // every argument named: the Python side calls these by keyword (a dropped
  // argument fails on the CPU signature test, tests/test_native_signatures.py)
  m.def("gbdt_grow", &gbdt_grow, py::arg("B"), py::arg("Bc"), py::arg("ridx0"), py::arg("gpair"),
        py::arg("qscale"), py::arg("valid"), py::arg("nbin"), py::arg("fgroups"), py::arg("max_fcnt"),
        py::arg("root_tot"), py::arg("cut_vals"), py::arg("cut_off"), py::arg("eta"), py::arg("alpha"),
        py::arg("reg_lambda"), py::arg("min_child_weight"), py::arg("max_depth"), py::arg("rt_eps"),
        py::arg("allreduce"), py::arg("mono") = py::none(), py::arg("fmask") = py::none(),
        py::arg("max_delta_step") = 0.0);
  m.def("gbdt_grow_dev", &gbdt_grow_dev, py::arg("B"), py::arg("Bc"), py::arg("ridx0"), py::arg("gpair"),
        py::arg("qscale"), py::arg("valid"), py::arg("nbin"), py::arg("fgroups"), py::arg("max_fcnt"),
        py::arg("root_tot"), py::arg("cut_vals"), py::arg("cut_off"), py::arg("eta"), py::arg("alpha"),
        py::arg("reg_lambda"), py::arg("min_child_weight"), py::arg("max_depth"), py::arg("rt_eps"),
        py::arg("allreduce"), py::arg("reduce_scatter") = py::none(), py::arg("pick") = py::none(),
        py::arg("f_lo") = 0, py::arg("walk") = false, py::arg("defer") = false,
        py::arg("mono") = py::none(), py::arg("fmask") = py::none(),
        py::arg("max_delta_step") = 0.0);
  m.def("gbdt_grow_leaf", &gbdt_grow_leaf, py::arg("B"), py::arg("Bc"), py::arg("ridx0"),
        py::arg("gpair"), py::arg("qscale"), py::arg("valid"), py::arg("nbin"), py::arg("fgroups"),
        py::arg("max_fcnt"), py::arg("root_tot"), py::arg("cut_vals"), py::arg("cut_off"),
        py::arg("eta"), py::arg("alpha"), py::arg("reg_lambda"), py::arg("min_child_weight"),
        py::arg("max_leaves"), py::arg("depth_cap"), py::arg("rt_eps"),
        py::arg("mono") = py::none(), py::arg("fmask") = py::none(),
        py::arg("max_delta_step") = 0.0, py::arg("walk_margin") = py::none(),
        py::arg("lds") = true);
  m.def("gbdt_leaf_tree_from_nodes", &gbdt_leaf_tree_from_nodes, py::arg("nodes"),
        py::arg("cut_vals"), py::arg("cut_off"));
  m.def("gbdt_tree_from_nodes", &gbdt_tree_from_nodes);
  m.def("gbdt_walk_heap", &gbdt_walk_heap, py::arg("B"), py::arg("nodes"), py::arg("margin"),
        py::arg("lds") = true);
  m.def("gbdt_gpair", &gbdt_gpair);
  m.def("gbdt_gpair_obj", &gbdt_gpair_obj, py::arg("margin"), py::arg("label"), py::arg("weight"),
        py::arg("objective"), py::arg("max_delta_step") = 0.0,
        py::arg("tweedie_variance_power") = 1.5, py::arg("huber_slope") = 1.0,
        py::arg("scale_pos_weight") = 1.0, py::arg("quantile_alpha") = 0.5);
  m.def("gbdt_quantile_eval", &gbdt_quantile_eval, py::arg("margin"), py::arg("label"),
        py::arg("weight"), py::arg("alphas"));
  // the adaptive objectives' leaf refresh, pass by pass
  m.def("gbdt_qsel_key", &gbdt_qsel_key, py::arg("ridx"), py::arg("label"), py::arg("at"),
        py::arg("weight") = py::none(), py::arg("keep") = py::none(),
        py::arg("scale") = py::none());
  m.def("gbdt_qsel_hist", &gbdt_qsel_hist, py::arg("key"), py::arg("u"), py::arg("seg_beg"),
        py::arg("seg_end"), py::arg("chunk"), py::arg("state"), py::arg("radix_pass"));
  m.def("gbdt_qsel_pick", &gbdt_qsel_pick, py::arg("hist"), py::arg("state"), py::arg("radix_pass"),
        py::arg("alpha"));
  m.def("gbdt_qsel_value", &gbdt_qsel_value, py::arg("state"));
  m.def("gbdt_obj_eval", &gbdt_obj_eval, py::arg("margin"), py::arg("label"), py::arg("weight"),
        py::arg("link"), py::arg("mask"), py::arg("tweedie_variance_power") = 1.5,
        py::arg("huber_slope") = 1.0);
  // survival: the plan and the tile need no GPU
  m.def("gbdt_cox_plan", &gbdt_cox_plan, py::arg("label"), py::arg("weight") = py::none());
  m.def("gbdt_cox_tile", &wh::gbdt_cox_tile);
  m.def("gbdt_gpair_cox", &gbdt_gpair_cox, py::arg("margin"), py::arg("order"), py::arg("delta"),
        py::arg("weight"), py::arg("run_events"), py::arg("ws"), py::arg("ticket"));
  m.def("gbdt_cox_scan_stages", &gbdt_cox_scan_stages, py::arg("margin"), py::arg("order"),
        py::arg("delta"), py::arg("run_events"), py::arg("ws"), py::arg("ticket"),
        py::arg("stages"));
  m.def("gbdt_cox_eval", &gbdt_cox_eval, py::arg("margin"), py::arg("order"), py::arg("delta"),
        py::arg("run_events"), py::arg("ws"), py::arg("ticket"));
  m.def("gbdt_gpair_aft", &gbdt_gpair_aft, py::arg("margin"), py::arg("lower"), py::arg("upper"),
        py::arg("weight"), py::arg("dist"), py::arg("sigma") = 1.0);
  m.def("gbdt_aft_eval", &gbdt_aft_eval, py::arg("margin"), py::arg("lower"), py::arg("upper"),
        py::arg("weight"), py::arg("dist"), py::arg("sigma") = 1.0);
  m.def("gbdt_gpair_softmax", &gbdt_gpair_softmax);
  m.def("gbdt_softmax_out", &gbdt_softmax_out);
  m.def("gbdt_multi_eval", &gbdt_multi_eval);
  m.def("gbdt_qscale", &gbdt_qscale);
  m.def("gbdt_bin_csr", &gbdt_bin_csr);
  m.def("gbdt_hist_csr", &gbdt_hist_csr);
  m.def("gbdt_split_csr", &gbdt_split_csr, py::arg("hist"), py::arg("totals"), py::arg("cut_off"),
        py::arg("fvalid"), py::arg("alpha"), py::arg("reg_lambda"), py::arg("min_child_weight"),
        py::arg("mono") = py::none(), py::arg("bounds") = py::none(),
        py::arg("fmask") = py::none(), py::arg("state") = py::none());
  m.def("gbdt_partition_csr", &gbdt_partition_csr);
  m.def("gbdt_predict_csr", &gbdt_predict_csr);
  // forest prediction: pack, plan and the capacity need no GPU
  m.def("gbdt_forest_pack", &gbdt_forest_pack, py::arg("feat"), py::arg("cond"), py::arg("left"),
        py::arg("right"), py::arg("defl"), py::arg("leaf"));
  m.def("gbdt_forest_plan", &gbdt_forest_plan, py::arg("tree_sizes"), py::arg("lds_nodes"));
  m.def("gbdt_forest_lds_nodes", &wh::gbdt_forest_lds_nodes);
  m.def("gbdt_predict_forest", &gbdt_predict_forest, py::arg("X"), py::arg("nodes"),
        py::arg("tree_off"), py::arg("chunks"), py::arg("max_feat"), py::arg("out"),
        py::arg("leaf") = false);
  m.def("gbdt_predict_forest_csr", &gbdt_predict_forest_csr, py::arg("row_off"), py::arg("fid"),
        py::arg("val"), py::arg("nodes"), py::arg("tree_off"), py::arg("chunks"), py::arg("out"),
        py::arg("leaf") = false);
  // DART dropout walk: pack, plan and the budget need no GPU
  m.def("gbdt_dart_pack", &gbdt_dart_pack, py::arg("feat"), py::arg("bin"), py::arg("cond"),
        py::arg("left"), py::arg("right"), py::arg("defl"), py::arg("leaf"), py::arg("cut_vals"),
        py::arg("cut_off"));
  m.def("gbdt_dart_plan", &gbdt_dart_plan, py::arg("tree_sizes"), py::arg("sel"),
        py::arg("lds_nodes"));
  m.def("gbdt_dart_lds_nodes", &wh::gbdt_dart_lds_nodes);
  m.def("gbdt_dart_max_f", [] { return (int64_t)wh::kDartMaxF; });
  m.def("gbdt_dart_max_trees", [] { return (int64_t)wh::kDartMaxTrees; });
  m.def("gbdt_leaf_limits", &gbdt_leaf_limits, py::arg("max_leaves"), py::arg("max_depth"));
  m.def("gbdt_leaf_depth_cap", &wh::gbdt_leaf_depth_cap);
  m.def("gbdt_dart_max_depth", [] { return (int64_t)wh::kDartMaxDepth; });
  m.def("gbdt_shap_max_path", [] { return (int64_t)wh::kShapMaxPath; });
  m.def("gbdt_leaf_max_leaves", [] { return (int64_t)wh::kLeafMaxLeaves; });
  m.def("gbdt_leaf_pick", &gbdt_leaf_pick, py::arg("node"), py::arg("depth"), py::arg("gain"),
        py::arg("rt_eps"), py::arg("depth_cap"));
  m.def("gbdt_dart_grid", &gbdt_dart_grid, py::arg("n"), py::arg("f"), py::arg("ntree"),
        py::arg("nnode"), py::arg("rows"));
  m.def("gbdt_dart_walk", &gbdt_dart_walk, py::arg("B"), py::arg("table"), py::arg("tree_off"),
        py::arg("tree_nn"), py::arg("stage_off"), py::arg("coef"), py::arg("out"),
        py::arg("rows"));
  // feature contributions: pack, plan, capacities and the host references
  // need no GPU
  m.def("gbdt_shap_pack", &gbdt_shap_pack, py::arg("feat"), py::arg("cond"), py::arg("left"),
        py::arg("right"), py::arg("defl"), py::arg("leaf"), py::arg("cover"),
        py::arg("num_class"), py::arg("lds_elems") = (int64_t)wh::kShapLdsElems);
  m.def("gbdt_shap_plan", &gbdt_shap_plan, py::arg("path_len"), py::arg("path_class"),
        py::arg("path_tree"), py::arg("lds_elems"));
  m.def("gbdt_shap_lds_elems", &wh::gbdt_shap_lds_elems);
  m.def("gbdt_shap_lds_cols", &wh::gbdt_shap_lds_cols);
  m.def("gbdt_shap_max_blocks", &gbdt_shap_max_blocks);
  m.def("gbdt_shap_rows", &gbdt_shap_rows, py::arg("feat"), py::arg("cond"), py::arg("left"),
        py::arg("right"), py::arg("defl"), py::arg("leaf"), py::arg("cover"),
        py::arg("num_class"), py::arg("base"), py::arg("X"), py::arg("approx") = false,
        py::arg("f32") = false);
  m.def("gbdt_shap_rows_csr", &gbdt_shap_rows_csr, py::arg("feat"), py::arg("cond"),
        py::arg("left"), py::arg("right"), py::arg("defl"), py::arg("leaf"), py::arg("cover"),
        py::arg("num_class"), py::arg("base"), py::arg("row_off"), py::arg("fid"), py::arg("val"),
        py::arg("approx") = false, py::arg("f32") = false);
  m.def("gbdt_shap", &gbdt_shap, py::arg("X"), py::arg("paths"), py::arg("elems"),
        py::arg("ecol"), py::arg("chunks"), py::arg("ncol"), py::arg("max_feat"), py::arg("out"));
  m.def("gbdt_shap_csr", &gbdt_shap_csr, py::arg("row_off"), py::arg("fid"), py::arg("val"),
        py::arg("paths"), py::arg("elems"), py::arg("ecol"), py::arg("chunks"), py::arg("ncol"),
        py::arg("out"));
  m.def("gbdt_shap_inter_lds_cols", &wh::gbdt_shap_inter_lds_cols);
  m.def("gbdt_shap_inter_rows", &gbdt_shap_inter_rows, py::arg("feat"), py::arg("cond"),
        py::arg("left"), py::arg("right"), py::arg("defl"), py::arg("leaf"), py::arg("cover"),
        py::arg("num_class"), py::arg("base"), py::arg("X"), py::arg("f32") = false);
  m.def("gbdt_shap_inter_rows_csr", &gbdt_shap_inter_rows_csr, py::arg("feat"), py::arg("cond"),
        py::arg("left"), py::arg("right"), py::arg("defl"), py::arg("leaf"), py::arg("cover"),
        py::arg("num_class"), py::arg("base"), py::arg("row_off"), py::arg("fid"), py::arg("val"),
        py::arg("f32") = false);
  m.def("gbdt_shap_inter", &gbdt_shap_inter, py::arg("X"), py::arg("paths"), py::arg("elems"),
        py::arg("ecol"), py::arg("chunks"), py::arg("ncol"), py::arg("max_feat"), py::arg("out"));
  m.def("gbdt_shap_inter_csr", &gbdt_shap_inter_csr, py::arg("row_off"), py::arg("fid"),
        py::arg("val"), py::arg("paths"), py::arg("elems"), py::arg("ecol"), py::arg("chunks"),
        py::arg("ncol"), py::arg("out"));
  m.def("gbdt_saabas", &gbdt_saabas, py::arg("X"), py::arg("nodes"), py::arg("tree_off"),
        py::arg("node_m"), py::arg("node_col"), py::arg("ncol"), py::arg("max_feat"),
        py::arg("out"));
  m.def("gbdt_saabas_csr", &gbdt_saabas_csr, py::arg("row_off"), py::arg("fid"), py::arg("val"),
        py::arg("nodes"), py::arg("tree_off"), py::arg("node_m"), py::arg("node_col"),
        py::arg("ncol"), py::arg("out"));
  m.def("gbdt_rank_plan", &gbdt_rank_plan, py::arg("group_off"), py::arg("n"),
        py::arg("lds_rows") = (int64_t)wh::kRankLdsRows);
  m.def("gbdt_rank_lds_rows", &wh::gbdt_rank_lds_rows);
  m.def("gbdt_gpair_rank", &gbdt_gpair_rank, py::arg("margin"), py::arg("label"),
        py::arg("group_off"), py::arg("small"), py::arg("block"), py::arg("tiled"),
        py::arg("block_rows"), py::arg("tiled_rows"), py::arg("ndcg"), py::arg("tile_rows") = 0);
  m.def("gbdt_rank_eval", &gbdt_rank_eval, py::arg("margin"), py::arg("label"),
        py::arg("group_off"), py::arg("small"), py::arg("block"), py::arg("tiled"),
        py::arg("block_rows"), py::arg("tiled_rows"), py::arg("kind"), py::arg("k"),
        py::arg("minus"),
        py::arg("tile_rows") = 0);
}

}  // namespace wh_bind
