// Bindings of the k-means family (module wormhole_amd._hip): packing, dense,
// split-precision and CSR assignment, accumulation, centroid update.
#include "bind_common.h"

namespace wh_bind {
namespace {

// ---------------------------------------------------------------- kmeans
Tensor kmeans_pack_x(const Tensor& X) {
  CHECK_IN(X, torch::kFloat32);
  TORCH_CHECK(X.dim() == 2, "X must be [n, f]");
  c10::DeviceGuard g(X.device());
  const int64_t n = X.size(0);
  const int f = (int)X.size(1);
  const int ks = wh::kmeans_ks(f);
  auto Xp = torch::empty({(n + 31) / 32 * ks * 64}, X.options());
  wh::kmeans_pack_x(ptr<float>(X), n, f, ptr<float>(Xp), cur_stream(X));
  return Xp;
}

Tensor kmeans_pack_c(const Tensor& C) {
  CHECK_IN(C, torch::kFloat32);
  TORCH_CHECK(C.dim() == 2, "C must be [k, f]");
  c10::DeviceGuard g(C.device());
  const int k = (int)C.size(0), f = (int)C.size(1);
  auto Cp = torch::empty({wh::kmeans_cp_elems(k, f)}, C.options());
  wh::kmeans_pack_c(ptr<float>(C), k, f, ptr<float>(Cp), cur_stream(C));
  return Cp;
}

std::vector<Tensor> kmeans_assign(const Tensor& Xp, int64_t n, int64_t f, const Tensor& Cp,
                                  int64_t k) {
  CHECK_IN(Xp, torch::kFloat32);
  CHECK_IN(Cp, torch::kFloat32);
  const int ks = wh::kmeans_ks((int)f);
  TORCH_CHECK(Xp.numel() == (n + 31) / 32 * ks * 64, "packed X size mismatch");
  TORCH_CHECK(Cp.numel() == wh::kmeans_cp_elems((int)k, (int)f), "packed C size mismatch");
  c10::DeviceGuard g(Xp.device());
  auto assign = torch::empty({n}, Xp.options().dtype(torch::kInt32));
  auto score = torch::empty({n}, Xp.options());
  wh::kmeans_assign(ptr<float>(Xp), n, (int)f, ptr<float>(Cp), (int)k, ptr<int32_t>(assign),
                    ptr<float>(score), cur_stream(Xp));
  return {assign, score};
}

// split precision: X [n, f] -> (packed bf16 hi/lo fragments (uint8), row norms)
std::vector<Tensor> kmeans_pack_x3(const Tensor& X) {
  CHECK_IN(X, torch::kFloat32);
  TORCH_CHECK(X.dim() == 2, "X must be [n, f]");
  c10::DeviceGuard g(X.device());
  const int64_t n = X.size(0);
  const int f = (int)X.size(1);
  TORCH_CHECK(wh::kmeans_x3_supported(f), "split-precision assign needs 1 <= f <= 128");
  auto Xp = torch::empty({wh::kmeans_x3_xp_bytes(n, f)}, X.options().dtype(torch::kUInt8));
  wh::kmeans_pack_x3(ptr<float>(X), n, f, Xp.data_ptr(), cur_stream(X));
  auto xn = X.norm(2, {1}).contiguous();
  return {Xp, xn};
}

Tensor kmeans_pack_c3(const Tensor& C) {
  CHECK_IN(C, torch::kFloat32);
  c10::DeviceGuard g(C.device());
  const int k = (int)C.size(0), f = (int)C.size(1);
  TORCH_CHECK(wh::kmeans_x3_supported(f), "split-precision assign needs 1 <= f <= 128");
  auto Cp = torch::empty({wh::kmeans_x3_cp_bytes(k, f)}, C.options().dtype(torch::kUInt8));
  wh::kmeans_pack_c3(ptr<float>(C), k, f, Cp.data_ptr(), cur_stream(C));
  return Cp;
}

// returns (assign i32 [n], score f32 [n], near-tie count (device i32 [1]))
std::vector<Tensor> kmeans_assign_x3(const Tensor& Xp, const Tensor& xnorm, const Tensor& X,
                                     const Tensor& Cp, const Tensor& C) {
  CHECK_IN(X, torch::kFloat32);
  CHECK_IN(C, torch::kFloat32);
  CHECK_IN(xnorm, torch::kFloat32);
  CHECK_DEV(Xp);
  CHECK_DEV(Cp);
  c10::DeviceGuard g(X.device());
  const int64_t n = X.size(0);
  const int f = (int)X.size(1), k = (int)C.size(0);
  TORCH_CHECK(C.size(1) == f && xnorm.numel() == n, "shape mismatch");
  TORCH_CHECK(Xp.numel() == wh::kmeans_x3_xp_bytes(n, f), "packed X size mismatch");
  TORCH_CHECK(Cp.numel() == wh::kmeans_x3_cp_bytes(k, f), "packed C size mismatch");
  auto assign = torch::empty({n}, X.options().dtype(torch::kInt32));
  auto score = torch::empty({n}, X.options());
  auto amb = torch::empty({n + 1}, X.options().dtype(torch::kInt32));
  auto ct = torch::empty({(int64_t)k * f}, X.options());
  wh::kmeans_assign_x3(Xp.data_ptr(), ptr<float>(xnorm), ptr<float>(X), n, f, Cp.data_ptr(),
                       ptr<float>(C), k, ptr<int32_t>(assign), ptr<float>(score),
                       ptr<int32_t>(amb), ptr<float>(ct), cur_stream(X));
  return {assign, score, amb.narrow(0, 0, 1)};
}

Tensor kmeans_accum(const Tensor& X, const Tensor& assign, int64_t k) {
  CHECK_IN(X, torch::kFloat32);
  CHECK_IN(assign, torch::kInt32);
  c10::DeviceGuard g(X.device());
  const int64_t n = X.size(0);
  const int f = (int)X.size(1);
  TORCH_CHECK(assign.numel() == n);
  auto sums = torch::zeros({k, f + 1}, X.options());
  // counting-sort path unless k / f are too large for it (then atomics)
  if (n > 0) {
    auto scratch = torch::empty({wh::kmeans_accum_scratch(n, (int)k)},
                                X.options().dtype(torch::kUInt8));
    if (wh::kmeans_accum_sorted(ptr<float>(X), n, f, (int)k, ptr<int32_t>(assign),
                                ptr<float>(sums), scratch.data_ptr(), cur_stream(X)))
      return sums;
  }
  wh::kmeans_accum(ptr<float>(X), n, f, ptr<int32_t>(assign), ptr<float>(sums), cur_stream(X));
  return sums;
}

// sparse k-means (CSR rows): offset int64 [n + 1] (offset[0] == 0), col int32
// [nnz] (all < F = Ct.size(0), checked by the caller once per dataset), val
// float [nnz] or None (all ones), Ct [F, Kp] float (transposed centroids)
Tensor kmeans_assign_csr(const Tensor& offset, const Tensor& col, const c10::optional<Tensor>& val,
                         const Tensor& Ct, int64_t K) {
  CHECK_IN(offset, torch::kInt64);
  CHECK_IN(col, torch::kInt32);
  CHECK_IN(Ct, torch::kFloat32);
  const int64_t n = offset.numel() - 1;
  TORCH_CHECK(n >= 0 && Ct.dim() == 2 && K >= 1 && Ct.size(1) >= K && Ct.size(1) % 4 == 0,
              "kmeans_assign_csr: Ct must be [F, Kp >= K], Kp % 4 == 0");
  const float* vp = nullptr;
  if (val.has_value() && val->defined()) {
    CHECK_IN((*val), torch::kFloat32);
    TORCH_CHECK(val->numel() == col.numel(), "kmeans_assign_csr: val / col size");
    vp = ptr<float>(*val);
  }
  c10::DeviceGuard g(Ct.device());
  auto assign = torch::empty({std::max<int64_t>(n, 0)}, Ct.options().dtype(torch::kInt32));
  wh::kmeans_assign_csr(ptr<int64_t>(offset), ptr<int32_t>(col), vp, n, ptr<float>(Ct), (int)K,
                        (int)Ct.size(1), ptr<int32_t>(assign), cur_stream(Ct));
  return assign;
}

Tensor kmeans_accum_csr(const Tensor& offset, const Tensor& col, const c10::optional<Tensor>& val,
                        const Tensor& assign, int64_t K, int64_t F) {
  CHECK_IN(offset, torch::kInt64);
  CHECK_IN(col, torch::kInt32);
  CHECK_IN(assign, torch::kInt32);
  const int64_t n = offset.numel() - 1;
  TORCH_CHECK(assign.numel() == n && K >= 1 && F >= 1, "kmeans_accum_csr: sizes");
  const float* vp = nullptr;
  if (val.has_value() && val->defined()) {
    CHECK_IN((*val), torch::kFloat32);
    vp = ptr<float>(*val);
  }
  c10::DeviceGuard g(col.device());
  auto sums = torch::zeros({K, F + 1}, col.options().dtype(torch::kFloat32));
  wh::kmeans_accum_csr(ptr<int64_t>(offset), ptr<int32_t>(col), vp, n, ptr<int32_t>(assign),
                       (int)F, ptr<float>(sums), cur_stream(col));
  return sums;
}

// (new C [k, f], empty-cluster count int64 [1]) from sums [k, f + 1] and C
std::vector<Tensor> kmeans_update(const Tensor& sums, const Tensor& C) {
  CHECK_IN(sums, torch::kFloat32);
  CHECK_IN(C, torch::kFloat32);
  TORCH_CHECK(C.dim() == 2 && sums.dim() == 2 && sums.size(0) == C.size(0) &&
                  sums.size(1) == C.size(1) + 1,
              "kmeans_update: sums must be [k, f + 1] for C [k, f]");
  c10::DeviceGuard g(C.device());
  auto out = torch::empty_like(C);
  auto nempty = torch::zeros({1}, C.options().dtype(torch::kInt64));
  wh::kmeans_update(ptr<float>(sums), ptr<float>(C), (int)C.size(0), (int)C.size(1),
                    ptr<float>(out), reinterpret_cast<unsigned long long*>(nempty.data_ptr()),
                    cur_stream(C));
  return {out, nempty};
}

}  // namespace

void bind_kmeans(py::module_& m) {
  m.def("kmeans_pack_x", &kmeans_pack_x);
  m.def("kmeans_pack_c", &kmeans_pack_c);
  m.def("kmeans_assign", &kmeans_assign);
  m.def("kmeans_accum", &kmeans_accum);
  m.def("kmeans_update", &kmeans_update);
  m.def("kmeans_assign_csr", &kmeans_assign_csr, py::arg("offset"), py::arg("col"),
        py::arg("val"), py::arg("Ct"), py::arg("K"));
  m.def("kmeans_accum_csr", &kmeans_accum_csr, py::arg("offset"), py::arg("col"), py::arg("val"),
        py::arg("assign"), py::arg("K"), py::arg("F"));
  m.def("kmeans_pack_x3", &kmeans_pack_x3);
  m.def("kmeans_pack_c3", &kmeans_pack_c3);
  m.def("kmeans_assign_x3", &kmeans_assign_x3);
}

}  // namespace wh_bind
