// Fused inference of a mu / sigma-head actor (use_mu_sigma_head: the reference's MuSigmaHead,
// src/algorithms/models/architectures/mu_sigma_head.py:52-82, on an MLPArchitecture.build backbone,
// rlmodules/base.py:213-252): backbone -> dual head -> head activations and the log_std clamp ->
// optional action sampling, in one launch of the kernels of mlp_kernels.hpp.
//
// The backbone ends in a Linear with no activation and the two heads are Linear, so the host folds
// that Linear into the heads (marlsc/mlp.py:fold_head, f64, rounded once): the kernel sees the
// hidden layers of a plain actor and a 2 K-row output layer, which it runs on the VALU as 2 x VKO
// per-lane sums (K <= 8). This translation unit only instantiates the dual-head forms (EP = MlpMuSigma)
// of the form table in mlp_dispatch.hpp, beside mlp.hip's, so that the two compile in parallel; per-head
// widths 2, 4, 5 and 8 (K = 1 runs as 2, 3 as 4, 6 and 7 as 8).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mlp_dispatch.hpp"
#include "mlp_kernels.hpp"

namespace msc {

int mlp_head_width(int K) {
  if (K < 1 || K > 8 || mlp3_valu_outputs(K) == 0) return 0;  // (MSC_MLP_V3=0: no VALU output layer)
  return K <= 2 ? 2 : K <= 4 ? 4 : K == 5 ? 5 : 8;
}

// [256, 256]: the interleaved forms (MSC_MLP_P8 = 41, 21) and the one-pass form (8); the losing A/B
// forms (4, 2: two waves per SIMD, spills) have no dual-head variant
bool mlp3_head_supported(int H1, int H2) {
  if (!mlp_hidden_ok(H1) || !mlp_hidden_ok(H2)) return false;
  return !(H1 == 256 && H2 == 256 && (mlp_p8() == 4 || mlp_p8() == 2));
}

// one hidden layer: the staged head weights (H1 x stride floats) must fit the 32 KiB the single-head
// form uses at its largest (1024 units), i.e. up to 512 units for heads wider than 4
bool mlp2_head_supported(int H1, int width) {
  return mlp2_supported(H1) && width > 0 && (size_t)H1 * mlp_head_stride(width) * sizeof(float) <= 32768;
}

// f(form, VK): mlp3_relu_kernel's instantiation for hidden sizes [H1, H2] and K actions per head
template <class F>
static bool head3_choose(int H1, int H2, int K, F&& f) {
  const int vk = mlp_head_width(K);
  if (vk == 0 || !mlp3_head_supported(H1, H2)) return false;
  return mlp3_relu_form<false>(H1, H2, mlp_p8(),
                               [&](auto form) { dispatch_int_or<8, 2, 4, 5>(vk, [&](auto v) { f(form, v); }); });
}

// f(TB, VK, dynamic LDS bytes): mlp2_relu_kernel's, which stages the head weights in LDS
template <class F>
static bool head2_choose(int H1, int K, F&& f) {
  const int vk = mlp_head_width(K);
  if (!mlp2_head_supported(H1, vk)) return false;
  const size_t lds = (size_t)H1 * mlp_head_stride(vk) * sizeof(float);
  mlp2_form(H1 / 32, true, [&](auto tb) { dispatch_int_or<8, 2, 4, 5>(vk, [&](auto v) { f(tb, v, lds); }); });
  return true;
}

hipError_t launch_mlp3_musigma(const float* x, int64_t n, int L, int H1, int H2, int K, const float* w1p, const float* b1,
                               const float* w2p, const float* b2, const float* whp, const float* bh, const float* pre1,
                               int grp, hipStream_t st, const MlpMuSigma& ep) {
  if (n == 0) return hipSuccess;
  const MlpGeom g = mlp_geom(n, L);
  const bool found = head3_choose(H1, H2, K, [&](auto form, auto vk) {
    using Fm = decltype(form);
    hipLaunchKernelGGL((mlp3_relu_kernel<Fm::nt1, Fm::nt2, Fm::p, Fm::wpe, decltype(vk)::value, Fm::il, MlpMuSigma>),
                       dim3(g.grid), dim3(256), 0, st, x, n, L, g.KS1, mlp_f4(w1p), b1, mlp_f4(w2p), b2, mlp_f4(whp), bh,
                       K, nullptr, pre1, grp, g.prio, ep);
  });
  return found ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_mlp2_musigma(const float* x, int64_t n, int L, int H1, int K, const float* w1p, const float* b1,
                               const float* whp, const float* bh, const float* pre1, int grp, hipStream_t st,
                               const MlpMuSigma& ep) {
  if (n == 0) return hipSuccess;
  const MlpGeom g = mlp_geom(n, L);
  const bool found = head2_choose(H1, K, [&](auto tb, auto vk, size_t lds) {
    constexpr int TB = decltype(tb)::value;
    hipLaunchKernelGGL((mlp2_relu_kernel<TB, mlp2_relu_wpe(TB), decltype(vk)::value, MlpMuSigma>), dim3(g.grid),
                       dim3(256), lds, st, x, n, L, g.KS1, H1 / 32, mlp_f4(w1p), b1, mlp_f4(whp), bh, K, nullptr, pre1,
                       grp, g.prio, ep);
  });
  return found ? hipGetLastError() : hipErrorInvalidValue;
}

bool mlp_musigma_plan(int H1, int H2, int K, int64_t rows, MlpPlan* p) {
  *p = MlpPlan{};
  p->grid = mlp_geom(rows, 0).grid;
  if (H2 != 0)
    return head3_choose(H1, H2, K, [&](auto form, auto vk) {
      using Fm = decltype(form);
      p->nt1 = Fm::nt1, p->nt2 = Fm::nt2, p->p = Fm::p, p->wpe = Fm::wpe, p->il = Fm::il, p->width = vk;
    });
  return head2_choose(H1, K, [&](auto tb, auto vk, size_t lds) {
    p->nt1 = H1 / 32, p->tb = tb, p->wpe = mlp2_relu_wpe(tb), p->width = vk, p->lds = (int64_t)lds;
  });
}

}  // namespace msc
