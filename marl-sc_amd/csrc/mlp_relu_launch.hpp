// Launchers of the plain-output kernels (mlp3_relu_kernel / mlp2_relu_kernel with EP = MlpSample) as
// templates over MULTI: mlp.hip instantiates the single-policy ones, mlp_multi.hip the per-agent ones, so
// the two compile in parallel and cannot pick different forms.
#pragma once
#include "mlp_dispatch.hpp"
#include "mlp_kernels.hpp"

namespace msc {

// f(form, VKO, IL): the instantiation for hidden sizes [H1, H2] and KO outputs. The output layer runs on
// the VALU for KO <= 8 (VKO = 1, 2, 4, 5 or 8: the next supported count >= KO) and on the MFMA otherwise
// (VKO = 0), which has no interleaved form. False: no kernel for these sizes.
template <class F>
bool mlp3_relu_choose(int H1, int H2, int KO, F&& f) {
  return mlp3_relu_form<true>(H1, H2, mlp_p8(), [&](auto form) {
    dispatch_int_or<0, 1, 2, 4, 5, 8>(mlp3_valu_outputs(KO), [&](auto vko) {
      f(form, vko, std::bool_constant<decltype(form)::il && (decltype(vko)::value > 0)>{});
    });
  });
}

// f(TB, VKO, dynamic LDS bytes): one hidden layer of H1 units; the VALU output layer stages w3 in LDS
template <class F>
bool mlp2_relu_choose(int H1, int KO, F&& f) {
  if (!mlp2_supported(H1)) return false;
  const int NT1 = H1 / 32, v = mlp3_valu_outputs(KO);
  const size_t lds = v > 0 ? (size_t)NT1 * 16 * 2 * 2 * sizeof(float4) : 0;
  mlp2_form(NT1, true, [&](auto tb) { dispatch_int_or<0, 1, 2, 4, 5, 8>(v, [&](auto vko) { f(tb, vko, lds); }); });
  return true;
}

// rows: per policy (MULTI: NP policies, one pre1 row per row) or in all (pre1 row per grp rows)
template <bool MULTI>
hipError_t launch_mlp3_relu_t(const float* x, int64_t rows, int grp, int L, int H1, int H2, int KO, const float* w1p,
                              const float* b1, const float* w2p, const float* b2, const float* w3p, const float* b3,
                              float* out, const float* pre1, hipStream_t st, const MlpSample* smp) {
  if (rows == 0) return hipSuccess;
  const MlpSample sm = smp ? *smp : MlpSample{};
  if (sm.act && mlp3_valu_outputs(KO) == 0) return hipErrorInvalidValue;  // sampling needs the VALU output layer
  const MlpGeom g = mlp_geom(rows, L, MULTI ? grp : 0);
  if (!g.ok) return hipErrorInvalidValue;
  const bool found = mlp3_relu_choose(H1, H2, KO, [&](auto form, auto vko, auto il) {
    using Fm = decltype(form);
    hipLaunchKernelGGL((mlp3_relu_kernel<Fm::nt1, Fm::nt2, Fm::p, Fm::wpe, decltype(vko)::value, decltype(il)::value,
                                         MlpSample, MULTI>),
                       dim3(g.grid), dim3(256), 0, st, x, rows, L, g.KS1, mlp_f4(w1p), b1, mlp_f4(w2p), b2, mlp_f4(w3p),
                       b3, KO, out, pre1, grp, g.prio, sm);
  });
  return found ? hipGetLastError() : hipErrorInvalidValue;
}

template <bool MULTI>
hipError_t launch_mlp2_relu_t(const float* x, int64_t rows, int grp, int L, int H1, int KO, const float* w1p,
                              const float* b1, const float* w3p, const float* b3, float* out, const float* pre1,
                              hipStream_t st, const MlpSample* smp) {
  if (rows == 0) return hipSuccess;
  const MlpSample sm = smp ? *smp : MlpSample{};
  if (sm.act && mlp3_valu_outputs(KO) == 0) return hipErrorInvalidValue;
  const MlpGeom g = mlp_geom(rows, L, MULTI ? grp : 0);
  if (!g.ok) return hipErrorInvalidValue;
  const bool found = mlp2_relu_choose(H1, KO, [&](auto tb, auto vko, size_t lds) {
    constexpr int TB = decltype(tb)::value;
    hipLaunchKernelGGL((mlp2_relu_kernel<TB, mlp2_relu_wpe(TB), decltype(vko)::value, MlpSample, MULTI>), dim3(g.grid),
                       dim3(256), lds, st, x, rows, L, g.KS1, H1 / 32, mlp_f4(w1p), b1, mlp_f4(w3p), b3, KO, out, pre1,
                       grp, g.prio, sm);
  });
  return found ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace msc
