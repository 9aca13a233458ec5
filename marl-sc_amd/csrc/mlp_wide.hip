// Fused inference of a wide-output policy MLP: the centralised (CPPO) actor maps the global
// observation to the joint action, W L -> hidden -> W K (8 L -> 256 -> 40 at C3, 16 L -> 256 -> 80 at
// C5; the reference's cppo.py builds it from MLPArchitecture.build, architectures/mlp.py:14-60).
// mlp.hip's kernels stop at one 32-row output tile and sample only on the VALU output layer (<= 8
// outputs); here the output layer is ceil(out_dim / 32) <= 4 MFMA tiles (v_mfma_f32_32x32x2_f32) and
// the rollout's Gaussian sampling runs in an LDS-staged epilogue (mlp_wide.hpp). With one hidden
// layer the output layer is about as much work as the first (256 x 40 against 208 x 256 at C3), so
// it belongs on the MFMA: per 32 samples at 208 -> 256 -> 40, 8 x 104 + 2 x 128 MFMAs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mlp_dispatch.hpp"
#include "mlp_wide.hpp"

namespace msc {

bool mlp_wide_supported(int H1, int H2, int KO) {
  if (KO < 1 || KO > 128) return false;
  return H2 == 0 ? mlp2_supported(H1) : (mlp_hidden_ok(H1) && mlp_hidden_ok(H2));
}

// f(form, NTO): mlp3_wide_kernel's instantiation for hidden sizes [H1, H2] and ceil(KO / 32) output tiles
template <class F>
static bool wide3_choose(int H1, int H2, int KO, F&& f) {
  if (H2 == 0 || !mlp_wide_supported(H1, H2, KO)) return false;
  return mlp3_wide_form(H1, H2, [&](auto form) { dispatch_int_or<4, 1, 2, 3>((KO + 31) / 32, [&](auto nto) { f(form, nto); }); });
}

// one hidden layer, two forms with the same accumulation order (bit-identical results):
// * up to 1,024 waves of 32 rows (at most one wave per SIMD of the chip exists, so nothing but the wave's
//   own prefetch hides an L2 round trip): groups of TB = 8 hidden tiles where the hidden size allows, 32
//   MFMAs per layer-1 k step behind each prefetch, one wave per SIMD (128 + 16 NTO accumulator registers);
// * more rows: groups of TB <= 4 (64 + 16 NTO accumulators), two waves per SIMD (the 64-KiB staging area
//   of four output tiles allows two blocks per CU).
constexpr int64_t WIDE2_DEEP_TILES = 1024;
// f(TB, NTO)
template <class F>
static bool wide2_choose(int H1, int KO, int64_t n, F&& f) {
  if (!mlp_wide_supported(H1, 0, KO)) return false;
  mlp2_form(H1 / 32, mlp_tiles(n) <= WIDE2_DEEP_TILES,
            [&](auto tb) { dispatch_int_or<4, 1, 2, 3>((KO + 31) / 32, [&](auto nto) { f(tb, nto); }); });
  return true;
}

hipError_t launch_mlp3_wide(const float* x, int64_t n, int L, int H1, int H2, int KO, const float* w1p, const float* b1,
                            const float* w2p, const float* b2, const float* w3p, const float* b3, float* out,
                            const float* pre1, int grp, hipStream_t st, const MlpSample* smp) {
  if (n == 0) return hipSuccess;
  const MlpSample sm = smp ? *smp : MlpSample{};
  const MlpGeom g = mlp_geom(n, L);
  const bool found = wide3_choose(H1, H2, KO, [&](auto form, auto nto) {
    using Fm = decltype(form);
    constexpr int NTO = decltype(nto)::value;
    hipLaunchKernelGGL((mlp3_wide_kernel<Fm::nt1, Fm::nt2, Fm::p, wide3_wpe(Fm::nt1, Fm::p, NTO), NTO>), dim3(g.grid),
                       dim3(256), 0, st, x, n, L, g.KS1, mlp_f4(w1p), b1, mlp_f4(w2p), b2, mlp_f4(w3p), b3, KO, out, pre1,
                       grp, g.prio, sm);
  });
  return found ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_mlp2_wide(const float* x, int64_t n, int L, int H1, int KO, const float* w1p, const float* b1,
                            const float* w3p, const float* b3, float* out, const float* pre1, int grp, hipStream_t st,
                            const MlpSample* smp) {
  if (n == 0) return hipSuccess;
  const MlpSample sm = smp ? *smp : MlpSample{};
  const MlpGeom g = mlp_geom(n, L);
  const bool found = wide2_choose(H1, KO, n, [&](auto tb, auto nto) {
    constexpr int TB = decltype(tb)::value;
    hipLaunchKernelGGL((mlp2_wide_kernel<TB, mlp2_wide_wpe(TB), decltype(nto)::value>), dim3(g.grid), dim3(256), 0, st, x,
                       n, L, g.KS1, H1 / 32, mlp_f4(w1p), b1, mlp_f4(w3p), b3, KO, out, pre1, grp, g.prio, sm);
  });
  return found ? hipGetLastError() : hipErrorInvalidValue;
}

// the staging area is static LDS: no dynamic bytes
bool mlp_wide_plan(int H1, int H2, int KO, int64_t rows, MlpPlan* p) {
  *p = MlpPlan{};
  p->grid = mlp_geom(rows, 0).grid;
  if (H2 != 0)
    return wide3_choose(H1, H2, KO, [&](auto form, auto nto) {
      using Fm = decltype(form);
      p->nt1 = Fm::nt1, p->nt2 = Fm::nt2, p->p = Fm::p, p->wpe = wide3_wpe(Fm::nt1, Fm::p, nto), p->width = nto;
    });
  return wide2_choose(H1, KO, rows, [&](auto tb, auto nto) {
    p->nt1 = H1 / 32, p->tb = tb, p->wpe = mlp2_wide_wpe(tb), p->width = nto;
  });
}

}  // namespace msc
