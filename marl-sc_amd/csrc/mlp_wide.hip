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

#include "env.hpp"
#include "mlp_wide.hpp"

namespace msc {

bool mlp_wide_supported(int H1, int H2, int KO) {
  auto hs = [](int h) { return h == 64 || h == 128 || h == 256 || h == 512; };
  if (KO < 1 || KO > 128) return false;
  return H2 == 0 ? mlp2_supported(H1) : (hs(H1) && hs(H2));
}

// registers per lane (estimate: accumulators + double-buffered fragments + addressing): at most 256
// for two waves per SIMD, else one
constexpr int wide3_wpe(int NT1, int P, int NTO) { return 16 * (NT1 + P + NTO) + 8 * (P + NTO) + 48 <= 240 ? 2 : 1; }

hipError_t launch_mlp3_wide(const float* x, int64_t n, int L, int H1, int H2, int KO, const float* w1p, const float* b1,
                            const float* w2p, const float* b2, const float* w3p, const float* b3, float* out,
                            const float* pre1, int grp, hipStream_t st, const MlpSample* smp) {
  if (n == 0) return hipSuccess;
  if (H2 == 0 || !mlp_wide_supported(H1, H2, KO)) return hipErrorInvalidValue;
  const MlpSample sm = smp ? *smp : MlpSample{};
  const int KS1 = (L + 1) / 2;
  const int64_t tiles = (n + 31) / 32;
  const dim3 grid((unsigned)((tiles + 3) / 4)), block(256);
  const float4* w1 = reinterpret_cast<const float4*>(w1p);
  const float4* w2 = reinterpret_cast<const float4*>(w2p);
  const float4* w3 = reinterpret_cast<const float4*>(w3p);
  const int nto = (KO + 31) / 32;
#define MSC_WIDE3_LAUNCH(NT1, NT2, P, NTO)                                                                            \
  hipLaunchKernelGGL((mlp3_wide_kernel<NT1, NT2, P, wide3_wpe(NT1, P, NTO), NTO>), grid, block, 0, st, x, n, L, KS1, \
                     w1, b1, w2, b2, w3, b3, KO, out, pre1, grp, mlp_prio(), sm)
#define MSC_WIDE3(NT1, NT2, P)                          \
  switch (nto) {                                        \
    case 1: MSC_WIDE3_LAUNCH(NT1, NT2, P, 1); break;    \
    case 2: MSC_WIDE3_LAUNCH(NT1, NT2, P, 2); break;    \
    case 3: MSC_WIDE3_LAUNCH(NT1, NT2, P, 3); break;    \
    default: MSC_WIDE3_LAUNCH(NT1, NT2, P, 4); break;   \
  }
  // H1 whole in registers, H2 in passes of P tiles (2 where H1 alone takes 256 registers)
  if (H1 == 64 && H2 == 64) MSC_WIDE3(2, 2, 2)
  else if (H1 == 64 && H2 == 128) MSC_WIDE3(2, 4, 4)
  else if (H1 == 64 && H2 == 256) MSC_WIDE3(2, 8, 4)
  else if (H1 == 64 && H2 == 512) MSC_WIDE3(2, 16, 4)
  else if (H1 == 128 && H2 == 64) MSC_WIDE3(4, 2, 2)
  else if (H1 == 128 && H2 == 128) MSC_WIDE3(4, 4, 4)
  else if (H1 == 128 && H2 == 256) MSC_WIDE3(4, 8, 4)
  else if (H1 == 128 && H2 == 512) MSC_WIDE3(4, 16, 4)
  else if (H1 == 256 && H2 == 64) MSC_WIDE3(8, 2, 2)
  else if (H1 == 256 && H2 == 128) MSC_WIDE3(8, 4, 4)
  else if (H1 == 256 && H2 == 256) MSC_WIDE3(8, 8, 4)
  else if (H1 == 256 && H2 == 512) MSC_WIDE3(8, 16, 4)
  else if (H1 == 512 && H2 == 64) MSC_WIDE3(16, 2, 2)
  else if (H1 == 512 && H2 == 128) MSC_WIDE3(16, 4, 2)
  else if (H1 == 512 && H2 == 256) MSC_WIDE3(16, 8, 2)
  else if (H1 == 512 && H2 == 512) MSC_WIDE3(16, 16, 2)
  else return hipErrorInvalidValue;
#undef MSC_WIDE3
#undef MSC_WIDE3_LAUNCH
  return hipGetLastError();
}

// one hidden layer, two forms with the same accumulation order (bit-identical results):
// * up to 1,024 waves of 32 rows (at most one wave per SIMD of the chip exists, so nothing but the wave's
//   own prefetch hides an L2 round trip): groups of TB = 8 hidden tiles where the hidden size allows, 32
//   MFMAs per layer-1 k step behind each prefetch, one wave per SIMD (128 + 16 NTO accumulator registers);
// * more rows: groups of TB <= 4 (64 + 16 NTO accumulators), two waves per SIMD (the 64-KiB staging area
//   of four output tiles allows two blocks per CU).
constexpr int64_t WIDE2_DEEP_TILES = 1024;
hipError_t launch_mlp2_wide(const float* x, int64_t n, int L, int H1, int KO, const float* w1p, const float* b1,
                            const float* w3p, const float* b3, float* out, const float* pre1, int grp, hipStream_t st,
                            const MlpSample* smp) {
  if (n == 0) return hipSuccess;
  if (!mlp_wide_supported(H1, 0, KO)) return hipErrorInvalidValue;
  const MlpSample sm = smp ? *smp : MlpSample{};
  const int KS1 = (L + 1) / 2, NT1 = H1 / 32;
  const int64_t tiles = (n + 31) / 32;
  const int TB = (NT1 % 8 == 0 && tiles <= WIDE2_DEEP_TILES) ? 8 : NT1 % 4 == 0 ? 4 : NT1 % 2 == 0 ? 2 : 1;
  const dim3 grid((unsigned)((tiles + 3) / 4)), block(256);
  const float4* w1 = reinterpret_cast<const float4*>(w1p);
  const float4* w3 = reinterpret_cast<const float4*>(w3p);
  const int nto = (KO + 31) / 32;
#define MSC_WIDE2_LAUNCH(TBV, NTO)                                                                                  \
  hipLaunchKernelGGL((mlp2_wide_kernel<TBV, (TBV == 8 ? 1 : 2), NTO>), grid, block, 0, st, x, n, L, KS1, NT1, w1, b1, \
                     w3, b3, KO, out, pre1, grp, mlp_prio(), sm)
#define MSC_WIDE2(TBV)                           \
  switch (nto) {                                 \
    case 1: MSC_WIDE2_LAUNCH(TBV, 1); break;     \
    case 2: MSC_WIDE2_LAUNCH(TBV, 2); break;     \
    case 3: MSC_WIDE2_LAUNCH(TBV, 3); break;     \
    default: MSC_WIDE2_LAUNCH(TBV, 4); break;    \
  }
  switch (TB) {
    case 8: MSC_WIDE2(8) break;
    case 4: MSC_WIDE2(4) break;
    case 2: MSC_WIDE2(2) break;
    default: MSC_WIDE2(1) break;
  }
#undef MSC_WIDE2
#undef MSC_WIDE2_LAUNCH
  return hipGetLastError();
}

}  // namespace msc
