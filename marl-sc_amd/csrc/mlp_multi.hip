// Per-agent policies (parameter_sharing: false, the reference schema's default: one RLModule per
// warehouse, ippo.py:106 / mappo.py:103) in one launch: P same-shaped MLPs with P weight sets over rows
// laid out [E envs][P policies], the MULTI instantiations of the kernel templates of mlp_kernels.hpp.
// The dispatch mirrors mlp.hip's (same hidden-size branches, pass forms and output-layer choice), so
// policy p's rows are bit-identical to launch_mlp{3,2}_relu on policy p's rows gathered contiguously.
//
// Work split: a wave owns 32 envs of one policy, a block 4 such tiles of the same policy (the VALU
// output layer stages one policy's w3 in LDS per block). The weight working set is P times the shared
// policy's (MAPPO actor [256, 256]: ~0.3 MB per policy, 4.9 MB at P = 16, more than one XCD's 4 MiB of
// L2), so the block order decides how many policies' weights an XCD's L2 sees -- blocks are observed
// (not promised) to be dealt round-robin over the 8 XCDs:
//   order 0, policy-major: block b -> policy b / nb, env block b % nb (every XCD sees every policy);
//   order 1, policy-minor: block b -> policy b % P, env block b / P (P a multiple of 8: a policy's
//            blocks are congruent mod 8, so an XCD sees P / 8 policies).
// MSC_MULTI_ORDER picks (read at each launch; default 1). tools/ab_multi.py measures both: policy-minor had
// the lower median in all eight isolated actor / critic timings at C3 and C5 (by 1 to 2 %, inside the
// spread of either) and no measurable difference in the rollout step (profiles/mlp_multi/ab_multi.txt).
// Correctness does not depend on placement.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "env.hpp"
#include "mlp_kernels.hpp"

namespace msc {

int mlp_multi_order() {
  const char* e = getenv("MSC_MULTI_ORDER");
  return (e && atoi(e) == 0) ? 0 : 1;
}

// blocks of 4 env tiles per policy times policies; 0 when the grid does not fit
static unsigned multi_grid(int64_t E, int NP) {
  const int64_t nb = ((E + 31) / 32 + 3) / 4;
  const int64_t g = nb * NP;
  return g > 0x7fffffff ? 0u : (unsigned)g;
}

hipError_t launch_mlp3_relu_multi(const float* x, int64_t E, int NP, int L, int H1, int H2, int KO, const float* w1p,
                                  const float* b1, const float* w2p, const float* b2, const float* w3p, const float* b3,
                                  float* out, const float* pre1, hipStream_t st, const MlpSample* smp) {
  if (E == 0) return hipSuccess;
  const MlpSample sm = smp ? *smp : MlpSample{};
  if (sm.act && mlp3_valu_outputs(KO) == 0) return hipErrorInvalidValue;  // sampling needs the VALU output layer
  const int KS1 = (L + 1) / 2;
  const unsigned g = multi_grid(E, NP);
  if (g == 0) return hipErrorInvalidValue;
  const dim3 grid(g), block(256);
  const int prio = mlp_prio() | (mlp_multi_order() << 1);
  const float4* w1 = reinterpret_cast<const float4*>(w1p);
  const float4* w2 = reinterpret_cast<const float4*>(w2p);
  const float4* w3 = reinterpret_cast<const float4*>(w3p);
#define MSC_MLP_LAUNCH_IL(NT1, NT2, P, WPE, VKO, IL)                                                                 \
  hipLaunchKernelGGL((mlp3_relu_kernel<NT1, NT2, P, WPE, VKO, IL, MlpSample, true>), grid, block, 0, st, x, E, L, KS1, \
                     w1, b1, w2, b2, w3, b3, KO, out, pre1, NP, prio, sm)
#define MSC_MLP_LAUNCH(NT1, NT2, P, WPE, VKO) MSC_MLP_LAUNCH_IL(NT1, NT2, P, WPE, VKO, false)
  const int vko = mlp3_valu_outputs(KO);
#define MSC_MLP_VKO(NT1, NT2, P, WPE)                                 \
  switch (vko) {                                                      \
    case 1: MSC_MLP_LAUNCH(NT1, NT2, P, WPE, 1); break;               \
    case 2: MSC_MLP_LAUNCH(NT1, NT2, P, WPE, 2); break;               \
    case 4: MSC_MLP_LAUNCH(NT1, NT2, P, WPE, 4); break;               \
    case 5: MSC_MLP_LAUNCH(NT1, NT2, P, WPE, 5); break;               \
    case 8: MSC_MLP_LAUNCH(NT1, NT2, P, WPE, 8); break;               \
    default: MSC_MLP_LAUNCH(NT1, NT2, P, WPE, 0); break;              \
  }
#define MSC_MLP_VKO_IL(NT1, NT2, P, WPE)                                 \
  switch (vko) {                                                         \
    case 1: MSC_MLP_LAUNCH_IL(NT1, NT2, P, WPE, 1, true); break;         \
    case 2: MSC_MLP_LAUNCH_IL(NT1, NT2, P, WPE, 2, true); break;         \
    case 4: MSC_MLP_LAUNCH_IL(NT1, NT2, P, WPE, 4, true); break;         \
    case 5: MSC_MLP_LAUNCH_IL(NT1, NT2, P, WPE, 5, true); break;         \
    case 8: MSC_MLP_LAUNCH_IL(NT1, NT2, P, WPE, 8, true); break;         \
    default: MSC_MLP_LAUNCH(NT1, NT2, P, WPE, 0); break;                 \
  }
  // the branches of launch_mlp3_relu (mlp.hip), form for form
  if (H1 == 256 && H2 == 256) {
    if (mlp_p8() == 41) MSC_MLP_VKO_IL(8, 8, 4, 1)
    else if (mlp_p8() == 21) MSC_MLP_VKO_IL(8, 8, 2, 1)
    else if (mlp_p8() == 8) MSC_MLP_VKO(8, 8, 8, 1)
    else if (mlp_p8() == 4) MSC_MLP_VKO(8, 8, 4, 2)
    else MSC_MLP_VKO(8, 8, 2, 2)
  } else if (H1 == 128 && H2 == 128) {
    MSC_MLP_VKO(4, 4, 4, 2)
  } else if (H1 == 64 && H2 == 64) {
    MSC_MLP_VKO(2, 2, 2, 4)
  } else if (H1 == 64 && H2 == 128) {
    MSC_MLP_VKO(2, 4, 2, 4)
  } else if (H1 == 64 && H2 == 256) {
    MSC_MLP_VKO(2, 8, 2, 4)
  } else if (H1 == 64 && H2 == 512) {
    MSC_MLP_VKO(2, 16, 2, 4)
  } else if (H1 == 128 && H2 == 64) {
    MSC_MLP_VKO(4, 2, 2, 2)
  } else if (H1 == 128 && H2 == 256) {
    MSC_MLP_VKO(4, 8, 4, 2)
  } else if (H1 == 128 && H2 == 512) {
    MSC_MLP_VKO(4, 16, 4, 2)
  } else if (H1 == 256 && H2 == 64) {
    MSC_MLP_VKO(8, 2, 2, 2)
  } else if (H1 == 256 && H2 == 128) {
    MSC_MLP_VKO(8, 4, 4, 2)
  } else if (H1 == 256 && H2 == 512) {
    MSC_MLP_VKO(8, 16, 8, 1)
  } else if (H1 == 512 && H2 == 64) {
    MSC_MLP_VKO(16, 2, 2, 1)
  } else if (H1 == 512 && H2 == 128) {
    MSC_MLP_VKO(16, 4, 4, 1)
  } else if (H1 == 512 && H2 == 256) {
    MSC_MLP_VKO(16, 8, 4, 1)
  } else if (H1 == 512 && H2 == 512) {
    MSC_MLP_VKO(16, 16, 4, 1)
  } else {
    return hipErrorInvalidValue;
  }
#undef MSC_MLP_VKO
#undef MSC_MLP_VKO_IL
#undef MSC_MLP_LAUNCH_IL
#undef MSC_MLP_LAUNCH
  return hipGetLastError();
}

hipError_t launch_mlp2_relu_multi(const float* x, int64_t E, int NP, int L, int H1, int KO, const float* w1p,
                                  const float* b1, const float* w3p, const float* b3, float* out, const float* pre1,
                                  hipStream_t st, const MlpSample* smp) {
  if (E == 0) return hipSuccess;
  if (!mlp2_supported(H1)) return hipErrorInvalidValue;
  const MlpSample sm = smp ? *smp : MlpSample{};
  if (sm.act && mlp3_valu_outputs(KO) == 0) return hipErrorInvalidValue;
  const int KS1 = (L + 1) / 2, NT1 = H1 / 32;
  const int TB = NT1 % 8 == 0 ? 8 : NT1 % 4 == 0 ? 4 : NT1 % 2 == 0 ? 2 : 1;
  const unsigned g = multi_grid(E, NP);
  if (g == 0) return hipErrorInvalidValue;
  const dim3 grid(g), block(256);
  const int prio = mlp_prio() | (mlp_multi_order() << 1);
  const float4* w1 = reinterpret_cast<const float4*>(w1p);
  const float4* w3 = reinterpret_cast<const float4*>(w3p);
  const int vko = mlp3_valu_outputs(KO);
  const size_t lds = vko > 0 ? (size_t)NT1 * 16 * 2 * 2 * sizeof(float4) : 0;
#define MSC_MLP2_LAUNCH(TBV, WPE, VKO)                                                                              \
  hipLaunchKernelGGL((mlp2_relu_kernel<TBV, WPE, VKO, MlpSample, true>), grid, block, lds, st, x, E, L, KS1, NT1, w1, \
                     b1, w3, b3, KO, out, pre1, NP, prio, sm)
#define MSC_MLP2_VKO(TBV, WPE)                  \
  switch (vko) {                                \
    case 1: MSC_MLP2_LAUNCH(TBV, WPE, 1); break; \
    case 2: MSC_MLP2_LAUNCH(TBV, WPE, 2); break; \
    case 4: MSC_MLP2_LAUNCH(TBV, WPE, 4); break; \
    case 5: MSC_MLP2_LAUNCH(TBV, WPE, 5); break; \
    case 8: MSC_MLP2_LAUNCH(TBV, WPE, 8); break; \
    default: MSC_MLP2_LAUNCH(TBV, WPE, 0); break; \
  }
  switch (TB) {  // the branches of launch_mlp2_relu (mlp.hip)
    case 8: MSC_MLP2_VKO(8, 2) break;
    case 4: MSC_MLP2_VKO(4, 4) break;
    case 2: MSC_MLP2_VKO(2, 4) break;
    default: MSC_MLP2_VKO(1, 4) break;
  }
#undef MSC_MLP2_VKO
#undef MSC_MLP2_LAUNCH
  return hipGetLastError();
}

}  // namespace msc
