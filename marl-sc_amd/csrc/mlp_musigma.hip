// Fused inference of a mu / sigma-head actor (use_mu_sigma_head: the reference's MuSigmaHead,
// src/algorithms/models/architectures/mu_sigma_head.py:52-82, on an MLPArchitecture.build backbone,
// rlmodules/base.py:213-252): backbone -> dual head -> head activations and the log_std clamp ->
// optional action sampling, in one launch of the kernels of mlp_kernels.hpp.
//
// The backbone ends in a Linear with no activation and the two heads are Linear, so the host folds
// that Linear into the heads (marlsc/mlp.py:fold_head, f64, rounded once): the kernel sees the
// hidden layers of a plain actor and a 2 K-row output layer, which it runs on the VALU as 2 x VKO
// per-lane sums (K <= 8). This translation unit only instantiates the dual-head forms, beside
// mlp.hip's, so that the two compile in parallel; per-head widths 2, 4, 5 and 8 (K = 1 runs as 2,
// 3 as 4, 6 and 7 as 8).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "env.hpp"
#include "mlp_kernels.hpp"

namespace msc {

int mlp_head_width(int K) {
  if (K < 1 || K > 8 || mlp3_valu_outputs(K) == 0) return 0;  // (MSC_MLP_V3=0: no VALU output layer)
  return K <= 2 ? 2 : K <= 4 ? 4 : K == 5 ? 5 : 8;
}

// [256, 256]: the interleaved forms (MSC_MLP_P8 = 41, 21) and the one-pass form (8); the losing A/B
// forms (4, 2: two waves per SIMD, spills) have no dual-head variant
bool mlp3_head_supported(int H1, int H2) {
  auto hs = [](int v) { return v == 64 || v == 128 || v == 256 || v == 512; };
  if (!hs(H1) || !hs(H2)) return false;
  return !(H1 == 256 && H2 == 256 && (mlp_p8() == 4 || mlp_p8() == 2));
}

hipError_t launch_mlp3_musigma(const float* x, int64_t n, int L, int H1, int H2, int K, const float* w1p, const float* b1,
                               const float* w2p, const float* b2, const float* whp, const float* bh, const float* pre1,
                               int grp, hipStream_t st, const MlpMuSigma& ep) {
  if (n == 0) return hipSuccess;
  const int vk = mlp_head_width(K);
  if (vk == 0 || !mlp3_head_supported(H1, H2)) return hipErrorInvalidValue;
  const int KS1 = (L + 1) / 2;
  const int64_t tiles = (n + 31) / 32;
  const dim3 grid((unsigned)((tiles + 3) / 4)), block(256);
  const float4* w1 = reinterpret_cast<const float4*>(w1p);
  const float4* w2 = reinterpret_cast<const float4*>(w2p);
  const float4* wh = reinterpret_cast<const float4*>(whp);
#define MSC_HEAD_LAUNCH(NT1, NT2, P, WPE, VK, IL)                                                                   \
  hipLaunchKernelGGL((mlp3_relu_kernel<NT1, NT2, P, WPE, VK, IL, MlpMuSigma>), grid, block, 0, st, x, n, L, KS1, w1, \
                     b1, w2, b2, wh, bh, K, nullptr, pre1, grp, mlp_prio(), ep)
#define MSC_HEAD_VK(NT1, NT2, P, WPE, IL)                      \
  switch (vk) {                                                \
    case 2: MSC_HEAD_LAUNCH(NT1, NT2, P, WPE, 2, IL); break;   \
    case 4: MSC_HEAD_LAUNCH(NT1, NT2, P, WPE, 4, IL); break;   \
    case 5: MSC_HEAD_LAUNCH(NT1, NT2, P, WPE, 5, IL); break;   \
    default: MSC_HEAD_LAUNCH(NT1, NT2, P, WPE, 8, IL); break;  \
  }
  // the tile shapes of launch_mlp3_relu (mlp.hip)
  if (H1 == 256 && H2 == 256) {
    if (mlp_p8() == 41) MSC_HEAD_VK(8, 8, 4, 1, true)
    else if (mlp_p8() == 21) MSC_HEAD_VK(8, 8, 2, 1, true)
    else MSC_HEAD_VK(8, 8, 8, 1, false)
  } else if (H1 == 128 && H2 == 128) {
    MSC_HEAD_VK(4, 4, 4, 2, false)
  } else if (H1 == 64 && H2 == 64) {
    MSC_HEAD_VK(2, 2, 2, 4, false)
  } else if (H1 == 64 && H2 == 128) {
    MSC_HEAD_VK(2, 4, 2, 4, false)
  } else if (H1 == 64 && H2 == 256) {
    MSC_HEAD_VK(2, 8, 2, 4, false)
  } else if (H1 == 64 && H2 == 512) {
    MSC_HEAD_VK(2, 16, 2, 4, false)
  } else if (H1 == 128 && H2 == 64) {
    MSC_HEAD_VK(4, 2, 2, 2, false)
  } else if (H1 == 128 && H2 == 256) {
    MSC_HEAD_VK(4, 8, 4, 2, false)
  } else if (H1 == 128 && H2 == 512) {
    MSC_HEAD_VK(4, 16, 4, 2, false)
  } else if (H1 == 256 && H2 == 64) {
    MSC_HEAD_VK(8, 2, 2, 2, false)
  } else if (H1 == 256 && H2 == 128) {
    MSC_HEAD_VK(8, 4, 4, 2, false)
  } else if (H1 == 256 && H2 == 512) {
    MSC_HEAD_VK(8, 16, 8, 1, false)
  } else if (H1 == 512 && H2 == 64) {
    MSC_HEAD_VK(16, 2, 2, 1, false)
  } else if (H1 == 512 && H2 == 128) {
    MSC_HEAD_VK(16, 4, 4, 1, false)
  } else if (H1 == 512 && H2 == 256) {
    MSC_HEAD_VK(16, 8, 4, 1, false)
  } else {
    MSC_HEAD_VK(16, 16, 4, 1, false)
  }
#undef MSC_HEAD_VK
#undef MSC_HEAD_LAUNCH
  return hipGetLastError();
}

// one hidden layer: the staged head weights (H1 x stride floats) must fit the 32 KiB the single-head
// form uses at its largest (1024 units), i.e. up to 512 units for heads wider than 4
bool mlp2_head_supported(int H1, int width) {
  return mlp2_supported(H1) && width > 0 && (size_t)H1 * mlp_head_stride(width) * sizeof(float) <= 32768;
}

hipError_t launch_mlp2_musigma(const float* x, int64_t n, int L, int H1, int K, const float* w1p, const float* b1,
                               const float* whp, const float* bh, const float* pre1, int grp, hipStream_t st,
                               const MlpMuSigma& ep) {
  if (n == 0) return hipSuccess;
  const int vk = mlp_head_width(K);
  if (!mlp2_head_supported(H1, vk)) return hipErrorInvalidValue;
  const int KS1 = (L + 1) / 2, NT1 = H1 / 32;
  const int TB = NT1 % 8 == 0 ? 8 : NT1 % 4 == 0 ? 4 : NT1 % 2 == 0 ? 2 : 1;
  const int64_t tiles = (n + 31) / 32;
  const dim3 grid((unsigned)((tiles + 3) / 4)), block(256);
  const float4* w1 = reinterpret_cast<const float4*>(w1p);
  const float4* wh = reinterpret_cast<const float4*>(whp);
  const size_t lds = (size_t)H1 * mlp_head_stride(vk) * sizeof(float);
#define MSC_HEAD2_LAUNCH(TBV, WPE, VK)                                                                             \
  hipLaunchKernelGGL((mlp2_relu_kernel<TBV, WPE, VK, MlpMuSigma>), grid, block, lds, st, x, n, L, KS1, NT1, w1, b1, \
                     wh, bh, K, nullptr, pre1, grp, mlp_prio(), ep)
#define MSC_HEAD2_VK(TBV, WPE)                         \
  switch (vk) {                                        \
    case 2: MSC_HEAD2_LAUNCH(TBV, WPE, 2); break;      \
    case 4: MSC_HEAD2_LAUNCH(TBV, WPE, 4); break;      \
    case 5: MSC_HEAD2_LAUNCH(TBV, WPE, 5); break;      \
    default: MSC_HEAD2_LAUNCH(TBV, WPE, 8); break;     \
  }
  switch (TB) {
    case 8: MSC_HEAD2_VK(8, 2) break;
    case 4: MSC_HEAD2_VK(4, 4) break;
    case 2: MSC_HEAD2_VK(2, 4) break;
    default: MSC_HEAD2_VK(1, 4) break;
  }
#undef MSC_HEAD2_VK
#undef MSC_HEAD2_LAUNCH
  return hipGetLastError();
}

}  // namespace msc
