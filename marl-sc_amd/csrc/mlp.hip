// Fused inference of the rollout's policy MLP: Linear -> ReLU -> Linear -> ReLU -> Linear
// (MLPArchitecture.build, src/algorithms/models/architectures/mlp.py:14-60, with the actor /
// critic configs of config_files/algorithms/{ippo,mappo}.yaml: hidden [256, 256] or [64, 64]) on
// the f32 MFMA of gfx950 (v_mfma_f32_32x32x2_f32: exact f32 products, f32 accumulation, the f32
// vector rate of 64 FLOP/clk/SIMD).
//
// One wave = 32 samples. Every layer is computed transposed, D = W * X^T (hidden units on the
// MFMA's row axis, samples on its column axis = the lane), because a 32x32 f32 accumulator holds
// column j on lane j & 31 and rows (r & 3) + 8 (r >> 2) + 4 (lane >> 5) in its 16 registers: used
// as the B operand of the next MFMA, register r of lane half h is exactly B[k = h][j] for the
// hidden pair {rho(r, 0), rho(r, 1)} of that tile. So the hidden activations never leave the
// registers (no LDS, no HBM round trip: hipBLASLt writes and re-reads 2 x 256 floats per sample),
// and only the weights are streamed, from L2, in the matching permuted k order: the host packs
// them once per weight version into lane-major fragments (w1p / w2p / w3p below) so that every
// weight load of a wave is one contiguous 1-KiB (float4 per lane) read.
//
// Per 32 samples at 34 -> 256 -> 256 -> 5: 8 x 17 + 8 x 128 + 128 MFMAs (the output layer padded
// to 32 rows), i.e. ~82 k MFMA cycles per wave. Biases initialise the accumulators, so every
// output is an f32 fma chain in k order (a different rounding order than hipBLASLt's: the
// tests compare with the torch layer sequence at f32 GEMM tolerance).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "env.hpp"
#include "mlp_kernels.hpp"  // mlp3_relu_kernel, mlp2_relu_kernel, sample_row

namespace msc {

// layer-2 output tiles per pass at 256 hidden units, 1 wave per SIMD: 41 (default) = passes of 4
// tiles with the VALU output layer of each pass interleaved into the next pass's MFMAs (IL; C3 MAPPO
// rollout 1.139 -> 1.093 ms per step beside the demand kernel, profiles/r06/ab_mlp_il.txt), 21 = the
// same with passes of 2, 8 = all of H2 in one pass and the output layer after it (rounds 2-5);
// 4 / 2 = passes of 4 / 2 without interleaving at 2 waves per SIMD (<= 256 VGPRs, spills; A/B).
// MSC_MLP_P8, read at each launch (a test compares the forms)
int mlp_p8() {
  const char* e = getenv("MSC_MLP_P8");
  const int v = e ? atoi(e) : 41;
  return (v == 8 || v == 4 || v == 2 || v == 41 || v == 21) ? v : 41;
}
// wave priority 3 (MSC_MLP_PRIO=0: default priority, A/B)
int mlp_prio() {
  static const int v = [] {
    const char* e = getenv("MSC_MLP_PRIO");
    return (e && atoi(e) == 0) ? 0 : 1;
  }();
  return v;
}

// outputs of the VALU output layer for KO outputs (0: MFMA output layer); MSC_MLP_V3=0 forces the
// MFMA one (A/B). The host's weight packing must agree: msc_mlp3_w3_layout reports it.
int mlp3_valu_outputs(int KO) {
  static const int off = [] {
    const char* e = getenv("MSC_MLP_V3");
    return (e && atoi(e) == 0) ? 1 : 0;
  }();
  if (off || KO > 8) return 0;
  return KO <= 2 ? KO : KO <= 4 ? 4 : KO == 5 ? 5 : 8;
}

hipError_t launch_mlp3_relu(const float* x, int64_t n, int L, int H1, int H2, int KO, const float* w1p, const float* b1,
                            const float* w2p, const float* b2, const float* w3p, const float* b3, float* out,
                            const float* pre1, int grp, hipStream_t st, const MlpSample* smp) {
  if (n == 0) return hipSuccess;
  const MlpSample sm = smp ? *smp : MlpSample{};
  if (sm.act && mlp3_valu_outputs(KO) == 0) return hipErrorInvalidValue;  // sampling needs the VALU output layer
  const int KS1 = (L + 1) / 2;
  const int64_t tiles = (n + 31) / 32;
  const dim3 grid((unsigned)((tiles + 3) / 4)), block(256);
  const float4* w1 = reinterpret_cast<const float4*>(w1p);
  const float4* w2 = reinterpret_cast<const float4*>(w2p);
  const float4* w3 = reinterpret_cast<const float4*>(w3p);
#define MSC_MLP_LAUNCH_IL(NT1, NT2, P, WPE, VKO, IL)                                                                   \
  hipLaunchKernelGGL((mlp3_relu_kernel<NT1, NT2, P, WPE, VKO, IL>), grid, block, 0, st, x, n, L, KS1, w1, b1, w2, b2,   \
                     w3, b3, KO, out, pre1, grp, mlp_prio(), sm)
#define MSC_MLP_LAUNCH(NT1, NT2, P, WPE, VKO) MSC_MLP_LAUNCH_IL(NT1, NT2, P, WPE, VKO, false)
  // the output layer on the VALU for KO <= 8 (VKO = 1, 2, 4, 5 or 8: the next supported count >= KO)
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
  // H1 held whole in registers, H2 in passes of P tiles; (NT1, P) sets the register budget
  // (16 NT1 + 24 P + ~48 per lane) and with it the waves per SIMD
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

// one hidden layer of H1 = 32 NT1 units (NT1 <= 32): TB tiles per group, the largest power of two
// <= 8 dividing NT1
bool mlp2_supported(int H1) { return H1 >= 32 && H1 <= 1024 && H1 % 32 == 0; }

hipError_t launch_mlp2_relu(const float* x, int64_t n, int L, int H1, int KO, const float* w1p, const float* b1,
                            const float* w3p, const float* b3, float* out, const float* pre1, int grp, hipStream_t st,
                            const MlpSample* smp) {
  if (n == 0) return hipSuccess;
  if (!mlp2_supported(H1)) return hipErrorInvalidValue;
  const MlpSample sm = smp ? *smp : MlpSample{};
  if (sm.act && mlp3_valu_outputs(KO) == 0) return hipErrorInvalidValue;
  const int KS1 = (L + 1) / 2, NT1 = H1 / 32;
  const int TB = NT1 % 8 == 0 ? 8 : NT1 % 4 == 0 ? 4 : NT1 % 2 == 0 ? 2 : 1;
  const int64_t tiles = (n + 31) / 32;
  const dim3 grid((unsigned)((tiles + 3) / 4)), block(256);
  const float4* w1 = reinterpret_cast<const float4*>(w1p);
  const float4* w3 = reinterpret_cast<const float4*>(w3p);
  const int vko = mlp3_valu_outputs(KO);
  const size_t lds = vko > 0 ? (size_t)NT1 * 16 * 2 * 2 * sizeof(float4) : 0;
#define MSC_MLP2_LAUNCH(TBV, WPE, VKO)                                                                              \
  hipLaunchKernelGGL((mlp2_relu_kernel<TBV, WPE, VKO>), grid, block, lds, st, x, n, L, KS1, NT1, w1, b1, w3, b3, KO, \
                     out, pre1, grp, mlp_prio(), sm)
#define MSC_MLP2_VKO(TBV, WPE)                  \
  switch (vko) {                                \
    case 1: MSC_MLP2_LAUNCH(TBV, WPE, 1); break; \
    case 2: MSC_MLP2_LAUNCH(TBV, WPE, 2); break; \
    case 4: MSC_MLP2_LAUNCH(TBV, WPE, 4); break; \
    case 5: MSC_MLP2_LAUNCH(TBV, WPE, 5); break; \
    case 8: MSC_MLP2_LAUNCH(TBV, WPE, 8); break; \
    default: MSC_MLP2_LAUNCH(TBV, WPE, 0); break; \
  }
  switch (TB) {
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
