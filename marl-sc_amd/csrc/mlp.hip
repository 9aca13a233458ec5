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
#include "mlp_relu_launch.hpp"  // the launchers over MULTI, instantiated here with MULTI = false

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
  return launch_mlp3_relu_t<false>(x, n, grp, L, H1, H2, KO, w1p, b1, w2p, b2, w3p, b3, out, pre1, st, smp);
}

// one hidden layer of H1 = 32 NT1 units (NT1 <= 32)
bool mlp2_supported(int H1) { return H1 >= 32 && H1 <= 1024 && H1 % 32 == 0; }

hipError_t launch_mlp2_relu(const float* x, int64_t n, int L, int H1, int KO, const float* w1p, const float* b1,
                            const float* w3p, const float* b3, float* out, const float* pre1, int grp, hipStream_t st,
                            const MlpSample* smp) {
  return launch_mlp2_relu_t<false>(x, n, grp, L, H1, KO, w1p, b1, w3p, b3, out, pre1, st, smp);
}

// what the launchers above (NP = 0) or mlp_multi.hip's (NP policies of `rows` rows each) would pick
bool mlp_relu_plan(int H1, int H2, int KO, int64_t rows, int NP, MlpPlan* p) {
  const MlpGeom g = mlp_geom(rows, 0, NP);
  *p = MlpPlan{};
  p->grid = g.grid;
  if (!g.ok) return false;
  if (H2 != 0)
    return mlp3_relu_choose(H1, H2, KO, [&](auto form, auto vko, auto il) {
      using Fm = decltype(form);
      p->nt1 = Fm::nt1, p->nt2 = Fm::nt2, p->p = Fm::p, p->wpe = Fm::wpe, p->il = il, p->width = vko;
    });
  return mlp2_relu_choose(H1, KO, [&](auto tb, auto vko, size_t lds) {
    p->nt1 = H1 / 32, p->tb = tb, p->wpe = mlp2_relu_wpe(tb), p->width = vko, p->lds = (int64_t)lds;
  });
}

}  // namespace msc
