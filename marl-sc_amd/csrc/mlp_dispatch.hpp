// Host-side choice of a fused-MLP instantiation, written once for the four launcher translation units
// (mlp.hip, mlp_multi.hip, mlp_musigma.hip, mlp_wide.hip): the hidden-size tables, the runtime integer ->
// template argument dispatch and the launch geometry. No kernel bodies and no HIP calls: a table hands
// the chosen form to a callable as a type, so a launcher passes a lambda that launches and msc_mlp_plan
// (capi.hip) reaches the same tables through a lambda that records (pinned on the CPU by
// tests/test_mlp_plan_host.py). All forms of a family give bit-identical results, so only that test and
// the clock can see a wrong entry here.
#pragma once
#include <stdint.h>

#include <type_traits>

#include "env.hpp"

namespace msc {

// hidden sizes of the two-hidden-layer kernels
inline bool mlp_hidden_ok(int h) { return h == 64 || h == 128 || h == 256 || h == 512; }

// NT1 / NT2: hidden tiles of 32 units; P: layer-2 output tiles per pass; WPE: waves per SIMD; IL: the
// VALU output layer of a pass interleaved into the next pass's MFMAs (mlp_kernels.hpp)
template <int NT1, int NT2, int P, int WPE, bool IL = false>
struct Mlp3Form {
  static constexpr int nt1 = NT1, nt2 = NT2, p = P, wpe = WPE;
  static constexpr bool il = IL;
};

// f(std::integral_constant<int, V>) for the V of Vs... equal to v, else for D
template <int D, int... Vs, class F>
void dispatch_int_or(int v, F&& f) {
  if (!((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...)) f(std::integral_constant<int, D>{});
}

// mlp3_relu_kernel's forms: H1 held whole in registers, H2 in passes of P tiles; (NT1, P) sets the
// register budget (16 NT1 + 24 P + ~48 per lane) and with it the waves per SIMD. p8 (MSC_MLP_P8) picks
// among the forms of [256, 256]. AB = false leaves out its two-waves-per-SIMD A/B forms (p8 = 4, 2):
// they are not instantiated and report false. False also for sizes outside the table.
template <bool AB, class F>
bool mlp3_relu_form(int H1, int H2, int p8, F&& f) {
  if (H1 == 256 && H2 == 256) {
    if (p8 == 41) f(Mlp3Form<8, 8, 4, 1, true>{});
    else if (p8 == 21) f(Mlp3Form<8, 8, 2, 1, true>{});
    else if (p8 == 8) f(Mlp3Form<8, 8, 8, 1>{});
    else if constexpr (AB) {
      if (p8 == 4) f(Mlp3Form<8, 8, 4, 2>{});
      else f(Mlp3Form<8, 8, 2, 2>{});
    } else return false;
  }
  else if (H1 == 128 && H2 == 128) f(Mlp3Form<4, 4, 4, 2>{});
  else if (H1 == 64 && H2 == 64) f(Mlp3Form<2, 2, 2, 4>{});
  else if (H1 == 64 && H2 == 128) f(Mlp3Form<2, 4, 2, 4>{});
  else if (H1 == 64 && H2 == 256) f(Mlp3Form<2, 8, 2, 4>{});
  else if (H1 == 64 && H2 == 512) f(Mlp3Form<2, 16, 2, 4>{});
  else if (H1 == 128 && H2 == 64) f(Mlp3Form<4, 2, 2, 2>{});
  else if (H1 == 128 && H2 == 256) f(Mlp3Form<4, 8, 4, 2>{});
  else if (H1 == 128 && H2 == 512) f(Mlp3Form<4, 16, 4, 2>{});
  else if (H1 == 256 && H2 == 64) f(Mlp3Form<8, 2, 2, 2>{});
  else if (H1 == 256 && H2 == 128) f(Mlp3Form<8, 4, 4, 2>{});
  else if (H1 == 256 && H2 == 512) f(Mlp3Form<8, 16, 8, 1>{});
  else if (H1 == 512 && H2 == 64) f(Mlp3Form<16, 2, 2, 1>{});
  else if (H1 == 512 && H2 == 128) f(Mlp3Form<16, 4, 4, 1>{});
  else if (H1 == 512 && H2 == 256) f(Mlp3Form<16, 8, 4, 1>{});
  else if (H1 == 512 && H2 == 512) f(Mlp3Form<16, 16, 4, 1>{});
  else return false;
  return true;
}

// mlp3_wide_kernel's forms (passes of 2 where H1 alone takes 256 registers); the waves per SIMD follow
// from the register estimate once the output tiles NTO are known: at most 256 per lane (accumulators +
// double-buffered fragments + addressing) for two waves, else one
constexpr int wide3_wpe(int NT1, int P, int NTO) { return 16 * (NT1 + P + NTO) + 8 * (P + NTO) + 48 <= 240 ? 2 : 1; }
template <int NT1, int NT2, int P>
struct WideForm {
  static constexpr int nt1 = NT1, nt2 = NT2, p = P;
};
template <class F>
bool mlp3_wide_form(int H1, int H2, F&& f) {
  if (H1 == 64 && H2 == 64) f(WideForm<2, 2, 2>{});
  else if (H1 == 64 && H2 == 128) f(WideForm<2, 4, 4>{});
  else if (H1 == 64 && H2 == 256) f(WideForm<2, 8, 4>{});
  else if (H1 == 64 && H2 == 512) f(WideForm<2, 16, 4>{});
  else if (H1 == 128 && H2 == 64) f(WideForm<4, 2, 2>{});
  else if (H1 == 128 && H2 == 128) f(WideForm<4, 4, 4>{});
  else if (H1 == 128 && H2 == 256) f(WideForm<4, 8, 4>{});
  else if (H1 == 128 && H2 == 512) f(WideForm<4, 16, 4>{});
  else if (H1 == 256 && H2 == 64) f(WideForm<8, 2, 2>{});
  else if (H1 == 256 && H2 == 128) f(WideForm<8, 4, 4>{});
  else if (H1 == 256 && H2 == 256) f(WideForm<8, 8, 4>{});
  else if (H1 == 256 && H2 == 512) f(WideForm<8, 16, 4>{});
  else if (H1 == 512 && H2 == 64) f(WideForm<16, 2, 2>{});
  else if (H1 == 512 && H2 == 128) f(WideForm<16, 4, 2>{});
  else if (H1 == 512 && H2 == 256) f(WideForm<16, 8, 2>{});
  else if (H1 == 512 && H2 == 512) f(WideForm<16, 16, 2>{});
  else return false;
  return true;
}

// one hidden layer of NT1 tiles, produced TB at a time: f(TB) with the largest power of two <= 8 dividing
// NT1 (deep = false: <= 4, the wide family's form past its deep-tiles threshold). The waves per SIMD of a
// TB are the family's: mlp2_relu_wpe for mlp2_relu_kernel, mlp2_wide_wpe for mlp2_wide_kernel.
template <class F>
void mlp2_form(int NT1, bool deep, F&& f) {
  dispatch_int_or<1, 8, 4, 2>((deep && NT1 % 8 == 0) ? 8 : NT1 % 4 == 0 ? 4 : NT1 % 2 == 0 ? 2 : 1, f);
}
constexpr int mlp2_relu_wpe(int TB) { return TB == 8 ? 2 : 4; }
constexpr int mlp2_wide_wpe(int TB) { return TB == 8 ? 1 : 2; }

// launch geometry: a wave owns a tile of 32 rows, a block of 256 threads 4 tiles. Multi-policy launches
// (NP > 0 policies over rows [E][NP]) have that many blocks per policy and carry the block order in
// prio bit 1 (mlp_kernels.hpp); ok = false when their grid does not fit
struct MlpGeom {
  int KS1;        // k steps of layer 1
  unsigned grid;  // blocks
  int prio;       // kernel argument
  bool ok;
};
inline int64_t mlp_tiles(int64_t rows) { return (rows + 31) / 32; }
inline int64_t mlp_blocks(int64_t rows, int NP) { return (mlp_tiles(rows) + 3) / 4 * (NP > 0 ? NP : 1); }
inline MlpGeom mlp_geom(int64_t rows, int L, int NP = 0) {
  const int64_t g = mlp_blocks(rows, NP);
  return {(L + 1) / 2, (unsigned)g, mlp_prio() | (NP > 0 ? mlp_multi_order() << 1 : 0), NP <= 0 || g <= 0x7fffffff};
}
inline const float4* mlp_f4(const float* p) { return reinterpret_cast<const float4*>(p); }

// what a launcher picked, as msc_mlp_plan reports it (unused fields stay 0)
struct MlpPlan {
  int nt1, nt2, p, wpe, il, width, tb;
  int64_t lds, grid;
};
// each family's launcher choice through a recording callable; false: no kernel (or the grid does not
// fit). rows: per policy for NP > 0 policies (mlp_multi.hip), H2 = 0: one hidden layer
bool mlp_relu_plan(int H1, int H2, int KO, int64_t rows, int NP, MlpPlan* p);
bool mlp_musigma_plan(int H1, int H2, int K, int64_t rows, MlpPlan* p);
bool mlp_wide_plan(int H1, int H2, int KO, int64_t rows, MlpPlan* p);

}  // namespace msc
