// demand_common.hpp -- pieces shared by the Poisson demand kernels (env_kernels.hip:
// demand_unit_kernel; demand_v3.hip: demand_v3_kernel; demand_seq.hip: demand_seq_kernel): the PCG64
// state I/O of the env's demand stream, the generator ring geometry and refill quota, the parser states, and the
// episode-ahead root derivation.
#pragma once
#include <hip/hip_runtime.h>

#include "env.hpp"
#include "kcommon.hpp"
#include "rng.hpp"

namespace msc {

__device__ __forceinline__ Pcg64 load_rng(const EnvState& s, int which, int64_t e, int64_t E) {
  Pcg64 r;
  const uint64_t* b = s.rng + (int64_t)which * 4 * E + e;
  r.s_hi = b[0];
  r.s_lo = b[E];
  r.i_hi = b[2 * E];
  r.i_lo = b[3 * E];
  r.has32 = s.rbuf[(int64_t)which * 2 * E + e];
  r.u32 = s.rbuf[(int64_t)which * 2 * E + E + e];
  return r;
}
// the demand stream as it was before this demand generation (see EnvState::rng_pre)
__device__ __forceinline__ void store_rng_pre(const EnvState& s, int64_t e, int64_t E, const Pcg64& r) {
  s.rng_pre[e] = r.s_hi;
  s.rng_pre[E + e] = r.s_lo;
  s.rng_pre[2 * E + e] = r.i_hi;
  s.rng_pre[3 * E + e] = r.i_lo;
  s.rbuf_pre[e] = r.has32;
  s.rbuf_pre[E + e] = r.u32;
}
__device__ __forceinline__ void store_rng(const EnvState& s, int which, int64_t e, int64_t E, const Pcg64& r) {
  uint64_t* b = s.rng + (int64_t)which * 4 * E + e;
  b[0] = r.s_hi;
  b[E] = r.s_lo;
  b[2 * E] = r.i_hi;
  b[3 * E] = r.i_lo;
  s.rbuf[(int64_t)which * 2 * E + e] = r.has32;
  s.rbuf[(int64_t)which * 2 * E + E + e] = r.u32;
}

constexpr int PS_MASK = 0, PS_ORD = 1, PS_QTY = 2, PS_DONE = 3;

#ifndef MSC_UD
#define MSC_UD 8
#endif
#ifndef MSC_UHS
#define MSC_UHS 4
#endif
constexpr int UD = MSC_UD;                  // uniforms per round
constexpr int UHS = MSC_UHS;                // rounds per chunk (<= UD * UHS draws per lane)
constexpr int pow2ceil(int x) { return x <= 1 ? 1 : 2 * pow2ceil((x + 1) / 2); }
#ifndef MSC_UCAP_X
#define MSC_UCAP_X 1  // A/B: ring capacity multiplier (deeper rings, fewer demand blocks per CU)
#endif
constexpr int UCAP = pow2ceil(2 * UD * UHS) * MSC_UCAP_X;  // ring capacity (positions), >= 2 chunks
constexpr int USLOTS = UCAP + UD;           // ring rows: UCAP + the UD - 1 mirrored ones + a dummy row
static_assert((UCAP & (UCAP - 1)) == 0, "ring layout");

#ifndef MSC_GEN_QUOTA
#define MSC_GEN_QUOTA 24  // positions added per lane per chunk (mean consumption ~18 at lambda 4-5)
#endif
// the generators' fill target for the next phase: QUOTA more positions, capped by the ring slots the
// parser's current chunk (starting at rdp) cannot read
__device__ __forceinline__ int unit_quota(int tgt, int rdp) {
  const int q = tgt + MSC_GEN_QUOTA, cap = rdp + UCAP;
  return q < cap ? q : cap;
}

// EA: the root seed of the episode a lane generates (reset_env's counter rule applied
// iters0 + k * iters_step times from the counter stored for from_slot, or for the lane's own slot
// when from_slot < 0); the counter after that reset goes to cnt_out
__device__ __forceinline__ uint32_t ea_root(const EnvConst& c, const EnvState& s, const EaLaunch& ea, int64_t e,
                                            int k, int slot, int& cnt_out) {
  int cnt = s.ea_cnt[(int64_t)(ea.from_slot < 0 ? slot : ea.from_slot) * c.E + e];
  const int iters = ea.iters0 + k * ea.iters_step;
  int wv = 0;
  for (int i = 0; i < iters; i++) {
    wv = (c.num_eval > 0 && cnt >= c.num_eval) ? 0 : cnt;
    cnt = wv + 1;
  }
  cnt_out = cnt;
  const uint32_t w2[2] = {s.orig_root[e], (uint32_t)wv};
  return ss_u32(w2, 2);
}

__host__ __device__ constexpr size_t unit_lds_fixed() {
  return (size_t)BS * USLOTS * sizeof(double) + (size_t)2 * BS * sizeof(int32_t);
}

// ---- the generator waves' draw: numpy's random() of a lane's state, then the state advanced by G
// stream positions, s <- s * M^G + C (mod 2^128), C the lane's stride increment (pcg_jump_coeffs).
//
// lcg128 (form 0) leaves the 128-bit expression to the backend: 23 VALU per step on gfx950, 10 of
// them the multiplies, 13 the moves, compares and adds that stitch zero-extended 64-bit partial sums
// together. Forms 1 and 2 are ten v_mad_u64_u32 whose 64-bit addends carry the partial sums, and four
// adds. gfx950 takes a 64-bit VGPR operand only as an even-aligned pair, so an addend cannot be "the
// high word of the last result followed by a held constant"; the products are summed instead in pairs
// of two phases that never exchange single words until the end (word w = 32 bits of weight 2^32w):
//   even pairs  E01 = s0 m0 + (c0, 0)                        words 0, 1   (cannot carry)
//               E23 = s0 m2 + s1 m1 + s2 m0 + (c2, c3)       words 2, 3   (carries are >= 2^128)
//   odd pair    O12 = s0 m1 + (c1, 0), then + s1 m0          words 1, 2   (second carries: kO, 2^96)
//   word 3      W   = s0 m3 + s1 m2 + s2 m1 + s3 m0          low word of a pair, high word unused
//   n0 = E0;  n1 = E1 + O1 -> ca;  n2 = E2 + O2 + ca -> ca';  n3 = (E3 + W + kO) + ca'
// The multiplier words are compile-time constants in scalar registers; (c0, 0), (c1, 0), (c2, c3)
// are held per lane. Form 1 takes kO from the multiply-add's own carry output (inline asm: no builtin
// exposes it), form 2 is the same chain in plain C++ (kO by a 64-bit compare).
#ifndef MSC_GEN_DRAW
#define MSC_GEN_DRAW 1  // A/B: 0 lcg128, 1 multiply-add chain with asm carries, 2 the chain in plain C++
#endif

constexpr unsigned __int128 pcg_mul_pow(int g) {
  unsigned __int128 r = 1;
  for (int i = 0; i < g; i++) r *= ((unsigned __int128)PCG_MUL_HI << 64) | PCG_MUL_LO;
  return r;
}

struct GenLane {
  uint32_t s0, s1, s2, s3;  // the state, s0 the lowest word
  uint64_t c0z, c1z, c23;   // the stride increment as the addend pairs (c0, 0), (c1, 0), (c2, c3)
  uint64_t ch, cl;          // (form 0 only)
};
__device__ __forceinline__ GenLane gen_lane(uint64_t sh, uint64_t sl, uint64_t ch, uint64_t cl) {
  GenLane L;
  L.s0 = (uint32_t)sl;
  L.s1 = (uint32_t)(sl >> 32);
  L.s2 = (uint32_t)sh;
  L.s3 = (uint32_t)(sh >> 32);
  L.c0z = (uint32_t)cl;
  L.c1z = cl >> 32;
  L.c23 = ch;
  L.ch = ch;
  L.cl = cl;
  return L;
}
__device__ __forceinline__ uint64_t gen_state_lo(const GenLane& L) { return ((uint64_t)L.s1 << 32) | L.s0; }
__device__ __forceinline__ uint64_t gen_state_hi(const GenLane& L) { return ((uint64_t)L.s3 << 32) | L.s2; }

template <int G>
__device__ __forceinline__ void gen_advance(GenLane& L) {
  constexpr unsigned __int128 M = pcg_mul_pow(G);
  constexpr uint32_t m0 = (uint32_t)M, m1 = (uint32_t)(M >> 32), m2 = (uint32_t)(M >> 64), m3 = (uint32_t)(M >> 96);
#if MSC_GEN_DRAW == 1
  // The compiler pads nothing inside an asm statement. Its own listing of this loop (lcg128 form)
  // keeps two wait states between a VALU that writes a carry mask and the VALU that reads it
  // (v_addc_co, one independent instruction, s_nop 0, v_addc_co), so every mask here is read at least
  // two states after it is written: kO five multiply-adds later at the earliest, ca after s_nop 1,
  // ca' after one instruction and s_nop 0. The three chains are interleaved so that no multiply-add
  // reads the result of the one before it.
  uint64_t O, W, E23, E01, kO, kj, ca;
  asm volatile(
      "v_mad_u64_u32 %0, %4, %5, %10, %13\n\t"  // O   = s0 m1 + (c1, 0)
      "v_mad_u64_u32 %1, %4, %5, %12, 0\n\t"    // W   = s0 m3
      "v_mad_u64_u32 %2, %4, %5, %11, %14\n\t"  // E23 = s0 m2 + (c2, c3)
      "v_mad_u64_u32 %0, %3, %6, %9, %0\n\t"    // O  += s1 m0, carry kO
      "v_mad_u64_u32 %1, %4, %6, %11, %1\n\t"   // W  += s1 m2
      "v_mad_u64_u32 %2, %4, %6, %10, %2\n\t"   // E23 += s1 m1
      "v_mad_u64_u32 %1, %4, %7, %10, %1\n\t"   // W  += s2 m1
      "v_mad_u64_u32 %2, %4, %7, %9, %2\n\t"    // E23 += s2 m0
      "v_mad_u64_u32 %1, %4, %8, %9, %1"         // W  += s3 m0
      : "=&v"(O), "=&v"(W), "=&v"(E23), "=&s"(kO), "=&s"(kj)
      : "v"(L.s0), "v"(L.s1), "v"(L.s2), "v"(L.s3), "s"(m0), "s"(m1), "s"(m2), "s"(m3), "v"(L.c1z), "v"(L.c23));
  // (s0's last use: the result may take the place of (s0, s1), and n1 below that of E1)
  asm volatile("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=v"(E01), "=s"(kj) : "v"(L.s0), "s"(m0), "v"(L.c0z));
  uint32_t n1 = (uint32_t)(E01 >> 32), n2, n3;
  asm volatile(
      "v_add_co_u32 %0, %3, %0, %5\n\t"         // n1 = E1 + O1 -> ca
      "s_nop 1\n\t"
      "v_addc_co_u32 %1, %3, %6, %7, %3\n\t"    // n2 = E2 + O2 + ca -> ca'
      "v_addc_co_u32 %2, %4, %8, %9, %10\n\t"   // n3 = E3 + W + kO
      "s_nop 0\n\t"
      "v_addc_co_u32 %2, %4, %2, 0, %3"          // n3 += ca'
      : "+v"(n1), "=&v"(n2), "=&v"(n3), "=&s"(ca), "=&s"(kj)
      : "v"((uint32_t)O), "v"((uint32_t)E23), "v"((uint32_t)(O >> 32)), "v"((uint32_t)(E23 >> 32)),
        "v"((uint32_t)W), "s"(kO));
  L.s0 = (uint32_t)E01;
  L.s1 = n1;
  L.s2 = n2;
  L.s3 = n3;
#elif MSC_GEN_DRAW == 2
  const uint64_t O1 = (uint64_t)L.s0 * m1 + L.c1z;
  const uint64_t O = (uint64_t)L.s1 * m0 + O1;
  const uint32_t kO = O < O1 ? 1u : 0u;
  const uint32_t W = L.s0 * m3 + L.s1 * m2 + L.s2 * m1 + L.s3 * m0;
  const uint64_t E23 = (uint64_t)L.s0 * m2 + L.c23 + (uint64_t)L.s1 * m1 + (uint64_t)L.s2 * m0;
  const uint64_t E01 = (uint64_t)L.s0 * m0 + L.c0z;
  const uint64_t t1 = (E01 >> 32) + (uint32_t)O;                                // word 1 and its carry
  const uint64_t t2 = (uint64_t)(uint32_t)E23 + (O >> 32) + (t1 >> 32);          // word 2 and its carry
  L.s0 = (uint32_t)E01;
  L.s1 = (uint32_t)t1;
  L.s2 = (uint32_t)t2;
  L.s3 = (uint32_t)(E23 >> 32) + W + kO + (uint32_t)(t2 >> 32);
#else
  uint64_t sh = gen_state_hi(L), sl = gen_state_lo(L);
  lcg128(sh, sl, (uint64_t)(M >> 64), (uint64_t)M, L.ch, L.cl);
  L.s0 = (uint32_t)sl;
  L.s1 = (uint32_t)(sl >> 32);
  L.s2 = (uint32_t)sh;
  L.s3 = (uint32_t)(sh >> 32);
#endif
}

// numpy random() of the lane's state: (x >> 11) 2^-53 of the XSL-RR output x, as the top 32 bits
// 2^-32 plus the next 21 bits 2^-53 (one exact fma, pcg_output_double; the high word converted by one
// v_cvt_f64_u32 -- laundered: the optimizer otherwise widens it into a 64-bit conversion with an add)
__device__ __forceinline__ double gen_uniform(const GenLane& L) {
  const uint64_t x = pcg_output(gen_state_hi(L), gen_state_lo(L));
  const double hi = (double)(uint32_t)vsettle((int)(uint32_t)(x >> 32));
  return fma(hi, 0x1p-32, (double)((uint32_t)x >> 11) * 0x1p-53);
}

#ifndef MSC_PARSER_PRIO
#define MSC_PARSER_PRIO 2  // s_setprio of the parser wave (generators: MSC_GEN_PRIO)
#endif
#ifndef MSC_GEN_PRIO
#define MSC_GEN_PRIO 1
#endif
#ifndef MSC_DEM_WPE
#define MSC_DEM_WPE 8  // <= 64 VGPRs: two demand waves fit beside four step_b waves on a SIMD
#endif

}  // namespace msc
