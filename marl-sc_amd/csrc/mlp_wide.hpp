// The fused policy-MLP kernels with a multi-tile MFMA output layer (up to 128 outputs: the joint
// action of a centralised policy) and a Gaussian-sampling epilogue staged through LDS. Instantiated
// by mlp_wide.hip; layers 1 and 2 are those of mlp_kernels.hpp (same fragment order, same
// accumulation order), the output layer holds NTO tiles of 32 rows in 16 NTO accumulator registers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "env.hpp"
#include "mlp_kernels.hpp"  // mlp_f32x16, mfma_row

namespace msc {

// floats of LDS one wave stages its 32 x (32 NTO) output tile in
template <int NTO>
constexpr int wide_stage_floats() { return 32 * 32 * NTO; }

// Epilogue of the wide output layer. After the output MFMAs lane (c, h) holds, for sample c of the
// wave's 32, rows 32 o + 8 g + 4 h + {0..3} of output tile o in registers 4 g .. 4 g + 3: a sample's
// outputs lie across two lanes and 16 NTO registers, and a store from there has a stride of KO floats
// between lanes. So the tile goes through LDS:
//  1. each lane writes its 4 NTO float4 groups (ds_write_b128) into st[c][.], row c's float4 chunks
//     rotated by c (chunk q at position (q + c) mod 8 NTO) so that the eight lanes of a write group
//     and the sixteen of a b128 read group fall on different banks;
//  2. the wave walks the [rows][KO] block of means in flat order f = row KO + k, lane l taking
//     f = l, l + 64, ..: means (out), eps, actions and clipped are contiguous runs of the row-major
//     arrays, 256 B per wave access. Each element gets msc_gaussian_sample's arithmetic, operation for
//     operation, and its log-probability term replaces the mean in LDS;
//  3. lane c < rows adds row c's KO terms sequentially in k, from 0.0f, exactly as
//     msc_gaussian_sample's loop does: logp is bit-identical to the separate kernel's.
// The staging area is private to the wave, LDS operations of a wave complete in order, so the phases
// need compiler ordering only (wavefront-scope fences), no block barrier: waves past the last row
// have already left. Nothing is read or written past `rows` rows or KO columns.
template <int NTO>
__device__ __forceinline__ void wide_epilogue(float* __restrict__ st, const mlp_f32x16 (&a3)[NTO], int lane, int64_t row0,
                                              int rows, int KO, float* __restrict__ out, const MlpSample& sm) {
  constexpr int NCH = NTO * 8;  // float4 chunks per staged row
  const int c = lane & 31, h = lane >> 5;
  float4* st4 = reinterpret_cast<float4*>(st);
#pragma unroll
  for (int o = 0; o < NTO; o++)
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const int q = o * 8 + 2 * g + h;
      st4[c * NCH + (q + c) % NCH] = make_float4(a3[o][4 * g], a3[o][4 * g + 1], a3[o][4 * g + 2], a3[o][4 * g + 3]);
    }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const float half_log_2pi = 0.91893853320467274178f;  // 0.5 * log(2 pi)
  const bool sample = sm.act != nullptr;
  const int total = rows * KO;  // <= 32 * 128
  const int64_t base = row0 * KO;
  // (r, k) of this lane's element and the log_std row of sample row0 + r, stepped without divisions
  int r = 0, k = lane;
  uint32_t lr = sample ? (uint32_t)(row0 % sm.ls_rows) : 0u;
  const uint32_t lsn = sample ? (uint32_t)sm.ls_rows : 1u;
  for (int f = lane; f < total; f += 64) {
    while (k >= KO) {
      k -= KO, r++;
      if (++lr == lsn) lr = 0;
    }
    const int a = (r * NCH + ((k >> 2) + r) % NCH) * 4 + (k & 3);
    const float m = st[a];
    if (out) out[base + f] = m;
    if (sample) {
      const float ls = fmaxf(sm.log_std[(int64_t)lr * KO + k], sm.floor_);
      const float sd = expf(ls);
      const float v = m + sd * sm.eps[base + f];
      sm.act[base + f] = v;
      const float d = v - m;
      st[a] = (-(d * d) / (2.0f * sd * sd) - ls) - half_log_2pi;
      sm.clipped[base + f] = fminf(fmaxf(v, -1.0f), 1.0f);
    }
    k += 64;
  }
  if (!sample) return;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (lane < rows) {
    float lp = 0.0f;
    for (int q = 0; q * 4 < KO; q++) {
      const float4 t = st4[c * NCH + (q + c) % NCH];
      lp += t.x;
      if (q * 4 + 1 < KO) lp += t.y;
      if (q * 4 + 2 < KO) lp += t.z;
      if (q * 4 + 3 < KO) lp += t.w;
    }
    sm.logp[row0 + c] = lp;
  }
}

// bias rows of the NTO output tiles (0 past KO: with the zero weight rows those accumulators stay 0)
template <int NTO>
__device__ __forceinline__ void wide_bias(mlp_f32x16 (&a3)[NTO], const float* __restrict__ b3, int KO, int h) {
#pragma unroll
  for (int o = 0; o < NTO; o++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int row = o * 32 + mfma_row(r, h);
      a3[o][r] = row < KO ? b3[row] : 0.0f;
    }
}

// Linear -> ReLU -> Linear -> ReLU -> Linear with up to 32 NTO outputs: layers 1 and 2 as
// mlp3_relu_kernel (H1 whole in registers, H2 in passes of P tiles, weights prefetched one step
// ahead), the output layer on the MFMA into NTO accumulator tiles. The packed w3 is the layout-0
// fragment order of mlp3_relu_kernel once per 32-row slice of W3, slices concatenated
// ([NTO][NT2 * 4][64] float4, zero rows past KO): slice o's fragment of hidden step u is one
// contiguous 1-KiB read, and the NTO MFMAs of a hidden pair are independent chains.
template <int NT1, int NT2, int P, int WPE, int NTO>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void mlp3_wide_kernel(
    const float* __restrict__ x, int64_t n, int L, int KS1, const float4* __restrict__ w1p, const float* __restrict__ b1,
    const float4* __restrict__ w2p, const float* __restrict__ b2, const float4* __restrict__ w3p,
    const float* __restrict__ b3, int KO, float* __restrict__ out, const float* __restrict__ pre1, int grp, int prio,
    MlpSample sm) {
  static_assert(NT2 % P == 0, "layer-2 passes");
  static_assert(NTO >= 1 && NTO <= 4, "output tiles");
  constexpr int S4 = NT1 * 4;  // layer-2 k steps of 4 MFMAs (2 hidden units each)
  __shared__ float stage[4 * wide_stage_floats<NTO>()];
  if (prio) __builtin_amdgcn_s_setprio(3);
  const int lane = threadIdx.x & 63, h = lane >> 5;
  const int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tile * 32 >= n) return;  // wave-uniform (no block-level synchronisation below)
  const int64_t j = tile * 32 + (lane & 31);
  const bool jv = j < n;
  const int M4 = (KS1 + 3) / 4;  // layer-1 k steps of 4 MFMAs

  mlp_f32x16 a1[NT1];
#pragma unroll
  for (int t = 0; t < NT1; t++)
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const float4 v = *reinterpret_cast<const float4*>(b1 + t * 32 + 8 * g + 4 * h);
      a1[t][4 * g] = v.x, a1[t][4 * g + 1] = v.y, a1[t][4 * g + 2] = v.z, a1[t][4 * g + 3] = v.w;
    }
  if (pre1 != nullptr) {
    const float* pg = pre1 + ((jv ? j : 0) / grp) * (int64_t)(NT1 * 32);
#pragma unroll
    for (int t = 0; t < NT1; t++)
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const float4 v = *reinterpret_cast<const float4*>(pg + t * 32 + 8 * g + 4 * h);
        a1[t][4 * g] += v.x, a1[t][4 * g + 1] += v.y, a1[t][4 * g + 2] += v.z, a1[t][4 * g + 3] += v.w;
      }
  }
  const float* xr = x + (jv ? j : 0) * (int64_t)L;
  auto load_x = [&](int m4, float (&xv)[4]) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int m = m4 * 4 + i, k = h * KS1 + m;
      xv[i] = (jv && m < KS1 && k < L) ? xr[k] : 0.0f;
    }
  };
  {
    float xc[4], xn[4];
    float4 wc[NT1], wn[NT1];
    load_x(0, xc);
#pragma unroll
    for (int t = 0; t < NT1; t++) wc[t] = w1p[((int64_t)t * M4) * 64 + lane];
    for (int m4 = 0; m4 < M4; m4++) {
      const bool more = m4 + 1 < M4;
      if (more) {
        load_x(m4 + 1, xn);
#pragma unroll
        for (int t = 0; t < NT1; t++) wn[t] = w1p[((int64_t)t * M4 + m4 + 1) * 64 + lane];
      }
      __builtin_amdgcn_sched_barrier(0);  // keep the prefetch ahead of this step's MFMAs
#pragma unroll
      for (int t = 0; t < NT1; t++) {
        a1[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(wc[t].x, xc[0], a1[t], 0, 0, 0);
        a1[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(wc[t].y, xc[1], a1[t], 0, 0, 0);
        a1[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(wc[t].z, xc[2], a1[t], 0, 0, 0);
        a1[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(wc[t].w, xc[3], a1[t], 0, 0, 0);
      }
      if (more) {
#pragma unroll
        for (int i = 0; i < 4; i++) xc[i] = xn[i];
#pragma unroll
        for (int t = 0; t < NT1; t++) wc[t] = wn[t];
      }
    }
  }
#pragma unroll
  for (int t = 0; t < NT1; t++)
#pragma unroll
    for (int r = 0; r < 16; r++) a1[t][r] = fmaxf(a1[t][r], 0.0f);

  mlp_f32x16 a3[NTO];
  wide_bias<NTO>(a3, b3, KO, h);
  float4 w[2][P];  // [step parity][tile]: the layer-2 fragments of step s4 and s4 + 1
#pragma unroll
  for (int q = 0; q < P; q++) w[0][q] = w2p[((int64_t)q * S4) * 64 + lane];
  for (int p = 0; p < NT2 / P; p++) {  // (S4 is even: the fragment buffer of a step is s4 & 1 in every pass)
    mlp_f32x16 a2[P];
#pragma unroll
    for (int q = 0; q < P; q++)
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const float4 v = *reinterpret_cast<const float4*>(b2 + (p * P + q) * 32 + 8 * g + 4 * h);
        a2[q][4 * g] = v.x, a2[q][4 * g + 1] = v.y, a2[q][4 * g + 2] = v.z, a2[q][4 * g + 3] = v.w;
      }
#pragma unroll
    for (int s4 = 0; s4 < S4; s4++) {
      const int cb = s4 & 1;
      if (s4 + 1 < S4) {
#pragma unroll
        for (int q = 0; q < P; q++) w[cb ^ 1][q] = w2p[((int64_t)(p * P + q) * S4 + s4 + 1) * 64 + lane];
      } else if (p + 1 < NT2 / P) {
#pragma unroll
        for (int q = 0; q < P; q++) w[cb ^ 1][q] = w2p[((int64_t)((p + 1) * P + q) * S4) * 64 + lane];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int s = s4 * 4 + i;
        const float bv = a1[s / 16][s % 16];
#pragma unroll
        for (int q = 0; q < P; q++) {
          const float4& wq = w[cb][q];
          const float wv = i == 0 ? wq.x : i == 1 ? wq.y : i == 2 ? wq.z : wq.w;
          a2[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv, bv, a2[q], 0, 0, 0);
        }
      }
    }
    // output layer on this pass's slice of H2: step u = (tile q, register group r4), the NTO
    // fragments of step u + 1 in flight during step u
    float4 w3[2][NTO];
#pragma unroll
    for (int o = 0; o < NTO; o++) w3[0][o] = w3p[((int64_t)o * NT2 * 4 + (p * P) * 4) * 64 + lane];
#pragma unroll
    for (int u = 0; u < P * 4; u++) {
      if (u + 1 < P * 4) {
#pragma unroll
        for (int o = 0; o < NTO; o++) w3[(u + 1) & 1][o] = w3p[((int64_t)o * NT2 * 4 + (p * P) * 4 + u + 1) * 64 + lane];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const float hv = fmaxf(a2[u / 4][(u % 4) * 4 + i], 0.0f);
#pragma unroll
        for (int o = 0; o < NTO; o++) {
          const float4& wq = w3[u & 1][o];
          const float wv = i == 0 ? wq.x : i == 1 ? wq.y : i == 2 ? wq.z : wq.w;
          a3[o] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv, hv, a3[o], 0, 0, 0);
        }
      }
    }
  }
  const int64_t left = n - tile * 32;
  wide_epilogue<NTO>(stage + (threadIdx.x >> 6) * wide_stage_floats<NTO>(), a3, lane, tile * 32,
                     left < 32 ? (int)left : 32, KO, out, sm);
}

// Linear -> ReLU -> Linear with up to 32 NTO outputs: the hidden layer TB tiles at a time, exactly as
// mlp2_relu_kernel produces it, folded into the NTO output tiles as soon as a group is final.
template <int TB, int WPE, int NTO>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void mlp2_wide_kernel(
    const float* __restrict__ x, int64_t n, int L, int KS1, int NT1, const float4* __restrict__ w1p,
    const float* __restrict__ b1, const float4* __restrict__ w3p, const float* __restrict__ b3, int KO,
    float* __restrict__ out, const float* __restrict__ pre1, int grp, int prio, MlpSample sm) {
  static_assert(NTO >= 1 && NTO <= 4, "output tiles");
  __shared__ float stage[4 * wide_stage_floats<NTO>()];
  if (prio) __builtin_amdgcn_s_setprio(3);
  const int lane = threadIdx.x & 63, h = lane >> 5;
  const int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tile * 32 >= n) return;  // wave-uniform
  const int64_t j = tile * 32 + (lane & 31);
  const bool jv = j < n;
  const int M4 = (KS1 + 3) / 4;
  const float* xr = x + (jv ? j : 0) * (int64_t)L;
  const float* pg = pre1 != nullptr ? pre1 + ((jv ? j : 0) / grp) * (int64_t)(NT1 * 32) : nullptr;
  auto load_x = [&](int m4, float (&xv)[4]) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int m = m4 * 4 + i, k = h * KS1 + m;
      xv[i] = (jv && m < KS1 && k < L) ? xr[k] : 0.0f;
    }
  };
  mlp_f32x16 a3[NTO];
  wide_bias<NTO>(a3, b3, KO, h);
  for (int g0 = 0; g0 < NT1; g0 += TB) {
    mlp_f32x16 a1[TB];
#pragma unroll
    for (int t = 0; t < TB; t++)
#pragma unroll
      for (int q = 0; q < 4; q++) {
        float4 v = *reinterpret_cast<const float4*>(b1 + (g0 + t) * 32 + 8 * q + 4 * h);
        if (pg != nullptr) {
          const float4 u = *reinterpret_cast<const float4*>(pg + (g0 + t) * 32 + 8 * q + 4 * h);
          v.x += u.x, v.y += u.y, v.z += u.z, v.w += u.w;
        }
        a1[t][4 * q] = v.x, a1[t][4 * q + 1] = v.y, a1[t][4 * q + 2] = v.z, a1[t][4 * q + 3] = v.w;
      }
    {
      float xc[4], xn[4];
      float4 wc[TB], wn[TB];
      load_x(0, xc);
#pragma unroll
      for (int t = 0; t < TB; t++) wc[t] = w1p[((int64_t)(g0 + t) * M4) * 64 + lane];
      for (int m4 = 0; m4 < M4; m4++) {
        const bool more = m4 + 1 < M4;
        if (more) {
          load_x(m4 + 1, xn);
#pragma unroll
          for (int t = 0; t < TB; t++) wn[t] = w1p[((int64_t)(g0 + t) * M4 + m4 + 1) * 64 + lane];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < TB; t++) {
          a1[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(wc[t].x, xc[0], a1[t], 0, 0, 0);
          a1[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(wc[t].y, xc[1], a1[t], 0, 0, 0);
          a1[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(wc[t].z, xc[2], a1[t], 0, 0, 0);
          a1[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(wc[t].w, xc[3], a1[t], 0, 0, 0);
        }
        if (more) {
#pragma unroll
          for (int i = 0; i < 4; i++) xc[i] = xn[i];
#pragma unroll
          for (int t = 0; t < TB; t++) wc[t] = wn[t];
        }
      }
    }
    // output layer over this group's hidden units (ReLU applied as they are read): step u = (tile,
    // register group), the NTO fragments of steps u + 1 and u + 2 in flight during step u (a step is
    // only 4 NTO MFMAs, less than an L2 round trip at one wave per SIMD)
    float4 w3[3][NTO];
#pragma unroll
    for (int o = 0; o < NTO; o++) {
      w3[0][o] = w3p[((int64_t)o * NT1 * 4 + g0 * 4) * 64 + lane];
      w3[1][o] = w3p[((int64_t)o * NT1 * 4 + g0 * 4 + 1) * 64 + lane];
    }
#pragma unroll
    for (int u = 0; u < TB * 4; u++) {
      if (u + 2 < TB * 4) {
#pragma unroll
        for (int o = 0; o < NTO; o++) w3[(u + 2) % 3][o] = w3p[((int64_t)o * NT1 * 4 + g0 * 4 + u + 2) * 64 + lane];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const float hv = fmaxf(a1[u / 4][(u % 4) * 4 + i], 0.0f);
#pragma unroll
        for (int o = 0; o < NTO; o++) {
          const float4& wq = w3[u % 3][o];
          const float wv = i == 0 ? wq.x : i == 1 ? wq.y : i == 2 ? wq.z : wq.w;
          a3[o] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv, hv, a3[o], 0, 0, 0);
        }
      }
    }
  }
  const int64_t left = n - tile * 32;
  wide_epilogue<NTO>(stage + (threadIdx.x >> 6) * wide_stage_floats<NTO>(), a3, lane, tile * 32,
                     left < 32 ? (int)left : 32, KO, out, sm);
}

}  // namespace msc
