// The fused policy-MLP kernel templates (see mlp.hip for the design): shared by mlp.hip (plain output
// layer, optional sampling epilogue), mlp_multi.hip (the same for per-agent policies) and mlp_musigma.hip
// (dual mu / sigma head), which instantiate them in separate translation units so that they compile in
// parallel. Which instantiation a launch takes is decided in one place, mlp_dispatch.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "env.hpp"

namespace msc {

typedef float mlp_f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ int mfma_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// Optional epilogue: the rollout's Gaussian action sampling (msc_gaussian_sample's arithmetic,
// operation for operation, so the results are bit-identical to the separate kernel) applied to the
// KO outputs of row j while they are in registers: one kernel launch and the mean's HBM round trip
// fewer per rollout step. act == nullptr: no sampling.
template <int VKO>
__device__ __forceinline__ void sample_row(const MlpSample& sm, int64_t j, int KO, const float (&m)[VKO]) {
  const float half_log_2pi = 0.91893853320467274178f;  // 0.5 * log(2 pi)
  const float* lsr = sm.log_std + (j % sm.ls_rows) * KO;
  float lp = 0.0f;
#pragma unroll
  for (int a = 0; a < VKO; a++) {
    if (a < KO) {
      const int64_t i = j * KO + a;
      const float ls = fmaxf(lsr[a], sm.floor_);
      const float sd = expf(ls);
      const float v = m[a] + sd * sm.eps[i];
      sm.act[i] = v;
      const float d = v - m[a];
      lp += (-(d * d) / (2.0f * sd * sd) - ls) - half_log_2pi;
      sm.clipped[i] = fminf(fmaxf(v, -1.0f), 1.0f);
    }
  }
  sm.logp[j] = lp;
}

// The mu / sigma head's activations (MSC_ACT_*: the reference's _get_activation names; GELU in its erf form)
__device__ __forceinline__ float head_act(int code, float v) {
  switch (code) {
    case 1: return fmaxf(v, 0.0f);
    case 2: return tanhf(v);
    case 3: return v > 0.0f ? v : expm1f(v);
    case 4: return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
    case 5: return 1.0f / (1.0f + expf(-v));
    default: return v;
  }
}

// Epilogue of the dual-head output layer (MuSigmaHead.forward, mu_sigma_head.py:52-82) on row j's
// sums o = [mu pre-activations (VK) | sigma pre-activations (VK)]: mu = act_mu(.), log_std =
// clamp(act_sigma(.), lo, hi), optionally stored as [mu || log_std], then msc_gaussian_sample's
// arithmetic operation for operation with floor = lo (a no-op after the clamp), so the launch is
// bit-identical to storing the distribution inputs and sampling from them with one log_std row per row.
template <int VK>
__device__ __forceinline__ void musigma_row(const MlpMuSigma& e, int64_t j, int K, const float (&o)[2 * VK]) {
  const float half_log_2pi = 0.91893853320467274178f;  // 0.5 * log(2 pi)
  float mu[VK], lsv[VK];
#pragma unroll
  for (int a = 0; a < VK; a++) {
    mu[a] = head_act(e.act_mu, o[a]);
    lsv[a] = fminf(fmaxf(head_act(e.act_sigma, o[VK + a]), e.lo), e.hi);
  }
  if (e.dist) {
#pragma unroll
    for (int a = 0; a < VK; a++)
      if (a < K) e.dist[j * (2 * K) + a] = mu[a], e.dist[j * (2 * K) + K + a] = lsv[a];
  }
  if (e.act) {
    float lp = 0.0f;
#pragma unroll
    for (int a = 0; a < VK; a++) {
      if (a < K) {
        const int64_t i = j * K + a;
        const float ls = fmaxf(lsv[a], e.lo);
        const float sd = expf(ls);
        const float v = mu[a] + sd * e.eps[i];
        e.act[i] = v;
        const float d = v - mu[a];
        lp += (-(d * d) / (2.0f * sd * sd) - ls) - half_log_2pi;
        e.clipped[i] = fminf(fmaxf(v, -1.0f), 1.0f);
      }
    }
    e.logp[j] = lp;
  }
}

// NT1 / NT2: hidden tiles of 32 units; P: output tiles of layer 2 held at once (register budget:
// 16 NT1 + 16 P + 16 accumulators + 2 x 4 P weight registers per lane).
// Weight fragments are software-pipelined one step ahead (the loads of step s + 1 are issued before
// the MFMAs of step s): with one wave per SIMD nothing else hides an L2 round trip, and a wait on
// each step's own loads cost ~35 % of the MFMA time.
// VKO > 0: the output layer (KO <= VKO <= 8 outputs) on the VALU instead of a 32-row MFMA tile
// padded from KO rows (an output MFMA tile of 5 actions is 84 % padding: 128 of the actor's 1,312
// MFMAs). Each lane accumulates its half of the hidden units into VKO f32 sums with the weights read
// from LDS (all lanes of a half read the same 32 bytes: broadcast), and the two halves are added
// with one lane exchange. The packed w3 is then [NT2 * 16][2][8] floats (zero past KO).
// IL (VKO > 0, P < NT2): the VALU output layer of pass p - 1 interleaved into the layer-2 MFMA stream
// of pass p (IPS units per k step), so its VALU work issues while the MFMAs execute instead of after
// them; only the last pass's output layer runs alone. Same accumulation order as IL = false.
// EP = MlpMuSigma (VKO > 0): the dual-head output layer of a mu / sigma-head actor whose last backbone
// Linear is folded into the heads -- KO actions, 2 VKO per-lane sums (mu, then sigma) over the same
// hidden-unit order, b3 = [b_mu | b_sigma] (2 KO), the packed weights [NT2 * 16][2][8 or 16] floats
// (mlp_head_stride: mu's in the first half, sigma's in the second), musigma_row as the epilogue.
// MULTI (mlp_multi.hip): grp same-shaped policies with grp weight sets in one launch over rows laid out
// [n envs][grp policies] (row e grp + pol belongs to policy pol). A block serves 4 env tiles of one
// policy -- the VALU output layer stages that policy's w3 slice in LDS -- and a wave's 32 rows are
// envs 32 tile .. 32 tile + 31 of it, so every row array is addressed with row stride grp and every
// weight / bias array is offset by pol single-policy sizes; log_std row pol applies (sample_row's
// j % ls_rows, ls_rows = grp or 1), pre1 is one row per row. prio bit 1 is the block order: clear =
// policy-major (a policy's blocks consecutive), set = policy-minor (pol = block % grp: with grp a
// multiple of 8 a policy's blocks are congruent mod 8). The arithmetic per row is the single-policy
// kernel's, operation for operation. MULTI = false compiles to the single-policy kernel as it was.
template <int NT1, int NT2, int P, int WPE, int VKO, bool IL = false, class EP = MlpSample, bool MULTI = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void mlp3_relu_kernel(
    const float* __restrict__ x, int64_t n, int L, int KS1, const float4* __restrict__ w1p, const float* __restrict__ b1,
    const float4* __restrict__ w2p, const float* __restrict__ b2, const float4* __restrict__ w3p,
    const float* __restrict__ b3, int KO, float* __restrict__ out, const float* __restrict__ pre1, int grp, int prio,
    EP sm) {
  static_assert(NT2 % P == 0, "layer-2 passes");
  static_assert(VKO >= 0 && VKO <= 8, "VALU output layer: at most 8 outputs");
  constexpr bool HEAD = std::is_same<EP, MlpMuSigma>::value;
  static_assert(!HEAD || VKO > 0, "the dual head runs on the VALU output layer");
  constexpr int F4 = HEAD && VKO > 4 ? 4 : 2;  // float4 per (hidden pair, lane half) in LDS
  constexpr int NO = HEAD ? 2 * VKO : VKO;     // per-lane output sums
  constexpr int S4 = NT1 * 4;  // layer-2 k steps of 4 MFMAs (2 hidden units each)
  // the policy forward is on the rollout's critical path (step t + 1 needs its actions), the
  // pipelined demand kernel of step t + 1 (priorities 1-2) is not: issue ahead of it
  if (MULTI ? (prio & 1) : prio) __builtin_amdgcn_s_setprio(3);
  const int lane = threadIdx.x & 63, h = lane >> 5;
  int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  int64_t pol = 0;
  if constexpr (MULTI) {  // n envs x grp policies: this block's policy and its 4 env tiles
    const unsigned nb = (unsigned)(((n + 31) / 32 + 3) / 4), np = (unsigned)grp;  // blocks per policy
    const unsigned be = (prio & 2) ? blockIdx.x / np : blockIdx.x % nb;
    pol = (prio & 2) ? blockIdx.x % np : blockIdx.x / nb;
    tile = (int64_t)be * 4 + (threadIdx.x >> 6);
    w1p += pol * (NT1 * ((KS1 + 3) / 4) * 64), b1 += pol * (NT1 * 32);
    w2p += pol * (NT2 * S4 * 64), b2 += pol * (NT2 * 32);
    w3p += pol * (VKO > 0 ? NT2 * 16 * 2 * F4 : NT2 * 4 * 64), b3 += pol * KO;
  }
  __shared__ float4 w3s[VKO > 0 ? NT2 * 16 * 2 * F4 : 1];  // [s][h][8 floats] (16 for a dual head wider than 4)
  if constexpr (VKO > 0) {
    for (int i = threadIdx.x; i < NT2 * 16 * 2 * F4; i += blockDim.x) w3s[i] = w3p[i];
    __syncthreads();
  }
  if (tile * 32 >= n) return;  // wave-uniform (no block-level synchronisation below)
  const int64_t e = tile * 32 + (lane & 31);
  const int64_t j = MULTI ? e * grp + pol : e;  // the lane's row
  const bool jv = e < n;
  if constexpr (MULTI) grp = 1;  // pre1: one row per row
  const int M4 = (KS1 + 3) / 4;  // layer-1 k steps of 4 MFMAs

  // layer 1: H1^T = W1 X^T + b1 (+ pre1 of the sample's group); lane half h feeds features
  // h KS1 + m, m < KS1, of its sample
  // (registers 4g .. 4g + 3 of a tile hold rows 8g + 4h .. 8g + 4h + 3: one float4 per group)
  mlp_f32x16 a1[NT1];
#pragma unroll
  for (int t = 0; t < NT1; t++)
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const float4 v = *reinterpret_cast<const float4*>(b1 + t * 32 + 8 * g + 4 * h);
      a1[t][4 * g] = v.x, a1[t][4 * g + 1] = v.y, a1[t][4 * g + 2] = v.z, a1[t][4 * g + 3] = v.w;
    }
  if (pre1 != nullptr) {  // a first-layer term shared by grp consecutive rows (MAPPO critic: the env's global block)
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

  // layers 2 and 3 in passes of P output tiles: the output layer accumulates each pass's slice of
  // the hidden units as soon as it is final, so H2 is never held whole
  mlp_f32x16 a3;
  float o3[VKO > 0 ? NO : 1];
  if constexpr (HEAD) {
#pragma unroll
    for (int a = 0; a < VKO; a++) {
      o3[a] = (h == 0 && a < KO) ? b3[a] : 0.0f;
      o3[VKO + a] = (h == 0 && a < KO) ? b3[KO + a] : 0.0f;
    }
  } else if constexpr (VKO > 0) {
#pragma unroll
    for (int a = 0; a < VKO; a++) o3[a] = (h == 0 && a < KO) ? b3[a] : 0.0f;
  } else {
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int row = mfma_row(r, h);
      a3[r] = row < KO ? b3[row] : 0.0f;
    }
  }
  // one unit of the VALU output layer: hidden unit (tile q of pass pp, register r) into the outputs
  auto l3_unit = [&](const mlp_f32x16 (&src)[P], int pp, int q, int r) {
    if constexpr (HEAD) {
      const float hv = fmaxf(src[q][r], 0.0f);
      const int sidx = ((pp * P + q) * 16 + r) * 2 + h;
      float wm[8], wg[8];  // this hidden unit's mu / sigma weights
#pragma unroll
      for (int f = 0; f < F4 / 2; f++) {
        const float4 u = w3s[sidx * F4 + f], v = w3s[sidx * F4 + F4 / 2 + f];
        wm[4 * f] = u.x, wm[4 * f + 1] = u.y, wm[4 * f + 2] = u.z, wm[4 * f + 3] = u.w;
        wg[4 * f] = v.x, wg[4 * f + 1] = v.y, wg[4 * f + 2] = v.z, wg[4 * f + 3] = v.w;
      }
#pragma unroll
      for (int a = 0; a < VKO; a++) {
        o3[a] = fmaf(wm[a], hv, o3[a]);
        o3[VKO + a] = fmaf(wg[a], hv, o3[VKO + a]);
      }
    } else if constexpr (VKO > 0) {
      const float hv = fmaxf(src[q][r], 0.0f);
      const int sidx = ((pp * P + q) * 16 + r) * 2 + h;
      const float4 wa = w3s[sidx * 2];
      const float wv[8] = {wa.x, wa.y, wa.z, wa.w, 0.f, 0.f, 0.f, 0.f};
      float wh[4] = {0.f, 0.f, 0.f, 0.f};
      if constexpr (VKO > 4) {
        const float4 wb = w3s[sidx * 2 + 1];
        wh[0] = wb.x, wh[1] = wb.y, wh[2] = wb.z, wh[3] = wb.w;
      }
#pragma unroll
      for (int a = 0; a < VKO; a++) o3[a] = fmaf(a < 4 ? wv[a] : wh[a - 4], hv, o3[a]);
    }
  };
  constexpr bool ILV = IL && VKO > 0 && P < NT2;
  constexpr int IPS = (P * 16 + S4 - 1) / S4;  // interleaved output-layer units per k step
  mlp_f32x16 a2p[ILV ? P : 1];                 // the previous pass's layer-2 sums (ILV)
  float4 w[2][P];  // [step parity][tile]: the fragments of step s4 and s4 + 1
#pragma unroll
  for (int q = 0; q < P; q++) w[0][q] = w2p[((int64_t)q * S4) * 64 + lane];
#pragma unroll
  for (int p = 0; p < NT2 / P; p++) {
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
      const int cb = (p * S4 + s4) & 1;
      // prefetch: the next step of this pass, or the first step of the next pass
      if (s4 + 1 < S4) {
#pragma unroll
        for (int q = 0; q < P; q++) w[cb ^ 1][q] = w2p[((int64_t)(p * P + q) * S4 + s4 + 1) * 64 + lane];
      } else if (p + 1 < NT2 / P) {
#pragma unroll
        for (int q = 0; q < P; q++) w[cb ^ 1][q] = w2p[((int64_t)((p + 1) * P + q) * S4) * 64 + lane];
      }
      // the scheduler would otherwise sink the prefetch into the registers this step frees last,
      // i.e. 8 MFMAs before their use instead of 4 P
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
      if constexpr (ILV) {  // the previous pass's output layer, IPS units behind these MFMAs
        if (p > 0) {
#pragma unroll
          for (int i = 0; i < IPS; i++) {
            const int u = s4 * IPS + i;
            if (u < P * 16) l3_unit(a2p, p - 1, u / 16, u % 16);
          }
        }
      }
    }
    if constexpr (VKO > 0) {  // layer 3 on the VALU: o[a] += W3[a][hidden] relu(h2) over this lane's half
      if constexpr (ILV) {
        if (p + 1 < NT2 / P) {  // (interleaved into the next pass)
#pragma unroll
          for (int q = 0; q < P; q++) a2p[q] = a2[q];
          continue;
        }
      }
#pragma unroll
      for (int q = 0; q < P; q++)
#pragma unroll
        for (int r = 0; r < 16; r++) l3_unit(a2, p, q, r);
      continue;
    }
    // layer 3 on this pass's slice: the fragments of tile q + 1 are in flight during tile q
    float4 w3[2][4];
#pragma unroll
    for (int r4 = 0; r4 < 4; r4++) w3[0][r4] = w3p[((int64_t)(p * P) * 4 + r4) * 64 + lane];
#pragma unroll
    for (int q = 0; q < P; q++) {
      if (q + 1 < P) {
#pragma unroll
        for (int r4 = 0; r4 < 4; r4++) w3[(q + 1) & 1][r4] = w3p[((int64_t)(p * P + q + 1) * 4 + r4) * 64 + lane];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int r4 = 0; r4 < 4; r4++) {
        const float4 wq = w3[q & 1][r4];
        a3 = __builtin_amdgcn_mfma_f32_32x32x2f32(wq.x, fmaxf(a2[q][r4 * 4 + 0], 0.0f), a3, 0, 0, 0);
        a3 = __builtin_amdgcn_mfma_f32_32x32x2f32(wq.y, fmaxf(a2[q][r4 * 4 + 1], 0.0f), a3, 0, 0, 0);
        a3 = __builtin_amdgcn_mfma_f32_32x32x2f32(wq.z, fmaxf(a2[q][r4 * 4 + 2], 0.0f), a3, 0, 0, 0);
        a3 = __builtin_amdgcn_mfma_f32_32x32x2f32(wq.w, fmaxf(a2[q][r4 * 4 + 3], 0.0f), a3, 0, 0, 0);
      }
    }
  }
  if constexpr (HEAD) {
#pragma unroll
    for (int a = 0; a < NO; a++) o3[a] += __shfl_xor(o3[a], 32);  // the other half's hidden units
    if (jv && h == 0) musigma_row<VKO>(sm, j, KO, o3);
  } else if constexpr (VKO > 0) {
#pragma unroll
    for (int a = 0; a < VKO; a++) o3[a] += __shfl_xor(o3[a], 32);  // the other half's hidden units
    if (jv && h == 0) {
      if (out) {
#pragma unroll
        for (int a = 0; a < VKO; a++)
          if (a < KO) out[j * KO + a] = o3[a];
      }
      if constexpr (VKO > 0) {
        if (sm.act) sample_row<VKO>(sm, j, KO, o3);
      }
    }
  } else if (jv && out) {  // (no sampling epilogue on the MFMA output layer: the host checks)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int row = mfma_row(r, h);
      if (row < KO) out[j * KO + row] = a3[r];
    }
  }
}

// Fused Linear -> ReLU -> Linear (one hidden layer: the reference's IPPO actor / critic [256],
// config_files/algorithms/ippo.yaml:46,52; the test configs' [128] and [1024] heads): the hidden
// layer is produced TB tiles of 32 units at a time (layer 1 exactly as in mlp3_relu_kernel) and
// folded into the output accumulators as soon as it is final, so any hidden size up to 1024 runs
// with 16 TB accumulator registers. VKO > 0: output layer on the VALU (weights in LDS), else on
// the MFMA (fragments from L2, KO <= 32 rows). EP = MlpMuSigma: the dual head, as in mlp3_relu_kernel.
// MULTI: as in mlp3_relu_kernel.
template <int TB, int WPE, int VKO, class EP = MlpSample, bool MULTI = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void mlp2_relu_kernel(
    const float* __restrict__ x, int64_t n, int L, int KS1, int NT1, const float4* __restrict__ w1p,
    const float* __restrict__ b1, const float4* __restrict__ w3p, const float* __restrict__ b3, int KO,
    float* __restrict__ out, const float* __restrict__ pre1, int grp, int prio, EP sm) {
  static_assert(VKO >= 0 && VKO <= 8, "VALU output layer: at most 8 outputs");
  constexpr bool HEAD = std::is_same<EP, MlpMuSigma>::value;
  static_assert(!HEAD || VKO > 0, "the dual head runs on the VALU output layer");
  constexpr int F4 = HEAD && VKO > 4 ? 4 : 2;  // float4 per (hidden pair, lane half) in LDS
  constexpr int NO = HEAD ? 2 * VKO : VKO;     // per-lane output sums
  if (MULTI ? (prio & 1) : prio) __builtin_amdgcn_s_setprio(3);
  const int lane = threadIdx.x & 63, h = lane >> 5;
  int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  int64_t pol = 0;
  if constexpr (MULTI) {  // n envs x grp policies: this block's policy and its 4 env tiles
    const unsigned nb = (unsigned)(((n + 31) / 32 + 3) / 4), np = (unsigned)grp;  // blocks per policy
    const unsigned be = (prio & 2) ? blockIdx.x / np : blockIdx.x % nb;
    pol = (prio & 2) ? blockIdx.x % np : blockIdx.x / nb;
    tile = (int64_t)be * 4 + (threadIdx.x >> 6);
    w1p += pol * (NT1 * ((KS1 + 3) / 4) * 64), b1 += pol * (NT1 * 32);
    w3p += pol * (VKO > 0 ? NT1 * 16 * 2 * F4 : NT1 * 4 * 64), b3 += pol * KO;
  }
  extern __shared__ float4 w3d[];  // VALU output layer: [NT1 * 16][2][8 floats] (16 for a dual head wider than 4)
  if constexpr (VKO > 0) {
    for (int i = threadIdx.x; i < NT1 * 16 * 2 * F4; i += blockDim.x) w3d[i] = w3p[i];
    __syncthreads();
  }
  if (tile * 32 >= n) return;  // wave-uniform
  const int64_t e = tile * 32 + (lane & 31);
  const int64_t j = MULTI ? e * grp + pol : e;  // the lane's row
  const bool jv = e < n;
  if constexpr (MULTI) grp = 1;  // pre1: one row per row
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
  mlp_f32x16 a3;
  float o3[VKO > 0 ? NO : 1];
  if constexpr (HEAD) {
#pragma unroll
    for (int a = 0; a < VKO; a++) {
      o3[a] = (h == 0 && a < KO) ? b3[a] : 0.0f;
      o3[VKO + a] = (h == 0 && a < KO) ? b3[KO + a] : 0.0f;
    }
  } else if constexpr (VKO > 0) {
#pragma unroll
    for (int a = 0; a < VKO; a++) o3[a] = (h == 0 && a < KO) ? b3[a] : 0.0f;
  } else {
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int row = mfma_row(r, h);
      a3[r] = row < KO ? b3[row] : 0.0f;
    }
  }
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
    // output layer over this group's hidden units (ReLU applied as they are read)
    if constexpr (HEAD) {
#pragma unroll
      for (int t = 0; t < TB; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const float hv = fmaxf(a1[t][r], 0.0f);
          const int sidx = ((g0 + t) * 16 + r) * 2 + h;
          float wm[8], wg[8];
#pragma unroll
          for (int f = 0; f < F4 / 2; f++) {
            const float4 u = w3d[sidx * F4 + f], v = w3d[sidx * F4 + F4 / 2 + f];
            wm[4 * f] = u.x, wm[4 * f + 1] = u.y, wm[4 * f + 2] = u.z, wm[4 * f + 3] = u.w;
            wg[4 * f] = v.x, wg[4 * f + 1] = v.y, wg[4 * f + 2] = v.z, wg[4 * f + 3] = v.w;
          }
#pragma unroll
          for (int a = 0; a < VKO; a++) {
            o3[a] = fmaf(wm[a], hv, o3[a]);
            o3[VKO + a] = fmaf(wg[a], hv, o3[VKO + a]);
          }
        }
    } else if constexpr (VKO > 0) {
#pragma unroll
      for (int t = 0; t < TB; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const float hv = fmaxf(a1[t][r], 0.0f);
          const int sidx = ((g0 + t) * 16 + r) * 2 + h;
          const float4 wa = w3d[sidx * 2];
          const float wv[4] = {wa.x, wa.y, wa.z, wa.w};
          float wh[4] = {0.f, 0.f, 0.f, 0.f};
          if constexpr (VKO > 4) {
            const float4 wb = w3d[sidx * 2 + 1];
            wh[0] = wb.x, wh[1] = wb.y, wh[2] = wb.z, wh[3] = wb.w;
          }
#pragma unroll
          for (int a = 0; a < VKO; a++) o3[a] = fmaf(a < 4 ? wv[a] : wh[a - 4], hv, o3[a]);
        }
    } else {
#pragma unroll
      for (int t = 0; t < TB; t++)
#pragma unroll
        for (int r4 = 0; r4 < 4; r4++) {
          const float4 wq = w3p[((int64_t)(g0 + t) * 4 + r4) * 64 + lane];
          a3 = __builtin_amdgcn_mfma_f32_32x32x2f32(wq.x, fmaxf(a1[t][r4 * 4 + 0], 0.0f), a3, 0, 0, 0);
          a3 = __builtin_amdgcn_mfma_f32_32x32x2f32(wq.y, fmaxf(a1[t][r4 * 4 + 1], 0.0f), a3, 0, 0, 0);
          a3 = __builtin_amdgcn_mfma_f32_32x32x2f32(wq.z, fmaxf(a1[t][r4 * 4 + 2], 0.0f), a3, 0, 0, 0);
          a3 = __builtin_amdgcn_mfma_f32_32x32x2f32(wq.w, fmaxf(a1[t][r4 * 4 + 3], 0.0f), a3, 0, 0, 0);
        }
    }
  }
  if constexpr (HEAD) {
#pragma unroll
    for (int a = 0; a < NO; a++) o3[a] += __shfl_xor(o3[a], 32);
    if (jv && h == 0) musigma_row<VKO>(sm, j, KO, o3);
  } else if constexpr (VKO > 0) {
#pragma unroll
    for (int a = 0; a < VKO; a++) o3[a] += __shfl_xor(o3[a], 32);
    if (jv && h == 0) {
      if (out) {
#pragma unroll
        for (int a = 0; a < VKO; a++)
          if (a < KO) out[j * KO + a] = o3[a];
      }
      if constexpr (VKO > 0) {
        if (sm.act) sample_row<VKO>(sm, j, KO, o3);
      }
    }
  } else if (jv && out) {  // (no sampling epilogue on the MFMA output layer: the host checks)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int row = mfma_row(r, h);
      if (row < KO) out[j * KO + row] = a3[r];
    }
  }
}

}  // namespace msc
