// Fused inference step of the rollout's GRU networks: one time step of a whole GRUNet -- nn.GRU
// (1 or 2 layers, batch_first, unidirectional) followed by its output projection [act,] Linear
// [, act] -- for n rows in one launch. Replaces GRUArchitecture.build's module
// (src/algorithms/models/architectures/gru.py:14-85) as BaseRLModule._forward_gru runs it on a
// [B, obs_dim] input (src/algorithms/models/rlmodules/base.py:99-141: gru(inputs, h) ->
// output_proj), with the state laid out as RLlib carries it, [B, num_layers, hidden]
// (get_initial_state, base.py:351-388).
//
// Same machinery as mlp.hip: one wave = 32 rows, every product computed transposed (hidden units on
// the MFMA's row axis, rows of the batch on its column axis = the lane) on v_mfma_f32_32x32x2_f32, the
// weights streamed from L2 as lane-major fragments packed once per weight version and prefetched one
// step ahead. Per tile of 32 hidden units a lane holds four accumulators
//   ar = b_ir + b_hr + W_ir x + W_hr h      az = b_iz + b_hz + W_iz x + W_hz h
//   ai = b_in + W_in x                      ah = b_hn + W_hn h
// and finishes the tile's h' = (1 - z) n + z h, r = sigma(ar), z = sigma(az), n = tanh(ai + r ah)
// (PyTorch's gate order and formula) into 16 kept registers: register 4g + i of lane half hf is hidden
// unit 32 t + 8 g + 4 hf + i, so the old state a tile needs element-wise is four float4 of h_in -- and
// the same four float4 of tile kt are the B operands of 16 k steps of W_h* (k permuted by the host
// packing, as the MLP's layer 2), so h_in is read in that one layout only, per tile, from cache.
// Layer 2 reads layer 1's h' straight from those kept registers; so does the output projection (MFMA,
// 32 outputs per pass). Registers per lane: 16 H/32 per held layer (two with 2 layers) + 64
// accumulators + 32 state fragments + 24 weight fragments. That fits the 512-register file in every
// form but 256 x 2, where the last layer's h' is kept in LDS instead (128 KiB per block, conflict-free,
// lane-private: see gru_layer's HS); the other forms use no LDS. No form uses scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>
#include <utility>

#include "env.hpp"
#include "mlp_kernels.hpp"  // mlp_f32x16, mfma_row, head_act

namespace msc {

#define MSC_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ void gru_acc_load(mlp_f32x16& a, const float* p, int hf) {
#pragma unroll
  for (int g = 0; g < 4; g++) {
    const float4 v = *reinterpret_cast<const float4*>(p + 8 * g + 4 * hf);
    a[4 * g] = v.x, a[4 * g + 1] = v.y, a[4 * g + 2] = v.z, a[4 * g + 3] = v.w;
  }
}

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>), in order
template <class F, int... Ts>
__device__ __forceinline__ void gru_static_for(F&& f, std::integer_sequence<int, Ts...>) {
  (f(std::integral_constant<int, Ts>{}), ...);
}

__device__ __forceinline__ float gru_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

// One GRU layer for the wave's 32 rows. FIRST: the input is x (features split between the lane
// halves as in mlp3_relu_kernel's layer 1, wi in its w1p layout over the 3 H gate rows); otherwise
// the input is the previous layer's h' in accumulator layout (wi in the w2p layout). hrow: the row's
// old state of this layer (h_in + (j layers + l) H); live = false reads it as zero (reset rows, rows
// past n). orow: where h' goes (nullptr: not stored).
// HS: h' goes to the block's LDS array hs ([NT 16][256 threads]: element (t, r) of a lane at
// (16 t + r) 256 + threadIdx.x, conflict-free and private to the lane, so no synchronisation) instead
// of hnew, with the output projection's act_pre (act_hs) already applied -- the 256 x 2 form, whose two held layers plus accumulators do not fit the register file.
template <int NT, bool FIRST, bool HS = false>
__device__ __forceinline__ void gru_layer(float* __restrict__ hs, const float* __restrict__ xr, bool jv, int L, int KS1,
                                          const mlp_f32x16 (&hprev)[NT], mlp_f32x16 (&hnew)[NT],
                                          const float4* __restrict__ wi, const float4* __restrict__ wh,
                                          const float* __restrict__ b, const float* __restrict__ hrow, bool live,
                                          float* __restrict__ orow, int lane, int hf, int act_hs = 0) {
  constexpr int H = NT * 32, S4 = NT * 4;
  const int M4 = (KS1 + 3) / 4;
  auto load_h = [&](int kt, mlp_f32x16& v) {
    gru_acc_load(v, hrow + kt * 32, hf);
#pragma unroll
    for (int r = 0; r < 16; r++) v[r] = live ? v[r] : 0.0f;
  };
  // one tile of 32 hidden units; t is a compile-time constant (gru_static_for), so hnew[t] / hprev[.]
  // are registers whatever the unroller's size limit makes of a loop this long
  auto tile = [&](auto tc) {
    constexpr int t = decltype(tc)::value;
    mlp_f32x16 ar, az, ai, ah;
    gru_acc_load(ar, b + t * 32, hf);
    gru_acc_load(az, b + H + t * 32, hf);
    gru_acc_load(ai, b + 2 * H + t * 32, hf);
    gru_acc_load(ah, b + 3 * H + t * 32, hf);
    // ---- input part: W_i{r,z,n} x ----
    if constexpr (FIRST) {
      const float4* pr = wi + ((int64_t)(0 * NT + t) * M4) * 64 + lane;
      const float4* pz = wi + ((int64_t)(1 * NT + t) * M4) * 64 + lane;
      const float4* pn = wi + ((int64_t)(2 * NT + t) * M4) * 64 + lane;
      auto load_x = [&](int m4, float (&xv)[4]) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int m = m4 * 4 + i, k = hf * KS1 + m;
          xv[i] = (jv && m < KS1 && k < L) ? xr[k] : 0.0f;
        }
      };
      float xc[4], xn[4];
      float4 cr = pr[0], cz = pz[0], cn = pn[0], nr, nz, nn;
      load_x(0, xc);
      for (int m4 = 0; m4 < M4; m4++) {
        const int nx = m4 + 1 < M4 ? m4 + 1 : m4;  // (the last step reloads itself: no branch)
        load_x(nx, xn);
        nr = pr[(int64_t)nx * 64], nz = pz[(int64_t)nx * 64], nn = pn[(int64_t)nx * 64];
        __builtin_amdgcn_sched_barrier(0);  // keep the prefetch ahead of this step's MFMAs
        ar = MSC_MFMA(cr.x, xc[0], ar), az = MSC_MFMA(cz.x, xc[0], az), ai = MSC_MFMA(cn.x, xc[0], ai);
        ar = MSC_MFMA(cr.y, xc[1], ar), az = MSC_MFMA(cz.y, xc[1], az), ai = MSC_MFMA(cn.y, xc[1], ai);
        ar = MSC_MFMA(cr.z, xc[2], ar), az = MSC_MFMA(cz.z, xc[2], az), ai = MSC_MFMA(cn.z, xc[2], ai);
        ar = MSC_MFMA(cr.w, xc[3], ar), az = MSC_MFMA(cz.w, xc[3], az), ai = MSC_MFMA(cn.w, xc[3], ai);
#pragma unroll
        for (int i = 0; i < 4; i++) xc[i] = xn[i];
        cr = nr, cz = nz, cn = nn;
      }
    } else {
      const float4* pr = wi + ((int64_t)(0 * NT + t) * S4) * 64 + lane;
      const float4* pz = wi + ((int64_t)(1 * NT + t) * S4) * 64 + lane;
      const float4* pn = wi + ((int64_t)(2 * NT + t) * S4) * 64 + lane;
      float4 w[2][3];
      w[0][0] = pr[0], w[0][1] = pz[0], w[0][2] = pn[0];
#pragma unroll
      for (int s4 = 0; s4 < S4; s4++) {
        const int cb = s4 & 1;
        if (s4 + 1 < S4) w[cb ^ 1][0] = pr[(s4 + 1) * 64], w[cb ^ 1][1] = pz[(s4 + 1) * 64], w[cb ^ 1][2] = pn[(s4 + 1) * 64];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int s = s4 * 4 + i;
          const float bv = hprev[s / 16][s % 16];
          const float4 &wr = w[cb][0], &wz = w[cb][1], &wn = w[cb][2];
          ar = MSC_MFMA(i == 0 ? wr.x : i == 1 ? wr.y : i == 2 ? wr.z : wr.w, bv, ar);
          az = MSC_MFMA(i == 0 ? wz.x : i == 1 ? wz.y : i == 2 ? wz.z : wz.w, bv, az);
          ai = MSC_MFMA(i == 0 ? wn.x : i == 1 ? wn.y : i == 2 ? wn.z : wn.w, bv, ai);
        }
      }
    }
    // ---- hidden part: W_h{r,z,n} h over the old state's tiles ----
    {
      const float4* pr = wh + ((int64_t)(0 * NT + t) * S4) * 64 + lane;
      const float4* pz = wh + ((int64_t)(1 * NT + t) * S4) * 64 + lane;
      const float4* pn = wh + ((int64_t)(2 * NT + t) * S4) * 64 + lane;
      mlp_f32x16 hc, hn;
      load_h(0, hc);
      float4 cr = pr[0], cz = pz[0], cn = pn[0], nr, nz, nn;
      for (int kt = 0; kt < NT; kt++) {
        load_h(kt + 1 < NT ? kt + 1 : kt, hn);
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int s4 = kt * 4 + q, nx = s4 + 1 < S4 ? s4 + 1 : s4;
          nr = pr[nx * 64], nz = pz[nx * 64], nn = pn[nx * 64];
          __builtin_amdgcn_sched_barrier(0);
          ar = MSC_MFMA(cr.x, hc[4 * q], ar), az = MSC_MFMA(cz.x, hc[4 * q], az), ah = MSC_MFMA(cn.x, hc[4 * q], ah);
          ar = MSC_MFMA(cr.y, hc[4 * q + 1], ar), az = MSC_MFMA(cz.y, hc[4 * q + 1], az), ah = MSC_MFMA(cn.y, hc[4 * q + 1], ah);
          ar = MSC_MFMA(cr.z, hc[4 * q + 2], ar), az = MSC_MFMA(cz.z, hc[4 * q + 2], az), ah = MSC_MFMA(cn.z, hc[4 * q + 2], ah);
          ar = MSC_MFMA(cr.w, hc[4 * q + 3], ar), az = MSC_MFMA(cz.w, hc[4 * q + 3], az), ah = MSC_MFMA(cn.w, hc[4 * q + 3], ah);
          cr = nr, cz = nz, cn = nn;
        }
        hc = hn;
      }
    }
    // ---- gates: this tile's h' (the old state element-wise: the same four float4 of tile t) ----
    mlp_f32x16 ho, hv;
    load_h(t, ho);
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const float rg = gru_sigmoid(ar[r]), zg = gru_sigmoid(az[r]);
      const float ng = tanhf(ai[r] + rg * ah[r]);
      hv[r] = (1.0f - zg) * ng + zg * ho[r];
    }
    if constexpr (HS) {
#pragma unroll
      for (int r = 0; r < 16; r++)
        hs[(t * 16 + r) * 256 + threadIdx.x] = act_hs != 0 ? head_act(act_hs, hv[r]) : hv[r];
    } else {
      hnew[t] = hv;
    }
    if (orow != nullptr && jv) {
#pragma unroll
      for (int g = 0; g < 4; g++)
        *reinterpret_cast<float4*>(orow + t * 32 + 8 * g + 4 * hf) =
            make_float4(hv[4 * g], hv[4 * g + 1], hv[4 * g + 2], hv[4 * g + 3]);
    }
  };
  gru_static_for(tile, std::make_integer_sequence<int, NT>{});
}

// The output projection on the last layer's h' (in registers), 32 outputs per pass:
// y = act_out(W_o act_pre(h') + b_o); wo in the w2p layout over ceil(KO / 32) 32 rows, zero past KO.
// HS: act_pre(h') is read from the lane's LDS column (gru_layer wrote it so) instead of hl.
template <int NT, bool HS = false>
__device__ __forceinline__ void gru_project(const float* __restrict__ hs, mlp_f32x16 (&hl)[NT], const float4* __restrict__ wo,
                                            const float* __restrict__ bo, int KO, int act_pre, int act_out,
                                            float* __restrict__ y, int64_t j, bool jv, int lane, int hf) {
  constexpr int S4 = NT * 4;
  if (!HS && act_pre != 0) {
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
      for (int r = 0; r < 16; r++) hl[t][r] = head_act(act_pre, hl[t][r]);
  }
  auto hval = [&](int u) {  // unit u = 16 tile + register of the last layer's h' (after act_pre)
    if constexpr (HS) {
      return hs[u * 256 + threadIdx.x];
    } else {
      return hl[u / 16][u % 16];
    }
  };
  const int OT = (KO + 31) / 32;
  const bool v4 = (KO & 3) == 0;  // rows 8g + 4hf .. + 3 of a pass are four consecutive outputs
  for (int q = 0; q < OT; q++) {
    mlp_f32x16 a3;
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int row = q * 32 + mfma_row(r, hf);
      a3[r] = row < KO ? bo[row] : 0.0f;
    }
    const float4* pq = wo + ((int64_t)q * S4) * 64 + lane;
    float4 wq[2];
    wq[0] = pq[0];
#pragma unroll
    for (int s4 = 0; s4 < S4; s4++) {
      const int cb = s4 & 1;
      if (s4 + 1 < S4) wq[cb ^ 1] = pq[(s4 + 1) * 64];
      __builtin_amdgcn_sched_barrier(0);
      a3 = MSC_MFMA(wq[cb].x, hval(s4 * 4 + 0), a3);
      a3 = MSC_MFMA(wq[cb].y, hval(s4 * 4 + 1), a3);
      a3 = MSC_MFMA(wq[cb].z, hval(s4 * 4 + 2), a3);
      a3 = MSC_MFMA(wq[cb].w, hval(s4 * 4 + 3), a3);
    }
    if (act_out != 0) {
#pragma unroll
      for (int r = 0; r < 16; r++) a3[r] = head_act(act_out, a3[r]);
    }
    if (jv) {
      float* yr = y + j * (int64_t)KO + q * 32;
      if (v4) {
#pragma unroll
        for (int g = 0; g < 4; g++)
          if (q * 32 + 8 * g + 4 * hf < KO)
            *reinterpret_cast<float4*>(yr + 8 * g + 4 * hf) =
                make_float4(a3[4 * g], a3[4 * g + 1], a3[4 * g + 2], a3[4 * g + 3]);
      } else {
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const int row = mfma_row(r, hf);
          if (q * 32 + row < KO) yr[row] = a3[r];
        }
      }
    }
  }
}

template <int NT, int LAYERS, int WPE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void gru_step_kernel(
    const float* __restrict__ x, int64_t n, int L, int KS1, const float* __restrict__ h_in, GruWeights w, int KO,
    int act_pre, int act_out, const uint8_t* __restrict__ reset, int grp, float* __restrict__ y,
    float* __restrict__ h_out) {
  static_assert(LAYERS == 1 || LAYERS == 2, "1 or 2 GRU layers");
  constexpr int H = NT * 32;
  const int lane = threadIdx.x & 63, hf = lane >> 5;
  const int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tile * 32 >= n) return;  // wave-uniform (no block-level synchronisation below)
  const int64_t j = tile * 32 + (lane & 31);
  const bool jv = j < n;
  const int64_t jc = jv ? j : 0;  // rows past n read row 0 and store nothing
  const bool live = jv && !(reset != nullptr && reset[jc / grp] != 0);
  const float* xr = x + jc * (int64_t)L;
  const float* hrow = h_in + jc * (int64_t)(LAYERS * H);
  float* orow = h_out != nullptr ? h_out + jc * (int64_t)(LAYERS * H) : nullptr;
  const float4* wo = reinterpret_cast<const float4*>(w.wo);

  constexpr bool HS = NT == 8 && LAYERS == 2;  // the last layer's h' in LDS (128 KiB per block of 4 waves)
  __shared__ float hs[HS ? NT * 16 * 256 : 1];
  mlp_f32x16 h1[NT];
  gru_layer<NT, true>(hs, xr, jv, L, KS1, h1, h1, reinterpret_cast<const float4*>(w.wi[0]),
                      reinterpret_cast<const float4*>(w.wh[0]), w.b[0], hrow, live, orow, lane, hf);
  if constexpr (LAYERS == 2 && HS) {  // (hnew is unused with HS)
    gru_layer<NT, false, true>(hs, xr, jv, L, KS1, h1, h1, reinterpret_cast<const float4*>(w.wi[1]),
                               reinterpret_cast<const float4*>(w.wh[1]), w.b[1], hrow + H, live,
                               orow != nullptr ? orow + H : nullptr, lane, hf, act_pre);
    gru_project<NT, true>(hs, h1, wo, w.bo, KO, act_pre, act_out, y, j, jv, lane, hf);
  } else if constexpr (LAYERS == 2) {
    mlp_f32x16 h2[NT];
    gru_layer<NT, false>(hs, xr, jv, L, KS1, h1, h2, reinterpret_cast<const float4*>(w.wi[1]),
                         reinterpret_cast<const float4*>(w.wh[1]), w.b[1], hrow + H, live,
                         orow != nullptr ? orow + H : nullptr, lane, hf);
    gru_project<NT>(hs, h2, wo, w.bo, KO, act_pre, act_out, y, j, jv, lane, hf);
  } else {
    gru_project<NT>(hs, h1, wo, w.bo, KO, act_pre, act_out, y, j, jv, lane, hf);
  }
}

bool gru_supported(int L, int H, int layers, int KO) {
  return (H == 64 || H == 128 || H == 256) && (layers == 1 || layers == 2) && L >= 1 && L <= 1024 &&
         ((KO >= 1 && KO <= 32) || (KO % 32 == 0 && KO <= 256));
}

hipError_t launch_gru_step(const float* x, int64_t n, int L, int H, int layers, int KO, const float* h_in,
                           const GruWeights& w, int act_pre, int act_out, const uint8_t* reset, int grp, float* y,
                           float* h_out, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (!gru_supported(L, H, layers, KO)) return hipErrorInvalidValue;
  const int KS1 = (L + 1) / 2;
  const int64_t tiles = (n + 31) / 32;
  const dim3 grid((unsigned)((tiles + 3) / 4)), block(256);
#define MSC_GRU_LAUNCH(NT, LY, WPE)                                                                                 \
  hipLaunchKernelGGL((gru_step_kernel<NT, LY, WPE>), grid, block, 0, st, x, n, L, KS1, h_in, w, KO, act_pre, act_out, \
                     reset, grp, y, h_out)
  // (NT, layers) sets the register budget (16 NT per held layer + ~150) and with it the waves per SIMD
  if (H == 64 && layers == 1) MSC_GRU_LAUNCH(2, 1, 2);
  else if (H == 64) MSC_GRU_LAUNCH(2, 2, 2);
  else if (H == 128 && layers == 1) MSC_GRU_LAUNCH(4, 1, 2);
  else if (H == 128) MSC_GRU_LAUNCH(4, 2, 1);
  else if (layers == 1) MSC_GRU_LAUNCH(8, 1, 1);
  else MSC_GRU_LAUNCH(8, 2, 1);
#undef MSC_GRU_LAUNCH
  return hipGetLastError();
}

}  // namespace msc
