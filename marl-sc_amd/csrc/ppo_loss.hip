// ppo_loss.hip -- the PPO minibatch loss, its statistics and its gradients with respect to the network
// outputs in one launch (RLlib 2.52.1 PPOTorchLearner.compute_loss_for_module with the reference's
// hysteretic advantage weighting, src/algorithms/learners/hysteretic_learner.py:35-42; restated in
// marlsc/ppo.py:ppo_loss, which stays the definition and the tests' float64 yardstick).
//
// Output row i reads batch row b = idx[i] (or i): the kernel gathers the minibatch itself. Per row,
// every operation a float32 + - * / or expf, none contracted, in torch's order where the order shows:
//   std = exp(ls), var = std std, d = a - m, t = d d / (2 var)
//   logp = sum_k (-t - ls) - K log(2 pi)/2,  ent = sum_k (ls + log(2 pi e)/2)
//   kl   = sum_k (((ls - ls0) + u) - 1/2),   u = (exp(2 ls0) + (m0 - m)^2) / (2 exp(2 ls))
//   (logp's constant enters once per row; at K = 1 every chain is torch's own, rounding for rounding)
//   r = exp(logp - logp_old), A' = A (A >= 0) or beta A, s1 = A' r, s2 = A' clamp(r, lo, hi)
//   surr = min(s1, s2), vf = (v - t)^2, vfc = clamp(vf, 0, vf_clip)
//   row loss = (-surr + c_v vfc) - c_e ent
// and total = mean(row loss) + kl_coeff mean(kl). The gradients are torch autograd's, kinks included:
//   w = A' when s1 < s2; A' [lo <= r <= hi] when s1 > s2; A'/2 + (A'/2) [lo <= r <= hi] at a tie
//       (torch.minimum splits a tie, torch.clamp passes the gradient at its bounds, inclusive);
//   g = (-w / n) r;  dtotal/dm_k = g d / var - (kl_coeff / n) (m0 - m) / exp(2 ls)
//   dtotal/dls_k = g (2 t - 1) - c_e / n + (kl_coeff / n) (1 - 2 u)
//   dtotal/dv = (c_v / n) 2 (v - t) [0 <= vf <= vf_clip]
// so a clipped surrogate (w = 0) without the KL term gives dtotal/dm = +-0 exactly and a clipped value
// error gives dtotal/dv = 0 exactly.
//
// Layout: a group of G lanes per row (G the smallest power of two >= K, one column per lane; 64 lanes
// with two columns each, k and k + 64, for 64 < K <= 128), 256 / G rows per block and grid-stride
// step. Consecutive lanes read consecutive floats of the [n][K] arrays, and with idx == NULL a wave
// reads 64 / G adjacent rows. The K-sums are xor butterflies inside the group (every lane ends with
// the same bits). The cross-row sums -- the five statistics, and the [K] gradient of a shared
// log_std row -- are float64: per lane over the grid-stride loop, per wave by butterfly, per block
// through LDS in wave order, into partials [grid][PL_PS] of the caller's workspace;
// ppo_loss_finalize_kernel (one block, same stream) adds the partials in block order inside up to 16
// segments and the segment sums in segment order. No atomics: the grid and the segments are functions of
// (n, K) alone, so the results are bitwise reproducible.
//
// Multi-policy form (msc_ppo_loss_multi): P policies' losses in one launch, grid (ppo_loss_grid(n, K), P) with
// blockIdx.y the policy. Output row i of policy p is element o = i P + p of the stacked [n][P][K] / [n][P]
// operands (and of idx; b = o without one); a shared log_std is row p of [P][K]. The rows of a policy map to
// blocks, lanes and loop steps exactly as in the single launch for (n, K), ppo_loss_rows is the one body of
// both, the partials are [P][grid][PL_PS] and the finalize launch has one block per policy, each the
// single-policy finalize on its policy's partials: per policy every output has the single launch's bits.
// kl_coeff alone differs per policy and travels in the kernel arguments (PL_MAX_POLICIES floats).
#include <hip/hip_runtime.h>
#include <math.h>

#include "env.hpp"

namespace msc {

constexpr int PL_BS = 256;
constexpr int PL_MAX_GRID = 2048;  // 256 CUs x 8 blocks; the rest by grid stride
constexpr int PL_NSTAT = 5;
constexpr int PL_LS0 = 8;             // first log_std column of a partial
constexpr int PL_PS = PL_LS0 + 128;   // doubles per block partial

__host__ __device__ constexpr int pl_group(int K) {
  int g = 1;
  while (g < K && g < 64) g <<= 1;
  return g;
}

// The block's share of one policy's rows. MULTI: policy p of P, operands stacked [n][P][..]; otherwise P = 1,
// p = 0 and the element index is the row.
template <int G, int E, bool MULTI>
__device__ __forceinline__ void ppo_loss_rows(const PpoLossArgs& a, const int64_t P, const int64_t p,
                                              const float kl_coeff, double* __restrict__ part) {
  constexpr int RPB = PL_BS / G;
  constexpr float HALF_LOG2PI = 0.91893853320467274178f, ENT_CONST = 1.41893853320467274178f;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k0 = tid % G;
  const int K = a.K;
  double acc[PL_NSTAT] = {0.0, 0.0, 0.0, 0.0, 0.0};
  double acc_ls[E];
#pragma unroll
  for (int e = 0; e < E; e++) acc_ls[e] = 0.0;
  const float gk = kl_coeff * a.inv_n, ge = a.c_e * a.inv_n, gv = a.c_v * a.inv_n;

  for (int64_t base = (int64_t)blockIdx.x * RPB; base < a.n; base += (int64_t)gridDim.x * RPB) {
    const int64_t row = base + tid / G;
    const bool act = row < a.n;
    const int64_t o = MULTI ? row * P + p : row;  // the row's element of mean / values / idx and their gradients
    const int64_t b = act ? (a.idx ? a.idx[o] : o) : 0;
    float lp = 0.0f, ent = 0.0f, kl = 0.0f;
    float dmu[E], dls[E], kmu[E], kls[E];
#pragma unroll
    for (int e = 0; e < E; e++) {
      const int k = k0 + 64 * e;
      dmu[e] = dls[e] = kmu[e] = kls[e] = 0.0f;
      if (act && k < K) {
        const float m = a.mean[o * K + k];
        const float ls = a.shared ? a.log_std[(MULTI ? p * K : 0) + k] : a.log_std[o * K + k];
        const float ac = a.actions[b * K + k];
        const float std_ = expf(ls);
        const float var = std_ * std_;
        const float d = ac - m;
        const float t = (d * d) / (2.0f * var);
        lp += -t - ls;
        ent += ls + ENT_CONST;
        dmu[e] = d / var;
        dls[e] = 2.0f * t - 1.0f;
        if (a.use_kl) {
          const float m0 = a.mean_old[b * K + k], ls0 = a.log_std_old[b * K + k];
          const float v0 = expf(2.0f * ls0), v1 = expf(2.0f * ls);
          const float dm = m0 - m;
          const float u = (v0 + dm * dm) / (2.0f * v1);
          kl += ((ls - ls0) + u) - 0.5f;
          kmu[e] = -(dm / v1);
          kls[e] = 1.0f - 2.0f * u;
        }
      }
    }
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) {  // the lane's own columns are summed already
      lp += __shfl_xor(lp, off);
      ent += __shfl_xor(ent, off);
      kl += __shfl_xor(kl, off);
    }
    // logp's constant once per row, not once per column: the error of logp is amplified by the ratio, and
    // K roundings of a sum near K log(2 pi)/2 are most of it. The entropy and the KL keep torch's
    // per-column constants: both can cancel to nearly nothing (log_std near -log(2 pi e)/2, a KL near
    // its target), and there the per-column form loses nothing.
    lp = lp - (float)K * HALF_LOG2PI;
    float g = 0.0f, gval = 0.0f, row_loss = 0.0f, surr = 0.0f, vfc = 0.0f;
    if (act) {
      float A = a.advantages[b];
      if (a.beta < 1.0f && !(A >= 0.0f)) A = A * a.beta;
      const float r = expf(lp - a.logp_old[b]);
      const float rc = fminf(fmaxf(r, a.lo), a.hi);
      const float s1 = A * r, s2 = A * rc;
      surr = fminf(s1, s2);
      const bool inr = r >= a.lo && r <= a.hi;
      float w;
      if (s1 < s2) w = A;
      else if (s1 > s2) w = inr ? A : 0.0f;
      else w = 0.5f * A + (inr ? 0.5f * A : 0.0f);
      g = (-a.inv_n * w) * r;
      const float dv = a.values[o] - a.value_targets[b];
      const float vf = dv * dv;
      vfc = fminf(fmaxf(vf, 0.0f), a.vf_clip);
      gval = (vf >= 0.0f && vf <= a.vf_clip) ? gv * (2.0f * dv) : 0.0f;
      row_loss = (-surr + a.c_v * vfc) - a.c_e * ent;
    }
#pragma unroll
    for (int e = 0; e < E; e++) {
      const int k = k0 + 64 * e;
      if (act && k < K) {
        float gm = g * dmu[e];
        float gl = g * dls[e] - ge;
        if (a.use_kl) {
          gm += gk * kmu[e];
          gl += gk * kls[e];
        }
        a.grad_mean[o * K + k] = gm;
        if (a.shared) acc_ls[e] += (double)gl;
        else a.grad_log_std[o * K + k] = gl;
      }
    }
    if (act && k0 == 0) {
      a.grad_values[o] = gval;
      acc[0] += (double)row_loss;
      acc[1] += (double)(-surr);
      acc[2] += (double)vfc;
      acc[3] += (double)ent;
      acc[4] += (double)kl;
    }
  }

  // block partial: butterflies over the wave, then the four waves in order
  __shared__ double sm[PL_BS / 64][PL_PS];
#pragma unroll
  for (int s = 0; s < PL_NSTAT; s++) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc[s] += __shfl_xor(acc[s], off);
  }
#pragma unroll
  for (int e = 0; e < E; e++) {
#pragma unroll
    for (int off = 32; off >= G; off >>= 1) acc_ls[e] += __shfl_xor(acc_ls[e], off);
  }
  if (lane == 0) {
#pragma unroll
    for (int s = 0; s < PL_NSTAT; s++) sm[wave][s] = acc[s];
  }
  if (lane < G) {
#pragma unroll
    for (int e = 0; e < E; e++) sm[wave][PL_LS0 + lane + 64 * e] = acc_ls[e];
  }
  __syncthreads();
  if (tid < PL_NSTAT || (tid >= PL_LS0 && tid - PL_LS0 < K)) {  // K <= G E: every column read was written
    double s = sm[0][tid];
#pragma unroll
    for (int w = 1; w < PL_BS / 64; w++) s += sm[w][tid];
    part[(int64_t)blockIdx.x * PL_PS + tid] = s;
  }
}

template <int G, int E>
__global__ __launch_bounds__(PL_BS) void ppo_loss_kernel(const PpoLossArgs a, double* __restrict__ part) {
  ppo_loss_rows<G, E, false>(a, 1, 0, a.kl_coeff, part);
}

template <int G, int E>
__global__ __launch_bounds__(PL_BS) void ppo_loss_multi_kernel(const PpoLossMultiArgs m, double* __restrict__ part) {
  const int p = blockIdx.y;
  ppo_loss_rows<G, E, true>(m.a, m.P, p, m.kl_coeff[p], part + (int64_t)p * gridDim.x * PL_PS);
}

// one block: every column of the partials summed over the blocks in a fixed order. The 256 threads are Q
// segments x Wc column slots (Wc the power of two >= the columns in use, at least 16: Q = 16 at K <= 8, 1 at
// K > 120); a thread adds its segment's blocks in block order, 16 loads in flight at a time, and the
// column's thread of segment 0 adds the Q segment sums in segment order.
__device__ __forceinline__ void ppo_loss_finalize(const double* __restrict__ part, int nblk, int64_t n, int K,
                                                  int shared, int accumulate, float kl_coeff,
                                                  float* __restrict__ grad_log_std, float* __restrict__ total,
                                                  double* __restrict__ stats) {
  __shared__ double seg[PL_BS];
  __shared__ double sm[PL_NSTAT];
  const int t = threadIdx.x;
  const int NC = PL_LS0 + (shared ? K : 0);
  int Wc = 16;
  while (Wc < NC) Wc <<= 1;
  const int Q = PL_BS / Wc;
  const int c = t % Wc, q = t / Wc;
  const bool used = c < PL_NSTAT || (c >= PL_LS0 && c < NC);
  const int per = (nblk + Q - 1) / Q;
  const int b0 = q * per, b1 = b0 + per < nblk ? b0 + per : nblk;
  double s = 0.0;
  if (used) {
    int b = b0;
    for (; b + 16 <= b1; b += 16) {
      double v[16];
#pragma unroll
      for (int j = 0; j < 16; j++) v[j] = part[(int64_t)(b + j) * PL_PS + c];
#pragma unroll
      for (int j = 0; j < 16; j++) s += v[j];
    }
    for (; b < b1; b++) s += part[(int64_t)b * PL_PS + c];
  }
  seg[t] = s;  // slot q * Wc + c
  __syncthreads();
  if (q == 0 && used) {
    double r = seg[c];
    for (int j = 1; j < Q; j++) r += seg[j * Wc + c];
    if (c >= PL_LS0) grad_log_std[c - PL_LS0] = (float)r;
    else sm[c] = r;
  }
  __syncthreads();
  if (t == 0) {
    const double inv = 1.0 / (double)n;
    const double kl = sm[4] * inv;
    const double tot = sm[0] * inv + (double)kl_coeff * kl;
    const double o[PL_NSTAT] = {tot, sm[1] * inv, sm[2] * inv, sm[3] * inv, kl};
    *total = (float)tot;
    for (int i = 0; i < PL_NSTAT; i++) stats[i] = accumulate ? stats[i] + o[i] : o[i];
  }
}

__global__ __launch_bounds__(PL_BS) void ppo_loss_finalize_kernel(const double* __restrict__ part, int nblk, int64_t n,
                                                                int K, int shared, int accumulate, float kl_coeff,
                                                                float* __restrict__ grad_log_std,
                                                                float* __restrict__ total, double* __restrict__ stats) {
  ppo_loss_finalize(part, nblk, n, K, shared, accumulate, kl_coeff, grad_log_std, total, stats);
}

// block p: policy p's partials into grad_log_std[p] (shared rows), totals[p] and stats[p]
__global__ __launch_bounds__(PL_BS) void ppo_loss_finalize_multi_kernel(const PpoLossMultiArgs m,
                                                                      const double* __restrict__ part, int nblk,
                                                                      int accumulate, float* __restrict__ totals,
                                                                      double* __restrict__ stats) {
  const int p = blockIdx.x;
  ppo_loss_finalize(part + (int64_t)p * nblk * PL_PS, nblk, m.a.n, m.a.K, m.a.shared, accumulate, m.kl_coeff[p],
                    m.a.grad_log_std + (int64_t)p * m.a.K, totals + p, stats + (int64_t)p * PL_NSTAT);
}

int ppo_loss_rows_per_block(int32_t K) { return PL_BS / pl_group(K); }
int ppo_loss_grid(int64_t n, int32_t K) {
  const int64_t rpb = ppo_loss_rows_per_block(K);
  const int64_t nb = (n + rpb - 1) / rpb;
  return (int)(nb < PL_MAX_GRID ? nb : PL_MAX_GRID);
}
int64_t ppo_loss_workspace_bytes(int64_t n, int32_t K) {
  return (int64_t)ppo_loss_grid(n, K) * PL_PS * (int64_t)sizeof(double);
}

// one (G, E) instantiation of KERNEL for K columns
#define PL_DISPATCH(K_, LAUNCH)      \
  do {                               \
    const int G_ = pl_group(K_);     \
    if ((K_) > 64) LAUNCH(64, 2);    \
    else if (G_ == 64) LAUNCH(64, 1); \
    else if (G_ == 32) LAUNCH(32, 1); \
    else if (G_ == 16) LAUNCH(16, 1); \
    else if (G_ == 8) LAUNCH(8, 1);  \
    else if (G_ == 4) LAUNCH(4, 1);  \
    else if (G_ == 2) LAUNCH(2, 1);  \
    else LAUNCH(1, 1);               \
  } while (0)

hipError_t launch_ppo_loss(const PpoLossArgs& a, int accumulate, float* total, double* stats, void* workspace,
                           hipStream_t st) {
  const int nb = ppo_loss_grid(a.n, a.K);
  double* part = (double*)workspace;
#define PL_LAUNCH(GG, EE) \
  hipLaunchKernelGGL((ppo_loss_kernel<GG, EE>), dim3(nb), dim3(PL_BS), 0, st, a, part)
  PL_DISPATCH(a.K, PL_LAUNCH);
#undef PL_LAUNCH
  hipLaunchKernelGGL(ppo_loss_finalize_kernel, dim3(1), dim3(PL_BS), 0, st, part, nb, a.n, a.K, a.shared, accumulate,
                     a.kl_coeff, a.grad_log_std, total, stats);
  return hipGetLastError();
}

hipError_t launch_ppo_loss_multi(const PpoLossMultiArgs& m, int accumulate, float* totals, double* stats,
                                 void* workspace, hipStream_t st) {
  const int nb = ppo_loss_grid(m.a.n, m.a.K);
  double* part = (double*)workspace;
#define PL_LAUNCH(GG, EE) \
  hipLaunchKernelGGL((ppo_loss_multi_kernel<GG, EE>), dim3(nb, m.P), dim3(PL_BS), 0, st, m, part)
  PL_DISPATCH(m.a.K, PL_LAUNCH);
#undef PL_LAUNCH
  hipLaunchKernelGGL(ppo_loss_finalize_multi_kernel, dim3(m.P), dim3(PL_BS), 0, st, m, part, nb, accumulate, totals,
                     stats);
  return hipGetLastError();
}

}  // namespace msc
