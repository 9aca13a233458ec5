// policy.hip -- the heuristic baseline policies' action kernel (msc_policy_act, include/marlsc.h).
//
// One launch writes the actions [E][W][K] of every env from the handle's own device state, between
// two env steps: fixed base-stock levels, the adaptive (rolling mean / variance) base-stock rule, or
// uniform random actions, each env with its own candidate index into small parameter tables, so a
// hyper-parameter sweep is one handle whose envs are (candidate, episode) pairs.
//
// Shape: a block owns 64 consecutive envs, one per lane, and its PW waves split the (warehouse, SKU)
// components between them. Every state field is [component][E], env fastest, so each load is one
// coalesced 256-B access per wave. The actions are [E][W][K]: a lane-per-env store would have a
// stride of W*K floats, so each chunk of up to PCH components is staged in LDS (row stride PCH + 1,
// odd: the 64 lanes of a wave write 64 different banks) and the block writes the chunk's
// [64][columns] range with consecutive threads on consecutive floats, as step_c_kernel does for the
// observations. K is a runtime value: the arithmetic per component is a handful of f64 operations
// behind RING + 1 (adaptive: + 2 n) loads, nothing a per-SKU-count instantiation would speed up.
//
// All arithmetic is what the reference's numpy does (run_baselines.py:193-205, :255-292), f64 unless
// numpy's is f32, and the build sets -ffp-contract=off: tests/test_gpu_baselines.py holds the actions
// to a numpy restatement bit for bit.
#include <hip/hip_runtime.h>

#include "env.hpp"
#include "kcommon.hpp"

namespace msc {

constexpr int PW = 8;    // waves per block: components i0 + wave, i0 + wave + PW, ...
constexpr int PCH = 64;  // components staged per chunk (16.25 KiB of LDS per block)
constexpr int PRS = PCH + 1;

template <int KIND>
__global__ __launch_bounds__(BS* PW) void policy_act_kernel(const DevEnv* __restrict__ dp, PolicyDev p,
                                                           float* __restrict__ actions) {
  const EnvConst& c = dp->c;
  const EnvState& s = dp->s;
  __shared__ float stg[BS * PRS];
  const int lane = (int)threadIdx.x & (BS - 1), wave = (int)threadIdx.x / BS;
  const int64_t E = c.E, e0 = (int64_t)blockIdx.x * BS, e = e0 + lane;
  const bool ev = e < E;  // tail lanes load and store nothing (they still reach every barrier)
  const int K = c.K, WK = c.W * K, RING = c.RING;
  const int nenv = E - e0 < BS ? (int)(E - e0) : BS;

  int ca = 0, t = 0, cnt = 0, H = 1;
  double z = 0.0;
  Pcg64 r = {};
  if (ev) {
    ca = gp(p.cand)[e];
    if (KIND == MSC_POLICY_ADAPTIVE) {
      t = s.t[e];
      cnt = gp(p.count)[e];
      z = gp(p.z)[ca];
      H = gp(p.H)[ca];
    }
    if (KIND == MSC_POLICY_RANDOM && wave == 0) {
      r.s_hi = gp(p.rng)[e];
      r.s_lo = gp(p.rng)[E + e];
      r.i_hi = gp(p.rng)[2 * E + e];
      r.i_lo = gp(p.rng)[3 * E + e];
    }
  }
  if (KIND == MSC_POLICY_ADAPTIVE) {
    __syncthreads();  // every wave has read the env's count before wave 0 replaces it
    if (ev && wave == 0) gp(p.count)[e] = t == 0 ? 0 : cnt + 1;
  }
  // adaptive: this call's demand goes to slot cnt % h_max; the window is the last n entries with it
  const int hm = p.h_max > 0 ? p.h_max : 1;
  const int slot_new = cnt % hm;
  const int n = cnt + 1 < H ? cnt + 1 : H;
  int slot_first = (cnt + 1 - n) % hm;

  // the action of component i given its order-up-to level S
  auto order_up_to = [&](int i, double S) -> float {
    const int inv = s.inv[(int64_t)i * E + e];
    const auto* rq = s.ring_q + (int64_t)i * RING * E + e;
    int pend = 0;  // arrived ring slots are zero: the pending total is the sum over the whole ring
#pragma unroll 4
    for (int jr = 0; jr < RING; jr++) pend += rq[(int64_t)jr * E];
    const double maxq = c.act_param[i % K];
    const double x = S - (double)inv - (double)pend;
    const double q = fmin(fmax(x, 0.0), maxq);
    return (float)(2.0 * q / maxq - 1.0);
  };

  for (int i0 = 0; i0 < WK; i0 += PCH) {
    const int nc = WK - i0 < PCH ? WK - i0 : PCH;
    if (KIND == MSC_POLICY_RANDOM) {
      // the env's stream is sequential in (agent, SKU) order: one wave draws the chunk
      if (ev && wave == 0)
        for (int j = 0; j < nc; j++) stg[lane * PRS + j] = (float)(-1.0 + 2.0 * pcg_double(r));
    } else if (ev) {
      for (int j = wave; j < nc; j += PW) {
        const int i = i0 + j;
        float a;
        if (KIND == MSC_POLICY_BASE_STOCK) {
          a = order_up_to(i, gp(p.S)[(int64_t)ca * WK + i]);
        } else if (t == 0) {
          a = -1.0f;  // no demand observed yet: order nothing
        } else {
          const int x_new = s.inc[(int64_t)i * E + e];
          int32_t MSC_GLOBAL* h = gp(p.hist) + (int64_t)i * E + e;  // slot q at h[q * WK * E]
          const int64_t hs = (int64_t)WK * E;
          h[slot_new * hs] = x_new;
          // numpy's axis-0 mean / var of the f32 window, oldest entry first
          float sum = 0.0f;
          int q = slot_first;
#pragma unroll 4
          for (int m = 0; m < n - 1; m++) {
            sum += (float)h[q * hs];
            q = q + 1 == hm ? 0 : q + 1;
          }
          sum += (float)x_new;
          const float mean = sum / (float)n;
          float var = mean;
          if (n > 1) {
            float sq = 0.0f;
            q = slot_first;
#pragma unroll 4
            for (int m = 0; m < n - 1; m++) {
              const float d = (float)h[q * hs] - mean;
              sq += d * d;
              q = q + 1 == hm ? 0 : q + 1;
            }
            const float d = (float)x_new - mean;
            sq += d * d;
            var = sq / (float)n;
          }
          const double L = (double)c.elt[i];
          a = order_up_to(i, L * (double)mean + z * sqrt(L * (double)var));
        }
        stg[lane * PRS + j] = a;
      }
    }
    __syncthreads();
    // the block's [nenv][nc] range of this chunk, consecutive threads on consecutive floats
    float* dst = actions + e0 * WK + i0;
    for (int idx = (int)threadIdx.x; idx < nenv * nc; idx += BS * PW) {
      const int el = idx / nc, j = idx - el * nc;
      dst[(int64_t)el * WK + j] = stg[el * PRS + j];
    }
    if (i0 + PCH < WK) __syncthreads();  // the next chunk rewrites the stage
  }
  if (KIND == MSC_POLICY_RANDOM && ev && wave == 0) {
    gp(p.rng)[e] = r.s_hi;
    gp(p.rng)[E + e] = r.s_lo;
  }
}

hipError_t launch_policy_act(const EnvConst& c, const DevEnv* d, const PolicyDev& p, float* actions, hipStream_t st) {
  if (c.E <= 0) return hipSuccess;
  const dim3 grid((unsigned)((c.E + BS - 1) / BS)), block(BS * PW);
  switch (p.kind) {
    case MSC_POLICY_BASE_STOCK:
      hipLaunchKernelGGL(policy_act_kernel<MSC_POLICY_BASE_STOCK>, grid, block, 0, st, d, p, actions);
      break;
    case MSC_POLICY_ADAPTIVE:
      hipLaunchKernelGGL(policy_act_kernel<MSC_POLICY_ADAPTIVE>, grid, block, 0, st, d, p, actions);
      break;
    case MSC_POLICY_RANDOM:
      hipLaunchKernelGGL(policy_act_kernel<MSC_POLICY_RANDOM>, grid, block, 0, st, d, p, actions);
      break;
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace msc
