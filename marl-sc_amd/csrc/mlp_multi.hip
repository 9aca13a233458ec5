// Per-agent policies (parameter_sharing: false, the reference schema's default: one RLModule per
// warehouse, ippo.py:106 / mappo.py:103) in one launch: P same-shaped MLPs with P weight sets over rows
// laid out [E envs][P policies], the MULTI instantiations of the kernel templates of mlp_kernels.hpp.
// The launchers are mlp.hip's (mlp_relu_launch.hpp, one template over MULTI: the same form table and
// output-layer choice), so policy p's rows are bit-identical to launch_mlp{3,2}_relu on policy p's rows
// gathered contiguously.
//
// Work split: a wave owns 32 envs of one policy, a block 4 such tiles of the same policy (the VALU
// output layer stages one policy's w3 in LDS per block). The weight working set is P times the shared
// policy's (MAPPO actor [256, 256]: ~0.3 MB per policy, 4.9 MB at P = 16, more than one XCD's 4 MiB of
// L2), so the block order decides how many policies' weights an XCD's L2 sees -- blocks are observed
// (not promised) to be dealt round-robin over the 8 XCDs:
//   order 0, policy-major: block b -> policy b / nb, env block b % nb (every XCD sees every policy);
//   order 1, policy-minor: block b -> policy b % P, env block b / P (P a multiple of 8: a policy's
//            blocks are congruent mod 8, so an XCD sees P / 8 policies).
// MSC_MULTI_ORDER picks (read at each launch; default 1). tools/ab_multi.py measures both: policy-minor had
// the lower median in all eight isolated actor / critic timings at C3 and C5 (by 1 to 2 %, inside the
// spread of either) and no measurable difference in the rollout step (profiles/mlp_multi/ab_multi.txt).
// Correctness does not depend on placement.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "env.hpp"
#include "mlp_relu_launch.hpp"

namespace msc {

int mlp_multi_order() {
  const char* e = getenv("MSC_MULTI_ORDER");
  return (e && atoi(e) == 0) ? 0 : 1;
}

hipError_t launch_mlp3_relu_multi(const float* x, int64_t E, int NP, int L, int H1, int H2, int KO, const float* w1p,
                                  const float* b1, const float* w2p, const float* b2, const float* w3p, const float* b3,
                                  float* out, const float* pre1, hipStream_t st, const MlpSample* smp) {
  return launch_mlp3_relu_t<true>(x, E, NP, L, H1, H2, KO, w1p, b1, w2p, b2, w3p, b3, out, pre1, st, smp);
}

hipError_t launch_mlp2_relu_multi(const float* x, int64_t E, int NP, int L, int H1, int KO, const float* w1p,
                                  const float* b1, const float* w3p, const float* b3, float* out, const float* pre1,
                                  hipStream_t st, const MlpSample* smp) {
  return launch_mlp2_relu_t<true>(x, E, NP, L, H1, KO, w1p, b1, w3p, b3, out, pre1, st, smp);
}

}  // namespace msc
