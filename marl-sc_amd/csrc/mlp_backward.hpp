// mlp_backward.hip's host interface (msc_mlp_relu_backward, capi.hip): the parameter gradients of the fused ReLU
// MLPs. Kept out of env.hpp so that only the two translation units that use it depend on it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace msc {

struct MlpBwdArgs {
  const float* x;  // [n][L]
  int64_t n;
  int L, H1, H2, KO;  // H2 = 0: one hidden layer
  const float *w1p, *b1, *w2p, *b2;  // the forward kernels' packs and biases (w2p / b2 unused with one hidden layer)
  const float* w2tp;                 // pack of W2^T (mlp.py:pack_w2t); unused with one hidden layer
  const float* w3;                   // [KO][H_last], torch's own layout
  const float* d_out;                // [n][KO]
  float scale;
  int accumulate;
  float *g_w1, *g_b1, *g_w2, *g_b2, *g_w3, *g_b3;  // torch layouts (g_w2 / g_b2 unused with one hidden layer)
};

// rows one round of launches covers (the workspace's cap), and the bytes for n rows: a function of the
// shape alone, monotone in n and constant from mlp_backward_round_rows on
int64_t mlp_backward_round_rows(int H1, int H2);
int64_t mlp_backward_workspace_bytes(int64_t n, int L, int H1, int H2, int KO);
// shapes as checked by the caller (capi.hip); n = 0 launches nothing
hipError_t launch_mlp_backward(const MlpBwdArgs& a, void* workspace, hipStream_t st);

// P same-shaped policies in three launches per round and group (msc_mlp_relu_backward_multi). n is the rows of ONE
// policy; what the call does for them is the single-policy geometry of n rows, per policy.
struct MlpBwdMultiPlan {
  int G, groups;         // policies per set of launches (a function of L, H1, H2, KO alone), ceil(P / G)
  int64_t rounds;        // rounds per policy
  int nslice;            // split-K slices of a (full) round
  int64_t tiles;         // row tiles of a (full) round
  int64_t policy_bytes;  // mlp_backward_workspace_bytes(n, ...): the workspace is G of them
};
MlpBwdMultiPlan mlp_backward_multi_plan(int64_t n, int P, int L, int H1, int H2, int KO);
// a: x [n][P][L] and d_out [n][P][KO]; packs, biases and w3 of the P policies one after the other; the six outputs
// stacked [P][...]; a.n rows per policy. Shapes and P as checked by the caller; n = 0 launches nothing.
hipError_t launch_mlp_backward_multi(const MlpBwdArgs& a, int P, void* workspace, hipStream_t st);

}  // namespace msc
