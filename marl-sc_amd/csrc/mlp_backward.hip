// mlp_backward.hip -- the parameter gradients of the fused ReLU MLPs (msc_mlp_relu_backward): what torch
// autograd computes through MLPArchitecture.build's module (src/algorithms/models/architectures/mlp.py:14-60)
// inside PPOTorchLearner.compute_gradients, for y = W3 relu(W2 relu(W1 x + b1) + b2) + b3 or the
// one-hidden-layer form, from an upstream gradient d_out [n][KO]. No input gradient: the observations are
// leaves.
//
// Nothing is saved by the forward. Per round of at most mlp_backward_round_rows rows, three launches:
//
// (a) mlp{3,2}_dgrad_kernel, one wave per tile of 32 rows, the forward kernels' geometry. It recomputes the
//     hidden pre-activations from x with the forward kernels' packs (w1p, w2p) in their accumulation order
//     (bias first, then the k steps in ascending order on v_mfma_f32_32x32x2_f32), so the masks z > 0 are
//     those of msc_mlp{3,2}_relu_forward bit for bit (zero gradient at z == 0, as torch). Then
//       d2 = (z2 > 0) . W3^T d3   on the VALU, the output layer run backwards over the w3 rows staged in LDS
//                                 (up to 64 KiB; a wider one-hidden-layer w3 is read from L2): the lane's 16
//                                 units of a tile times the row's d_out, one output at a time in ascending
//                                 order, w3 read as float4 at one address per lane half (a broadcast);
//       d1 = (z1 > 0) . W2^T d2   on the MFMA with the pack of W2^T (w2tp, the layer-2 pack's index map on
//                                 the transposed matrix): d2 in accumulator layout is the B operand as it
//                                 stands, as h1 is in the forward.
//     h1, d1, h2, d2 go to the workspace in the layout [tile][unit][32 rows]: register r of lane (c, h) is
//     unit 32 t + rho(r, h) of row c, so every register store is two 128-byte lines, the wave re-reads its
//     own d2 as B operand from the same addresses, and rows past n are stored as zeros.
// (b) mlp_wgrad_kernel: dW = d h^T reduces over rows, so rows are the MFMA's k dimension (lane l holds
//     A[l & 31][l >> 5] and B[l >> 5][l & 31]). A wave owns one 32 x 32 tile of one weight matrix and one
//     slice of the row tiles (split-K); per row tile, lane (c, h) reads rows 16 h .. 16 h + 15 of unit
//     j0 + c -- 64 contiguous bytes of the layout above -- for both operands, and MFMA step i takes rows
//     i and 16 + i; a tile's chain starts from zero and is added to the slice's sum, so no f32 chain is
//     longer than 32 products. x and d_out are read where they lie, row-major. The waves of column tile 0
//     also sum their unit's rows in f64 for the bias gradient. Partials [slice][...] go to the workspace.
// (c) mlp_bwd_finalize_kernel: every gradient element = scale x (its partials summed in slice order),
//     written or added to the torch-layout output.
//
// The multi-policy call (msc_mlp_relu_backward_multi: the P same-shaped networks of per-agent policies, rows laid out
// [n / P][P]) runs the same three kernels, instantiated with a trailing MbPol argument, over a group of G policies
// per launch: every policy keeps the geometry above for its own n / P rows in a workspace section of its own, so its
// gradients are the single-policy call's on its gathered rows bit for bit.
//
// Deterministic: no atomics; tiles, slices and rounds are functions of the shape arguments alone.
// Exact on integers: every product is exact in f32 and every sum is an f32 accumulation (the bias gradients'
// an f64 one, rounded to f32 once per slice), so integer data whose absolute-value evaluation stays below 2^24
// gives the int64 result bit for bit.
#include "mlp_backward.hpp"

#include "mlp_dispatch.hpp"
#include "mlp_kernels.hpp"

namespace msc {

constexpr int MB_SLICE_TILES = 1;  // a split-K slice has at least this many row tiles ...
constexpr int MB_MAX_SLICES = 8;   // ... and there are at most this many slices

// rows per round: the workspace holds 2 (H1 + H2) floats per row, 64 MiB at either value
int64_t mlp_backward_round_rows(int H1, int H2) { return H1 + H2 <= 512 ? 16384 : 8192; }

struct MbGeom {
  int64_t tiles;  // row tiles of a (full) round
  int nslice;
  int64_t ps;     // floats of one slice's partials
  int64_t o_w1, o_b1, o_w2, o_b2, o_w3, o_b3;
  int I1;         // padded columns of the W1 partial
};

static MbGeom mb_geom(int64_t n, int L, int H1, int H2, int KO) {
  MbGeom g{};
  const int64_t rr = mlp_backward_round_rows(H1, H2);
  g.tiles = ((n < rr ? n : rr) + 31) / 32;
  const int64_t s = (g.tiles + MB_SLICE_TILES - 1) / MB_SLICE_TILES;
  g.nslice = (int)(s < 1 ? 1 : s > MB_MAX_SLICES ? MB_MAX_SLICES : s);
  const int HL = H2 ? H2 : H1;
  g.I1 = (L + 31) / 32 * 32;
  int64_t o = 0;
  g.o_w1 = o, o += (int64_t)H1 * g.I1;
  g.o_b1 = o, o += H1;
  g.o_w2 = o, o += (int64_t)H2 * H1;
  g.o_b2 = o, o += H2;
  g.o_w3 = o, o += 32 * (int64_t)HL;
  g.o_b3 = o, o += 32;
  g.ps = o;
  return g;
}

int64_t mlp_backward_workspace_bytes(int64_t n, int L, int H1, int H2, int KO) {
  const MbGeom g = mb_geom(n, L, H1, H2, KO);
  return (g.tiles * 32 * 2 * (H1 + H2) + g.nslice * g.ps) * (int64_t)sizeof(float);
}

// ws sections of a round of `tiles` row tiles: h1, d1 (H1 units), then h2, d2 (H2 units)
__device__ __forceinline__ float* mb_sec(float* ws, int64_t tiles, int H1, int H2, int which) {
  const int64_t s1 = tiles * 32 * H1, s2 = tiles * 32 * H2;
  return ws + (which == 0 ? 0 : which == 1 ? s1 : which == 2 ? 2 * s1 : 2 * s1 + s2);
}

// w3 [KO][H_last] (count floats, a multiple of 32) into the block's dynamic LDS; every thread of the block calls it
constexpr int MB_W3_LDS_MAX = 64 * 1024;  // bytes: what a launch may ask for without an attribute
template <bool W3S>
__device__ __forceinline__ const float* mb_stage_w3(const float* __restrict__ w3, int count) {
  if constexpr (W3S) {
    extern __shared__ float4 mb_w3s[];
    const float4* src = reinterpret_cast<const float4*>(w3);
    for (int i = threadIdx.x; i < count / 4; i += blockDim.x) mb_w3s[i] = src[i];
    __syncthreads();
    return reinterpret_cast<const float*>(mb_w3s);
  } else {
    return w3;
  }
}

// what a kernel of a multi-policy launch gets on top of the single-policy kernel's arguments
struct MbPol {
  int G;             // policies of this launch
  int ldx, ldd;      // floats between two rows of a policy in x / d_out: P L, P KO
  int64_t wss;       // floats of one policy's workspace
  int64_t w1p, w2p;  // floats of one policy's w1p; of its w2p, and of its w2tp
};
__device__ __forceinline__ MbPol mb_pol(const MbPol m) { return m; }  // (the one element of a kernel's Pol pack)

// two hidden layers; NT1 / NT2: hidden tiles of 32 units. Layer 2 and both dgrads run in passes of 2 tiles, so
// a lane holds 16 NT1 + 64 accumulators and the fragments: one wave per SIMD (512 registers) from H1 = 128 on.
constexpr int mb_wpe(int NT1) { return NT1 >= 4 ? 1 : 2; }
// W3S: the block stages w3 [KO][H_last] in (dynamic) LDS and the output layer runs backwards over those rows --
// every lane of a half reads the same 16 bytes, a broadcast; false (w3 larger than MB_W3_LDS_MAX): from L2.
//
// Pol: nothing (the single-policy kernel, msc_mlp_relu_backward) or one MbPol (msc_mlp_relu_backward_multi: the G
// policies of a group in one launch). Block b then works for policy b % G of the group (policy-minor, as the multi
// forward's default order) as that policy's block b / G, so a block's four tiles, its staged w3 and every wave's
// policy index are one policy's. The pointers arrive at the group's first policy; policy p's rows lie at stride
// ldx / ldd (the [rows][policies] layout), its packs, biases, w3 and workspace at p times the per-policy sizes. A
// policy's blocks do what the single-policy kernel's do on its gathered rows, in the same order.
template <int NT1, int NT2, bool W3S, class... Pol>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(mb_wpe(NT1), mb_wpe(NT1)))) void mlp3_dgrad_kernel(const float* __restrict__ x, int64_t n, int L, int KS1,
                                                         const float4* __restrict__ w1p, const float* __restrict__ b1,
                                                         const float4* __restrict__ w2p, const float* __restrict__ b2,
                                                         const float4* __restrict__ w2tp, const float* __restrict__ w3,
                                                         const float* __restrict__ d_out, int KO, float* ws,
                                                         int64_t tiles, const Pol... pol) {
  constexpr int H1 = NT1 * 32, H2 = NT2 * 32;
  constexpr int S4 = NT1 * 4;   // layer-2 k steps of 4 MFMAs
  constexpr int S4T = NT2 * 4;  // the same for W2^T
  constexpr bool MP = sizeof...(Pol) > 0;
  const int lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
  unsigned blk = blockIdx.x;
  int ldx = L, ldd = KO;
  if constexpr (MP) {
    const MbPol m = mb_pol(pol...);
    const int64_t p = blk % (unsigned)m.G;
    blk /= (unsigned)m.G, ldx = m.ldx, ldd = m.ldd;
    x += p * L, d_out += p * KO, ws += p * m.wss;
    w1p += p * (m.w1p / 4), b1 += p * H1, w2p += p * (m.w2p / 4), b2 += p * H2, w2tp += p * (m.w2p / 4), w3 += p * KO * H2;
  }
  const int64_t tile = (int64_t)blk * 4 + (threadIdx.x >> 6);
  const float* const w3r = mb_stage_w3<W3S>(w3, KO * H2);
  if (tile >= tiles) return;  // wave-uniform (no block-level synchronisation below)
  const int64_t j = tile * 32 + c;
  const bool jv = j < n;
  const int M4 = (KS1 + 3) / 4;
  float* const ws_h1 = mb_sec(ws, tiles, H1, H2, 0) + tile * 32 * H1 + c;
  float* const ws_d1 = mb_sec(ws, tiles, H1, H2, 1) + tile * 32 * H1 + c;
  float* const ws_h2 = mb_sec(ws, tiles, H1, H2, 2) + tile * 32 * H2 + c;
  float* const ws_d2 = mb_sec(ws, tiles, H1, H2, 3) + tile * 32 * H2 + c;

  // layer 1, as mlp3_relu_kernel's
  mlp_f32x16 a1[NT1];
#pragma unroll
  for (int t = 0; t < NT1; t++)
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const float4 v = *reinterpret_cast<const float4*>(b1 + t * 32 + 8 * g + 4 * h);
      a1[t][4 * g] = v.x, a1[t][4 * g + 1] = v.y, a1[t][4 * g + 2] = v.z, a1[t][4 * g + 3] = v.w;
    }
  const float* xr = x + (jv ? j : 0) * (int64_t)ldx;
  for (int m4 = 0; m4 < M4; m4++) {
    float xv[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int m = m4 * 4 + i, k = h * KS1 + m;
      xv[i] = (jv && m < KS1 && k < L) ? xr[k] : 0.0f;
    }
#pragma unroll
    for (int t = 0; t < NT1; t++) {
      const float4 w = w1p[((int64_t)t * M4 + m4) * 64 + lane];
      a1[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.x, xv[0], a1[t], 0, 0, 0);
      a1[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.y, xv[1], a1[t], 0, 0, 0);
      a1[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.z, xv[2], a1[t], 0, 0, 0);
      a1[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.w, xv[3], a1[t], 0, 0, 0);
    }
  }
#pragma unroll
  for (int t = 0; t < NT1; t++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      a1[t][r] = fmaxf(a1[t][r], 0.0f);
      ws_h1[(t * 32 + mfma_row(r, h)) * 32] = jv ? a1[t][r] : 0.0f;
    }

  // layer 2 in passes of 2 tiles, and d2 of the pass's units
#pragma unroll 1
  for (int p = 0; p < NT2 / 2; p++) {
    mlp_f32x16 a2[2];
#pragma unroll
    for (int q = 0; q < 2; q++)
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const float4 v = *reinterpret_cast<const float4*>(b2 + (p * 2 + q) * 32 + 8 * g + 4 * h);
        a2[q][4 * g] = v.x, a2[q][4 * g + 1] = v.y, a2[q][4 * g + 2] = v.z, a2[q][4 * g + 3] = v.w;
      }
#pragma unroll
    for (int s4 = 0; s4 < S4; s4++) {
      float4 w[2];
#pragma unroll
      for (int q = 0; q < 2; q++) w[q] = w2p[((int64_t)(p * 2 + q) * S4 + s4) * 64 + lane];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int s = s4 * 4 + i;
        const float bv = a1[s / 16][s % 16];
#pragma unroll
        for (int q = 0; q < 2; q++) {
          const float wv = i == 0 ? w[q].x : i == 1 ? w[q].y : i == 2 ? w[q].z : w[q].w;
          a2[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv, bv, a2[q], 0, 0, 0);
        }
      }
    }
    float dd[2][16];
#pragma unroll
    for (int q = 0; q < 2; q++)
#pragma unroll
      for (int r = 0; r < 16; r++) dd[q][r] = 0.0f;
    for (int a = 0; a < KO; a++) {
      const float dv = jv ? d_out[j * ldd + a] : 0.0f;
#pragma unroll
      for (int q = 0; q < 2; q++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
          const float4 w = *reinterpret_cast<const float4*>(w3r + a * H2 + (p * 2 + q) * 32 + 8 * g + 4 * h);
          dd[q][4 * g] = fmaf(w.x, dv, dd[q][4 * g]);
          dd[q][4 * g + 1] = fmaf(w.y, dv, dd[q][4 * g + 1]);
          dd[q][4 * g + 2] = fmaf(w.z, dv, dd[q][4 * g + 2]);
          dd[q][4 * g + 3] = fmaf(w.w, dv, dd[q][4 * g + 3]);
        }
    }
#pragma unroll
    for (int q = 0; q < 2; q++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int u = ((p * 2 + q) * 32 + mfma_row(r, h)) * 32;
        const float z = a2[q][r];
        ws_h2[u] = jv ? fmaxf(z, 0.0f) : 0.0f;
        ws_d2[u] = z > 0.0f ? dd[q][r] : 0.0f;  // rows past n: dd = 0
      }
  }

  // d1 = (z1 > 0) . W2^T d2 in passes of 2 tiles of H1: the wave's own d2, read back as the B operand
#pragma unroll
  for (int p = 0; p < NT1 / 2; p++) {
    mlp_f32x16 acc[2];
#pragma unroll
    for (int q = 0; q < 2; q++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[q][r] = 0.0f;
#pragma unroll 1
    for (int s4 = 0; s4 < S4T; s4++) {
      float4 w[2];
#pragma unroll
      for (int q = 0; q < 2; q++) w[q] = w2tp[((int64_t)(p * 2 + q) * S4T + s4) * 64 + lane];
      // steps 4 s4 .. 4 s4 + 3 are registers 4 (s4 & 3) .. + 3 of tile s4 >> 2: four consecutive units
      const float* bp = ws_d2 + ((s4 >> 2) * 32 + 8 * (s4 & 3) + 4 * h) * 32;
      const float bv[4] = {bp[0], bp[32], bp[64], bp[96]};
#pragma unroll
      for (int q = 0; q < 2; q++) {
        acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[q].x, bv[0], acc[q], 0, 0, 0);
        acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[q].y, bv[1], acc[q], 0, 0, 0);
        acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[q].z, bv[2], acc[q], 0, 0, 0);
        acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[q].w, bv[3], acc[q], 0, 0, 0);
      }
    }
#pragma unroll
    for (int q = 0; q < 2; q++)
#pragma unroll
      for (int r = 0; r < 16; r++)
        ws_d1[((p * 2 + q) * 32 + mfma_row(r, h)) * 32] = a1[p * 2 + q][r] > 0.0f ? acc[q][r] : 0.0f;
  }
}

// one hidden layer of NT1 tiles, one tile at a time: layer 1 as mlp2_relu_kernel's, d1 = (z1 > 0) . W3^T d3
template <bool W3S, class... Pol>
__global__ __launch_bounds__(256) void mlp2_dgrad_kernel(const float* __restrict__ x, int64_t n, int L, int KS1, int NT1,
                                                         const float4* __restrict__ w1p, const float* __restrict__ b1,
                                                         const float* __restrict__ w3, const float* __restrict__ d_out,
                                                         int KO, float* ws, int64_t tiles, const Pol... pol) {
  const int lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
  unsigned blk = blockIdx.x;
  int ldx = L, ldd = KO;
  if constexpr (sizeof...(Pol) > 0) {
    const MbPol m = mb_pol(pol...);
    const int64_t p = blk % (unsigned)m.G;
    blk /= (unsigned)m.G, ldx = m.ldx, ldd = m.ldd;
    x += p * L, d_out += p * KO, ws += p * m.wss;
    w1p += p * (m.w1p / 4), b1 += p * NT1 * 32, w3 += p * KO * NT1 * 32;
  }
  const int64_t tile = (int64_t)blk * 4 + (threadIdx.x >> 6);
  const int H1 = NT1 * 32;
  const float* const w3r = mb_stage_w3<W3S>(w3, KO * H1);
  if (tile >= tiles) return;  // wave-uniform (no block-level synchronisation below)
  const int64_t j = tile * 32 + c;
  const bool jv = j < n;
  const int M4 = (KS1 + 3) / 4;
  float* const ws_h1 = mb_sec(ws, tiles, H1, 0, 0) + tile * 32 * H1 + c;
  float* const ws_d1 = mb_sec(ws, tiles, H1, 0, 1) + tile * 32 * H1 + c;
  const float* xr = x + (jv ? j : 0) * (int64_t)ldx;
  for (int t = 0; t < NT1; t++) {
    mlp_f32x16 a1;
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const float4 v = *reinterpret_cast<const float4*>(b1 + t * 32 + 8 * g + 4 * h);
      a1[4 * g] = v.x, a1[4 * g + 1] = v.y, a1[4 * g + 2] = v.z, a1[4 * g + 3] = v.w;
    }
    for (int m4 = 0; m4 < M4; m4++) {
      float xv[4];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int m = m4 * 4 + i, k = h * KS1 + m;
        xv[i] = (jv && m < KS1 && k < L) ? xr[k] : 0.0f;
      }
      const float4 w = w1p[((int64_t)t * M4 + m4) * 64 + lane];
      a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(w.x, xv[0], a1, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(w.y, xv[1], a1, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(w.z, xv[2], a1, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(w.w, xv[3], a1, 0, 0, 0);
    }
    float dd[16];
#pragma unroll
    for (int r = 0; r < 16; r++) dd[r] = 0.0f;
    for (int a = 0; a < KO; a++) {
      const float dv = jv ? d_out[j * ldd + a] : 0.0f;
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const float4 w = *reinterpret_cast<const float4*>(w3r + a * H1 + t * 32 + 8 * g + 4 * h);
        dd[4 * g] = fmaf(w.x, dv, dd[4 * g]);
        dd[4 * g + 1] = fmaf(w.y, dv, dd[4 * g + 1]);
        dd[4 * g + 2] = fmaf(w.z, dv, dd[4 * g + 2]);
        dd[4 * g + 3] = fmaf(w.w, dv, dd[4 * g + 3]);
      }
    }
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int u = (t * 32 + mfma_row(r, h)) * 32;
      const float z = a1[r];
      ws_h1[u] = jv ? fmaxf(z, 0.0f) : 0.0f;
      ws_d1[u] = z > 0.0f ? dd[r] : 0.0f;  // rows past n: dd = 0
    }
  }
}

// one weight gradient dW [32 JT][32 IT] = A^T B over the round's rows. An operand is a workspace section
// ([tile][ld units][32 rows]) or a row-major matrix [n][ld] of which `cols` columns exist (x, d_out).
struct MbGemm {
  const float *A, *B;
  int a_rm, a_ld, a_cols;
  int b_rm, b_ld, b_cols;
  int IT;
  int first;  // first (tile) job of this matrix
  int64_t o_w, o_b;
};
struct MbWgrad {
  MbGemm g[3];
  int jobs;  // tile jobs of all matrices
  int nslice;
  int64_t tiles, n, ps;
};

__device__ __forceinline__ void mb_operand(const float* p, int rm, int ld, int cols, int64_t tile, int u0, int c, int h,
                                           int64_t n, float (&v)[16]) {
  if (rm) {
    const int col = u0 + c;
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const int64_t row = tile * 32 + 16 * h + i;
      v[i] = (row < n && col < cols) ? p[row * ld + col] : 0.0f;
    }
  } else {
    const float4* q = reinterpret_cast<const float4*>(p + ((tile * ld + u0 + c) * 32 + 16 * h));
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const float4 f = q[i];
      v[4 * i] = f.x, v[4 * i + 1] = f.y, v[4 * i + 2] = f.z, v[4 * i + 3] = f.w;
    }
  }
}

// Pol as in the dgrad kernels. Policy p of a multi-policy launch: its partials are p workspaces on, a row-major
// operand's pointer moves on by p rows' worth of columns (its ld is then the stride of the [rows][policies]
// layout), a workspace section's by p workspaces
template <class... Pol>
__global__ __launch_bounds__(256) void mlp_wgrad_kernel(const MbWgrad a, float* __restrict__ part, const Pol... pol) {
  constexpr bool MP = sizeof...(Pol) > 0;
  const int lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
  unsigned blk = blockIdx.x;
  int64_t p = 0, wss = 0;
  if constexpr (MP) {
    const MbPol m = mb_pol(pol...);
    p = blk % (unsigned)m.G, blk /= (unsigned)m.G, wss = m.wss;
    part += p * wss;
  }
  const int64_t job = (int64_t)blk * 4 + (threadIdx.x >> 6);
  if (job >= (int64_t)a.jobs * a.nslice) return;  // wave-uniform
  const int ks = (int)(job % a.nslice), tj = (int)(job / a.nslice);
  MbGemm G = a.g[0];
  if (tj >= a.g[1].first) G = a.g[1];
  if (tj >= a.g[2].first) G = a.g[2];
  if constexpr (MP) {
    G.A += G.a_rm ? p * G.a_cols : p * wss;
    G.B += G.b_rm ? p * G.b_cols : p * wss;
  }
  const int jt = (tj - G.first) / G.IT, it = (tj - G.first) % G.IT;
  const int64_t per = (a.tiles + a.nslice - 1) / a.nslice;
  const int64_t t0 = ks * per, t1 = t0 + per < a.tiles ? t0 + per : a.tiles;
  // two levels, so that no f32 chain is longer than a tile's 32 products: the MFMA chain of a row tile
  // starts from zero and is added to the slice's sum. The bias gradient (column tile 0's waves) is the
  // lane's own f64 sum of its unit's rows, rounded once per slice.
  mlp_f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; r++) acc[r] = 0.0f;
  double sb = 0.0;
  for (int64_t tile = t0; tile < t1; tile++) {
    float av[16], bv[16];
    mb_operand(G.A, G.a_rm, G.a_ld, G.a_cols, tile, jt * 32, c, h, a.n, av);
    mb_operand(G.B, G.b_rm, G.b_ld, G.b_cols, tile, it * 32, c, h, a.n, bv);
    mlp_f32x16 at;
#pragma unroll
    for (int r = 0; r < 16; r++) at[r] = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; i++) at = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[i], at, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] += at[r];
    if (it == 0) {
#pragma unroll
      for (int i = 0; i < 16; i++) sb += (double)av[i];
    }
  }
  float* pw = part + ks * a.ps + G.o_w + ((int64_t)jt * 32) * (G.IT * 32) + it * 32 + c;
#pragma unroll
  for (int r = 0; r < 16; r++) pw[(int64_t)mfma_row(r, h) * (G.IT * 32)] = acc[r];
  if (it == 0) {
    sb += __shfl_xor(sb, 32);  // rows 16 .. 31 of every tile
    if (h == 0) part[ks * a.ps + G.o_b + jt * 32 + c] = (float)sb;
  }
}

// the six outputs as segments of one index space: element e of segment s is row e / cols, column e % cols
struct MbFinal {
  float* g[6];
  int cols[6], ld[6];  // columns of the output, leading dimension of its partial
  int64_t off[6], end[6];  // the partial's offset; the segment's end in the index space
  int nslice, accumulate;
  int64_t ps;
  float scale;
};

// Pol as in the dgrad kernels: policy p of a multi-policy launch reads its own partials and writes the p-th of the
// stacked outputs
template <class... Pol>
__global__ __launch_bounds__(256) void mlp_bwd_finalize_kernel(const MbFinal f, const float* __restrict__ part,
                                                               const Pol... pol) {
  constexpr bool MP = sizeof...(Pol) > 0;
  unsigned blk = blockIdx.x;
  int64_t pi = 0;
  if constexpr (MP) {
    const MbPol m = mb_pol(pol...);
    pi = blk % (unsigned)m.G, blk /= (unsigned)m.G;
    part += pi * m.wss;
  }
  const int64_t e = (int64_t)blk * 256 + threadIdx.x;
  if (e >= f.end[5]) return;
  float* g = f.g[0];
  int cols = f.cols[0], ld = f.ld[0];
  int64_t off = f.off[0], beg = 0;
#pragma unroll
  for (int s = 1; s < 6; s++)
    if (e >= f.end[s - 1]) g = f.g[s], cols = f.cols[s], ld = f.ld[s], off = f.off[s], beg = f.end[s - 1];
  if constexpr (MP) {
    int64_t end = f.end[0];
#pragma unroll
    for (int s = 1; s < 6; s++)
      if (e >= f.end[s - 1]) end = f.end[s];
    g += pi * (end - beg);
  }
  const int64_t i = e - beg;
  const float* p = part + off + (i / cols) * ld + i % cols;
  float s = p[0];
  for (int k = 1; k < f.nslice; k++) s += p[k * f.ps];  // slice order
  s = f.scale * s;
  g[i] = f.accumulate ? g[i] + s : s;
}

template <class F>
static bool mb_form(int H1, int H2, F&& f) {
  bool ok = true;
  auto second = [&](auto nt1) {
    dispatch_int_or<0, 2, 4, 8, 16>(H2 / 32, [&](auto nt2) {
      if constexpr (decltype(nt2)::value == 0) ok = false;
      else f(nt1, nt2);
    });
  };
  dispatch_int_or<0, 2, 4, 8, 16>(H1 / 32, [&](auto nt1) {
    if constexpr (decltype(nt1)::value == 0) ok = false;
    else second(nt1);
  });
  return ok;
}

// The launches of one group of policies over all rounds. P = 0 is the single-policy call (a's pointers as they
// are, the single-policy kernels, grids of one policy's blocks). P > 0: a's pointers are at the group's first
// policy, a.n is the rows of ONE policy, rows lie at stride P, and the multi kernels run G policies per launch
// with G times the blocks; every policy's geometry (mb_geom of its own rows) is the single call's.
static hipError_t mb_launch(const MlpBwdArgs& a, int P, int G, int64_t wss, void* workspace, hipStream_t st) {
  if (a.n == 0) return hipSuccess;
  const bool two = a.H2 != 0, multi = P > 0;
  if (two ? !(mlp_hidden_ok(a.H1) && mlp_hidden_ok(a.H2)) : !mlp2_supported(a.H1)) return hipErrorInvalidValue;
  const int HL = two ? a.H2 : a.H1, KS1 = (a.L + 1) / 2;
  const int RS = multi ? P : 1;  // rows of the arrays per row of a policy
  const int ldx = RS * a.L, ldd = RS * a.KO;
  const unsigned NG = multi ? (unsigned)G : 1u;
  const MbPol pol{G, ldx, ldd, wss, (int64_t)(a.H1 / 32) * ((KS1 + 3) / 4) * 256, (int64_t)a.H1 * a.H2};
  const int64_t rr = mlp_backward_round_rows(a.H1, a.H2);
  float* ws = (float*)workspace;
  for (int64_t r0 = 0; r0 < a.n; r0 += rr) {
    const int64_t n = a.n - r0 < rr ? a.n - r0 : rr;
    const MbGeom g = mb_geom(n, a.L, a.H1, a.H2, a.KO);
    const float* x = a.x + r0 * ldx;
    const float* d_out = a.d_out + r0 * ldd;
    float* part = ws + g.tiles * 32 * 2 * (a.H1 + a.H2);
    const unsigned grid = (unsigned)((g.tiles + 3) / 4) * NG;
    const size_t w3_bytes = (size_t)a.KO * HL * sizeof(float);
    const bool staged = w3_bytes <= (size_t)MB_W3_LDS_MAX;  // (always, with two hidden layers: 32 x 512 floats)
    const size_t lds = staged ? w3_bytes : 0;
    if (two) {
      const bool found = mb_form(a.H1, a.H2, [&](auto nt1, auto nt2) {
        constexpr int N1 = decltype(nt1)::value, N2 = decltype(nt2)::value;
        if (multi)
          hipLaunchKernelGGL((mlp3_dgrad_kernel<N1, N2, true, MbPol>), dim3(grid), dim3(256), lds, st, x, n, a.L, KS1,
                             mlp_f4(a.w1p), a.b1, mlp_f4(a.w2p), a.b2, mlp_f4(a.w2tp), a.w3, d_out, a.KO, ws, g.tiles, pol);
        else
          hipLaunchKernelGGL((mlp3_dgrad_kernel<N1, N2, true>), dim3(grid), dim3(256), lds, st, x, n, a.L, KS1,
                             mlp_f4(a.w1p), a.b1, mlp_f4(a.w2p), a.b2, mlp_f4(a.w2tp), a.w3, d_out, a.KO, ws, g.tiles);
      });
      if (!found) return hipErrorInvalidValue;
    } else if (multi) {
      if (staged)
        hipLaunchKernelGGL((mlp2_dgrad_kernel<true, MbPol>), dim3(grid), dim3(256), lds, st, x, n, a.L, KS1, a.H1 / 32,
                           mlp_f4(a.w1p), a.b1, a.w3, d_out, a.KO, ws, g.tiles, pol);
      else
        hipLaunchKernelGGL((mlp2_dgrad_kernel<false, MbPol>), dim3(grid), dim3(256), 0, st, x, n, a.L, KS1, a.H1 / 32,
                           mlp_f4(a.w1p), a.b1, a.w3, d_out, a.KO, ws, g.tiles, pol);
    } else if (staged) {
      hipLaunchKernelGGL(mlp2_dgrad_kernel<true>, dim3(grid), dim3(256), lds, st, x, n, a.L, KS1, a.H1 / 32,
                         mlp_f4(a.w1p), a.b1, a.w3, d_out, a.KO, ws, g.tiles);
    } else {
      hipLaunchKernelGGL(mlp2_dgrad_kernel<false>, dim3(grid), dim3(256), 0, st, x, n, a.L, KS1, a.H1 / 32,
                         mlp_f4(a.w1p), a.b1, a.w3, d_out, a.KO, ws, g.tiles);
    }
    const int64_t s1 = g.tiles * 32 * a.H1, s2 = g.tiles * 32 * a.H2;
    const float *h1 = ws, *d1 = ws + s1, *h2 = ws + 2 * s1, *d2 = ws + 2 * s1 + s2;
    MbWgrad w{};
    int jobs = 0, k = 0;
    // dW1 = d1^T x
    w.g[k++] = MbGemm{d1, x, 0, a.H1, a.H1, 1, ldx, a.L, g.I1 / 32, jobs, g.o_w1, g.o_b1};
    jobs += (a.H1 / 32) * (g.I1 / 32);
    if (two) {  // dW2 = d2^T h1
      w.g[k++] = MbGemm{d2, h1, 0, a.H2, a.H2, 0, a.H1, a.H1, a.H1 / 32, jobs, g.o_w2, g.o_b2};
      jobs += (a.H2 / 32) * (a.H1 / 32);
    }
    // dW3 = d_out^T h_last: one tile of output rows, KO of them real
    w.g[k++] = MbGemm{d_out, two ? h2 : h1, 1, ldd, a.KO, 0, HL, HL, HL / 32, jobs, g.o_w3, g.o_b3};
    jobs += HL / 32;
    for (; k < 3; k++) w.g[k] = MbGemm{nullptr, nullptr, 0, 0, 0, 0, 0, 0, 1, 0x7fffffff, 0, 0};
    w.jobs = jobs, w.nslice = g.nslice, w.tiles = g.tiles, w.n = n, w.ps = g.ps;
    const dim3 wgrid((unsigned)(((int64_t)jobs * g.nslice + 3) / 4) * NG);
    if (multi) hipLaunchKernelGGL(mlp_wgrad_kernel<MbPol>, wgrid, dim3(256), 0, st, w, part, pol);
    else hipLaunchKernelGGL(mlp_wgrad_kernel<>, wgrid, dim3(256), 0, st, w, part);
    MbFinal f{};
    int64_t end = 0;
    auto seg = [&](int s, float* gp, int64_t rows, int cols, int ld, int64_t off) {
      end += gp ? rows * cols : 0;  // (an absent matrix is an empty segment)
      f.g[s] = gp, f.cols[s] = cols > 0 ? cols : 1, f.ld[s] = ld, f.off[s] = off, f.end[s] = end;
    };
    seg(0, a.g_w1, a.H1, a.L, g.I1, g.o_w1);
    seg(1, a.g_b1, a.H1, 1, 1, g.o_b1);
    seg(2, two ? a.g_w2 : nullptr, a.H2, a.H1, a.H1, g.o_w2);
    seg(3, two ? a.g_b2 : nullptr, a.H2, 1, 1, g.o_b2);
    seg(4, a.g_w3, a.KO, HL, HL, g.o_w3);
    seg(5, a.g_b3, a.KO, 1, 1, g.o_b3);
    f.nslice = g.nslice, f.accumulate = (a.accumulate || r0 > 0) ? 1 : 0, f.ps = g.ps, f.scale = a.scale;
    const dim3 fgrid((unsigned)((end + 255) / 256) * NG);
    if (multi) hipLaunchKernelGGL(mlp_bwd_finalize_kernel<MbPol>, fgrid, dim3(256), 0, st, f, part, pol);
    else hipLaunchKernelGGL(mlp_bwd_finalize_kernel<>, fgrid, dim3(256), 0, st, f, part);
  }
  return hipGetLastError();
}

hipError_t launch_mlp_backward(const MlpBwdArgs& a, void* workspace, hipStream_t st) {
  return mb_launch(a, 0, 1, 0, workspace, st);
}

// Policies per set of launches: the largest count whose workspaces, each at its cap (a full round: what
// mlp_backward_workspace_bytes returns from mlp_backward_round_rows rows on), fit MB_MULTI_WS_CAP; at least 1.
// It does not look at n, so the bytes G x (one policy's bytes for its rows) stay monotone in n, and a caller's
// workspace grows with the rows it actually trains on. 1 GiB is a design constant, not a measured one: it keeps
// 15 policies of the largest form (64 MiB of operands each) in one group, so the per-agent sets of the shipped
// environments (up to 16 warehouses) with the shipped networks (32 MiB at [256]) are one group.
constexpr int64_t MB_MULTI_WS_CAP = (int64_t)1 << 30;

MlpBwdMultiPlan mlp_backward_multi_plan(int64_t n, int P, int L, int H1, int H2, int KO) {
  MlpBwdMultiPlan p{};
  const int64_t rr = mlp_backward_round_rows(H1, H2);
  const int64_t cap = MB_MULTI_WS_CAP / mlp_backward_workspace_bytes(rr, L, H1, H2, KO);
  p.G = (int)(cap < 1 ? 1 : cap > P ? P : cap);
  p.groups = (P + p.G - 1) / p.G;
  p.rounds = (n + rr - 1) / rr;
  const MbGeom g = mb_geom(n, L, H1, H2, KO);
  p.nslice = g.nslice, p.tiles = g.tiles;
  p.policy_bytes = mlp_backward_workspace_bytes(n, L, H1, H2, KO);
  return p;
}

hipError_t launch_mlp_backward_multi(const MlpBwdArgs& a, int P, void* workspace, hipStream_t st) {
  const MlpBwdMultiPlan p = mlp_backward_multi_plan(a.n, P, a.L, a.H1, a.H2, a.KO);
  const int HL = a.H2 ? a.H2 : a.H1, M4 = ((a.L + 1) / 2 + 3) / 4;
  const int64_t wss = p.policy_bytes / (int64_t)sizeof(float);
  for (int p0 = 0; p0 < P; p0 += p.G) {  // policies are independent: every group reuses the workspace in stream order
    MlpBwdArgs b = a;
    const int64_t q = p0;
    b.x += q * a.L, b.d_out += q * a.KO;
    b.w1p += q * (a.H1 / 32) * M4 * 256, b.b1 += q * a.H1, b.w3 += q * a.KO * HL;
    b.g_w1 += q * a.H1 * a.L, b.g_b1 += q * a.H1, b.g_w3 += q * a.KO * HL, b.g_b3 += q * a.KO;
    if (a.H2) {
      b.w2p += q * a.H1 * a.H2, b.b2 += q * a.H2, b.w2tp += q * a.H1 * a.H2;
      b.g_w2 += q * a.H2 * a.H1, b.g_b2 += q * a.H2;
    }
    const int G = P - p0 < p.G ? P - p0 : p.G;
    if (const hipError_t e = mb_launch(b, P, G, wss, workspace, st)) return e;
  }
  return hipSuccess;
}

}  // namespace msc
