// adam_clip.hip -- the learner's per-group global-norm gradient clip and its Adam step over every parameter
// tensor of every group in one call (msc_adam_clip_step; torch.nn.utils.clip_grad_norm_ per policy followed
// by torch.optim.Adam.step without weight decay or amsgrad, restated; the arithmetic is pinned in
// include/marlsc.h and restated operation by operation in tests/adam_emulation.py).
//
// Scheme: torch's multi_tensor_apply. The caller's table is a HOST array whose gradient pointers change
// every step, so nothing of it is kept or copied to the device: it travels by value in the kernel
// arguments, AC_CAP tensors per launch. A block owns one slice of AC_CHUNK consecutive elements of one
// tensor; an entry names the first block of its tensor (blk0) and a block finds its entry by a scan over at
// most AC_CAP entries that is uniform over the block. The host orders the entries by group (stably), so the
// blocks of a group, over all launches, are one range of consecutive partial slots [ps0, ps1):
//   adam_clip_norm_kernel    one launch per AC_CAP entries: block b writes the float64 sum of squares of its
//                            slice to part[slot0 + b] (per thread in element order, per wave by butterfly,
//                            the four waves in order);
//   adam_clip_update_kernel  one launch per AC_CAP entries, after every norm launch: a block adds its
//                            group's partials (thread t slots ps0 + t, ps0 + t + 256, ... in order, then the
//                            same butterfly and wave order), forms the norm and the clip coefficient and
//                            updates its slice. The block of slot ps0 writes norms_out[group].
// No atomics and no dependence on block scheduling: equal calls give equal bits. With the clip off and no
// norms_out the norm launches are skipped. A tensor takes the float4 path when p, g, m and v (g alone in the
// norm kernel) are 16-byte aligned -- slices start at multiples of AC_CHUNK floats, so the tensor's base
// decides -- and the scalar path otherwise; a tail of n % 4 elements is scalar either way. Tensors longer
// than AC_PIECE elements are cut into entries of AC_PIECE, so an entry's length and a launch's block count
// stay inside int32.
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>
#include <vector>

#include "env.hpp"

namespace msc {

constexpr int AC_BS = 256;
constexpr int AC_CHUNK = 2048;              // elements per block: two float4 per thread
constexpr int AC_CAP = 64;                  // table entries per launch (56 B each in the kernel arguments)
constexpr int64_t AC_PIECE = 1ll << 30;     // elements per entry at most; a multiple of AC_CHUNK

struct AdamClipEntry {
  float* p;
  float* g;
  float* m;
  float* v;
  int32_t n;      // elements, in [1, AC_PIECE]
  int32_t blk0;   // first block of this entry in its launch
  int32_t ps0;    // the group's partial slots [ps0, ps1)
  int32_t ps1;
  int32_t group;
  int32_t pad;
};

struct AdamClipArgs {
  AdamClipEntry e[AC_CAP];
  double* part;        // the workspace: one float64 per block of the call
  double* norms_out;   // [n_groups] or nullptr
  double max_norm;
  int32_t nt;          // entries in use
  int32_t slot0;       // partial slot of this launch's block 0
  int32_t clip;        // max_norm > 0
  int32_t write_g;
  float b2, omb1, omb2, eps, step_size, bc2s;
};
static_assert(sizeof(AdamClipArgs) <= 3840, "the table must fit the kernel argument segment");

// sum over the block in a fixed order: butterflies inside a wave (every lane ends with the same bits), the
// waves in order through LDS; every thread returns the same bits
__device__ inline double ac_block_sum(double s, double* sm) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
  __syncthreads();
  double r = sm[0];
#pragma unroll
  for (int w = 1; w < AC_BS / 64; w++) r += sm[w];
  __syncthreads();
  return r;
}

__device__ inline int ac_entry(const AdamClipArgs& a, int b) {
  int e = 0;
  while (e + 1 < a.nt && a.e[e + 1].blk0 <= b) e++;
  return e;
}

__global__ __launch_bounds__(AC_BS) void adam_clip_norm_kernel(const AdamClipArgs a) {
  __shared__ double sm[AC_BS / 64];
  const int b = blockIdx.x, t = threadIdx.x;
  const AdamClipEntry& en = a.e[ac_entry(a, b)];
  const int off = (b - en.blk0) * AC_CHUNK;
  const int len = min(AC_CHUNK, en.n - off);
  const float* g = en.g + off;
  double s = 0.0;
  if (((uintptr_t)g & 15) == 0) {
    const int nvec = len >> 2;
    for (int i = t; i < nvec; i += AC_BS) {
      const float4 x = reinterpret_cast<const float4*>(g)[i];
      s += (double)x.x * (double)x.x;
      s += (double)x.y * (double)x.y;
      s += (double)x.z * (double)x.z;
      s += (double)x.w * (double)x.w;
    }
    const int i = 4 * nvec + t;
    if (i < len) s += (double)g[i] * (double)g[i];
  } else {
    for (int i = t; i < len; i += AC_BS) s += (double)g[i] * (double)g[i];
  }
  s = ac_block_sum(s, sm);
  if (t == 0) a.part[a.slot0 + b] = s;
}

struct AcCoef {
  float c, b2, omb1, omb2, eps, step_size, bc2s;
};

// one element: every operation a float32 + - * / or sqrt, rounded once, none contracted
__device__ inline void ac_update(const AcCoef& k, float& p, float& g, float& m, float& v) {
  g = g * k.c;
  m = m + k.omb1 * (g - m);
  v = k.b2 * v + (k.omb2 * g) * g;
  const float denom = sqrtf(v) / k.bc2s + k.eps;
  p = p - k.step_size * (m / denom);
}

__global__ __launch_bounds__(AC_BS) void adam_clip_update_kernel(const AdamClipArgs a) {
  __shared__ double sm[AC_BS / 64];
  const int b = blockIdx.x, t = threadIdx.x;
  const AdamClipEntry& en = a.e[ac_entry(a, b)];
  AcCoef k = {1.0f, a.b2, a.omb1, a.omb2, a.eps, a.step_size, a.bc2s};
  if (a.clip || a.norms_out) {
    double s = 0.0;
    for (int i = en.ps0 + t; i < en.ps1; i += AC_BS) s += a.part[i];
    s = ac_block_sum(s, sm);
    const double norm = sqrt(s);
    if (a.clip) k.c = (float)fmin(1.0, a.max_norm / (norm + 1e-6));
    if (a.norms_out && t == 0 && a.slot0 + b == en.ps0) a.norms_out[en.group] = norm;
  }
  const int off = (b - en.blk0) * AC_CHUNK;
  const int len = min(AC_CHUNK, en.n - off);
  float* p = en.p + off;
  float* g = en.g + off;
  float* m = en.m + off;
  float* v = en.v + off;
  const bool wg = a.write_g != 0;
  if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0) {
    const int nvec = len >> 2;
    for (int i = t; i < nvec; i += AC_BS) {
      float4 pp = reinterpret_cast<float4*>(p)[i], gg = reinterpret_cast<const float4*>(g)[i];
      float4 mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
      ac_update(k, pp.x, gg.x, mm.x, vv.x);
      ac_update(k, pp.y, gg.y, mm.y, vv.y);
      ac_update(k, pp.z, gg.z, mm.z, vv.z);
      ac_update(k, pp.w, gg.w, mm.w, vv.w);
      reinterpret_cast<float4*>(p)[i] = pp;
      reinterpret_cast<float4*>(m)[i] = mm;
      reinterpret_cast<float4*>(v)[i] = vv;
      if (wg) reinterpret_cast<float4*>(g)[i] = gg;
    }
    const int i = 4 * nvec + t;
    if (i < len) {
      float gi = g[i];
      ac_update(k, p[i], gi, m[i], v[i]);
      if (wg) g[i] = gi;
    }
  } else {
    for (int i = t; i < len; i += AC_BS) {
      float gi = g[i];
      ac_update(k, p[i], gi, m[i], v[i]);
      if (wg) g[i] = gi;
    }
  }
}

int adam_clip_chunk() { return AC_CHUNK; }
int adam_clip_table_capacity() { return AC_CAP; }

// one slot per block: a tensor of n elements takes ceil(n / AC_CHUNK) <= n / AC_CHUNK + 1 blocks (cutting
// it into pieces of AC_PIECE, a multiple of AC_CHUNK, adds none)
int64_t adam_clip_workspace_bytes(int32_t n_tensors, int64_t total_elems) {
  return (total_elems / AC_CHUNK + n_tensors) * (int64_t)sizeof(double);
}

// The caller (capi.hip) has checked the arguments. Host work: one pass that cuts the table into entries
// ordered by group, one that numbers the blocks; then the launches. No allocation on the device, no copy,
// no synchronisation.
hipError_t launch_adam_clip(const msc_adam_clip_desc& d, const msc_opt_tensor* tensors, int32_t n_tensors,
                            int32_t n_groups, double* norms_out, void* workspace, hipStream_t st) {
  std::vector<AdamClipEntry> ent;
  ent.reserve(n_tensors);
  std::vector<int32_t> order(n_tensors);
  for (int32_t i = 0; i < n_tensors; i++) order[i] = i;
  std::stable_sort(order.begin(), order.end(),
                   [&](int32_t x, int32_t y) { return tensors[x].group < tensors[y].group; });
  for (int32_t i : order) {
    const msc_opt_tensor& x = tensors[i];
    for (int64_t off = 0; off < x.n; off += AC_PIECE) {
      const int64_t n = std::min<int64_t>(AC_PIECE, x.n - off);
      ent.push_back({x.p + off, x.g + off, x.m + off, x.v + off, (int32_t)n, 0, 0, 0, x.group, 0});
    }
  }
  // partial slots: the blocks of the entries in order; a group's entries are adjacent
  std::vector<int64_t> g0(n_groups, 0), g1(n_groups, 0);
  int64_t slot = 0;
  for (const AdamClipEntry& e : ent) {
    if (g1[e.group] == 0) g0[e.group] = slot;
    slot += (e.n + AC_CHUNK - 1) / AC_CHUNK;
    g1[e.group] = slot;
  }
  if (slot > INT32_MAX) return hipErrorInvalidValue;
  const bool clip = d.max_norm > 0.0;
  if (norms_out && std::any_of(g1.begin(), g1.end(), [](int64_t s) { return s == 0; })) {
    // a group without elements has norm 0 and no block to say so
    const hipError_t err = hipMemsetAsync(norms_out, 0, sizeof(double) * (size_t)n_groups, st);
    if (err != hipSuccess) return err;
  }
  AdamClipArgs a{};
  a.part = (double*)workspace, a.norms_out = norms_out, a.max_norm = d.max_norm;
  a.clip = clip ? 1 : 0, a.write_g = d.write_clipped_grads ? 1 : 0;
  const double bc1 = 1.0 - pow(d.beta1, (double)d.step), bc2 = 1.0 - pow(d.beta2, (double)d.step);
  a.b2 = (float)d.beta2, a.omb1 = (float)(1.0 - d.beta1), a.omb2 = (float)(1.0 - d.beta2), a.eps = (float)d.eps;
  a.step_size = (float)(d.lr / bc1), a.bc2s = (float)sqrt(bc2);
  for (int pass = (clip || norms_out) ? 0 : 1; pass < 2; pass++) {
    int64_t slot0 = 0;
    for (size_t i0 = 0; i0 < ent.size(); i0 += AC_CAP) {
      a.nt = (int32_t)std::min<size_t>(AC_CAP, ent.size() - i0);
      a.slot0 = (int32_t)slot0;
      int32_t nb = 0;
      for (int32_t j = 0; j < a.nt; j++) {
        AdamClipEntry& e = a.e[j];
        e = ent[i0 + j];
        e.blk0 = nb, e.ps0 = (int32_t)g0[e.group], e.ps1 = (int32_t)g1[e.group];
        nb += (e.n + AC_CHUNK - 1) / AC_CHUNK;
      }
      if (pass == 0) hipLaunchKernelGGL(adam_clip_norm_kernel, dim3(nb), dim3(AC_BS), 0, st, a);
      else hipLaunchKernelGGL(adam_clip_update_kernel, dim3(nb), dim3(AC_BS), 0, st, a);
      slot0 += nb;
    }
  }
  return hipGetLastError();
}

}  // namespace msc
