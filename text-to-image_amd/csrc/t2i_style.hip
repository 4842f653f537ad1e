// t2i_style.hip — the style-based generator's layer epilogue (Karras et al., "A Style-Based Generator Architecture for Generative
// Adversarial Networks", CVPR 2019; not in the reference): per-pixel noise, activation, instance norm and the style's affine map in
// at most three launches forward and four backward.  DESIGN.md section 4.42.
//
// For x [B,R,C] (R = H W rows of a sample, NHWC), noise [B,R], strength [C], ys, yb [B,C] (rows `sstride` floats apart):
//
//   u = act(x + strength[c] noise[b,r])                        act in {none, relu, lrelu(alpha >= 0)}; without noise u = act(x)
//   mu[b,c], var[b,c] = biased moments of u over r             rstd = rsqrt(var + eps)
//   y = (u - mu) rstd (1 + ys[b,c]) + yb[b,c]
//
// Work split, the same in all four tensor kernels: an item is (sample b, chunk of kChunk rows, tile of kTileC channels), numbered
// tile-fastest, and a grid of at most kMaxBlocks workgroups walks the items with a stride: no grid dimension is derived from B.  Inside
// an item the 256 threads are LX lanes along the channels (V floats each: V = 4 with 16-byte accesses when C % 4 == 0 and the tensors
// are 16-byte aligned, V = 1 for any other C or base) by TY lanes along the rows, each of which takes every TY-th row of the chunk.
//
//   adain_stats_kernel<V>      a thread runs Welford's update over its rows (the divisor k is a compile-time constant), the TY row
//                              lanes of a channel are merged through LDS in ascending order with Chan's update, and (mean, M2) of
//                              the chunk goes to the workspace [B][chunks][2][C]; a chunk's count follows from its number
//   adain_merge_kernel         per (b, 16 channels): 16 lanes merge every 16th chunk in ascending order, then the 16 in ascending
//                              order, all with Chan's update -> mean [B,C], rstd [B,C].  Never E[u^2] - mu^2.
//   adain_apply_kernel<V>      recomputes u, writes y.  No plane of u or of the normalised u is stored.
//   adain_bwd_sums_kernel<V>   recomputes u and uh = (u - mu) rstd; per-chunk sums of g and g uh -> workspace [B][chunks][2][C]
//   adain_sum_kernel           fixed-order sum of such partials over their second axis: dyb = sum g, dys = sum g uh; dstrength below
//   adain_bwd_apply_kernel<V>  dx = act'(u) rstd (1 + ys) (g - mean(g) - uh mean(g uh)), act' from the sign of the recomputed
//                              pre-activation, and per-item sums of dx noise -> workspace [B chunks][C], summed into dstrength [C]
//
// x + strength noise is one fmaf everywhere, so every kernel recomputes the same u bit for bit and strength = 0 gives x exactly.  A
// channel that is constant over a sample keeps mean = the constant and M2 = 0 exactly through Welford and Chan (every delta is 0), so
// its output is yb exactly.  No atomics; the split depends on R and C alone, so a sample's mean, rstd, y, dx, dys and dyb do not
// depend on its batch; nothing is read back, every launch can be captured.
#include <hip/hip_runtime.h>
#include <math.h>

#include "t2i_internal.h"

namespace t2i {
namespace {

constexpr int kThreads = 256;
constexpr int kChunk = T2I_ADAIN_CHUNK_ROWS;         // rows of a sample per item
constexpr int kTileC = 64;                           // channels per item
constexpr int kFinC = 16, kFinL = kThreads / kFinC;  // the finishing reductions: channels per workgroup, lanes along the partials
constexpr int kMaxBlocks = 65535;                    // workgroups of one launch; the items beyond are reached by the stride
constexpr long long kMaxElems = 1ll << 31;

int launched(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return T2I_OK;
  set_error("%s: %s", what, hipGetErrorString(e));
  return T2I_ERR_LAUNCH;
}

template <int V> struct Lay {
  static constexpr int LX = kTileC / V, TY = kThreads / LX, RPT = kChunk / TY;      // V = 4: 16 x 16, 4 rows; V = 1: 64 x 4, 16 rows
};

struct AdainParams {
  const float* x;
  const float* g;
  const float* noise;      // [B,R] or NULL
  const float* strength;   // [C] or NULL, with noise
  const float* mean;
  const float* rstd;
  const float* ys;
  const float* yb;
  const float* dys;
  const float* dyb;
  float* out;              // y or dx
  float* part;             // workspace partials (NULL in bwd_apply: no dstrength wanted)
  long long R, items;
  int B, C, chunks, ctiles, act, sstride;
  float alpha, inv_n;
};

template <int V> __device__ __forceinline__ void load_v(const float* p, float (&v)[V]);
template <> __device__ __forceinline__ void load_v<4>(const float* p, float (&v)[4]) {
  const float4 t = *reinterpret_cast<const float4*>(p);
  v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
template <> __device__ __forceinline__ void load_v<1>(const float* p, float (&v)[1]) { v[0] = *p; }
template <int V> __device__ __forceinline__ void store_v(float* p, const float (&v)[V]);
template <> __device__ __forceinline__ void store_v<4>(float* p, const float (&v)[4]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
template <> __device__ __forceinline__ void store_v<1>(float* p, const float (&v)[1]) { *p = v[0]; }

// the pre-activation: ONE fmaf in every kernel
__device__ __forceinline__ float pre_act(float x, float s, float n) { return fmaf(s, n, x); }
__device__ __forceinline__ float act_of(float p, int act, float alpha) {
  return act == T2I_ACT_NONE ? p : (p > 0.f ? p : (act == T2I_ACT_RELU ? 0.f : alpha * p));
}
__device__ __forceinline__ float dact_of(float p, int act, float alpha) {
  return act == T2I_ACT_NONE ? 1.f : (p > 0.f ? 1.f : (act == T2I_ACT_RELU ? 0.f : alpha));
}

// Chan et al.: (na, ma, Ma) <- merged with (nb, mb, Mb)
__device__ __forceinline__ void chan(float& na, float& ma, float& Ma, float nb, float mb, float Mb) {
  if (nb == 0.f) return;
  if (na == 0.f) { na = nb; ma = mb; Ma = Mb; return; }
  const float n = na + nb, d = mb - ma, f = nb / n;
  ma = fmaf(d, f, ma);
  Ma = Ma + Mb + d * d * na * f;
  na = n;
}

struct Item { int b, ch, c0, nrows; long long row0; };

template <int V> __device__ __forceinline__ Item item_of(const AdainParams& P, long long id, int tx) {
  Item it;
  const int ct = (int)(id % P.ctiles);
  const long long r = id / P.ctiles;
  it.ch = (int)(r % P.chunks);
  it.b = (int)(r / P.chunks);
  it.c0 = ct * kTileC + tx * V;
  const long long first = (long long)it.ch * kChunk;
  it.row0 = (long long)it.b * P.R + first;
  const long long left = P.R - first;
  it.nrows = left < kChunk ? (int)left : kChunk;
  return it;
}

template <int V>
__global__ __launch_bounds__(kThreads) void adain_stats_kernel(const AdainParams P) {
  typedef Lay<V> L;
  __shared__ float s_mean[L::TY][kTileC], s_m2[L::TY][kTileC];
  const int tid = threadIdx.x, tx = tid % L::LX, ty = tid / L::LX;
  for (long long id = blockIdx.x; id < P.items; id += gridDim.x) {
    const Item it = item_of<V>(P, id, tx);
    float mean[V], m2[V], s[V];
#pragma unroll
    for (int j = 0; j < V; ++j) { mean[j] = 0.f; m2[j] = 0.f; s[j] = 0.f; }
    if (it.c0 < P.C) {                                 // (V = 4: C % 4 == 0, so the four channels are inside together)
      if (P.noise) {
#pragma unroll
        for (int j = 0; j < V; ++j) s[j] = P.strength[it.c0 + j];
      }
#pragma unroll
      for (int k = 0; k < L::RPT; ++k) {
        const int lr = ty + k * L::TY;
        if (lr < it.nrows) {                           // a thread's rows are a prefix of k: this is its (k + 1)-th value
          const long long row = it.row0 + lr;
          float v[V];
          load_v<V>(P.x + row * P.C + it.c0, v);
          const float nz = P.noise ? P.noise[row] : 0.f;
          const float rk = 1.0f / (float)(k + 1);
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const float u = act_of(pre_act(v[j], s[j], nz), P.act, P.alpha);
            const float d = u - mean[j];
            mean[j] = fmaf(d, rk, mean[j]);
            m2[j] = fmaf(d, u - mean[j], m2[j]);
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) { s_mean[ty][tx * V + j] = mean[j]; s_m2[ty][tx * V + j] = m2[j]; }
    __syncthreads();
    if (tid < kTileC) {
      const int c = it.c0 - tx * V + tid;              // the tile's first channel + tid
      if (c < P.C) {
        float na = 0.f, ma = 0.f, Ma = 0.f;
        for (int t = 0; t < L::TY; ++t) {
          const int nt = it.nrows > t ? (it.nrows - t + L::TY - 1) / L::TY : 0;
          chan(na, ma, Ma, (float)nt, s_mean[t][tid], s_m2[t][tid]);
        }
        float* o = P.part + ((size_t)it.b * P.chunks + it.ch) * 2 * P.C + c;
        o[0] = ma;
        o[P.C] = Ma;
      }
    }
    __syncthreads();                                   // the next item overwrites the LDS
  }
}

// part [B][chunks][2][C] -> mean [B,C], rstd [B,C]
__global__ __launch_bounds__(kThreads) void adain_merge_kernel(const float* part, long long R, int B, int C, int chunks, float eps,
                                                             float* mean, float* rstd) {
  __shared__ float s_n[kFinL][kFinC], s_mean[kFinL][kFinC], s_m2[kFinL][kFinC];
  const int tid = threadIdx.x, tx = tid % kFinC, ty = tid / kFinC;
  const int ctiles = (C + kFinC - 1) / kFinC;
  const long long items = (long long)B * ctiles;
  for (long long id = blockIdx.x; id < items; id += gridDim.x) {
    const int b = (int)(id / ctiles), c = (int)(id % ctiles) * kFinC + tx;
    float na = 0.f, ma = 0.f, Ma = 0.f;
    if (c < C) {
      for (int p = ty; p < chunks; p += kFinL) {
        const long long left = R - (long long)p * kChunk;
        const float* q = part + ((size_t)b * chunks + p) * 2 * C + c;
        chan(na, ma, Ma, (float)(left < kChunk ? left : kChunk), q[0], q[C]);
      }
    }
    s_n[ty][tx] = na; s_mean[ty][tx] = ma; s_m2[ty][tx] = Ma;
    __syncthreads();
    if (ty == 0 && c < C) {
      na = 0.f; ma = 0.f; Ma = 0.f;
      for (int t = 0; t < kFinL; ++t) chan(na, ma, Ma, s_n[t][tx], s_mean[t][tx], s_m2[t][tx]);
      mean[(size_t)b * C + c] = ma;
      rstd[(size_t)b * C + c] = rsqrtf(Ma / na + eps);
    }
    __syncthreads();
  }
}

// part [G][P][ncomp][C] -> out0 [G,C] (and out1 [G,C] when ncomp == 2): fixed-order sums over P
__global__ __launch_bounds__(kThreads) void adain_sum_kernel(const float* part, int G, int Pn, int ncomp, int C, float* out0, float* out1) {
  __shared__ float s_a[kFinL][kFinC], s_b[kFinL][kFinC];
  const int tid = threadIdx.x, tx = tid % kFinC, ty = tid / kFinC;
  const int ctiles = (C + kFinC - 1) / kFinC;
  const long long items = (long long)G * ctiles;
  for (long long id = blockIdx.x; id < items; id += gridDim.x) {
    const int g = (int)(id / ctiles), c = (int)(id % ctiles) * kFinC + tx;
    float a = 0.f, b2 = 0.f;
    if (c < C) {
      // four partials in flight per lane (the loads of a plain running sum would wait for one another): lane ty owns the partials
      // ty + kFinL k; those with k = 0, 1, 2, 3 (mod 4) go to four sums that are joined in a fixed order
      float a1 = 0.f, a2 = 0.f, a3 = 0.f, b1 = 0.f, b3 = 0.f, b4 = 0.f;
      const size_t step = (size_t)kFinL * ncomp * C;
      int p = ty;
      for (; p + 3 * kFinL < Pn; p += 4 * kFinL) {
        const float* q = part + ((size_t)g * Pn + p) * ncomp * C + c;
        a += q[0]; a1 += q[step]; a2 += q[2 * step]; a3 += q[3 * step];
        if (ncomp == 2) { b2 += q[C]; b1 += q[step + C]; b3 += q[2 * step + C]; b4 += q[3 * step + C]; }
      }
      for (; p < Pn; p += kFinL) {
        const float* q = part + ((size_t)g * Pn + p) * ncomp * C + c;
        a += q[0];
        if (ncomp == 2) b2 += q[C];
      }
      a = (a + a1) + (a2 + a3);
      b2 = (b2 + b1) + (b3 + b4);
    }
    s_a[ty][tx] = a; s_b[ty][tx] = b2;
    __syncthreads();
    if (ty == 0 && c < C) {
      a = 0.f; b2 = 0.f;
      for (int t = 0; t < kFinL; ++t) { a += s_a[t][tx]; b2 += s_b[t][tx]; }
      out0[(size_t)g * C + c] = a;
      if (ncomp == 2) out1[(size_t)g * C + c] = b2;
    }
    __syncthreads();
  }
}

template <int V>
__global__ __launch_bounds__(kThreads) void adain_apply_kernel(const AdainParams P) {
  typedef Lay<V> L;
  const int tid = threadIdx.x, tx = tid % L::LX, ty = tid / L::LX;
  for (long long id = blockIdx.x; id < P.items; id += gridDim.x) {
    const Item it = item_of<V>(P, id, tx);
    if (it.c0 >= P.C) continue;
    float s[V], mu[V], a[V], sh[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int c = it.c0 + j;
      s[j] = P.noise ? P.strength[c] : 0.f;
      mu[j] = P.mean[(size_t)it.b * P.C + c];
      a[j] = P.rstd[(size_t)it.b * P.C + c];
      sh[j] = P.yb[(size_t)it.b * P.sstride + c];
    }
    float sc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) sc[j] = 1.0f + P.ys[(size_t)it.b * P.sstride + it.c0 + j];
#pragma unroll
    for (int k = 0; k < L::RPT; ++k) {
      const int lr = ty + k * L::TY;
      if (lr < it.nrows) {
        const long long row = it.row0 + lr;
        float v[V];
        load_v<V>(P.x + row * P.C + it.c0, v);
        const float nz = P.noise ? P.noise[row] : 0.f;
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float u = act_of(pre_act(v[j], s[j], nz), P.act, P.alpha);
          v[j] = fmaf((u - mu[j]) * a[j], sc[j], sh[j]);
        }
        store_v<V>(P.out + row * P.C + it.c0, v);
      }
    }
  }
}

template <int V>
__global__ __launch_bounds__(kThreads) void adain_bwd_sums_kernel(const AdainParams P) {
  typedef Lay<V> L;
  __shared__ float s_a[L::TY][kTileC], s_b[L::TY][kTileC];
  const int tid = threadIdx.x, tx = tid % L::LX, ty = tid / L::LX;
  for (long long id = blockIdx.x; id < P.items; id += gridDim.x) {
    const Item it = item_of<V>(P, id, tx);
    float sg[V], sgu[V];
#pragma unroll
    for (int j = 0; j < V; ++j) { sg[j] = 0.f; sgu[j] = 0.f; }
    if (it.c0 < P.C) {
      float s[V], mu[V], a[V];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const int c = it.c0 + j;
        s[j] = P.noise ? P.strength[c] : 0.f;
        mu[j] = P.mean[(size_t)it.b * P.C + c];
        a[j] = P.rstd[(size_t)it.b * P.C + c];
      }
#pragma unroll
      for (int k = 0; k < L::RPT; ++k) {
        const int lr = ty + k * L::TY;
        if (lr < it.nrows) {
          const long long row = it.row0 + lr;
          float v[V], g[V];
          load_v<V>(P.x + row * P.C + it.c0, v);
          load_v<V>(P.g + row * P.C + it.c0, g);
          const float nz = P.noise ? P.noise[row] : 0.f;
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const float uh = (act_of(pre_act(v[j], s[j], nz), P.act, P.alpha) - mu[j]) * a[j];
            sg[j] += g[j];
            sgu[j] = fmaf(g[j], uh, sgu[j]);
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) { s_a[ty][tx * V + j] = sg[j]; s_b[ty][tx * V + j] = sgu[j]; }
    __syncthreads();
    if (tid < kTileC) {
      const int c = it.c0 - tx * V + tid;
      if (c < P.C) {
        float a = 0.f, b2 = 0.f;
        for (int t = 0; t < L::TY; ++t) { a += s_a[t][tid]; b2 += s_b[t][tid]; }
        float* o = P.part + ((size_t)it.b * P.chunks + it.ch) * 2 * P.C + c;
        o[0] = b2;                                     // component 0: sum g uh (dys), component 1: sum g (dyb)
        o[P.C] = a;
      }
    }
    __syncthreads();
  }
}

template <int V>
__global__ __launch_bounds__(kThreads) void adain_bwd_apply_kernel(const AdainParams P) {
  typedef Lay<V> L;
  __shared__ float s_a[L::TY][kTileC];
  const int tid = threadIdx.x, tx = tid % L::LX, ty = tid / L::LX;
  for (long long id = blockIdx.x; id < P.items; id += gridDim.x) {
    const Item it = item_of<V>(P, id, tx);
    float dn[V];
#pragma unroll
    for (int j = 0; j < V; ++j) dn[j] = 0.f;
    if (it.c0 < P.C) {
      float s[V], mu[V], a[V], k1[V], mg[V], mgu[V];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const int c = it.c0 + j;
        s[j] = P.noise ? P.strength[c] : 0.f;
        mu[j] = P.mean[(size_t)it.b * P.C + c];
        a[j] = P.rstd[(size_t)it.b * P.C + c];
        k1[j] = a[j] * (1.0f + P.ys[(size_t)it.b * P.sstride + c]);
        mg[j] = P.dyb[(size_t)it.b * P.C + c] * P.inv_n;
        mgu[j] = P.dys[(size_t)it.b * P.C + c] * P.inv_n;
      }
#pragma unroll
      for (int k = 0; k < L::RPT; ++k) {
        const int lr = ty + k * L::TY;
        if (lr < it.nrows) {
          const long long row = it.row0 + lr;
          float v[V], g[V];
          load_v<V>(P.x + row * P.C + it.c0, v);
          load_v<V>(P.g + row * P.C + it.c0, g);
          const float nz = P.noise ? P.noise[row] : 0.f;
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const float p = pre_act(v[j], s[j], nz);
            const float uh = (act_of(p, P.act, P.alpha) - mu[j]) * a[j];
            const float dx = dact_of(p, P.act, P.alpha) * k1[j] * ((g[j] - mg[j]) - uh * mgu[j]);
            dn[j] = fmaf(dx, nz, dn[j]);
            v[j] = dx;
          }
          store_v<V>(P.out + row * P.C + it.c0, v);
        }
      }
    }
    if (P.part) {                                      // (uniform over the launch)
#pragma unroll
      for (int j = 0; j < V; ++j) s_a[ty][tx * V + j] = dn[j];
      __syncthreads();
      if (tid < kTileC) {
        const int c = it.c0 - tx * V + tid;
        if (c < P.C) {
          float a = 0.f;
          for (int t = 0; t < L::TY; ++t) a += s_a[t][tid];
          P.part[((size_t)it.b * P.chunks + it.ch) * P.C + c] = a;
        }
      }
      __syncthreads();
    }
  }
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + nb && b0 < a0 + na;
}

bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr) {
  return !((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15);
}

// the checks every entry shares; fills the geometry of P.  what: the entry's name
int geometry(const char* what, int32_t B, int64_t R, int32_t C, int act, float alpha, const float* noise, const float* strength, AdainParams& P) {
  if (B < 1 || R < 1 || C < 1) {
    set_error("%s: bad argument (x [%d, %lld, %d]: every size must be at least 1)", what, (int)B, (long long)R, (int)C);
    return T2I_ERR_INVALID;
  }
  if (R >= kMaxElems || (long long)C * R >= kMaxElems || (long long)C * R * B >= kMaxElems) {
    set_error("%s: bad argument (x [%d, %lld, %d] has 2^31 elements or more)", what, (int)B, (long long)R, (int)C);
    return T2I_ERR_INVALID;
  }
  if (act != T2I_ACT_NONE && act != T2I_ACT_RELU && act != T2I_ACT_LRELU) {
    set_error("%s: bad argument (act %d: none, relu or lrelu)", what, act);
    return T2I_ERR_INVALID;
  }
  if (act == T2I_ACT_LRELU && !(alpha >= 0.f)) {
    set_error("%s: bad argument (lrelu slope %g: the derivative is read from the sign, which needs a slope >= 0)", what, (double)alpha);
    return T2I_ERR_INVALID;
  }
  if ((noise == nullptr) != (strength == nullptr)) {
    set_error("%s: bad argument (noise and strength come together or not at all)", what);
    return T2I_ERR_INVALID;
  }
  P.noise = noise; P.strength = strength;
  P.B = B; P.R = R; P.C = C; P.act = act; P.alpha = alpha;
  P.chunks = (int)((R + kChunk - 1) / kChunk);
  P.ctiles = (C + kTileC - 1) / kTileC;
  P.items = (long long)B * P.chunks * P.ctiles;        // at most one per element: < 2^31
  P.inv_n = (float)(1.0 / (double)R);
  P.sstride = C;
  return T2I_OK;
}

int workspace_ok(const char* what, const void* ws, size_t ws_bytes, size_t need) {
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 15) || ws_bytes < need) {
    set_error("%s: workspace is NULL, misaligned (16 bytes) or %zu bytes where %zu are needed", what, ws_bytes, need);
    return T2I_ERR_WORKSPACE;
  }
  return T2I_OK;
}

unsigned blocks_for(long long items) { return (unsigned)(items < kMaxBlocks ? items : kMaxBlocks); }

}  // namespace
}  // namespace t2i

using namespace t2i;

int32_t t2i_adain_chunk_rows(void) { return kChunk; }

size_t t2i_adain_workspace_bytes(int32_t B, int64_t R, int32_t C) {
  if (B < 1 || R < 1 || C < 1 || R >= kMaxElems || (long long)C * R >= kMaxElems || (long long)C * R * B >= kMaxElems) return 0;
  const size_t chunks = (size_t)((R + kChunk - 1) / kChunk);
  return ((size_t)B * chunks * 2 * (size_t)C * sizeof(float) + 255) & ~(size_t)255;
}

int t2i_adain_stats(const float* x, const float* noise, const float* strength, int32_t B, int64_t R, int32_t C, int act, float alpha,
                    float eps, float* mean, float* rstd, void* ws, size_t ws_bytes, t2i_stream_t stream) {
  const char* what = "t2i_adain_stats";
  if (!x || !mean || !rstd) { set_error("%s: bad argument (a NULL pointer)", what); return T2I_ERR_INVALID; }
  AdainParams P = {};
  if (int rc = geometry(what, B, R, C, act, alpha, noise, strength, P)) return rc;
  if (!(eps >= 0.f) || !isfinite(eps)) { set_error("%s: bad argument (eps %g: finite and >= 0)", what, (double)eps); return T2I_ERR_INVALID; }
  if (int rc = workspace_ok(what, ws, ws_bytes, t2i_adain_workspace_bytes(B, R, C))) return rc;
  P.x = x; P.part = static_cast<float*>(ws);
  const hipStream_t st = (hipStream_t)stream;
  if (C % 4 == 0 && aligned16(x)) hipLaunchKernelGGL((adain_stats_kernel<4>), dim3(blocks_for(P.items)), dim3(kThreads), 0, st, P);
  else hipLaunchKernelGGL((adain_stats_kernel<1>), dim3(blocks_for(P.items)), dim3(kThreads), 0, st, P);
  if (int rc = launched(what)) return rc;
  const long long fin = (long long)B * ((C + kFinC - 1) / kFinC);
  hipLaunchKernelGGL(adain_merge_kernel, dim3(blocks_for(fin)), dim3(kThreads), 0, st, P.part, P.R, B, C, P.chunks, eps, mean, rstd);
  return launched(what);
}

int t2i_adain_apply(const float* x, const float* noise, const float* strength, const float* mean, const float* rstd, const float* ys,
                    const float* yb, int32_t style_stride, int32_t B, int64_t R, int32_t C, int act, float alpha, float* y,
                    t2i_stream_t stream) {
  const char* what = "t2i_adain_apply";
  if (!x || !mean || !rstd || !ys || !yb || !y) { set_error("%s: bad argument (a NULL pointer)", what); return T2I_ERR_INVALID; }
  AdainParams P = {};
  if (int rc = geometry(what, B, R, C, act, alpha, noise, strength, P)) return rc;
  if (style_stride < C) { set_error("%s: bad argument (style rows %d floats apart, below C = %d)", what, (int)style_stride, (int)C); return T2I_ERR_INVALID; }
  const size_t bytes = (size_t)B * (size_t)R * (size_t)C * 4;
  if (overlap(x, bytes, y, bytes)) { set_error("%s: bad argument (x and y overlap)", what); return T2I_ERR_INVALID; }
  P.x = x; P.mean = mean; P.rstd = rstd; P.ys = ys; P.yb = yb; P.sstride = style_stride; P.out = y;
  const hipStream_t st = (hipStream_t)stream;
  if (C % 4 == 0 && aligned16(x, y)) hipLaunchKernelGGL((adain_apply_kernel<4>), dim3(blocks_for(P.items)), dim3(kThreads), 0, st, P);
  else hipLaunchKernelGGL((adain_apply_kernel<1>), dim3(blocks_for(P.items)), dim3(kThreads), 0, st, P);
  return launched(what);
}

int t2i_adain_bwd_sums(const float* g, const float* x, const float* noise, const float* strength, const float* mean, const float* rstd,
                       int32_t B, int64_t R, int32_t C, int act, float alpha, float* dys, float* dyb, void* ws, size_t ws_bytes,
                       t2i_stream_t stream) {
  const char* what = "t2i_adain_bwd_sums";
  if (!g || !x || !mean || !rstd || !dys || !dyb) { set_error("%s: bad argument (a NULL pointer)", what); return T2I_ERR_INVALID; }
  AdainParams P = {};
  if (int rc = geometry(what, B, R, C, act, alpha, noise, strength, P)) return rc;
  if (int rc = workspace_ok(what, ws, ws_bytes, t2i_adain_workspace_bytes(B, R, C))) return rc;
  P.x = x; P.g = g; P.mean = mean; P.rstd = rstd; P.part = static_cast<float*>(ws);
  const hipStream_t st = (hipStream_t)stream;
  if (C % 4 == 0 && aligned16(x, g)) hipLaunchKernelGGL((adain_bwd_sums_kernel<4>), dim3(blocks_for(P.items)), dim3(kThreads), 0, st, P);
  else hipLaunchKernelGGL((adain_bwd_sums_kernel<1>), dim3(blocks_for(P.items)), dim3(kThreads), 0, st, P);
  if (int rc = launched(what)) return rc;
  const long long fin = (long long)B * ((C + kFinC - 1) / kFinC);
  hipLaunchKernelGGL(adain_sum_kernel, dim3(blocks_for(fin)), dim3(kThreads), 0, st, P.part, B, P.chunks, 2, C, dys, dyb);
  return launched(what);
}

int t2i_adain_bwd_apply(const float* g, const float* x, const float* noise, const float* strength, const float* mean, const float* rstd,
                        const float* ys, int32_t style_stride, const float* dys, const float* dyb, int32_t B, int64_t R, int32_t C,
                        int act, float alpha, float* dx, float* dstrength, void* ws, size_t ws_bytes, t2i_stream_t stream) {
  const char* what = "t2i_adain_bwd_apply";
  if (!g || !x || !mean || !rstd || !ys || !dys || !dyb || !dx) { set_error("%s: bad argument (a NULL pointer)", what); return T2I_ERR_INVALID; }
  AdainParams P = {};
  if (int rc = geometry(what, B, R, C, act, alpha, noise, strength, P)) return rc;
  if (style_stride < C) { set_error("%s: bad argument (style rows %d floats apart, below C = %d)", what, (int)style_stride, (int)C); return T2I_ERR_INVALID; }
  if (dstrength && !noise) { set_error("%s: bad argument (dstrength without noise)", what); return T2I_ERR_INVALID; }
  const size_t bytes = (size_t)B * (size_t)R * (size_t)C * 4;
  if (overlap(x, bytes, dx, bytes) || overlap(g, bytes, dx, bytes)) { set_error("%s: bad argument (dx overlaps x or g)", what); return T2I_ERR_INVALID; }
  if (dstrength)
    if (int rc = workspace_ok(what, ws, ws_bytes, t2i_adain_workspace_bytes(B, R, C))) return rc;
  P.x = x; P.g = g; P.mean = mean; P.rstd = rstd; P.ys = ys; P.sstride = style_stride; P.dys = dys; P.dyb = dyb; P.out = dx;
  P.part = dstrength ? static_cast<float*>(ws) : nullptr;
  const hipStream_t st = (hipStream_t)stream;
  if (C % 4 == 0 && aligned16(x, g, dx)) hipLaunchKernelGGL((adain_bwd_apply_kernel<4>), dim3(blocks_for(P.items)), dim3(kThreads), 0, st, P);
  else hipLaunchKernelGGL((adain_bwd_apply_kernel<1>), dim3(blocks_for(P.items)), dim3(kThreads), 0, st, P);
  if (int rc = launched(what)) return rc;
  if (!dstrength) return T2I_OK;
  hipLaunchKernelGGL(adain_sum_kernel, dim3(blocks_for((C + kFinC - 1) / kFinC)), dim3(kThreads), 0, st, P.part, 1, B * P.chunks, 1, C,
                     dstrength, static_cast<float*>(nullptr));
  return launched(what);
}
