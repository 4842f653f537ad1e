// t2i_ops.hip — the rest of the reference's operator surface (reference utils/ops.py:94-116,145-148): pixel_norm, nearest-neighbour
// resize (upscale / downscale by any factor) and its adjoint, tf.nn.pool with window = stride = s under SAME padding (AVG / MAX, any
// extents) with its backward and second-order maps, the multiplicative noise gn, and the double backward of pixel_norm and layer_norm
// (normalised critics under the gradient penalty).  All of them are memory-bound single passes:
// 16-byte accesses where C % 4 == 0 and the tensors are 16-byte aligned, a scalar form for any other C (C = 3 and C = 9 occur); no
// atomics anywhere, every sum has a fixed order, so results repeat bit for bit.  The entry points (declared in include/t2i_hip.h)
// are at the end of this file: they validate, pick the form and enqueue on the caller's stream — no allocation, no synchronisation.
#include <hip/hip_runtime.h>
#include <math.h>

#include "t2i_internal.h"

namespace t2i {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1 << 20;

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline unsigned blocks_for(size_t items) {
  size_t b = (items + kThreads - 1) / kThreads;
  if (b < 1) b = 1;
  if (b > (size_t)kMaxBlocks) b = kMaxBlocks;       // the kernels below stride over the grid
  return (unsigned)b;
}

int launched(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return T2I_OK;
  set_error("%s: %s", what, hipGetErrorString(e));
  return T2I_ERR_LAUNCH;
}

// ---- lane-wise helpers on float / float4 -----------------------------------------------------------------------------------
template <typename T> struct Lanes;
template <> struct Lanes<float> {
  static constexpr int N = 1;
  static __device__ __forceinline__ float get(const float& v, int) { return v; }
  static __device__ __forceinline__ void set(float& v, int, float x) { v = x; }
};
template <> struct Lanes<float4> {
  static constexpr int N = 4;
  static __device__ __forceinline__ float get(const float4& v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }
  static __device__ __forceinline__ void set(float4& v, int i, float x) {
    if (i == 0) v.x = x; else if (i == 1) v.y = x; else if (i == 2) v.z = x; else v.w = x;
  }
};
template <typename T> struct IdxOf;
template <> struct IdxOf<float> { typedef int type; };
template <> struct IdxOf<float4> { typedef int4 type; };
__device__ __forceinline__ int iget(const int& v, int) { return v; }
__device__ __forceinline__ int iget(const int4& v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }
__device__ __forceinline__ void iset(int& v, int, int x) { v = x; }
__device__ __forceinline__ void iset(int4& v, int i, int x) {
  if (i == 0) v.x = x; else if (i == 1) v.y = x; else if (i == 2) v.z = x; else v.w = x;
}
template <typename T> __device__ __forceinline__ T splat(float x);
template <> __device__ __forceinline__ float splat<float>(float x) { return x; }
template <> __device__ __forceinline__ float4 splat<float4>(float x) { return make_float4(x, x, x, x); }

// ---------------------------------------------------------------------------------------------------------------------------
// pixel_norm (reference utils/ops.py:94-97): u = act(x), y = u / sqrt(mean_c(u^2) + eps) over x [R, C].
// A row belongs to a group of G lanes of one wave, G a power of two sized by the row (G = 64 from C >= 256 in the 16-byte form),
// so narrow rows share a wave64.  The group sum is a butterfly of cross-lane shuffles; with at most PER units per lane the row
// stays in registers between the reduction and the scaling (IN_REG), wider rows are read a second time.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int kPer = 8;           // units (float4 or float) a lane keeps in registers

__device__ __forceinline__ float group_sum(float s, int G) {
  for (int o = G >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);      // G | 64 and groups are G-aligned: partners stay in the group
  return s;
}

template <typename T, bool IN_REG>
__global__ __launch_bounds__(kThreads) void pixel_norm_fwd_kernel(const T* __restrict__ x, long long R, int units, int C, int G, float eps,
                                                                   int act, float alpha, T* __restrict__ y, float* __restrict__ rnorm) {
  const int lane = threadIdx.x & (G - 1);
  const long long row = (long long)blockIdx.x * (kThreads / G) + threadIdx.x / G;
  const bool live = row < R;                 // a ragged last block: its idle lanes still take part in the shuffles
  const T* xr = x + (live ? row : 0) * units;
  T* yr = y + (live ? row : 0) * units;
  T v[kPer];
  float ss = 0.f;
  if (IN_REG) {
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const int j = lane + k * G;
      if (live && j < units) {
        T t = xr[j];
#pragma unroll
        for (int e = 0; e < Lanes<T>::N; ++e) {
          const float u = apply_act(Lanes<T>::get(t, e), act, alpha);
          Lanes<T>::set(t, e, u);
          ss += u * u;
        }
        v[k] = t;
      }
    }
  } else {
    for (int j = lane; live && j < units; j += G) {
      const T t = xr[j];
#pragma unroll
      for (int e = 0; e < Lanes<T>::N; ++e) {
        const float u = apply_act(Lanes<T>::get(t, e), act, alpha);
        ss += u * u;
      }
    }
  }
  ss = group_sum(ss, G);
  const float rn = 1.0f / sqrtf(ss / (float)C + eps);
  if (!live) return;
  if (lane == 0) rnorm[row] = rn;
  if (IN_REG) {
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const int j = lane + k * G;
      if (j < units) {
        T t = v[k];
#pragma unroll
        for (int e = 0; e < Lanes<T>::N; ++e) Lanes<T>::set(t, e, Lanes<T>::get(t, e) * rn);
        yr[j] = t;
      }
    }
  } else {
    for (int j = lane; j < units; j += G) {
      T t = xr[j];
#pragma unroll
      for (int e = 0; e < Lanes<T>::N; ++e) Lanes<T>::set(t, e, apply_act(Lanes<T>::get(t, e), act, alpha) * rn);
      yr[j] = t;
    }
  }
}

// du = s (g - y mean_c(g y)), dx = du act'(.), with u = y / s: lrelu / relu read the derivative from the sign of y, tanh is 1 - u^2.
// The sign of y is the sign of x only for alpha >= 0: the entry points refuse a negative lrelu slope.
__device__ __forceinline__ float pixel_norm_dx(float g, float yv, float m, float s, int act, float alpha) {
  const float du = s * (g - yv * m);
  switch (act) {
    case T2I_ACT_LRELU: return yv > 0.f ? du : alpha * du;
    case T2I_ACT_RELU: return yv > 0.f ? du : 0.f;
    case T2I_ACT_TANH: { const float u = yv / s; return du * (1.f - u * u); }
    default: return du;
  }
}

template <typename T, bool IN_REG>
__global__ __launch_bounds__(kThreads) void pixel_norm_bwd_kernel(const T* __restrict__ g, const T* __restrict__ y,
                                                                   const float* __restrict__ rnorm, long long R, int units, int C, int G,
                                                                   int act, float alpha, T* __restrict__ dx) {
  const int lane = threadIdx.x & (G - 1);
  const long long row = (long long)blockIdx.x * (kThreads / G) + threadIdx.x / G;
  const bool live = row < R;
  const size_t base = (size_t)(live ? row : 0) * units;
  const T* gr = g + base;
  const T* yr = y + base;
  T* dr = dx + base;
  T gv[kPer], yv[kPer];
  float dot = 0.f;
  if (IN_REG) {
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const int j = lane + k * G;
      if (live && j < units) {
        gv[k] = gr[j];
        yv[k] = yr[j];
#pragma unroll
        for (int e = 0; e < Lanes<T>::N; ++e) dot += Lanes<T>::get(gv[k], e) * Lanes<T>::get(yv[k], e);
      }
    }
  } else {
    for (int j = lane; live && j < units; j += G) {
      const T a = gr[j], b = yr[j];
#pragma unroll
      for (int e = 0; e < Lanes<T>::N; ++e) dot += Lanes<T>::get(a, e) * Lanes<T>::get(b, e);
    }
  }
  dot = group_sum(dot, G);
  if (!live) return;
  const float m = dot / (float)C;
  const float s = rnorm[row];
  if (IN_REG) {
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const int j = lane + k * G;
      if (j < units) {
        T t;
#pragma unroll
        for (int e = 0; e < Lanes<T>::N; ++e)
          Lanes<T>::set(t, e, pixel_norm_dx(Lanes<T>::get(gv[k], e), Lanes<T>::get(yv[k], e), m, s, act, alpha));
        dr[j] = t;
      }
    }
  } else {
    for (int j = lane; j < units; j += G) {
      const T a = gr[j], b = yr[j];
      T t;
#pragma unroll
      for (int e = 0; e < Lanes<T>::N; ++e) Lanes<T>::set(t, e, pixel_norm_dx(Lanes<T>::get(a, e), Lanes<T>::get(b, e), m, s, act, alpha));
      dr[j] = t;
    }
  }
}

inline int group_lanes(int units) {
  int G = 1;
  while (G < units && G < 64) G <<= 1;
  return G;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Second order of the two normalisations: the derivatives of L = <v, dx> for the cotangent v of a first-order
// input gradient dx.  lrelu / relu are piecewise linear, so only their slope d = act'(.) enters, read from the sign of the output
// like everywhere else; tanh has a second derivative of its own and is refused by the entry points.
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float act_slope(float yv, int act, float alpha) {
  return (act == T2I_ACT_NONE || yv > 0.f) ? 1.f : (act == T2I_ACT_LRELU ? alpha : 0.f);
}

// pixel_norm: dx = s (g - y mean_c(g y)) d.  With w = v d and the per-pixel means m_wy, m_gy, m_wg:
//   dL/dg = s (w - y m_wy),   dL/dx = -s^2 (y m_wg + w m_gy + g m_wy - 3 y m_wy m_gy) d.
// Same lane-group scheme as the first-order pair; three tensors stay in registers for rows of up to 2048 floats.  The register arrays
// are sized by the row (PER units per lane and tensor): with the full kPer = 8 the 16-byte form needs 134 VGPRs (3 waves per SIMD), and
// the rows a critic has (C <= 512: at most 2 units per lane) would pay for registers they never fill.
template <typename T, int PER>       // PER: units a lane keeps in registers (1, 2, 4 or kPer); 0: the row is read twice
__global__ __launch_bounds__(kThreads) void pixel_norm_bwd2_kernel(const T* __restrict__ v, const T* __restrict__ g, const T* __restrict__ y,
                                                                    const float* __restrict__ rnorm, long long R, int units, int C, int G,
                                                                    int act, float alpha, T* __restrict__ dg, T* __restrict__ dx) {
  const int lane = threadIdx.x & (G - 1);
  const long long row = (long long)blockIdx.x * (kThreads / G) + threadIdx.x / G;
  const bool live = row < R;
  const size_t base = (size_t)(live ? row : 0) * units;
  const T* vr = v + base;
  const T* gr = g + base;
  const T* yr = y + base;
  constexpr bool IN_REG = PER > 0;
  constexpr int NK = PER > 0 ? PER : 1;
  T wv[NK], gv[NK], yv[NK];
  float swy = 0.f, sgy = 0.f, swg = 0.f;
  if (IN_REG) {
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const int j = lane + k * G;
      if (live && j < units) {
        T a = vr[j];
        gv[k] = gr[j];
        yv[k] = yr[j];
#pragma unroll
        for (int e = 0; e < Lanes<T>::N; ++e) {
          const float yy = Lanes<T>::get(yv[k], e), gg = Lanes<T>::get(gv[k], e);
          const float w = Lanes<T>::get(a, e) * act_slope(yy, act, alpha);
          Lanes<T>::set(a, e, w);
          swy += w * yy; sgy += gg * yy; swg += w * gg;
        }
        wv[k] = a;
      }
    }
  } else {
    for (int j = lane; live && j < units; j += G) {
      const T a = vr[j], b = gr[j], c = yr[j];
#pragma unroll
      for (int e = 0; e < Lanes<T>::N; ++e) {
        const float yy = Lanes<T>::get(c, e), gg = Lanes<T>::get(b, e);
        const float w = Lanes<T>::get(a, e) * act_slope(yy, act, alpha);
        swy += w * yy; sgy += gg * yy; swg += w * gg;
      }
    }
  }
  swy = group_sum(swy, G); sgy = group_sum(sgy, G); swg = group_sum(swg, G);
  if (!live) return;
  const float m_wy = swy / (float)C, m_gy = sgy / (float)C, m_wg = swg / (float)C;
  const float s = rnorm[row];
  const float ns2 = -s * s, m3 = 3.f * m_wy * m_gy;
  T* dgr = dg + base;
  T* dxr = dx + base;
  if (IN_REG) {
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const int j = lane + k * G;
      if (j < units) {
        T o, p;
#pragma unroll
        for (int e = 0; e < Lanes<T>::N; ++e) {
          const float yy = Lanes<T>::get(yv[k], e), gg = Lanes<T>::get(gv[k], e), w = Lanes<T>::get(wv[k], e);
          Lanes<T>::set(o, e, s * (w - yy * m_wy));
          Lanes<T>::set(p, e, ns2 * (yy * m_wg + w * m_gy + gg * m_wy - yy * m3) * act_slope(yy, act, alpha));
        }
        dgr[j] = o;
        dxr[j] = p;
      }
    }
  } else {
    for (int j = lane; j < units; j += G) {
      const T a = vr[j], b = gr[j], c = yr[j];
      T o, p;
#pragma unroll
      for (int e = 0; e < Lanes<T>::N; ++e) {
        const float yy = Lanes<T>::get(c, e), gg = Lanes<T>::get(b, e);
        const float d = act_slope(yy, act, alpha), w = Lanes<T>::get(a, e) * d;
        Lanes<T>::set(o, e, s * (w - yy * m_wy));
        Lanes<T>::set(p, e, ns2 * (yy * m_wg + w * m_gy + gg * m_wy - yy * m3) * d);
      }
      dgr[j] = o;
      dxr[j] = p;
    }
  }
}

// layer_norm: per sample of n elements, xhat = (x - mu) r, g = gamma_c gz, gz = gy d, dx = r (g - mean(g) - xhat mean(g xhat)).
// Five per-sample sums S = (sum v, sum v xhat, sum g, sum g xhat, sum v g) give everything (means m_* = S_* / n):
//   hg = dL/dg = r (v - m_v - xhat m_vx),   dL/dgy = hg gamma_c d,   dL/dgamma_c = sum over rows of hg gz,
//   q = -r (v m_gx + m_vx g),   dL/dx = r (q - mean(q) - xhat mean(q xhat)) - r^2 xhat (S_vg - m_g S_v - m_gx S_vx) / n
//   with mean(q) = -r (m_gx m_v + m_vx m_g) and mean(q xhat) = -2 r m_gx m_vx.
// A sample is a whole image (up to ~1 M floats at a handful of samples), so the sums are taken in two fixed-order levels like
// row_moments (t2i_aux.hip): grid (chunks, B) partials of five floats (up to 256 chunks of at least 4096 floats), then one wave
// per sample adds its chunks in a fixed order.
// The channel of a row element is i % C: a multiply-high (FastDiv), not an integer division per element.
constexpr int kLnChunksMax = 256;
constexpr int kLnChunkFloats = 4096;        // a sample longer than this is split over several workgroups (16 floats per thread; at
                                            // 16384 per workgroup and 64 chunks, 512 workgroups left the 256 CUs at 0.65 of a copy)
constexpr int kLnSums = 5;

struct LnSplit { int chunks; size_t per_chunk; };
inline LnSplit ln_split(int64_t per, bool vec) {        // per, per_chunk in floats; per_chunk a multiple of 4 in the 16-byte form
  int64_t c = (per + kLnChunkFloats - 1) / kLnChunkFloats;
  if (c > kLnChunksMax) c = kLnChunksMax;
  if (c < 1) c = 1;
  size_t per_chunk = ((size_t)per + (size_t)c - 1) / (size_t)c;
  if (vec) per_chunk = (per_chunk + 3) & ~(size_t)3;
  LnSplit s;
  s.per_chunk = per_chunk;
  s.chunks = (int)(((size_t)per + per_chunk - 1) / per_chunk);
  return s;
}

template <typename T>       // per, per_chunk, Cu counted in units of T
__global__ __launch_bounds__(kThreads) void layer_norm_bwd2_sums_kernel(const T* __restrict__ v, const T* __restrict__ gy,
                                                                         const T* __restrict__ xhat, const T* __restrict__ y,
                                                                         const T* __restrict__ gamma, int per, int per_chunk, int Cu,
                                                                         FastDiv div_c, int act, float alpha, float* __restrict__ part) {
  __shared__ float red[kLnSums][kThreads / 64];
  const int beg = blockIdx.x * per_chunk;
  const int end = beg + per_chunk < per ? beg + per_chunk : per;
  const size_t rb = (size_t)blockIdx.y * per;
  float acc[kLnSums] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int i = beg + threadIdx.x; i < end; i += kThreads) {
    const int c = i - div_c.div(i) * Cu;
    const T a = v[rb + i], b = gy[rb + i], x = xhat[rb + i], ga = gamma[c];
    const T yy = y ? y[rb + i] : a;
#pragma unroll
    for (int e = 0; e < Lanes<T>::N; ++e) {
      const float d = y ? act_slope(Lanes<T>::get(yy, e), act, alpha) : 1.f;
      const float gg = Lanes<T>::get(ga, e) * (Lanes<T>::get(b, e) * d), vv = Lanes<T>::get(a, e), xx = Lanes<T>::get(x, e);
      acc[0] += vv; acc[1] += vv * xx; acc[2] += gg; acc[3] += gg * xx; acc[4] += vv * gg;
    }
  }
#pragma unroll
  for (int q = 0; q < kLnSums; ++q) {
    const float s = group_sum(acc[q], 64);
    if ((threadIdx.x & 63) == 0) red[q][threadIdx.x >> 6] = s;
  }
  __syncthreads();
  if (threadIdx.x < kLnSums)
    part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kLnSums + threadIdx.x] =
        (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
}

// one wave per sample: lane l adds the chunks l, l + 64, ... in order, then the butterfly joins the 64 lanes — a fixed order, and no
// chain of up to 256 dependent loads (one thread per sum took 50 us over 256 chunks: each load waited for the one before it)
__global__ __launch_bounds__(64) void layer_norm_bwd2_sums_stage2(const float* __restrict__ part, int chunks, float* __restrict__ sums) {
  const int r = blockIdx.x;
  float a[kLnSums] = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (int k = threadIdx.x; k < chunks; k += 64) {
    const float* p = part + ((size_t)r * chunks + k) * kLnSums;
#pragma unroll
    for (int q = 0; q < kLnSums; ++q) a[q] += p[q];
  }
#pragma unroll
  for (int q = 0; q < kLnSums; ++q) a[q] = group_sum(a[q], 64);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < kLnSums; ++q) sums[(size_t)r * kLnSums + q] = a[q];
  }
}

template <typename T>       // n, per, Cu counted in units of T; p may be NULL
__global__ __launch_bounds__(kThreads) void layer_norm_bwd2_apply_kernel(const T* __restrict__ v, const T* __restrict__ gy,
                                                                          const T* __restrict__ xhat, const T* __restrict__ y,
                                                                          const T* __restrict__ gamma, const float* __restrict__ rstd,
                                                                          const float* __restrict__ sums, int n, int per, int Cu,
                                                                          FastDiv div_per, FastDiv div_c, float inv_n, int act, float alpha,
                                                                          T* __restrict__ dgy, T* __restrict__ dx, T* __restrict__ p) {
  for (size_t it = (size_t)blockIdx.x * kThreads + threadIdx.x; it < (size_t)n; it += (size_t)gridDim.x * kThreads) {
    const int i = (int)it;
    const int row = div_per.div(i);
    const int j = i - row * per;
    const int c = j - div_c.div(j) * Cu;
    const float* S = sums + (size_t)row * kLnSums;
    const float r = rstd[row];
    const float m_v = S[0] * inv_n, m_vx = S[1] * inv_n, m_g = S[2] * inv_n, m_gx = S[3] * inv_n;
    const float sva = (S[4] - m_g * S[0] - m_gx * S[1]) * inv_n;           // <v, a> / n,  a = g - m_g - xhat m_gx
    const float mq = -r * (m_gx * m_v + m_vx * m_g), mqx = -2.f * r * m_gx * m_vx;
    const float r2sva = r * r * sva;
    const T a = v[i], b = gy[i], x = xhat[i], ga = gamma[c];
    const T yy = y ? y[i] : a;
    T o, w, z;
#pragma unroll
    for (int e = 0; e < Lanes<T>::N; ++e) {
      const float d = y ? act_slope(Lanes<T>::get(yy, e), act, alpha) : 1.f;
      const float gam = Lanes<T>::get(ga, e), gz = Lanes<T>::get(b, e) * d, gg = gam * gz;
      const float vv = Lanes<T>::get(a, e), xx = Lanes<T>::get(x, e);
      const float hg = r * (vv - m_v - xx * m_vx);
      const float q = -r * (vv * m_gx + m_vx * gg);
      Lanes<T>::set(o, e, hg * gam * d);
      Lanes<T>::set(w, e, r * (q - mq - xx * mqx) - xx * r2sva);
      Lanes<T>::set(z, e, hg * gz);
    }
    dgy[i] = o;
    dx[i] = w;
    if (p) p[i] = z;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Nearest-neighbour resize (tf.image.resize_nearest_neighbor, align_corners = False; reference utils/ops.py:104-116):
// source row of output row r = min(int(floorf(r * hs)), H - 1) with hs = float(H) / float(Ho) in fp32, columns alike.
// The map is monotone, so its adjoint is a gather too: input row i owns the output rows [first(i), first(i + 1)).
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int nn_src(int r, float scale, int n_in) {
  const int s = (int)floorf(__fmul_rn((float)r, scale));
  return s < n_in - 1 ? s : n_in - 1;
}

// smallest r in [0, n_out] with nn_src(r) >= i (n_out if there is none): an estimate, then corrected with the forward rule itself
__device__ __forceinline__ int nn_first(int i, float scale, int n_in, int n_out) {
  if (i >= n_in) return n_out;
  int r = (int)ceilf((float)i / scale);
  r = r < 0 ? 0 : (r > n_out ? n_out : r);
  while (r > 0 && nn_src(r - 1, scale, n_in) >= i) --r;
  while (r < n_out && nn_src(r, scale, n_in) < i) ++r;
  return r;
}

template <typename T>       // C counted in units of T
__global__ __launch_bounds__(kThreads) void resize_nearest_kernel(const T* __restrict__ x, int H, int W, int C, int Ho, int Wo, float hs,
                                                                   float ws, size_t n_out, T* __restrict__ y) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_out; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    size_t p = i / C;
    const int w = (int)(p % Wo); p /= Wo;
    const int h = (int)(p % Ho);
    const size_t b = p / Ho;
    y[i] = x[((b * H + nn_src(h, hs, H)) * W + nn_src(w, ws, W)) * C + c];
  }
}

template <typename T>       // dx [B,H,W,C] from g [B,Ho,Wo,C]: each input pixel sums its block of output pixels, rows then columns
__global__ __launch_bounds__(kThreads) void resize_nearest_adj_kernel(const T* __restrict__ g, int H, int W, int C, int Ho, int Wo, float hs,
                                                                       float ws, size_t n_in, T* __restrict__ dx) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_in; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    size_t p = i / C;
    const int w = (int)(p % W); p /= W;
    const int h = (int)(p % H);
    const size_t b = p / H;
    const int r0 = nn_first(h, hs, H, Ho), r1 = nn_first(h + 1, hs, H, Ho);
    const int c0 = nn_first(w, ws, W, Wo), c1 = nn_first(w + 1, ws, W, Wo);
    T acc = splat<T>(0.f);
    for (int r = r0; r < r1; ++r)
      for (int q = c0; q < c1; ++q) {
        const T t = g[((b * Ho + r) * Wo + q) * C + c];
#pragma unroll
        for (int e = 0; e < Lanes<T>::N; ++e) Lanes<T>::set(acc, e, Lanes<T>::get(acc, e) + Lanes<T>::get(t, e));
      }
    dx[i] = acc;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// tf.nn.pool(window = stride = s, SAME) (reference utils/ops.py:100-101): Ho = ceil(H / s); the padding Ho s - H is split with the
// smaller half in front (pt, pl).  AVG divides by the number of taps inside the image, MAX ignores the padding and records the
// window offset ky * s + kx of its FIRST maximum in row-major window order.  Windows do not overlap, so every backward is a gather.
// ---------------------------------------------------------------------------------------------------------------------------
template <typename T, bool MAX>
__global__ __launch_bounds__(kThreads) void pool_same_fwd_kernel(const T* __restrict__ x, int H, int W, int C, int s, int pt, int pl, int Ho,
                                                                  int Wo, size_t n_out, T* __restrict__ y,
                                                                  typename IdxOf<T>::type* __restrict__ idx) {
  typedef typename IdxOf<T>::type I;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_out; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    size_t p = i / C;
    const int ow = (int)(p % Wo); p /= Wo;
    const int oh = (int)(p % Ho);
    const size_t b = p / Ho;
    const int h0 = oh * s - pt, w0 = ow * s - pl;
    const int ha = h0 < 0 ? 0 : h0, hb = h0 + s < H ? h0 + s : H;
    const int wa = w0 < 0 ? 0 : w0, wb = w0 + s < W ? w0 + s : W;
    T acc = splat<T>(0.f);
    I at = I();
    bool first = true;
    for (int h = ha; h < hb; ++h)
      for (int w = wa; w < wb; ++w) {
        const T t = x[((b * H + h) * W + w) * C + c];
        const int k = (h - h0) * s + (w - w0);
#pragma unroll
        for (int e = 0; e < Lanes<T>::N; ++e) {
          const float v = Lanes<T>::get(t, e);
          if (MAX) {
            if (first || v > Lanes<T>::get(acc, e)) { Lanes<T>::set(acc, e, v); iset(at, e, k); }
          } else {
            Lanes<T>::set(acc, e, Lanes<T>::get(acc, e) + v);
          }
        }
        first = false;
      }
    if (!MAX) {
      const float cnt = (float)((hb - ha) * (wb - wa));
#pragma unroll
      for (int e = 0; e < Lanes<T>::N; ++e) Lanes<T>::set(acc, e, Lanes<T>::get(acc, e) / cnt);
    }
    y[i] = acc;
    if (MAX && idx) idx[i] = at;
  }
}

// per-input gather: AVG dx = g[window] / count(window); MAX dx = g[window] where the recorded offset is this pixel's, else 0
template <typename T, bool MAX>
__global__ __launch_bounds__(kThreads) void pool_same_bwd_kernel(const T* __restrict__ g, const typename IdxOf<T>::type* __restrict__ idx,
                                                                  int H, int W, int C, int s, int pt, int pl, int Ho, int Wo, size_t n_in,
                                                                  T* __restrict__ dx) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_in; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    size_t p = i / C;
    const int w = (int)(p % W); p /= W;
    const int h = (int)(p % H);
    const size_t b = p / H;
    const int oh = (h + pt) / s, ow = (w + pl) / s;
    const size_t o = ((b * Ho + oh) * Wo + ow) * C + c;
    T t = g[o];
    if (MAX) {
      const int k = (h + pt - oh * s) * s + (w + pl - ow * s);
      const typename IdxOf<T>::type at = idx[o];
#pragma unroll
      for (int e = 0; e < Lanes<T>::N; ++e)
        if (iget(at, e) != k) Lanes<T>::set(t, e, 0.f);
    } else {
      const int h0 = oh * s - pt, w0 = ow * s - pl;
      const int ha = h0 < 0 ? 0 : h0, hb = h0 + s < H ? h0 + s : H;
      const int wa = w0 < 0 ? 0 : w0, wb = w0 + s < W ? w0 + s : W;
      const float cnt = (float)((hb - ha) * (wb - wa));
#pragma unroll
      for (int e = 0; e < Lanes<T>::N; ++e) Lanes<T>::set(t, e, Lanes<T>::get(t, e) / cnt);
    }
    dx[i] = t;
  }
}

// y[o] = x[the pixel of o's window at the recorded offset]: MAX pooling as the linear map it is once the offsets are fixed
// (the backward of the MAX backward).  An offset that leaves the image reads nothing and gives 0.
template <typename T>
__global__ __launch_bounds__(kThreads) void pool_same_take_kernel(const float* __restrict__ x, const typename IdxOf<T>::type* __restrict__ idx,
                                                                   int H, int W, int C /* floats */, int s, int pt, int pl, int Ho, int Wo,
                                                                   size_t n_out, T* __restrict__ y) {
  const int Cu = C / Lanes<T>::N;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_out; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % Cu);
    size_t p = i / Cu;
    const int ow = (int)(p % Wo); p /= Wo;
    const int oh = (int)(p % Ho);
    const size_t b = p / Ho;
    const typename IdxOf<T>::type at = idx[i];
    T t;
#pragma unroll
    for (int e = 0; e < Lanes<T>::N; ++e) {
      const int k = iget(at, e);
      const int h = oh * s - pt + (k >= 0 ? k / s : -1), w = ow * s - pl + (k >= 0 ? k % s : -1);
      const bool in = k >= 0 && k < s * s && h >= 0 && h < H && w >= 0 && w < W;
      Lanes<T>::set(t, e, in ? x[((b * H + h) * W + w) * (size_t)C + (size_t)c * Lanes<T>::N + e] : 0.f);
    }
    y[i] = t;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// gn (reference utils/ops.py:145-148): y = x * m^n, n ~ N(0, 1) per element; f = exp(n log m) is kept for the backward g * f.
// Normals: Box-Muller on the four 24-bit uniforms of one Philox4x32-10 call per four elements, keyed by (seed) and counted by
// (offset + element / 4) with the third counter word set to kPhiloxGn — t2i_trunc_normal's is kPhiloxTruncNormal (t2i_internal.h
// holds the generator and both constants), so the two streams never share a counter.  log m = 0 gives f = exp(0) = 1 and y = x bit for bit.
// ---------------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(kThreads) void gn_fwd_kernel(const float* __restrict__ x, size_t n, float log_m, unsigned long long seed,
                                                           unsigned long long offset, float* __restrict__ y, float* __restrict__ f) {
  const size_t quads = (n + 3) >> 2;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (size_t)gridDim.x * blockDim.x) {
    const unsigned long long ctr = offset + q;
    unsigned r[4];
    philox4x32_10((unsigned)ctr, (unsigned)(ctr >> 32), kPhiloxGn, 0u, (unsigned)seed, (unsigned)(seed >> 32), r);
    float fac[4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float u1 = ((float)(r[2 * h] >> 8) + 0.5f) * (1.0f / 16777216.0f);        // (0, 1), 24 bits
      const float u2 = ((float)(r[2 * h + 1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
      const float rad = sqrtf(-2.f * logf(u1));
      float sn, cs;
      sincosf(6.28318530718f * u2, &sn, &cs);
      fac[2 * h] = expf(rad * cs * log_m);
      fac[2 * h + 1] = expf(rad * sn * log_m);
    }
    const size_t i0 = q * 4;
    if (VEC && i0 + 4 <= n) {
      const float4 xv = *reinterpret_cast<const float4*>(x + i0);
      *reinterpret_cast<float4*>(y + i0) = make_float4(xv.x * fac[0], xv.y * fac[1], xv.z * fac[2], xv.w * fac[3]);
      if (f) *reinterpret_cast<float4*>(f + i0) = make_float4(fac[0], fac[1], fac[2], fac[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (i0 + e < n) { y[i0 + e] = x[i0 + e] * fac[e]; if (f) f[i0 + e] = fac[e]; }
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void mul_kernel(const float* __restrict__ a, const float* __restrict__ b, size_t n, float* __restrict__ y) {
  const size_t quads = (n + 3) >> 2;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (size_t)gridDim.x * blockDim.x) {
    const size_t i0 = q * 4;
    if (VEC && i0 + 4 <= n) {
      const float4 av = *reinterpret_cast<const float4*>(a + i0), bv = *reinterpret_cast<const float4*>(b + i0);
      *reinterpret_cast<float4*>(y + i0) = make_float4(av.x * bv.x, av.y * bv.y, av.z * bv.z, av.w * bv.w);
    } else {
      for (int e = 0; e < 4; ++e)
        if (i0 + e < n) y[i0 + e] = a[i0 + e] * b[i0 + e];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Minibatch standard deviation (the PGGAN paper's critic layer) with its backward and double backward.
// x [B,H,W,C]; sample n is in group n / G (contiguous rows), channel c in chunk c / (C/F).  Per column j = (h, w, c) of a group:
//   mu = mean_g x,  d_g = x_g - mu,  sigma = sqrt(mean_g d_g^2 + eps);   stat[m, f] = mean of sigma over the Nf = H W C/F columns of chunk f.
// With k = (sum_g gs[g, f]) / (Nf G), and v the cotangent of dx:
//   dx_g = k d_g / sigma;   dL/dgs = (1 / (Nf G)) sum_{g, j} v_g d_g / sigma;
//   dL/dx_g = k [(v_g - mean_g v) / sigma - d_g (sum_g v_g d_g) / (G sigma^3)].
// A thread owns one unit (float4 or float) of a column block and holds it for the G samples of its group in registers (G <= 16:
// 64 VGPRs of float4), so mu and the centred variance come from the registers in two passes — no E[x^2] - mu^2.  A workgroup
// covers kMbBlockUnits units of one (group, chunk), grid (blocks, F, B / G): how a group is cut depends on the sample's shape
// alone, never on the number of groups, so the statistic of a batch is bit for bit the statistics of its parts (the critic's 3B
// pass relies on it).  Sums: the G samples in order in a thread, the wave's butterfly, the four waves in a fixed tree, then one wave
// per (group, chunk) joins the workgroups' partials in a fixed order.  The register arrays are sized by GMAX in {2, 4, 8, 16}.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int kMbGroupMax = 16;
constexpr int kMbBlockUnits = kThreads;      // one unit per thread

struct MbGeom {        // counted in units of T
  int nfu;             // units of one (group, chunk) = H W cfu
  int cfu, cu;         // units per pixel of a chunk / of all chunks
  size_t pu;           // units per sample
  FastDiv div_cf;
};

template <typename T, int GMAX>
__device__ __forceinline__ void mb_load(const T* __restrict__ p, size_t base, size_t pu, int G, T (&r)[GMAX]) {
#pragma unroll
  for (int g = 0; g < GMAX; ++g) r[g] = g < G ? p[base + (size_t)g * pu] : splat<T>(0.f);
}

template <typename T, int GMAX>
__device__ __forceinline__ void mb_store(T* __restrict__ p, size_t base, size_t pu, int G, const T (&r)[GMAX]) {
#pragma unroll
  for (int g = 0; g < GMAX; ++g)
    if (g < G) p[base + (size_t)g * pu] = r[g];
}

template <typename T, int GMAX>
__device__ __forceinline__ void mb_stats(const T (&r)[GMAX], int e, int G, float eps, float& mu, float& sigma) {
  float s = 0.f;
#pragma unroll
  for (int g = 0; g < GMAX; ++g)
    if (g < G) s += Lanes<T>::get(r[g], e);
  mu = s / (float)G;
  float q = 0.f;
#pragma unroll
  for (int g = 0; g < GMAX; ++g)
    if (g < G) { const float d = Lanes<T>::get(r[g], e) - mu; q += d * d; }
  sigma = sqrtf(q / (float)G + eps);
}

// the unit's offset inside its sample; q < nfu
__device__ __forceinline__ size_t mb_offset(const MbGeom& ge, int q, int f) {
  const int p = ge.div_cf.div(q);
  return (size_t)p * ge.cu + (size_t)f * ge.cfu + (size_t)(q - p * ge.cfu);
}

__device__ __forceinline__ float mb_gbar(const float* __restrict__ gs, int m, int f, int G, int F) {
  float s = 0.f;
  for (int g = 0; g < G; ++g) s += gs[((size_t)m * G + g) * F + f];
  return s;
}

// every thread of the workgroup calls this: the workgroup's sum, written by thread 0
__device__ __forceinline__ void mb_block_partial(float acc, float* red, float* __restrict__ part) {
  const float s = group_sum(acc, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

template <typename T, int GMAX>
__global__ __launch_bounds__(kThreads) void mbstd_fwd_kernel(const T* __restrict__ x, MbGeom ge, int G, float eps, float* __restrict__ part) {
  __shared__ float red[kThreads / 64];
  const int q = blockIdx.x * kMbBlockUnits + threadIdx.x;
  float acc = 0.f;
  if (q < ge.nfu) {
    const size_t base = (size_t)blockIdx.z * G * ge.pu + mb_offset(ge, q, blockIdx.y);
    T r[GMAX];
    mb_load<T, GMAX>(x, base, ge.pu, G, r);
#pragma unroll
    for (int e = 0; e < Lanes<T>::N; ++e) {
      float mu, sigma;
      mb_stats<T, GMAX>(r, e, G, eps, mu, sigma);
      acc += sigma;
    }
  }
  mb_block_partial(acc, red, part);
}

// grid (F, B / G), one wave: lane l adds the partials l, l + 64, ... in order, the butterfly joins the lanes; the G rows of the group
// all receive sum / denom
__global__ __launch_bounds__(64) void mbstd_join_kernel(const float* __restrict__ part, int nblk, int G, float denom, float* __restrict__ out) {
  const int f = blockIdx.x, F = gridDim.x, m = blockIdx.y;
  const float* p = part + ((size_t)m * F + f) * nblk;
  float a = 0.f;
  for (int k = threadIdx.x; k < nblk; k += 64) a += p[k];
  a = group_sum(a, 64);
  if ((int)threadIdx.x < G) out[((size_t)m * G + threadIdx.x) * F + f] = a / denom;
}

template <typename T, int GMAX>
__global__ __launch_bounds__(kThreads) void mbstd_bwd_kernel(const float* __restrict__ gs, const T* __restrict__ x, MbGeom ge, int G, float eps,
                                                              float denom, T* __restrict__ dx) {
  const int q = blockIdx.x * kMbBlockUnits + threadIdx.x;
  if (q >= ge.nfu) return;
  const float k = mb_gbar(gs, blockIdx.z, blockIdx.y, G, gridDim.y) / denom;
  const size_t base = (size_t)blockIdx.z * G * ge.pu + mb_offset(ge, q, blockIdx.y);
  T r[GMAX];
  mb_load<T, GMAX>(x, base, ge.pu, G, r);
#pragma unroll
  for (int e = 0; e < Lanes<T>::N; ++e) {
    float mu, sigma;
    mb_stats<T, GMAX>(r, e, G, eps, mu, sigma);
    const float ks = k / sigma;
#pragma unroll
    for (int g = 0; g < GMAX; ++g)
      if (g < G) Lanes<T>::set(r[g], e, ks * (Lanes<T>::get(r[g], e) - mu));
  }
  mb_store<T, GMAX>(dx, base, ge.pu, G, r);
}

template <typename T, int GMAX>
__global__ __launch_bounds__(kThreads) void mbstd_bwd2_kernel(const T* __restrict__ v, const T* __restrict__ x, const float* __restrict__ gs,
                                                               MbGeom ge, int G, float eps, float denom, T* __restrict__ dxx,
                                                               float* __restrict__ part) {
  __shared__ float red[kThreads / 64];
  const int q = blockIdx.x * kMbBlockUnits + threadIdx.x;
  float acc = 0.f;
  if (q < ge.nfu) {
    const float k = mb_gbar(gs, blockIdx.z, blockIdx.y, G, gridDim.y) / denom;
    const size_t base = (size_t)blockIdx.z * G * ge.pu + mb_offset(ge, q, blockIdx.y);
    T r[GMAX], w[GMAX];
    mb_load<T, GMAX>(x, base, ge.pu, G, r);
    mb_load<T, GMAX>(v, base, ge.pu, G, w);
#pragma unroll
    for (int e = 0; e < Lanes<T>::N; ++e) {
      float mu, sigma;
      mb_stats<T, GMAX>(r, e, G, eps, mu, sigma);
      float sv = 0.f, t = 0.f;
#pragma unroll
      for (int g = 0; g < GMAX; ++g)
        if (g < G) { const float vv = Lanes<T>::get(w[g], e); sv += vv; t += vv * (Lanes<T>::get(r[g], e) - mu); }
      const float vbar = sv / (float)G, is = 1.0f / sigma;
      const float a = k * is, b = k * t * (is * is * is) / (float)G;
#pragma unroll
      for (int g = 0; g < GMAX; ++g)
        if (g < G) Lanes<T>::set(w[g], e, a * (Lanes<T>::get(w[g], e) - vbar) - b * (Lanes<T>::get(r[g], e) - mu));
      acc += t * is;
    }
    mb_store<T, GMAX>(dxx, base, ge.pu, G, w);
  }
  mb_block_partial(acc, red, part);
}

inline MbGeom mb_geom(int H, int W, int C, int F, bool v4) {
  const int sh = v4 ? 2 : 0;
  MbGeom ge;
  ge.cfu = (C / F) >> sh;
  ge.cu = C >> sh;
  ge.nfu = H * W * ge.cfu;
  ge.pu = (size_t)H * W * ge.cu;
  ge.div_cf.set((uint32_t)ge.cfu);
  return ge;
}

inline int mb_blocks(int nfu) { return (nfu + kMbBlockUnits - 1) / kMbBlockUnits; }

constexpr long long kMaxElems = (1ll << 30) - 16;        // include/t2i_hip.h: no tensor may exceed 2^30 - 16 elements

// G in 1..16 dividing B, F >= 1 dividing C; the grid is (blocks, F, B / G)
inline bool mb_shape_ok(int32_t B, int32_t H, int32_t W, int32_t C, int32_t G, int32_t F) {
  return B > 0 && H > 0 && W > 0 && C > 0 && G >= 1 && G <= kMbGroupMax && B % G == 0 && F >= 1 && F <= 65535 && C % F == 0 &&
         B / G <= 65535 && (long long)B * H * W <= kMaxElems / C;
}

inline bool act_ok(int act, float alpha) {       // lrelu: a slope >= 0 only (pixel_norm_dx)
  return act == T2I_ACT_NONE || (act == T2I_ACT_LRELU && alpha >= 0.f) || act == T2I_ACT_RELU || act == T2I_ACT_TANH;
}

}  // namespace
}  // namespace t2i

using namespace t2i;

int t2i_pixel_norm_fwd(const float* x, int64_t rows, int32_t C, float eps, int act, float alpha, float* y, float* rnorm,
                       t2i_stream_t stream) {
  if (!x || !y || !rnorm || rows <= 0 || C <= 0 || !act_ok(act, alpha) || rows > kMaxElems / C) {
    set_error("t2i_pixel_norm_fwd: bad argument (rows=%lld C=%d act=%d alpha=%g; an lrelu slope must be >= 0)", (long long)rows, C, act, (double)alpha);
    return T2I_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  const bool v4 = (C & 3) == 0 && al16(x) && al16(y);
  const int units = v4 ? C >> 2 : C;
  const int G = group_lanes(units);
  const bool reg = units <= kPer * G;
  const dim3 grid((unsigned)((rows + kThreads / G - 1) / (kThreads / G)));
#define T2I_PN(TT, RR)                                                                                                                   \
  hipLaunchKernelGGL((pixel_norm_fwd_kernel<TT, RR>), grid, dim3(kThreads), 0, st, reinterpret_cast<const TT*>(x), (long long)rows, units, C, \
                     G, eps, act, alpha, reinterpret_cast<TT*>(y), rnorm)
  if (v4) { if (reg) T2I_PN(float4, true); else T2I_PN(float4, false); }
  else { if (reg) T2I_PN(float, true); else T2I_PN(float, false); }
#undef T2I_PN
  return launched("t2i_pixel_norm_fwd");
}

int t2i_pixel_norm_bwd(const float* g, const float* y, const float* rnorm, int64_t rows, int32_t C, int act, float alpha, float* dx,
                       t2i_stream_t stream) {
  if (!g || !y || !rnorm || !dx || rows <= 0 || C <= 0 || !act_ok(act, alpha) || rows > kMaxElems / C) {
    set_error("t2i_pixel_norm_bwd: bad argument (rows=%lld C=%d act=%d alpha=%g; an lrelu slope must be >= 0)", (long long)rows, C, act, (double)alpha);
    return T2I_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  const bool v4 = (C & 3) == 0 && al16(g) && al16(y) && al16(dx);
  const int units = v4 ? C >> 2 : C;
  const int G = group_lanes(units);
  const bool reg = units <= kPer * G;
  const dim3 grid((unsigned)((rows + kThreads / G - 1) / (kThreads / G)));
#define T2I_PN(TT, RR)                                                                                                             \
  hipLaunchKernelGGL((pixel_norm_bwd_kernel<TT, RR>), grid, dim3(kThreads), 0, st, reinterpret_cast<const TT*>(g),                 \
                     reinterpret_cast<const TT*>(y), rnorm, (long long)rows, units, C, G, act, alpha, reinterpret_cast<TT*>(dx))
  if (v4) { if (reg) T2I_PN(float4, true); else T2I_PN(float4, false); }
  else { if (reg) T2I_PN(float, true); else T2I_PN(float, false); }
#undef T2I_PN
  return launched("t2i_pixel_norm_bwd");
}

// second order: lrelu (slope >= 0) and relu only — tanh has a second derivative these kernels do not carry
static bool act2_ok(int act, float alpha) { return act_ok(act, alpha) && act != T2I_ACT_TANH; }

int t2i_pixel_norm_bwd2(const float* v, const float* g, const float* y, const float* rnorm, int64_t rows, int32_t C, int act, float alpha,
                        float* dg, float* dx, t2i_stream_t stream) {
  if (!v || !g || !y || !rnorm || !dg || !dx || rows <= 0 || C <= 0 || !act2_ok(act, alpha) || rows > kMaxElems / C) {
    set_error("t2i_pixel_norm_bwd2: bad argument (rows=%lld C=%d act=%d alpha=%g; none, relu or an lrelu slope >= 0)", (long long)rows, C, act,
              (double)alpha);
    return T2I_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  const bool v4 = (C & 3) == 0 && al16(v) && al16(g) && al16(y) && al16(dg) && al16(dx);
  const int units = v4 ? C >> 2 : C;
  const int G = group_lanes(units);
  const int per_lane = (units + G - 1) / G;
  const dim3 grid((unsigned)((rows + kThreads / G - 1) / (kThreads / G)));
#define T2I_PN(TT, PP)                                                                                                                    \
  hipLaunchKernelGGL((pixel_norm_bwd2_kernel<TT, PP>), grid, dim3(kThreads), 0, st, reinterpret_cast<const TT*>(v),                       \
                     reinterpret_cast<const TT*>(g), reinterpret_cast<const TT*>(y), rnorm, (long long)rows, units, C, G, act, alpha,     \
                     reinterpret_cast<TT*>(dg), reinterpret_cast<TT*>(dx))
#define T2I_PN_PER(TT)                                                                                                                    \
  do {                                                                                                                                    \
    if (per_lane <= 1) T2I_PN(TT, 1); else if (per_lane <= 2) T2I_PN(TT, 2); else if (per_lane <= 4) T2I_PN(TT, 4);                       \
    else if (per_lane <= kPer) T2I_PN(TT, kPer); else T2I_PN(TT, 0);                                                                      \
  } while (0)
  if (v4) T2I_PN_PER(float4); else T2I_PN_PER(float);
#undef T2I_PN_PER
#undef T2I_PN
  return launched("t2i_pixel_norm_bwd2");
}

static bool ln2_args_ok(const void* v, const void* gy, const void* xhat, const void* y, const void* gamma, int32_t B, int64_t per, int32_t C,
                        int act, float alpha) {
  return v && gy && xhat && gamma && B > 0 && B <= 65535 && C > 0 && per > 0 && per % C == 0 && per <= kMaxElems / B && act2_ok(act, alpha) &&
         (act == T2I_ACT_NONE || y);
}

size_t t2i_layer_norm_bwd2_workspace_bytes(int32_t B) { return B > 0 ? (size_t)B * kLnChunksMax * kLnSums * sizeof(float) : 0; }

int t2i_layer_norm_bwd2_sums(const float* v, const float* gy, const float* xhat, const float* y, const float* gamma, int32_t B,
                             int64_t per_sample, int32_t C, int act, float alpha, float* sums, void* ws, size_t ws_bytes,
                             t2i_stream_t stream) {
  if (!ln2_args_ok(v, gy, xhat, y, gamma, B, per_sample, C, act, alpha) || !sums) {
    set_error("t2i_layer_norm_bwd2_sums: bad argument (B=%d per_sample=%lld C=%d act=%d alpha=%g)", B, (long long)per_sample, C, act, (double)alpha);
    return T2I_ERR_INVALID;
  }
  if (!ws || ws_bytes < t2i_layer_norm_bwd2_workspace_bytes(B)) { set_error("t2i_layer_norm_bwd2_sums: workspace too small"); return T2I_ERR_WORKSPACE; }
  hipStream_t st = (hipStream_t)stream;
  if (act == T2I_ACT_NONE) y = nullptr;
  const bool v4 = (C & 3) == 0 && al16(v) && al16(gy) && al16(xhat) && al16(y) && al16(gamma);
  const LnSplit sp = ln_split(per_sample, v4);
  float* part = reinterpret_cast<float*>(ws);
  FastDiv div_c;
  const dim3 grid((unsigned)sp.chunks, (unsigned)B);
  if (v4) {
    div_c.set((uint32_t)(C >> 2));
    hipLaunchKernelGGL(layer_norm_bwd2_sums_kernel<float4>, grid, dim3(kThreads), 0, st, reinterpret_cast<const float4*>(v),
                       reinterpret_cast<const float4*>(gy), reinterpret_cast<const float4*>(xhat), reinterpret_cast<const float4*>(y),
                       reinterpret_cast<const float4*>(gamma), (int)(per_sample >> 2), (int)(sp.per_chunk >> 2), C >> 2, div_c, act, alpha, part);
  } else {
    div_c.set((uint32_t)C);
    hipLaunchKernelGGL(layer_norm_bwd2_sums_kernel<float>, grid, dim3(kThreads), 0, st, v, gy, xhat, y, gamma, (int)per_sample,
                       (int)sp.per_chunk, C, div_c, act, alpha, part);
  }
  hipLaunchKernelGGL(layer_norm_bwd2_sums_stage2, dim3((unsigned)B), dim3(64), 0, st, part, sp.chunks, sums);
  return launched("t2i_layer_norm_bwd2_sums");
}

int t2i_layer_norm_bwd2_apply(const float* v, const float* gy, const float* xhat, const float* y, const float* gamma, const float* rstd,
                              const float* sums, int32_t B, int64_t per_sample, int32_t C, int act, float alpha, float* dgy, float* dx,
                              float* hgz, t2i_stream_t stream) {
  if (!ln2_args_ok(v, gy, xhat, y, gamma, B, per_sample, C, act, alpha) || !rstd || !sums || !dgy || !dx) {
    set_error("t2i_layer_norm_bwd2_apply: bad argument (B=%d per_sample=%lld C=%d act=%d alpha=%g)", B, (long long)per_sample, C, act, (double)alpha);
    return T2I_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  if (act == T2I_ACT_NONE) y = nullptr;
  const bool v4 = (C & 3) == 0 && al16(v) && al16(gy) && al16(xhat) && al16(y) && al16(gamma) && al16(dgy) && al16(dx) && al16(hgz);
  const float inv_n = 1.0f / (float)per_sample;
  FastDiv div_per, div_c;
  if (v4) {
    const size_t n = (size_t)B * (size_t)(per_sample >> 2);
    div_per.set((uint32_t)(per_sample >> 2));
    div_c.set((uint32_t)(C >> 2));
    hipLaunchKernelGGL(layer_norm_bwd2_apply_kernel<float4>, dim3(blocks_for(n)), dim3(kThreads), 0, st, reinterpret_cast<const float4*>(v),
                       reinterpret_cast<const float4*>(gy), reinterpret_cast<const float4*>(xhat), reinterpret_cast<const float4*>(y),
                       reinterpret_cast<const float4*>(gamma), rstd, sums, (int)n, (int)(per_sample >> 2), C >> 2, div_per, div_c, inv_n, act,
                       alpha, reinterpret_cast<float4*>(dgy), reinterpret_cast<float4*>(dx), reinterpret_cast<float4*>(hgz));
  } else {
    const size_t n = (size_t)B * (size_t)per_sample;
    div_per.set((uint32_t)per_sample);
    div_c.set((uint32_t)C);
    hipLaunchKernelGGL(layer_norm_bwd2_apply_kernel<float>, dim3(blocks_for(n)), dim3(kThreads), 0, st, v, gy, xhat, y, gamma, rstd, sums, (int)n,
                       (int)per_sample, C, div_per, div_c, inv_n, act, alpha, dgy, dx, hgz);
  }
  return launched("t2i_layer_norm_bwd2_apply");
}

static bool resize_args_ok(const void* a, const void* b, int32_t B, int32_t H, int32_t W, int32_t C, int32_t Ho, int32_t Wo) {
  return a && b && B > 0 && H > 0 && W > 0 && C > 0 && Ho > 0 && Wo > 0 && (long long)B * H * W <= kMaxElems / C &&
         (long long)B * Ho * Wo <= kMaxElems / C;
}

int t2i_resize_nearest(const float* x, int32_t B, int32_t H, int32_t W, int32_t C, int32_t Ho, int32_t Wo, float* y, t2i_stream_t stream) {
  if (!resize_args_ok(x, y, B, H, W, C, Ho, Wo)) {
    set_error("t2i_resize_nearest: bad argument (B=%d %dx%dx%d -> %dx%d)", B, H, W, C, Ho, Wo);
    return T2I_ERR_INVALID;
  }
  const float hs = (float)H / (float)Ho, ws = (float)W / (float)Wo;
  hipStream_t st = (hipStream_t)stream;
  if ((C & 3) == 0 && al16(x) && al16(y)) {
    const size_t n = (size_t)B * Ho * Wo * (C >> 2);
    hipLaunchKernelGGL(resize_nearest_kernel<float4>, dim3(blocks_for(n)), dim3(kThreads), 0, st, reinterpret_cast<const float4*>(x), H, W,
                       C >> 2, Ho, Wo, hs, ws, n, reinterpret_cast<float4*>(y));
  } else {
    const size_t n = (size_t)B * Ho * Wo * C;
    hipLaunchKernelGGL(resize_nearest_kernel<float>, dim3(blocks_for(n)), dim3(kThreads), 0, st, x, H, W, C, Ho, Wo, hs, ws, n, y);
  }
  return launched("t2i_resize_nearest");
}

int t2i_resize_nearest_adj(const float* g, int32_t B, int32_t H, int32_t W, int32_t C, int32_t Ho, int32_t Wo, float* dx,
                           t2i_stream_t stream) {
  if (!resize_args_ok(g, dx, B, H, W, C, Ho, Wo)) {
    set_error("t2i_resize_nearest_adj: bad argument (B=%d %dx%dx%d <- %dx%d)", B, H, W, C, Ho, Wo);
    return T2I_ERR_INVALID;
  }
  const float hs = (float)H / (float)Ho, ws = (float)W / (float)Wo;
  hipStream_t st = (hipStream_t)stream;
  if ((C & 3) == 0 && al16(g) && al16(dx)) {
    const size_t n = (size_t)B * H * W * (C >> 2);
    hipLaunchKernelGGL(resize_nearest_adj_kernel<float4>, dim3(blocks_for(n)), dim3(kThreads), 0, st, reinterpret_cast<const float4*>(g), H,
                       W, C >> 2, Ho, Wo, hs, ws, n, reinterpret_cast<float4*>(dx));
  } else {
    const size_t n = (size_t)B * H * W * C;
    hipLaunchKernelGGL(resize_nearest_adj_kernel<float>, dim3(blocks_for(n)), dim3(kThreads), 0, st, g, H, W, C, Ho, Wo, hs, ws, n, dx);
  }
  return launched("t2i_resize_nearest_adj");
}

// shared by the three pool entry points: extents, padding and the size limits
static bool pool_geom(const char* what, int32_t B, int32_t H, int32_t W, int32_t C, int32_t s, int* Ho, int* Wo, int* pt, int* pl) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || s <= 0 || s > 32768 || (long long)B * H * W > kMaxElems / C) {
    set_error("%s: bad argument (B=%d %dx%dx%d, window %d; 1 <= window <= 32768)", what, B, H, W, C, s);
    return false;
  }
  *Ho = (H + s - 1) / s;
  *Wo = (W + s - 1) / s;
  *pt = (*Ho * s - H) / 2;
  *pl = (*Wo * s - W) / 2;
  return true;
}

int t2i_pool_same_fwd(const float* x, int32_t B, int32_t H, int32_t W, int32_t C, int32_t s, int32_t op, float* y, int32_t* idx,
                      t2i_stream_t stream) {
  int Ho, Wo, pt, pl;
  if (!pool_geom("t2i_pool_same_fwd", B, H, W, C, s, &Ho, &Wo, &pt, &pl)) return T2I_ERR_INVALID;
  if (!x || !y || (op != T2I_POOL_MAX && op != T2I_POOL_AVG) || (op == T2I_POOL_AVG && idx)) {
    set_error("t2i_pool_same_fwd: bad argument (null tensor, unknown op %d, or offsets asked of AVG)", op);
    return T2I_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  const bool v4 = (C & 3) == 0 && al16(x) && al16(y) && al16(idx);
#define T2I_PL(TT, MX, CC)                                                                                                              \
  do {                                                                                                                                  \
    const size_t n = (size_t)B * Ho * Wo * (CC);                                                                                        \
    hipLaunchKernelGGL((pool_same_fwd_kernel<TT, MX>), dim3(blocks_for(n)), dim3(kThreads), 0, st, reinterpret_cast<const TT*>(x), H, W, \
                       (CC), s, pt, pl, Ho, Wo, n, reinterpret_cast<TT*>(y), reinterpret_cast<IdxOf<TT>::type*>(idx));                   \
  } while (0)
  if (v4) { if (op == T2I_POOL_MAX) T2I_PL(float4, true, C >> 2); else T2I_PL(float4, false, C >> 2); }
  else { if (op == T2I_POOL_MAX) T2I_PL(float, true, C); else T2I_PL(float, false, C); }
#undef T2I_PL
  return launched("t2i_pool_same_fwd");
}

int t2i_pool_same_bwd(const float* g, const int32_t* idx, int32_t B, int32_t H, int32_t W, int32_t C, int32_t s, int32_t op, float* dx,
                      t2i_stream_t stream) {
  int Ho, Wo, pt, pl;
  if (!pool_geom("t2i_pool_same_bwd", B, H, W, C, s, &Ho, &Wo, &pt, &pl)) return T2I_ERR_INVALID;
  if (!g || !dx || (op != T2I_POOL_MAX && op != T2I_POOL_AVG) || (op == T2I_POOL_MAX && !idx)) {
    set_error("t2i_pool_same_bwd: bad argument (null tensor, unknown op %d, or MAX without offsets)", op);
    return T2I_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  const bool v4 = (C & 3) == 0 && al16(g) && al16(dx) && al16(idx);
#define T2I_PL(TT, MX, CC)                                                                                                              \
  do {                                                                                                                                  \
    const size_t n = (size_t)B * H * W * (CC);                                                                                          \
    hipLaunchKernelGGL((pool_same_bwd_kernel<TT, MX>), dim3(blocks_for(n)), dim3(kThreads), 0, st, reinterpret_cast<const TT*>(g),       \
                       reinterpret_cast<const IdxOf<TT>::type*>(idx), H, W, (CC), s, pt, pl, Ho, Wo, n, reinterpret_cast<TT*>(dx));      \
  } while (0)
  if (v4) { if (op == T2I_POOL_MAX) T2I_PL(float4, true, C >> 2); else T2I_PL(float4, false, C >> 2); }
  else { if (op == T2I_POOL_MAX) T2I_PL(float, true, C); else T2I_PL(float, false, C); }
#undef T2I_PL
  return launched("t2i_pool_same_bwd");
}

int t2i_pool_same_take(const float* x, const int32_t* idx, int32_t B, int32_t H, int32_t W, int32_t C, int32_t s, float* y,
                       t2i_stream_t stream) {
  int Ho, Wo, pt, pl;
  if (!pool_geom("t2i_pool_same_take", B, H, W, C, s, &Ho, &Wo, &pt, &pl)) return T2I_ERR_INVALID;
  if (!x || !idx || !y) { set_error("t2i_pool_same_take: null tensor"); return T2I_ERR_INVALID; }
  hipStream_t st = (hipStream_t)stream;
  if ((C & 3) == 0 && al16(y) && al16(idx)) {
    const size_t n = (size_t)B * Ho * Wo * (C >> 2);
    hipLaunchKernelGGL(pool_same_take_kernel<float4>, dim3(blocks_for(n)), dim3(kThreads), 0, st, x, reinterpret_cast<const int4*>(idx), H, W, C,
                       s, pt, pl, Ho, Wo, n, reinterpret_cast<float4*>(y));
  } else {
    const size_t n = (size_t)B * Ho * Wo * C;
    hipLaunchKernelGGL(pool_same_take_kernel<float>, dim3(blocks_for(n)), dim3(kThreads), 0, st, x, idx, H, W, C, s, pt, pl, Ho, Wo, n, y);
  }
  return launched("t2i_pool_same_take");
}

int t2i_gn_fwd(const float* x, int64_t n, float log_m, uint64_t seed, uint64_t offset, float* y, float* f, t2i_stream_t stream) {
  if (!x || !y || n <= 0 || n > kMaxElems || !(log_m >= 0.f) || !(log_m < 64.f)) {
    set_error("t2i_gn_fwd: bad argument (n=%lld log_m=%g)", (long long)n, (double)log_m);
    return T2I_ERR_INVALID;
  }
  const size_t quads = ((size_t)n + 3) >> 2;
  if (al16(x) && al16(y) && al16(f))
    hipLaunchKernelGGL(gn_fwd_kernel<true>, dim3(blocks_for(quads)), dim3(kThreads), 0, (hipStream_t)stream, x, (size_t)n, log_m,
                       (unsigned long long)seed, (unsigned long long)offset, y, f);
  else
    hipLaunchKernelGGL(gn_fwd_kernel<false>, dim3(blocks_for(quads)), dim3(kThreads), 0, (hipStream_t)stream, x, (size_t)n, log_m,
                       (unsigned long long)seed, (unsigned long long)offset, y, f);
  return launched("t2i_gn_fwd");
}

int t2i_mul(const float* a, const float* b, int64_t n, float* y, t2i_stream_t stream) {
  if (!a || !b || !y || n <= 0 || n > kMaxElems) {
    set_error("t2i_mul: bad argument (n=%lld)", (long long)n);
    return T2I_ERR_INVALID;
  }
  const size_t quads = ((size_t)n + 3) >> 2;
  if (al16(a) && al16(b) && al16(y))
    hipLaunchKernelGGL(mul_kernel<true>, dim3(blocks_for(quads)), dim3(kThreads), 0, (hipStream_t)stream, a, b, (size_t)n, y);
  else
    hipLaunchKernelGGL(mul_kernel<false>, dim3(blocks_for(quads)), dim3(kThreads), 0, (hipStream_t)stream, a, b, (size_t)n, y);
  return launched("t2i_mul");
}

// ---- minibatch standard deviation ------------------------------------------------------------------------------------------------
#define T2I_MB_GMAX(KERNEL, TT, ...)                                                                                                      \
  do {                                                                                                                                    \
    if (G <= 2) hipLaunchKernelGGL((KERNEL<TT, 2>), grid, dim3(kThreads), 0, st, __VA_ARGS__);                                            \
    else if (G <= 4) hipLaunchKernelGGL((KERNEL<TT, 4>), grid, dim3(kThreads), 0, st, __VA_ARGS__);                                       \
    else if (G <= 8) hipLaunchKernelGGL((KERNEL<TT, 8>), grid, dim3(kThreads), 0, st, __VA_ARGS__);                                       \
    else hipLaunchKernelGGL((KERNEL<TT, kMbGroupMax>), grid, dim3(kThreads), 0, st, __VA_ARGS__);                                         \
  } while (0)

// the partials of the scalar form, which cuts a (group, chunk) into the most workgroups: the form is chosen at the call, by alignment
size_t t2i_minibatch_stddev_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t C, int32_t G, int32_t F) {
  if (!mb_shape_ok(B, H, W, C, G, F)) return 0;
  return (size_t)(B / G) * (size_t)F * (size_t)mb_blocks(H * W * (C / F)) * sizeof(float);
}

int t2i_minibatch_stddev_fwd(const float* x, int32_t B, int32_t H, int32_t W, int32_t C, int32_t G, int32_t F, float eps, float* stat,
                             void* ws, size_t ws_bytes, t2i_stream_t stream) {
  if (!x || !stat || !mb_shape_ok(B, H, W, C, G, F) || !(eps > 0.f)) {
    set_error("t2i_minibatch_stddev_fwd: bad argument (B=%d H=%d W=%d C=%d G=%d F=%d eps=%g; 1 <= G <= 16 divides B, F >= 1 divides C, eps > 0)", B, H,
              W, C, G, F, (double)eps);
    return T2I_ERR_INVALID;
  }
  if (!ws || ws_bytes < t2i_minibatch_stddev_workspace_bytes(B, H, W, C, G, F)) {
    set_error("t2i_minibatch_stddev_fwd: workspace too small (%zu bytes, %zu needed)", ws ? ws_bytes : (size_t)0,
              t2i_minibatch_stddev_workspace_bytes(B, H, W, C, G, F));
    return T2I_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  const bool v4 = ((C / F) & 3) == 0 && al16(x);
  const MbGeom ge = mb_geom(H, W, C, F, v4);
  const int nblk = mb_blocks(ge.nfu);
  float* part = reinterpret_cast<float*>(ws);
  const dim3 grid((unsigned)nblk, (unsigned)F, (unsigned)(B / G));
  if (v4) T2I_MB_GMAX(mbstd_fwd_kernel, float4, reinterpret_cast<const float4*>(x), ge, G, eps, part);
  else T2I_MB_GMAX(mbstd_fwd_kernel, float, x, ge, G, eps, part);
  hipLaunchKernelGGL(mbstd_join_kernel, dim3((unsigned)F, (unsigned)(B / G)), dim3(64), 0, st, part, nblk, G,
                     (float)((long long)H * W * (C / F)), stat);
  return launched("t2i_minibatch_stddev_fwd");
}

int t2i_minibatch_stddev_bwd(const float* gs, const float* x, int32_t B, int32_t H, int32_t W, int32_t C, int32_t G, int32_t F, float eps,
                             float* dx, t2i_stream_t stream) {
  if (!gs || !x || !dx || !mb_shape_ok(B, H, W, C, G, F) || !(eps > 0.f)) {
    set_error("t2i_minibatch_stddev_bwd: bad argument (B=%d H=%d W=%d C=%d G=%d F=%d eps=%g; 1 <= G <= 16 divides B, F >= 1 divides C, eps > 0)", B, H,
              W, C, G, F, (double)eps);
    return T2I_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  const bool v4 = ((C / F) & 3) == 0 && al16(x) && al16(dx);
  const MbGeom ge = mb_geom(H, W, C, F, v4);
  const float denom = (float)((long long)H * W * (C / F)) * (float)G;
  const dim3 grid((unsigned)mb_blocks(ge.nfu), (unsigned)F, (unsigned)(B / G));
  if (v4) T2I_MB_GMAX(mbstd_bwd_kernel, float4, gs, reinterpret_cast<const float4*>(x), ge, G, eps, denom, reinterpret_cast<float4*>(dx));
  else T2I_MB_GMAX(mbstd_bwd_kernel, float, gs, x, ge, G, eps, denom, dx);
  return launched("t2i_minibatch_stddev_bwd");
}

int t2i_minibatch_stddev_bwd2(const float* v, const float* x, const float* gs, int32_t B, int32_t H, int32_t W, int32_t C, int32_t G,
                              int32_t F, float eps, float* dxx, float* dgs, void* ws, size_t ws_bytes, t2i_stream_t stream) {
  if (!v || !x || !gs || !dxx || !dgs || !mb_shape_ok(B, H, W, C, G, F) || !(eps > 0.f)) {
    set_error("t2i_minibatch_stddev_bwd2: bad argument (B=%d H=%d W=%d C=%d G=%d F=%d eps=%g; 1 <= G <= 16 divides B, F >= 1 divides C, eps > 0)", B, H,
              W, C, G, F, (double)eps);
    return T2I_ERR_INVALID;
  }
  if (!ws || ws_bytes < t2i_minibatch_stddev_workspace_bytes(B, H, W, C, G, F)) {
    set_error("t2i_minibatch_stddev_bwd2: workspace too small (%zu bytes, %zu needed)", ws ? ws_bytes : (size_t)0,
              t2i_minibatch_stddev_workspace_bytes(B, H, W, C, G, F));
    return T2I_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  const bool v4 = ((C / F) & 3) == 0 && al16(v) && al16(x) && al16(dxx);
  const MbGeom ge = mb_geom(H, W, C, F, v4);
  const int nblk = mb_blocks(ge.nfu);
  const float denom = (float)((long long)H * W * (C / F)) * (float)G;
  float* part = reinterpret_cast<float*>(ws);
  const dim3 grid((unsigned)nblk, (unsigned)F, (unsigned)(B / G));
  if (v4)
    T2I_MB_GMAX(mbstd_bwd2_kernel, float4, reinterpret_cast<const float4*>(v), reinterpret_cast<const float4*>(x), gs, ge, G, eps, denom,
                reinterpret_cast<float4*>(dxx), part);
  else
    T2I_MB_GMAX(mbstd_bwd2_kernel, float, v, x, gs, ge, G, eps, denom, dxx, part);
  hipLaunchKernelGGL(mbstd_join_kernel, dim3((unsigned)F, (unsigned)(B / G)), dim3(64), 0, st, part, nblk, G, denom, dgs);
  return launched("t2i_minibatch_stddev_bwd2");
}
#undef T2I_MB_GMAX
