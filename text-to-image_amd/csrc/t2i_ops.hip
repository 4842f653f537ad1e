// t2i_ops.hip — the rest of the reference's operator surface (reference utils/ops.py:94-116,145-148): pixel_norm, nearest-neighbour
// resize (upscale / downscale by any factor) and its adjoint, tf.nn.pool with window = stride = s under SAME padding (AVG / MAX, any
// extents) with its backward and second-order maps, and the multiplicative noise gn.  All of them are memory-bound single passes:
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

constexpr long long kMaxElems = (1ll << 30) - 16;        // include/t2i_hip.h: no tensor may exceed 2^30 - 16 elements

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
