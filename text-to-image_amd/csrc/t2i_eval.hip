// t2i_eval.hip — the evaluator's kernels around InceptionV3's convolutions (reference evaluation/inception_score.py,
// evaluation/fid.py, utils/utils.py prep_incep_img; the convolutions themselves are t2i_conv2d_fwd):
//
//   resample_h_kernel / resample_v_kernel   Pillow's two-pass 8-bit bilinear resize (Image.resize(BILINEAR)): a horizontal
//                           pass from the uint8 source (or fp32 generator output, denormalised in-kernel as
//                           ((x + 1) * 127.5).astype(uint8) does) into a uint8 intermediate, then a vertical pass that writes
//                           either u / 127.5 - 1 in fp32 (prep_incep_img) or the uint8 pixel.  The filter tables (bounds and
//                           22-bit fixed-point coefficients) are Pillow's, computed on the host per (in, out) size, so
//                           upscaling and antialiased downscaling are the same code.  An optional row-index array gathers the
//                           batch from a larger store.
//   pool_kernel             TF max / average pooling, SAME or VALID, written into a channel slice of a wider buffer (a
//                           concatenation); average divides by the number of in-bounds taps, as TF does.
//   slice_copy_kernel       [rows, C] into channels [c0, c0 + C) of [rows, ld]: the concatenation of conv-branch outputs.
//   gram_kernel / colsum_kernel   FID statistics: (X - s)^T (X - s) on the fp32 matrix pipe (v_mfma_f32_32x32x2_f32) and
//                           sum (X - s), both added into fp64 accumulators.  Each output element is owned by one lane of one
//                           workgroup and summed in a fixed order: no atomics, bitwise-repeatable.
//   cosine_kernel           IMD (reference evaluation/imd.py, scipy.spatial.distance.cosine): one wave64 per row pair; each
//                           lane sums u.v, u.u and v.v of a fixed stride of columns in fp64, then a fixed butterfly across
//                           the wave.  No atomics, bitwise-repeatable.
//   bytescale_minmax_kernel / bytescale_gather_kernel   the caption sheets' scipy.misc.imresize(float image, 'nearest'): scipy's
//                           per-image bytescale and Pillow's NEAREST resize, bit for bit (described at the kernels).
// The element-wise kernels read and write 16-byte vectors over channels where C % 4 == 0 (and the slice is aligned).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "t2i_internal.h"

namespace t2i {

namespace {

constexpr int kThreads = 256;
constexpr int kPrec = 22;                // Pillow PRECISION_BITS for 8-bit images (32 - 8 - 2)

__device__ __forceinline__ int clip8(int v) {       // Pillow clip8: v >> 22 clamped to [0, 255]
  const int s = v >> kPrec;
  return s < 0 ? 0 : (s > 255 ? 255 : s);
}

// ((x + 1) * 127.5).astype(uint8) in fp32 (denormalize_images), saturated to [0, 255] (the generator's tanh never leaves it)
__device__ __forceinline__ int denorm_u8(float x) {
  float v;
  {
#pragma clang fp contract(off)
    v = (x + 1.0f) * 127.5f;
  }
  if (!(v > 0.0f)) return 0;                // also NaN
  return v >= 255.0f ? 255 : (int)v;
}

// Horizontal pass: tmp[b, iy, ox, c] = clip8(2^21 + sum_i px(b, iy, xmin + i, c) * xk[ox, i]) for every source row iy.
template <bool kF32>
__global__ __launch_bounds__(kThreads) void resample_h_kernel(const void* __restrict__ src, int64_t N, int Hi, int Wi,
                                                              const int32_t* __restrict__ rows, int Wo,
                                                              const int32_t* __restrict__ xb, const int32_t* __restrict__ xk,
                                                              int kx, uint8_t* __restrict__ tmp) {
  const int e = blockIdx.x * kThreads + threadIdx.x;
  const int iy = blockIdx.y, b = blockIdx.z;
  if (e >= Wo * 3) return;
  const int ox = e / 3, c = e - 3 * ox;
  const int64_t n = rows ? (int64_t)rows[b] : (int64_t)b;
  int acc = 1 << (kPrec - 1);
  if (n >= 0 && n < N) {
    const int x0 = xb[2 * ox];
    const int cnt = min(xb[2 * ox + 1], kx);
    const size_t base = ((size_t)n * Hi + iy) * (size_t)Wi * 3 + c;
    for (int i = 0; i < cnt; ++i) {
      const int x = x0 + i;
      if (x < 0 || x >= Wi) continue;
      const int px = kF32 ? denorm_u8(static_cast<const float*>(src)[base + 3 * (size_t)x])
                          : (int)static_cast<const uint8_t*>(src)[base + 3 * (size_t)x];
      acc += px * xk[ox * kx + i];
    }
  }
  tmp[(((size_t)b * Hi + iy) * Wo) * 3 + e] = (uint8_t)clip8(acc);
}

// Vertical pass over the intermediate; writes u / 127.5 - 1 (fp32) or u (uint8).
template <bool kU8>
__global__ __launch_bounds__(kThreads) void resample_v_kernel(const uint8_t* __restrict__ tmp, int Hi, int Wo,
                                                              const int32_t* __restrict__ yb, const int32_t* __restrict__ yk,
                                                              int ky, int Ho, void* __restrict__ y) {
  const int e = blockIdx.x * kThreads + threadIdx.x;
  const int oy = blockIdx.y, b = blockIdx.z;
  const int W3 = Wo * 3;
  if (e >= W3) return;
  const int y0 = yb[2 * oy];
  const int cnt = min(yb[2 * oy + 1], ky);
  const uint8_t* col = tmp + (size_t)b * Hi * W3 + e;
  int acc = 1 << (kPrec - 1);
  for (int i = 0; i < cnt; ++i) {
    const int r = y0 + i;
    if (r < 0 || r >= Hi) continue;
    acc += (int)col[(size_t)r * W3] * yk[oy * ky + i];
  }
  const int u = clip8(acc);
  const size_t o = ((size_t)b * Ho + oy) * W3 + e;
  if (kU8) {
    static_cast<uint8_t*>(y)[o] = (uint8_t)u;
  } else {
    // fl32(fl32(u / 127.5) - 1): the fp64 quotient rounds to the correctly rounded fp32 one for every u in [0, 255]
#pragma clang fp contract(off)
    static_cast<float*>(y)[o] = (float)((double)u / 127.5) - 1.0f;
  }
}

template <int V>
struct Vec { using T = float; };
template <>
struct Vec<4> { using T = float4; };

__device__ __forceinline__ float vmax(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ float4 vmax(float4 a, float4 b) { return make_float4(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w)); }
__device__ __forceinline__ float vadd(float a, float b) { return a + b; }
__device__ __forceinline__ float4 vadd(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float vdiv(float a, float d) { return a / d; }
__device__ __forceinline__ float4 vdiv(float4 a, float d) { return make_float4(a.x / d, a.y / d, a.z / d, a.w / d); }
__device__ __forceinline__ float vfill(float v, float) { return v; }
__device__ __forceinline__ float4 vfill(float v, float4) { return make_float4(v, v, v, v); }

// One thread per (b, oy, ox, group of V channels).  Taps in row-major order; MAX ignores padded taps, AVG divides the fp32
// sum of the in-bounds taps by their count.
template <int V, bool kMax>
__global__ __launch_bounds__(kThreads) void pool_kernel(const float* __restrict__ x, int64_t total, int H, int W, int C,
                                                        int KH, int KW, int SH, int SW, int pt, int pl, int Ho, int Wo,
                                                        float* __restrict__ y, int y_ld, int y_c0) {
  using T = typename Vec<V>::T;
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= total) return;
  const int CV = C / V;
  const int cv = (int)(idx % CV);
  const int64_t pix = idx / CV;
  const int ox = (int)(pix % Wo);
  const int oy = (int)((pix / Wo) % Ho);
  const int64_t b = pix / ((int64_t)Wo * Ho);
  const int iy0 = oy * SH - pt, ix0 = ox * SW - pl;
  T acc = vfill(kMax ? -INFINITY : 0.0f, T());
  int cnt = 0;
  for (int i = 0; i < KH; ++i) {
    const int iy = iy0 + i;
    if (iy < 0 || iy >= H) continue;
    for (int j = 0; j < KW; ++j) {
      const int ix = ix0 + j;
      if (ix < 0 || ix >= W) continue;
      const T v = reinterpret_cast<const T*>(x + ((b * H + iy) * W + ix) * (int64_t)C)[cv];
      acc = kMax ? vmax(acc, v) : vadd(acc, v);
      ++cnt;
    }
  }
  if (!kMax) acc = vdiv(acc, (float)max(cnt, 1));
  *reinterpret_cast<T*>(y + pix * (int64_t)y_ld + y_c0 + cv * V) = acc;
}

template <int V>
__global__ __launch_bounds__(kThreads) void slice_copy_kernel(const float* __restrict__ x, int64_t total, int C,
                                                              float* __restrict__ y, int y_ld, int y_c0) {
  using T = typename Vec<V>::T;
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= total) return;
  const int CV = C / V;
  const int64_t r = idx / CV;
  const int cv = (int)(idx - r * CV);
  *reinterpret_cast<T*>(y + r * y_ld + y_c0 + cv * V) = reinterpret_cast<const T*>(x)[idx];
}

// ---- FID statistics ---------------------------------------------------------------------------------------------------
using f32x16 = __attribute__((ext_vector_type(16))) float;
constexpr int kGramTile = 64;            // a workgroup's square of G: 2 x 2 waves of 32 x 32
constexpr int kGramFlush = 64;           // rows summed in fp32 on the matrix pipe before each fp64 flush
constexpr int kGramUnroll = 8;           // MFMA steps (2 rows each) whose loads are issued together

// G[ti + i][tj + j] += sum_k (X[k][ti + i] - s[ti + i]) (X[k][tj + j] - s[tj + j]).  v_mfma_f32_32x32x2_f32: lane l holds
// A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]; D register r of lane l is row (r & 3) + 8 (r >> 2) + 4 (l >> 5),
// column l & 31.  Runs of kGramFlush rows are one exact-fp32 fma chain each; the runs are added in fp64 in row order.
__global__ __launch_bounds__(kThreads) void gram_kernel(const float* __restrict__ X, int n, int d, const float* __restrict__ s,
                                                        double* __restrict__ G) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ti = blockIdx.x * kGramTile + (wave & 1) * 32, tj = blockIdx.y * kGramTile + (wave >> 1) * 32;
  if (ti >= d || tj >= d) return;              // whole wave: no barrier below
  const int ci = ti + (lane & 31), cj = tj + (lane & 31), kk = lane >> 5;
  const bool oi = ci < d, oj = cj < d;
  const float si = oi ? s[ci] : 0.0f, sj = oj ? s[cj] : 0.0f;
  double acc64[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) acc64[r] = 0.0;
  for (int k0 = 0; k0 < n; k0 += kGramFlush) {
    f32x16 acc = {};
    const int k1 = min(n, k0 + kGramFlush);
    for (int k = k0; k < k1; k += 2 * kGramUnroll) {
      float a[kGramUnroll], bv[kGramUnroll];
#pragma unroll
      for (int u = 0; u < kGramUnroll; ++u) {
        const int row = k + 2 * u + kk;
        const bool ok = row < k1;
        const float* p = X + (size_t)(ok ? row : 0) * d;
        a[u] = (ok && oi) ? p[ci] - si : 0.0f;
        bv[u] = (ok && oj) ? p[cj] - sj : 0.0f;
      }
#pragma unroll
      for (int u = 0; u < kGramUnroll; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], bv[u], acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) acc64[r] += (double)acc[r];
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = ti + (r & 3) + 8 * (r >> 2) + 4 * kk;
    if (i < d && oj) G[(size_t)i * d + cj] += acc64[r];
  }
}

// sum[j] += sum_k (double)(X[k][j] - s[j]), rows in order (the MFMA operands' fp32 differences).
__global__ __launch_bounds__(kThreads) void colsum_kernel(const float* __restrict__ X, int n, int d, const float* __restrict__ s,
                                                          double* __restrict__ sum) {
  const int j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= d) return;
  const float sj = s[j];
  double acc = 0.0;
  for (int k = 0; k < n; ++k) acc += (double)(X[(size_t)k * d + j] - sj);
  sum[j] += acc;
}

// ---- IMD: per-pair cosine distance -------------------------------------------------------------------------------------
constexpr int kCosWaves = kThreads / 64;   // row pairs per workgroup

__device__ __forceinline__ void cos_acc(float u, float v, double& uv, double& uu, double& vv) {
  const double a = u, b = v;               // fp32 x fp32 is exact in fp64: fma or not, the same sum
  uv += a * b;
  uu += a * a;
  vv += b * b;
}

// out[i] = clip(1 - a_i.b_i / sqrt(|a_i|^2 |b_i|^2), 0, 2), NaN if either norm is 0 (scipy's statement).  Lane l reads the
// columns l, l + 64, ... (V == 4: the float4 columns), so a wave's loads are 64 consecutive elements (or 16-byte vectors).
template <int V>
__global__ __launch_bounds__(kThreads) void cosine_kernel(const float* __restrict__ a, int64_t lda, const float* __restrict__ b,
                                                          int64_t ldb, int64_t n, int d, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kCosWaves + (threadIdx.x >> 6);
  if (row >= n) return;                    // whole wave: no barrier below
  const float* pa = a + row * lda;
  const float* pb = b + row * ldb;
  double uv = 0.0, uu = 0.0, vv = 0.0;
  if (V == 4) {
    const float4* qa = reinterpret_cast<const float4*>(pa);
    const float4* qb = reinterpret_cast<const float4*>(pb);
    for (int k = lane; k < d / 4; k += 64) {
      const float4 x = qa[k], y = qb[k];
      cos_acc(x.x, y.x, uv, uu, vv);
      cos_acc(x.y, y.y, uv, uu, vv);
      cos_acc(x.z, y.z, uv, uu, vv);
      cos_acc(x.w, y.w, uv, uu, vv);
    }
  } else {
    for (int k = lane; k < d; k += 64) cos_acc(pa[k], pb[k], uv, uu, vv);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    uv += __shfl_xor(uv, off, 64);
    uu += __shfl_xor(uu, off, 64);
    vv += __shfl_xor(vv, off, 64);
  }
  if (lane == 0) {
    double r;
    if (uu == 0.0 || vv == 0.0) {
      r = __longlong_as_double(0x7ff8000000000000LL);
    } else {
      r = 1.0 - uv / sqrt(uu * vv);
      r = r < 0.0 ? 0.0 : (r > 2.0 ? 2.0 : r);
    }
    out[row] = r;
  }
}

// ---- bytescale + nearest resize: scipy.misc.imresize(float_image, (size, size), 'nearest') before its / 127.5 - 1 ----------
// Per image: v = fl32(fl32(x + 1) * 127.5); cmin / cmax = min / max of v over the whole image; cscale = fl32(cmax - cmin), 1 when
// that is 0; scale = fl32(255 / cscale); u8 = (uint8) trunc(clip(fl32(fl32(v - cmin) * scale), 0, 255) + 0.5) — every operation
// rounded to fp32 on its own (no fused multiply-add), as NumPy evaluates scipy's bytescale on a float32 array.  Output pixel
// (r, c) takes source pixel (floor((r + 0.5) * h / size), floor((c + 0.5) * w / size)), in exact integer arithmetic.
// Inputs are finite by contract (a generator's tanh output, clipped or not): there is no NaN policy.
// Two launches, no atomics (min and max do not depend on order, so the result is bitwise repeatable):
//   bytescale_minmax_kernel   one workgroup per (image, chunk of kBsChunk elements): partial min / max of v into the workspace;
//   bytescale_gather_kernel   one workgroup per (image, tile of output rows): folds its image's partials, then quantises only
//                             the source pixels it gathers.
constexpr int kBsChunk = kThreads * 4 * 8;          // elements of one image that one workgroup of the first pass reduces
constexpr int kBsTileBytes = kThreads * 4 * 4;      // output bytes one workgroup of the second pass writes (whole rows)

__device__ __forceinline__ float bs_value(float x) {
#pragma clang fp contract(off)
  const float s = x + 1.0f;
  return s * 127.5f;
}

__device__ __forceinline__ uint32_t bs_quant(float v, float cmin, float scale) {
#pragma clang fp contract(off)
  const float d = v - cmin;
  float b = d * scale;
  b = fminf(fmaxf(b, 0.0f), 255.0f);
  const float r = b + 0.5f;
  return (uint32_t)(int)r;
}

// min / max over the workgroup: a butterfly across each wave64, then LDS across the waves.  Every thread returns the result.
__device__ __forceinline__ void block_minmax(float& lo, float& hi, float* s_lo, float* s_hi) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, off, 64));
    hi = fmaxf(hi, __shfl_xor(hi, off, 64));
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_lo[wave] = lo;
    s_hi[wave] = hi;
  }
  __syncthreads();
  lo = s_lo[0];
  hi = s_hi[0];
#pragma unroll
  for (int k = 1; k < kThreads / 64; ++k) {
    lo = fminf(lo, s_lo[k]);
    hi = fmaxf(hi, s_hi[k]);
  }
}

// kVec: per % 4 == 0 and x 16-byte aligned, so every image and every chunk starts on a 16-byte boundary and ends on a whole float4.
template <bool kVec>
__global__ __launch_bounds__(kThreads) void bytescale_minmax_kernel(const float* __restrict__ x, int per, int chunks,
                                                                    float* __restrict__ part) {
  __shared__ float s_lo[kThreads / 64], s_hi[kThreads / 64];
  const int n = blockIdx.x / chunks, ch = blockIdx.x - n * chunks;
  const float* img = x + (size_t)n * per;
  const int beg = ch * kBsChunk;
  const int end = min(beg + kBsChunk, per);
  float lo = __builtin_inff(), hi = -__builtin_inff();
  if (kVec) {
    for (int i = beg + (int)threadIdx.x * 4; i < end; i += kThreads * 4) {
      const float4 q = *reinterpret_cast<const float4*>(img + i);
      const float a = bs_value(q.x), b = bs_value(q.y), c = bs_value(q.z), d = bs_value(q.w);
      lo = fminf(lo, fminf(fminf(a, b), fminf(c, d)));
      hi = fmaxf(hi, fmaxf(fmaxf(a, b), fmaxf(c, d)));
    }
  } else {
    for (int i = beg + (int)threadIdx.x; i < end; i += kThreads) {
      const float a = bs_value(img[i]);
      lo = fminf(lo, a);
      hi = fmaxf(hi, a);
    }
  }
  block_minmax(lo, hi, s_lo, s_hi);
  if (threadIdx.x == 0) {
    part[2 * (size_t)blockIdx.x] = lo;
    part[2 * (size_t)blockIdx.x + 1] = hi;
  }
}

// kPack: size * C % 4 == 0 and y 4-byte aligned, so every tile starts on a 4-byte boundary and holds whole 4-byte words.
template <bool kPack>
__global__ __launch_bounds__(kThreads) void bytescale_gather_kernel(const float* __restrict__ x, int h, int w, int C, int size,
                                                                    int tiles, int tile_rows, const float* __restrict__ part,
                                                                    int chunks, uint8_t* __restrict__ y) {
  __shared__ float s_lo[kThreads / 64], s_hi[kThreads / 64];
  const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
  float lo = __builtin_inff(), hi = -__builtin_inff();
  for (int k = threadIdx.x; k < chunks; k += kThreads) {
    lo = fminf(lo, part[2 * ((size_t)n * chunks + k)]);
    hi = fmaxf(hi, part[2 * ((size_t)n * chunks + k) + 1]);
  }
  block_minmax(lo, hi, s_lo, s_hi);
  const float cmin = lo;
  float cscale = hi - lo;
  if (cscale == 0.0f) cscale = 1.0f;
  const float scale = __fdiv_rn(255.0f, cscale);

  const float* img = x + (size_t)n * h * w * C;
  uint8_t* out = y + (size_t)n * size * size * C;
  const int row_bytes = size * C;
  const int beg = t * tile_rows * row_bytes;
  const int end = min(t * tile_rows + tile_rows, size) * row_bytes;
  const int64_t den = 2 * (int64_t)size;
  for (int i = beg + (int)threadIdx.x * 4; i < end; i += kThreads * 4) {
    const int cnt = min(4, end - i);
    uint32_t word = 0;
    for (int k = 0; k < cnt; ++k) {
      const int e = i + k;
      const int r = e / row_bytes, rem = e - r * row_bytes;
      const int c = rem / C, chn = rem - c * C;
      const int sr = (int)(((2 * (int64_t)r + 1) * h) / den);          // floor((r + 0.5) * h / size) < h
      const int sc = (int)(((2 * (int64_t)c + 1) * w) / den);
      const uint32_t u = bs_quant(bs_value(img[((size_t)sr * w + sc) * C + chn]), cmin, scale);
      if (kPack)
        word |= u << (8 * k);
      else
        out[e] = (uint8_t)u;
    }
    if (kPack) *reinterpret_cast<uint32_t*>(out + i) = word;
  }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline int bs_chunks(int64_t per) { return (int)((per + kBsChunk - 1) / kBsChunk); }

}  // namespace

size_t bytescale_nearest_ws(int64_t N, int64_t per) { return ((size_t)N * bs_chunks(per) * 2 * sizeof(float) + 255) & ~(size_t)255; }

// The caller (t2i_capi.hip) has checked: per = h * w * C and size * size * C fit in 2^30, N * chunks and N * tiles fit in int32.
hipError_t bytescale_nearest_launch(const float* x, int64_t N, int h, int w, int C, int size, uint8_t* y, void* ws,
                                    hipStream_t stream) {
  const int per = h * w * C;
  const int chunks = bs_chunks(per);
  float* part = static_cast<float*>(ws);
  const dim3 g1((unsigned)(N * chunks));
  if (per % 4 == 0 && al16(x))
    hipLaunchKernelGGL(bytescale_minmax_kernel<true>, g1, dim3(kThreads), 0, stream, x, per, chunks, part);
  else
    hipLaunchKernelGGL(bytescale_minmax_kernel<false>, g1, dim3(kThreads), 0, stream, x, per, chunks, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int row_bytes = size * C;
  const int tile_rows = row_bytes >= kBsTileBytes ? 1 : kBsTileBytes / row_bytes;
  const int tiles = (size + tile_rows - 1) / tile_rows;
  const dim3 g2((unsigned)(N * tiles));
  if (row_bytes % 4 == 0 && (reinterpret_cast<uintptr_t>(y) & 3) == 0)
    hipLaunchKernelGGL(bytescale_gather_kernel<true>, g2, dim3(kThreads), 0, stream, x, h, w, C, size, tiles, tile_rows, part, chunks, y);
  else
    hipLaunchKernelGGL(bytescale_gather_kernel<false>, g2, dim3(kThreads), 0, stream, x, h, w, C, size, tiles, tile_rows, part, chunks, y);
  return hipGetLastError();
}

size_t resample_bilinear_ws(int B, int Hi, int Wo) { return (((size_t)B * Hi * Wo * 3) + 255) & ~(size_t)255; }

hipError_t resample_bilinear_launch(const void* src, bool src_f32, int64_t N, int Hi, int Wi, const int32_t* rows, int B, int Ho,
                                    int Wo, const int32_t* xb, const int32_t* xk, int kx, const int32_t* yb, const int32_t* yk,
                                    int ky, void* y, bool out_u8, void* ws, hipStream_t stream) {
  uint8_t* tmp = static_cast<uint8_t*>(ws);
  const int gx = (Wo * 3 + kThreads - 1) / kThreads;
  if (src_f32)
    hipLaunchKernelGGL(resample_h_kernel<true>, dim3(gx, Hi, B), dim3(kThreads), 0, stream, src, N, Hi, Wi, rows, Wo, xb, xk, kx, tmp);
  else
    hipLaunchKernelGGL(resample_h_kernel<false>, dim3(gx, Hi, B), dim3(kThreads), 0, stream, src, N, Hi, Wi, rows, Wo, xb, xk, kx, tmp);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (out_u8)
    hipLaunchKernelGGL(resample_v_kernel<true>, dim3(gx, Ho, B), dim3(kThreads), 0, stream, tmp, Hi, Wo, yb, yk, ky, Ho, y);
  else
    hipLaunchKernelGGL(resample_v_kernel<false>, dim3(gx, Ho, B), dim3(kThreads), 0, stream, tmp, Hi, Wo, yb, yk, ky, Ho, y);
  return hipGetLastError();
}

hipError_t pool2d_launch(const float* x, int B, int H, int W, int C, int KH, int KW, int SH, int SW, int pt, int pl, int Ho,
                         int Wo, bool is_max, float* y, int y_ld, int y_c0, hipStream_t stream) {
  const bool v4 = (C % 4 == 0) && (y_ld % 4 == 0) && (y_c0 % 4 == 0) && al16(x) && al16(y);
  const int V = v4 ? 4 : 1;
  const int64_t total = (int64_t)B * Ho * Wo * (C / V);
  const dim3 grid((unsigned)((total + kThreads - 1) / kThreads));
#define T2I_POOL(VV, MX)                                                                                                    \
  hipLaunchKernelGGL((pool_kernel<VV, MX>), grid, dim3(kThreads), 0, stream, x, total, H, W, C, KH, KW, SH, SW, pt, pl, Ho, \
                     Wo, y, y_ld, y_c0)
  if (v4) {
    if (is_max) T2I_POOL(4, true); else T2I_POOL(4, false);
  } else {
    if (is_max) T2I_POOL(1, true); else T2I_POOL(1, false);
  }
#undef T2I_POOL
  return hipGetLastError();
}

hipError_t channel_slice_copy_launch(const float* x, int64_t rows, int C, float* y, int y_ld, int y_c0, hipStream_t stream) {
  const bool v4 = (C % 4 == 0) && (y_ld % 4 == 0) && (y_c0 % 4 == 0) && al16(x) && al16(y);
  const int V = v4 ? 4 : 1;
  const int64_t total = rows * (C / V);
  const dim3 grid((unsigned)((total + kThreads - 1) / kThreads));
  if (v4)
    hipLaunchKernelGGL(slice_copy_kernel<4>, grid, dim3(kThreads), 0, stream, x, total, C, y, y_ld, y_c0);
  else
    hipLaunchKernelGGL(slice_copy_kernel<1>, grid, dim3(kThreads), 0, stream, x, total, C, y, y_ld, y_c0);
  return hipGetLastError();
}

hipError_t gram_accumulate_launch(const float* X, int n, int d, const float* s, double* sum, double* G, hipStream_t stream) {
  const int t = (d + kGramTile - 1) / kGramTile;
  hipLaunchKernelGGL(gram_kernel, dim3(t, t), dim3(kThreads), 0, stream, X, n, d, s, G);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(colsum_kernel, dim3((d + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, X, n, d, s, sum);
  return hipGetLastError();
}

hipError_t cosine_distance_launch(const float* a, int64_t lda, const float* b, int64_t ldb, int64_t n, int d, double* out,
                                  hipStream_t stream) {
  const bool v4 = (d % 4 == 0) && (lda % 4 == 0) && (ldb % 4 == 0) && al16(a) && al16(b);
  const dim3 grid((unsigned)((n + kCosWaves - 1) / kCosWaves));
  if (v4)
    hipLaunchKernelGGL(cosine_kernel<4>, grid, dim3(kThreads), 0, stream, a, lda, b, ldb, n, d, out);
  else
    hipLaunchKernelGGL(cosine_kernel<1>, grid, dim3(kThreads), 0, stream, a, lda, b, ldb, n, d, out);
  return hipGetLastError();
}

}  // namespace t2i
