// t2i_nearest.hip — closest training image of each generated image (reference utils/visualize.py closest_image /
// closest_images_of_batch): for every query q and train image n the squared L2 distance between the clipped query and
// query q's own crop / flip / [-1,1] normalisation of image n, then the lowest-index argmin per query.
//
// Two launches, both stream-ordered and free of atomics, so the result is bitwise the same whatever order the workgroups
// run in:
//   nearest_partial_kernel  one workgroup per run of R consecutive train images.  The R uint8 source images are staged in
//                           LDS once (17 328 B each at S = 76; an arbitrary col0 rules out aligned vector loads from HBM, and
//                           a flipped crop reads its row backwards), then scored against every query.  A thread loads a chunk
//                           of K query elements into registers (clipped, widened to fp64) once per query and reuses it for the
//                           R images.  Sums are fp64 per lane, reduced in a fixed order (wave butterfly, then the 4 waves in
//                           index order) and written to ws[q*N + n].
//   nearest_argmin_kernel   one workgroup per query: the minimum of ws[q, :] with the lowest index on ties.
// Images too large for the LDS budget are read straight from the store (same arithmetic, L1/L2 do the reuse).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "t2i_internal.h"

namespace t2i {

namespace {

constexpr int kThreads = 256;
constexpr int kRun = 4;                  // max train images per workgroup
constexpr int kChunk = 16;               // query elements per thread held in registers at a time
constexpr size_t kLdsBudget = 64 * 1024; // staged bytes per workgroup: 3 images at S = 76

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// fl32(fl32(u * fl32(2/255)) - 1): the value crop_flip_normalize_kernel produces (no fused multiply-add)
__device__ __forceinline__ double real_of(uint8_t u) {
  float v;
  {
#pragma clang fp contract(off)
    const float prod = (float)u * 0.00784313725490196f;
    v = prod - 1.0f;
  }
  return (double)v;
}

// One chunk of kThreads * kChunk query elements against the run's images: element i is row r = i / W3, x = i % W3 =
// 3 * column + channel of the crop.  Full chunks (kTail false) have no per-element predicate, so the byte reads of a chunk
// issue back to back; the tail chunk masks the elements past the image with a select instead of a branch.
template <bool kTail>
__device__ __forceinline__ void score_chunk(const uint8_t* imgs, const float* __restrict__ qp, int c, int per, int W3, int S3,
                                            float lo, float hi, int nr, const int* base, const bool* fl, double* acc) {
  double fd[kChunk];
  int off_n[kChunk], off_f[kChunk];
  bool ok[kChunk];
  const int i0 = c + threadIdx.x;
  int r = i0 / W3, x = i0 - r * W3;
  const int dr = kThreads / W3, dx = kThreads - dr * W3;       // i advances by kThreads per k
#pragma unroll
  for (int k = 0; k < kChunk; ++k) {
    const int i = i0 + k * kThreads;
    ok[k] = !kTail || i < per;
    const int ch = x % 3;
    fd[k] = ok[k] ? (double)fminf(fmaxf(qp[kTail ? (ok[k] ? i : 0) : i], lo), hi) : 0.0;
    off_n[k] = ok[k] ? r * S3 + x : 0;                          // column c0 + c
    off_f[k] = ok[k] ? r * S3 - x + 2 * ch : 0;                 // column c0 + out - 1 - c
    r += dr; x += dx;
    if (x >= W3) { x -= W3; ++r; }
  }
#pragma unroll
  for (int j = 0; j < kRun; ++j) {
    if (j >= nr) break;
    const uint8_t* p = imgs + base[j];
    double a = acc[j];
    if (fl[j]) {
#pragma unroll
      for (int k = 0; k < kChunk; ++k) {
        const double d = fd[k] - real_of(p[off_f[k]]);
        a = fma(kTail && !ok[k] ? 0.0 : d, d, a);
      }
    } else {
#pragma unroll
      for (int k = 0; k < kChunk; ++k) {
        const double d = fd[k] - real_of(p[off_n[k]]);
        a = fma(kTail && !ok[k] ? 0.0 : d, d, a);
      }
    }
    acc[j] = a;
  }
}

template <bool kLds>
__global__ __launch_bounds__(kThreads) void nearest_partial_kernel(const uint8_t* __restrict__ src, int N, int S,
                                                                   const int32_t* __restrict__ row0,
                                                                   const int32_t* __restrict__ col0,
                                                                   const int32_t* __restrict__ flip,
                                                                   const float* __restrict__ queries, int Q, int out,
                                                                   float lo, float hi, int R, double* __restrict__ ws) {
  extern __shared__ __align__(16) uint8_t stage[];
  __shared__ double red[kThreads / 64][kRun];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int n0 = blockIdx.x * R;
  const int nr = min(R, N - n0);
  const int img_bytes = S * S * 3;
  const uint8_t* imgs;
  if (kLds) {
    const uint8_t* g = src + (size_t)n0 * img_bytes;
    const int total = nr * img_bytes;
    if ((total & 15) == 0 && (reinterpret_cast<uintptr_t>(g) & 15) == 0) {
      const uint4* g4 = reinterpret_cast<const uint4*>(g);
      uint4* s4 = reinterpret_cast<uint4*>(stage);
      for (int i = t; i < total / 16; i += kThreads) s4[i] = g4[i];
    } else {
      for (int i = t; i < total; i += kThreads) stage[i] = g[i];
    }
    __syncthreads();
    imgs = stage;
  } else {
    imgs = src + (size_t)n0 * img_bytes;
  }
  const int per = out * out * 3, W3 = out * 3, S3 = S * 3;
  for (int q = 0; q < Q; ++q) {
    // crop origin of each image of the run for this query; a flipped crop starts at its last column
    int base[kRun];
    bool fl[kRun];
    double acc[kRun];
#pragma unroll
    for (int j = 0; j < kRun; ++j) {
      acc[j] = 0.0;
      fl[j] = false;
      base[j] = 0;
      if (j < nr) {
        int r0 = 0, c0 = 0, f = 0;
        if (row0) {
          const size_t e = (size_t)q * N + n0 + j;
          r0 = row0[e]; c0 = col0[e]; f = flip[e];
        }
        fl[j] = f != 0;
        base[j] = j * img_bytes + r0 * S3 + c0 * 3 + (fl[j] ? (out - 1) * 3 : 0);
      }
    }
    const float* qp = queries + (size_t)q * per;
    const int full = per - per % (kThreads * kChunk);
    for (int c = 0; c < full; c += kThreads * kChunk)
      score_chunk<false>(imgs, qp, c, per, W3, S3, lo, hi, nr, base, fl, acc);
    if (full < per) score_chunk<true>(imgs, qp, full, per, W3, S3, lo, hi, nr, base, fl, acc);
    // fixed-order reduction: butterfly within each wave, then the waves in index order
#pragma unroll
    for (int j = 0; j < kRun; ++j) {
      const double v = wave_sum_f64(acc[j]);
      if (lane == 0) red[wave][j] = v;
    }
    __syncthreads();
    if (t < nr) {
      double s = red[0][t];
#pragma unroll
      for (int w = 1; w < kThreads / 64; ++w) s += red[w][t];
      ws[(size_t)q * N + n0 + t] = s;
    }
    __syncthreads();                 // red is rewritten by the next query
  }
}

__global__ __launch_bounds__(kThreads) void nearest_argmin_kernel(const double* __restrict__ ws, int N,
                                                                  int32_t* __restrict__ idx, double* __restrict__ dist2) {
  __shared__ double sv[kThreads / 64];
  __shared__ int si[kThreads / 64];
  const int q = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const double* row = ws + (size_t)q * N;
  double best = __builtin_inf();
  int bi = N;                                       // sentinel: larger than every index
  for (int n = t; n < N; n += kThreads) {           // n rises per thread: strict < keeps the lowest index
    const double v = row[n];
    if (v < best) { best = v; bi = n; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov < best || (ov == best && oi < bi)) { best = ov; bi = oi; }
  }
  if (lane == 0) { sv[wave] = best; si[wave] = bi; }
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < kThreads / 64; ++w)
      if (sv[w] < best || (sv[w] == best && si[w] < bi)) { best = sv[w]; bi = si[w]; }
    if (bi == N) { bi = 0; best = row[0]; }         // every distance NaN: report image 0 with its (NaN) distance
    idx[q] = bi;
    dist2[q] = best;
  }
}

}  // namespace

size_t nearest_images_ws(int Q, int64_t N) { return (((size_t)Q * (size_t)N * sizeof(double)) + 255) & ~(size_t)255; }

hipError_t nearest_images_launch(const uint8_t* src, int N, int S, const int32_t* row0, const int32_t* col0,
                                 const int32_t* flip, const float* queries, int Q, int out, float lo, float hi,
                                 int32_t* idx, double* dist2, void* ws, hipStream_t stream) {
  const size_t img_bytes = (size_t)S * S * 3;
  double* partial = static_cast<double*>(ws);
  if (img_bytes <= kLdsBudget) {
    int R = (int)(kLdsBudget / img_bytes);
    if (R > kRun) R = kRun;
    const int blocks = (N + R - 1) / R;
    hipLaunchKernelGGL(nearest_partial_kernel<true>, dim3(blocks), dim3(kThreads), R * img_bytes, stream, src, N, S, row0,
                       col0, flip, queries, Q, out, lo, hi, R, partial);
  } else {
    const int blocks = (N + kRun - 1) / kRun;
    hipLaunchKernelGGL(nearest_partial_kernel<false>, dim3(blocks), dim3(kThreads), 0, stream, src, N, S, row0, col0, flip,
                       queries, Q, out, lo, hi, kRun, partial);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(nearest_argmin_kernel, dim3(Q), dim3(kThreads), 0, stream, partial, N, idx, dist2);
  return hipGetLastError();
}

}  // namespace t2i
