// t2i_swd.hip — the sliced Wasserstein distance of Laplacian-pyramid patch descriptors (Karras et al., "Progressive growing of
// GANs", sliced_wasserstein.py; the reference has no such metric).  All tensors fp32 NHWC / row-major, C in 1..4:
//
//   pyr_reduce_kernel       g_{i+1} = (5 x 5 binomial of g_i, scipy.ndimage 'mirror' edges)[::2, ::2], only the kept pixels.  A
//                           workgroup stages the raw (2 kPyrTy + 3) x (2 kPyrTx + 3) x C input tile in LDS once (about 4.5 global
//                           reads per output instead of 25), filters it horizontally into a second LDS tile, then vertically.
//   pyr_lap_kernel          lap_i = g_i - up(g_{i+1}): the zero-insert + 4 F convolution in its polyphase form per axis,
//                           out[2i] = (g[i-1] + 6 g[i] + g[i+1]) / 8, out[2i+1] = (g[i] + g[i+1]) / 2 with g[-1] := g[1] and
//                           g[h] := g[h-1]; up-sample, subtract and store in one pass, nothing of up(.) reaches memory.
//   swd_descriptor_kernel   the 7 x 7 x C neighbourhoods around given centres, flattened (c, dy, dx): a pure gather, bit-exact.
//                           Centres are clamped to [3, side - 3): no address is formed from an unchecked value.
//   swd_moment_kernel / swd_fold_kernel   per-channel mean and population standard deviation in fp64: mean first, then the
//                           centred squares; at most kStatBlocks per-workgroup partials, folded by one workgroup in a fixed order.
//   swd_project_kernel      out[s][r] = sum_j ((A[r][j] - mean_c(j)) / std_c(j)) dirs[j][s]: a tile of kProjRows rows is
//                           standardised (in fp64, one rounding to fp32) while it is loaded into LDS, transposed, so that the
//                           standardised matrix never exists in memory; every lane owns one row and kProjCols slices, whose
//                           dirs entries are wave-uniform.  fp32 fma chain over j in order.  The output is transposed (a slice is
//                           one contiguous run) and padded with +inf up to rows_pad.  Bandwidth-bound (K <= 196): plain FMA.
//   sort_lds_kernel / sort_global_kernel   ascending bitonic sort of every segment of a [segments, len] array, len a power of two.
//                           kSortChunk = 4096 floats (16 KiB of LDS, so eight workgroups stay resident per CU) are sorted, or a
//                           merge finished (all strides < kSortChunk), entirely in LDS; for each larger merge size the strides
//                           >= kSortChunk run as global compare-exchange passes, up to three strides per pass (eight 16-byte
//                           vectors per thread, the butterflies in registers).  Inputs hold no NaN by contract; +inf sorts last.
//   l1_partial_kernel / swd_fold_kernel    sum |a - b| over the first `rows` entries of every segment in fp64, fixed order, divided
//                           by segments * rows; the padding is never read.
// No atomics anywhere: results are bitwise identical from call to call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "t2i_internal.h"

namespace t2i {

namespace {

constexpr int kThreads = 256;

// ---- Laplacian pyramid --------------------------------------------------------------------------------------------------------
constexpr int kPyrTy = 8, kPyrTx = 32;                  // output tile of one workgroup of pyr_reduce_kernel
constexpr int kPyrInY = 2 * kPyrTy + 3, kPyrInX = 2 * kPyrTx + 3;
constexpr int kMaxC = 4;

// scipy.ndimage 'mirror': reflect about the centre of the edge pixel (n >= 3 here, one reflection is enough), then clamp so that
// no address leaves the image whatever the tile asks for beyond the last output.
__device__ __forceinline__ int mirror(int i, int n) {
  if (i < 0) i = -i;
  if (i >= n) i = 2 * n - 2 - i;
  return min(max(i, 0), n - 1);
}

__global__ __launch_bounds__(kThreads) void pyr_reduce_kernel(const float* __restrict__ g, int H, int W, int C,
                                                              float* __restrict__ out) {
  __shared__ float s_raw[kPyrInY * kPyrInX * kMaxC];
  __shared__ float s_h[kPyrInY * kPyrTx * kMaxC];
  const int Ho = H >> 1, Wo = W >> 1;
  const int ox0 = blockIdx.x * kPyrTx, oy0 = blockIdx.y * kPyrTy;
  const size_t n = blockIdx.z;
  const float* img = g + n * (size_t)H * W * C;
  const int rawW = kPyrInX * C, hW = kPyrTx * C;
  for (int e = threadIdx.x; e < kPyrInY * rawW; e += kThreads) {
    const int ry = e / rawW, rem = e - ry * rawW;
    const int rx = rem / C, c = rem - rx * C;
    const int y = mirror(2 * oy0 - 2 + ry, H), x = mirror(2 * ox0 - 2 + rx, W);
    s_raw[e] = img[((size_t)y * W + x) * C + c];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < kPyrInY * hW; e += kThreads) {
    const int ry = e / hW, rem = e - ry * hW;
    const int tx = rem / C, c = rem - tx * C;
    const float* p = s_raw + ry * rawW + (2 * tx) * C + c;
    s_h[e] = (p[0] + p[4 * C]) * 0.0625f + (p[C] + p[3 * C]) * 0.25f + p[2 * C] * 0.375f;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < kPyrTy * hW; e += kThreads) {
    const int ty = e / hW, rem = e - ty * hW;
    const int tx = rem / C, c = rem - tx * C;
    const int oy = oy0 + ty, ox = ox0 + tx;
    if (oy >= Ho || ox >= Wo) continue;
    const float* p = s_h + (2 * ty) * hW + rem;
    const float v = (p[0] + p[4 * hW]) * 0.0625f + (p[hW] + p[3 * hW]) * 0.25f + p[2 * hW] * 0.375f;
    out[((n * Ho + oy) * (size_t)Wo + ox) * C + c] = v;
  }
}

// one row of the coarse image, up-sampled to fine column x (polyphase along x)
__device__ __forceinline__ float up_row(const float* __restrict__ row, int x, int w, int C, int c) {
  const int i = x >> 1;
  const int ip = min(i + 1, w - 1);                       // g[w] := g[w-1]
  if (x & 1) return (row[(size_t)i * C + c] + row[(size_t)ip * C + c]) * 0.5f;
  const int im = i == 0 ? 1 : i - 1;                      // g[-1] := g[1]
  return (row[(size_t)im * C + c] + row[(size_t)ip * C + c]) * 0.125f + row[(size_t)i * C + c] * 0.75f;
}

// fine [N, 2h, 2w, C], coarse [N, h, w, C] -> lap = fine - up(coarse); one thread per element
__global__ __launch_bounds__(kThreads) void pyr_lap_kernel(const float* __restrict__ fine, const float* __restrict__ coarse,
                                                           int64_t total, int h, int w, int C, float* __restrict__ lap) {
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % C);
  const int64_t pix = idx / C;
  const int x = (int)(pix % (2 * w));
  const int y = (int)((pix / (2 * w)) % (2 * h));
  const int64_t n = pix / ((int64_t)4 * w * h);
  const float* img = coarse + n * (int64_t)h * w * C;
  const int i = y >> 1;
  const int ip = min(i + 1, h - 1);
  float up;
  if (y & 1) {
    up = (up_row(img + (size_t)i * w * C, x, w, C, c) + up_row(img + (size_t)ip * w * C, x, w, C, c)) * 0.5f;
  } else {
    const int im = i == 0 ? 1 : i - 1;
    up = (up_row(img + (size_t)im * w * C, x, w, C, c) + up_row(img + (size_t)ip * w * C, x, w, C, c)) * 0.125f +
         up_row(img + (size_t)i * w * C, x, w, C, c) * 0.75f;
  }
  lap[idx] = fine[idx] - up;
}

// ---- descriptors ---------------------------------------------------------------------------------------------------------------
// out[(row0 + n P + p) D + c 49 + dy 7 + dx] = level[n, y + dy - 3, x + dx - 3, c], (y, x) = pos[n, p], D = 49 C
__global__ __launch_bounds__(kThreads) void swd_descriptor_kernel(const float* __restrict__ level, int h, int w, int C,
                                                                  const int32_t* __restrict__ pos, int64_t total,
                                                                  int P, float* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= total) return;
  const int D = 49 * C;
  const int j = (int)(idx % D);
  const int64_t np = idx / D;                             // n P + p
  const int64_t n = np / P;
  const int c = j / 49, t = j - 49 * c;
  const int dy = t / 7, dx = t - 7 * dy;
  const int y = min(max(pos[2 * np], 3), h - 4) + dy - 3;
  const int x = min(max(pos[2 * np + 1], 3), w - 4) + dx - 3;
  out[idx] = level[((n * h + y) * (int64_t)w + x) * C + c];
}

// ---- fixed-order fp64 reductions ------------------------------------------------------------------------------------------------
constexpr int kStatBlocks = 1024;                        // most partials a reduction leaves for its fold
constexpr int kStatTile = kThreads * 16;                 // elements a workgroup takes per step

// sum over the workgroup: a butterfly across each wave64, then the waves in order.  Every thread returns the result.
__device__ __forceinline__ double block_sum(double v, double* s) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();                                        // s may still be read from the previous call
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = s[0];
#pragma unroll
  for (int k = 1; k < kThreads / 64; ++k) r += s[k];
  return r;
}

// part[block][c] = sum over the block's tiles of x (kSquare: of (x - mean_c)^2) of channel c = (column / 49) of A [rows, 49 C].
// Tiles of kStatTile consecutive elements go to the workgroups round-robin; a thread's elements keep their order.
template <bool kSquare>
__global__ __launch_bounds__(kThreads) void swd_moment_kernel(const float* __restrict__ A, int64_t total, int C,
                                                              const double* __restrict__ mean, double* __restrict__ part) {
  __shared__ double s[kThreads / 64];
  const int D = 49 * C;
  double acc[kMaxC] = {0.0, 0.0, 0.0, 0.0};
  double mu[kMaxC] = {0.0, 0.0, 0.0, 0.0};
  if (kSquare)
    for (int c = 0; c < C; ++c) mu[c] = mean[c];
  for (int64_t t0 = (int64_t)blockIdx.x * kStatTile; t0 < total; t0 += (int64_t)gridDim.x * kStatTile) {
    const int64_t t1 = min(t0 + kStatTile, total);
    for (int64_t e = t0 + threadIdx.x; e < t1; e += kThreads) {
      const int c = (int)(e % D) / 49;
      const double v = (double)A[e];
#pragma unroll
      for (int k = 0; k < kMaxC; ++k) {
        const double d = kSquare ? (v - mu[k]) * (v - mu[k]) : v;
        acc[k] += (k == c) ? d : 0.0;
      }
    }
  }
  for (int c = 0; c < C; ++c) {
    const double r = block_sum(acc[c], s);
    if (threadIdx.x == 0) part[(size_t)blockIdx.x * kMaxC + c] = r;
  }
}

// out[c] = f(sum_b part[b][c] / count) for c < C (part rows of kMaxC), f = sqrt if kSqrt: one workgroup, thread t takes
// the partials t, t + kThreads, ... in order.
template <bool kSqrt>
__global__ __launch_bounds__(kThreads) void swd_fold_kernel(const double* __restrict__ part, int nparts, int C, double count,
                                                            double* __restrict__ out) {
  __shared__ double s[kThreads / 64];
  for (int c = 0; c < C; ++c) {
    double acc = 0.0;
    for (int b = threadIdx.x; b < nparts; b += kThreads) acc += part[(size_t)b * kMaxC + c];
    const double r = block_sum(acc, s) / count;
    if (threadIdx.x == 0) out[c] = kSqrt ? sqrt(r) : r;
  }
}

// part[(seg, block)][0] = sum |a - b| over the block's share of the first `rows` entries of segment seg
__global__ __launch_bounds__(kThreads) void l1_partial_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                              int64_t len, int64_t rows, double* __restrict__ part) {
  __shared__ double s[kThreads / 64];
  const float* pa = a + (size_t)blockIdx.y * len;
  const float* pb = b + (size_t)blockIdx.y * len;
  double acc = 0.0;
  for (int64_t t0 = (int64_t)blockIdx.x * kStatTile; t0 < rows; t0 += (int64_t)gridDim.x * kStatTile) {
    const int64_t t1 = min(t0 + kStatTile, rows);
    for (int64_t e = t0 + threadIdx.x; e < t1; e += kThreads) acc += fabs((double)pa[e] - (double)pb[e]);
  }
  const double r = block_sum(acc, s);
  if (threadIdx.x == 0) part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kMaxC] = r;
}

// ---- projection ---------------------------------------------------------------------------------------------------------------
constexpr int kProjRows = 64;                            // rows of A per workgroup: one per lane
constexpr int kProjCols = 32;                            // slices per wave (accumulators per lane)
constexpr int kProjSlices = kProjCols * (kThreads / 64); // slices per workgroup
constexpr int kProjLd = kProjRows + 1;                   // LDS row stride of the transposed tile: odd, so the transposing stores spread over the banks

__global__ __launch_bounds__(kThreads) void swd_project_kernel(const float* __restrict__ A, int64_t rows, int C,
                                                               const double* __restrict__ mean, const double* __restrict__ stdv,
                                                               const float* __restrict__ dirs, int S, float* __restrict__ out,
                                                               int64_t rows_pad) {
  __shared__ float s_a[49 * kMaxC * kProjLd];
  const int D = 49 * C;
  const int lane = threadIdx.x & 63;
  const int s0 = blockIdx.y * kProjSlices + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * kProjCols;
  const int64_t r0 = (int64_t)blockIdx.x * kProjRows;
  const int64_t r = r0 + lane;
  if (r0 >= rows) {                                       // a tile of padding only (whole workgroup: no barrier below)
    if (r < rows_pad)
      for (int k = 0; k < kProjCols; ++k)
        if (s0 + k < S) out[(size_t)(s0 + k) * rows_pad + r] = __builtin_inff();
    return;
  }
  double mu[kMaxC], inv[kMaxC];
  for (int c = 0; c < kMaxC; ++c) {
    mu[c] = c < C ? mean[c] : 0.0;
    inv[c] = c < C ? 1.0 / stdv[c] : 0.0;
  }
  const int nr = (int)min((int64_t)kProjRows, rows - r0);
  const float* tile = A + (size_t)r0 * D;
  for (int e = threadIdx.x; e < kProjRows * D; e += kThreads) {
    const int rl = e / D, j = e - rl * D;
    float v = 0.0f;
    if (rl < nr) {
      const int c = j / 49;
      v = (float)(((double)tile[e] - mu[c]) * inv[c]);
    }
    s_a[j * kProjLd + rl] = v;
  }
  __syncthreads();
  float acc[kProjCols];
#pragma unroll
  for (int k = 0; k < kProjCols; ++k) acc[k] = 0.0f;
  const bool full = s0 + kProjCols <= S;
  if (full) {
    for (int j = 0; j < D; ++j) {
      const float a = s_a[j * kProjLd + lane];
      const float* d = dirs + (size_t)j * S + s0;        // wave-uniform
#pragma unroll
      for (int k = 0; k < kProjCols; ++k) acc[k] = fmaf(a, d[k], acc[k]);
    }
  } else {
    for (int j = 0; j < D; ++j) {
      const float a = s_a[j * kProjLd + lane];
      const float* d = dirs + (size_t)j * S;
#pragma unroll
      for (int k = 0; k < kProjCols; ++k) acc[k] = fmaf(a, d[min(s0 + k, S - 1)], acc[k]);
    }
  }
  if (r < rows_pad) {
    const bool pad = r >= rows;
#pragma unroll
    for (int k = 0; k < kProjCols; ++k)
      if (s0 + k < S) out[(size_t)(s0 + k) * rows_pad + r] = pad ? __builtin_inff() : acc[k];
  }
}

// ---- segmented bitonic sort ------------------------------------------------------------------------------------------------------
constexpr int kSortChunk = T2I_SORT_CHUNK;               // floats sorted or merged in LDS by one workgroup: 4096, 16 KiB

// The network: for k = 2, 4, ..., len and j = k/2, ..., 1, elements i and i ^ j (bit j of i clear) are ordered ascending where
// (i & k) == 0 and descending elsewhere, i the index inside the segment.
__device__ __forceinline__ void cmpx(float& a, float& b, bool up) {
  const bool swap = (a > b) == up;                       // no NaN by contract; a swap of equal values changes nothing
  const float t = swap ? b : a;
  b = swap ? a : b;
  a = t;
}

// All steps with j < n = min(len, kSortChunk) of the merge sizes k0 .. k1, on one chunk of n elements held in LDS.
__global__ __launch_bounds__(kThreads) void sort_lds_kernel(float* __restrict__ data, int64_t len, int n, int64_t k0, int64_t k1) {
  __shared__ float s[kSortChunk];
  const int64_t base = (int64_t)blockIdx.x * n;          // index of the chunk's first element inside its segment
  float* p = data + (size_t)blockIdx.y * len + base;
  if (n >= 4) {
    for (int e = threadIdx.x * 4; e < n; e += kThreads * 4) *reinterpret_cast<float4*>(s + e) = *reinterpret_cast<const float4*>(p + e);
  } else {
    for (int e = threadIdx.x; e < n; e += kThreads) s[e] = p[e];
  }
  __syncthreads();
  for (int64_t k = k0; k <= k1; k <<= 1) {
    for (int j = (int)min(k, (int64_t)n) >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < n / 2; t += kThreads) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));        // bit j clear
        float a = s[i], b = s[i | j];
        cmpx(a, b, ((base + i) & k) == 0);
        s[i] = a;
        s[i | j] = b;
      }
      __syncthreads();
    }
  }
  if (n >= 4) {
    for (int e = threadIdx.x * 4; e < n; e += kThreads * 4) *reinterpret_cast<float4*>(p + e) = *reinterpret_cast<const float4*>(s + e);
  } else {
    for (int e = threadIdx.x; e < n; e += kThreads) p[e] = s[e];
  }
}

__device__ __forceinline__ void cmpx4(float4& a, float4& b, bool up) {
  cmpx(a.x, b.x, up);
  cmpx(a.y, b.y, up);
  cmpx(a.z, b.z, up);
  cmpx(a.w, b.w, up);
}

// R steps of merge size k in one pass: strides j, j/2, ..., j >> (R-1), all >= kSortChunk.  A thread owns the 2^R float4 whose
// indices differ in those R bits, runs the butterflies in registers and writes them back: 2 len * 4 bytes move per pass.
template <int R>
__global__ __launch_bounds__(kThreads) void sort_global_kernel(float* __restrict__ data, int64_t len, int64_t k, int64_t j) {
  constexpr int M = 1 << R;
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;          // over len / 4 / M
  if (t >= len / 4 / M) return;
  const int64_t low = j >> (R - 1);                                        // the smallest stride, in floats
  const int64_t q = low / 4;                                               // ... in float4
  const int64_t i = (((t / q) * q) << R | (t % q)) * 4;                    // the R stride bits clear
  float* p = data + (size_t)blockIdx.y * len + i;
  const bool up = (i & k) == 0;                                            // k > j: the same for all M
  float4 v[M];
#pragma unroll
  for (int m = 0; m < M; ++m) v[m] = *reinterpret_cast<const float4*>(p + m * low);
#pragma unroll
  for (int b = M >> 1; b > 0; b >>= 1) {
#pragma unroll
    for (int m = 0; m < M; ++m)
      if ((m & b) == 0) cmpx4(v[m], v[m | b], up);
  }
#pragma unroll
  for (int m = 0; m < M; ++m) *reinterpret_cast<float4*>(p + m * low) = v[m];
}

inline int stat_blocks(int64_t total) { return (int)min((int64_t)kStatBlocks, (total + kStatTile - 1) / kStatTile); }
inline int l1_blocks(int64_t rows) { return (int)min((int64_t)64, (rows + kStatTile - 1) / kStatTile); }

}  // namespace

// The callers (t2i_capi.hip) have checked every extent: C in 1..4, tensors below 2^31 elements, grids within the limits.

// elements of level i of an [N, H, W, C] pyramid and the offset of that level in the packed output
size_t pyramid_level_elems(int64_t N, int H, int W, int C, int i) { return (size_t)N * (H >> i) * (W >> i) * C; }

size_t laplacian_pyramid_ws(int64_t N, int H, int W, int C, int levels) {
  size_t elems = 0;
  for (int i = 1; i + 1 < levels; ++i) elems += pyramid_level_elems(N, H, W, C, i);     // g_1 .. g_{L-2}; g_{L-1} is lap_{L-1}
  return (elems * sizeof(float) + 255) & ~(size_t)255;
}

hipError_t laplacian_pyramid_launch(const float* x, int64_t N, int H, int W, int C, int levels, float* out, void* ws,
                                    hipStream_t stream) {
  if (levels == 1) return hipMemcpyAsync(out, x, pyramid_level_elems(N, H, W, C, 0) * sizeof(float), hipMemcpyDeviceToDevice, stream);
  float* chain = static_cast<float*>(ws);
  size_t out_off = 0;
  for (int i = 0; i + 1 < levels; ++i) out_off += pyramid_level_elems(N, H, W, C, i);
  // the Gaussian chain, top down
  const float* g = x;
  size_t ws_off = 0;
  for (int i = 0; i + 1 < levels; ++i) {
    const int h = H >> i, w = W >> i;
    float* dst = (i + 2 == levels) ? out + out_off : chain + ws_off;
    const dim3 grid(((w >> 1) + kPyrTx - 1) / kPyrTx, ((h >> 1) + kPyrTy - 1) / kPyrTy, (unsigned)N);
    hipLaunchKernelGGL(pyr_reduce_kernel, grid, dim3(kThreads), 0, stream, g, h, w, C, dst);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (i + 2 < levels) ws_off += pyramid_level_elems(N, H, W, C, i + 1);
    g = dst;
  }
  // lap_i = g_i - up(g_{i+1})
  g = x;
  ws_off = 0;
  size_t off = 0;
  for (int i = 0; i + 1 < levels; ++i) {
    const float* coarse = (i + 2 == levels) ? out + out_off : chain + ws_off;
    const int64_t total = (int64_t)pyramid_level_elems(N, H, W, C, i);
    hipLaunchKernelGGL(pyr_lap_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, g, coarse,
                       total, H >> (i + 1), W >> (i + 1), C, out + off);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    off += (size_t)total;
    if (i + 2 < levels) ws_off += pyramid_level_elems(N, H, W, C, i + 1);
    g = coarse;
  }
  return hipSuccess;
}

hipError_t swd_descriptors_launch(const float* level, int64_t N, int h, int w, int C, const int32_t* pos, int P, float* out,
                                  int64_t row0, hipStream_t stream) {
  const int64_t total = N * P * 49 * C;
  hipLaunchKernelGGL(swd_descriptor_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, level, h,
                     w, C, pos, total, P, out + (size_t)row0 * 49 * C);
  return hipGetLastError();
}

size_t swd_channel_stats_ws(int64_t rows, int C) { return ((size_t)stat_blocks(rows * 49 * C) * kMaxC * sizeof(double) + 255) & ~(size_t)255; }

hipError_t swd_channel_stats_launch(const float* A, int64_t rows, int C, double* mean64, double* std64, void* ws, hipStream_t stream) {
  const int64_t total = rows * 49 * C;
  const int nb = stat_blocks(total);
  double* part = static_cast<double*>(ws);
  const double count = (double)(rows * 49);
  hipLaunchKernelGGL(swd_moment_kernel<false>, dim3(nb), dim3(kThreads), 0, stream, A, total, C, (const double*)nullptr, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(swd_fold_kernel<false>, dim3(1), dim3(kThreads), 0, stream, part, nb, C, count, mean64);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(swd_moment_kernel<true>, dim3(nb), dim3(kThreads), 0, stream, A, total, C, mean64, part);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(swd_fold_kernel<true>, dim3(1), dim3(kThreads), 0, stream, part, nb, C, count, std64);
  return hipGetLastError();
}

hipError_t swd_project_launch(const float* A, int64_t rows, int C, const double* mean64, const double* std64, const float* dirs,
                              int S, float* out, int64_t rows_pad, hipStream_t stream) {
  const dim3 grid((unsigned)((rows_pad + kProjRows - 1) / kProjRows), (S + kProjSlices - 1) / kProjSlices);
  hipLaunchKernelGGL(swd_project_kernel, grid, dim3(kThreads), 0, stream, A, rows, C, mean64, std64, dirs, S, out, rows_pad);
  return hipGetLastError();
}

int segmented_sort_chunk() { return kSortChunk; }

hipError_t segmented_sort_launch(float* data, int segments, int64_t len, hipStream_t stream) {
  if (len < 2) return hipSuccess;
  const int n = (int)min(len, (int64_t)kSortChunk);
  const dim3 lds_grid((unsigned)(len / n), segments);
  hipLaunchKernelGGL(sort_lds_kernel, lds_grid, dim3(kThreads), 0, stream, data, len, n, (int64_t)2, (int64_t)n);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  for (int64_t k = 2 * (int64_t)n; k <= len; k <<= 1) {
    int64_t j = k >> 1;
    while (j >= kSortChunk) {
      int R = 0;
      for (int64_t jj = j; jj >= kSortChunk && R < 3; jj >>= 1) ++R;
      const dim3 grid((unsigned)((len / 4 / (1 << R) + kThreads - 1) / kThreads), segments);
      if (R == 3) hipLaunchKernelGGL(sort_global_kernel<3>, grid, dim3(kThreads), 0, stream, data, len, k, j);
      else if (R == 2) hipLaunchKernelGGL(sort_global_kernel<2>, grid, dim3(kThreads), 0, stream, data, len, k, j);
      else hipLaunchKernelGGL(sort_global_kernel<1>, grid, dim3(kThreads), 0, stream, data, len, k, j);
      if ((e = hipGetLastError()) != hipSuccess) return e;
      j >>= R;
    }
    hipLaunchKernelGGL(sort_lds_kernel, lds_grid, dim3(kThreads), 0, stream, data, len, n, k, k);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

size_t sorted_l1_mean_ws(int segments, int64_t rows) { return ((size_t)segments * l1_blocks(rows) * kMaxC * sizeof(double) + 255) & ~(size_t)255; }

hipError_t sorted_l1_mean_launch(const float* a, const float* b, int segments, int64_t len, int64_t rows, double* out64, void* ws,
                                 hipStream_t stream) {
  const int nb = l1_blocks(rows);
  double* part = static_cast<double*>(ws);
  hipLaunchKernelGGL(l1_partial_kernel, dim3(nb, segments), dim3(kThreads), 0, stream, a, b, len, rows, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(swd_fold_kernel<false>, dim3(1), dim3(kThreads), 0, stream, part, segments * nb, 1, (double)segments * (double)rows, out64);
  return hipGetLastError();
}

}  // namespace t2i
