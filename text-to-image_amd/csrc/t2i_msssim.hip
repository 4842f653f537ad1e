// t2i_msssim.hip — one scale of the multi-scale structural similarity (MS-SSIM) between pairs of images (Karras et al.,
// "Progressive growing of GANs", ms_ssim.py, which is the TensorFlow-compression msssim; the reference has no such metric).
// Tensors fp32 NHWC, C in 1..4, below 2^31 elements.
//
//   ssim_scale_kernel   One workgroup owns a kSsimTy x (kSsimTileF / C) pixel tile of the VALID map (h - S + 1) x (w - S + 1) of one
//                       pair.  It stages the (kSsimTy + S - 1) x (kSsimTileF / C + S - 1) x C input tile of both images in LDS
//                       once, filters the five products a, b, a^2, b^2, ab along x into a second LDS tile and then along y — every
//                       windowed moment is accumulated in fp64 (E[a^2] - mu^2 cancels about 4e4 against c2 = 58.5: fp32 moments
//                       are off by 7e-5 in ssim on flat images) —, evaluates the cs and ssim maps in registers and leaves one fp64 pair
//                       (sum ssim, sum cs) for the workgroup: the moment maps never reach memory.  Rows are handled in the
//                       flattened (x, c) coordinate — the taps of one channel are C floats apart — and kSsimTileF = 24 is a
//                       multiple of every C, so a tile starts on a pixel whatever C is.  The window (S <= 11 doubles) arrives by
//                       value in the kernel's arguments; the tap loops are unrolled so that it is read with constant indices
//                       (scalar registers, no scratch).
//                       With a_half / b_half the same launch writes the next scale, out[i, j] = ((x[2i, 2j] + x[2i, j']) +
//                       (x[i', 2j] + x[i', j'])) * 0.25 with i' = min(2i + 1, h - 1), j' = min(2j + 1, w - 1), in fp32 and in that
//                       association (scipy.ndimage.convolve(x, ones(2, 2) / 4, 'reflect')[::2, ::2]), from the tile it holds: a
//                       tile owns the half-resolution pixels whose even corner (2i, 2j) lies in its kSsimTy x kSsimTileF / C
//                       core, the last tile of each direction also those of its S - 1 halo rows / columns, so every pixel is
//                       written by exactly one workgroup (tile origins are even).
//   ssim_fold_kernel    One wave per pair: lane t adds the pair's partials t, t + 64, ... in order, a butterfly adds the lanes, and
//                       the sums are divided by (h - S + 1)(w - S + 1) C.
// No atomics: results are bitwise identical from call to call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "t2i_internal.h"

namespace t2i {

namespace {

constexpr int kThreads = 256;
constexpr int kSsimMaxWindow = 11;                       // T2I_SSIM_MAX_WINDOW
constexpr int kSsimTy = 16;                              // rows of the valid map per tile: 36 KB of LDS at C = 3, S = 11, four workgroups per CU
constexpr int kSsimTileF = 24;                           // flattened (x, c) columns of the valid map per tile: 24, 12, 8, 6 pixels
constexpr int64_t kSsimMaxGrid = 1 << 20;                // workgroups per launch; a larger problem strides over its tiles / pairs

struct SsimWindow {
  double g[kSsimMaxWindow];
};

// sum over the workgroup: a butterfly across each wave64, then the waves in order.  Every thread returns the result.
__device__ __forceinline__ double ssim_block_sum(double v, double* s) {
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

// dynamic LDS: double s_x[5][inH][kSsimTileF], float s_a[inH][inW], float s_b[inH][inW]; inH = kSsimTy + S - 1,
// inW = kSsimTileF + (S - 1) C (ssim_lds_bytes below)
__global__ __launch_bounds__(kThreads) void ssim_scale_kernel(const float* __restrict__ a, const float* __restrict__ b, int H, int W,
                                                              int C, int S, SsimWindow win, double c1, double c2, int tiles_x,
                                                              int tiles_y, unsigned total, double* __restrict__ part,
                                                              float* __restrict__ a_half, float* __restrict__ b_half) {
  extern __shared__ double s_dyn[];
  __shared__ double s_red[kThreads / 64];
  const int inH = kSsimTy + S - 1, inW = kSsimTileF + (S - 1) * C;
  const int plane = inH * kSsimTileF;
  double* s_x = s_dyn;
  float* s_a = reinterpret_cast<float*>(s_dyn + 5 * plane);
  float* s_b = s_a + inH * inW;

  const int tpx = kSsimTileF / C;
  const int WC = W * C;
  const int Hm = H - S + 1, Fm = (W - S + 1) * C;
  for (unsigned blk = blockIdx.x; blk < total; blk += gridDim.x) {         // (the block sums below end in barriers: the LDS is free)
    const int tx = (int)(blk % (unsigned)tiles_x);
    const unsigned rest = blk / (unsigned)tiles_x;
    const int ty = (int)(rest % (unsigned)tiles_y);
    const size_t n = rest / (unsigned)tiles_y;
    const int y0 = ty * kSsimTy, x0 = tx * tpx, f0 = x0 * C;
    const size_t img = n * (size_t)H * WC;

    // the input tile of both images; indices beyond the image are clamped (their values feed masked outputs only)
    for (int e = threadIdx.x; e < inH * inW; e += kThreads) {
      const int ry = e / inW, rf = e - ry * inW;
      const size_t at = img + (size_t)min(y0 + ry, H - 1) * WC + min(f0 + rf, WC - 1);
      s_a[e] = a[at];
      s_b[e] = b[at];
    }
    __syncthreads();

    if (a_half) {                                           // the next scale, from the tile (uniform branch)
      const int Hh = (H + 1) >> 1, Wh = (W + 1) >> 1;
      const int i0 = y0 >> 1, j0 = x0 >> 1;
      const int i1 = (ty == tiles_y - 1) ? Hh : (y0 + kSsimTy) >> 1;
      const int j1 = (tx == tiles_x - 1) ? Wh : (x0 + tpx) >> 1;
      const int rowF = (j1 - j0) * C;
      for (int e = threadIdx.x; e < (i1 - i0) * rowF; e += kThreads) {
        const int di = e / rowF, rem = e - di * rowF;
        const int dj = rem / C, c = rem - dj * C;
        const int i = i0 + di, j = j0 + dj;
        const int r0 = 2 * i - y0, r1 = min(2 * i + 1, H - 1) - y0;
        const int q0 = (2 * j - x0) * C + c, q1 = (min(2 * j + 1, W - 1) - x0) * C + c;
        const size_t o = ((n * Hh + i) * (size_t)Wh + j) * C + c;
        a_half[o] = ((s_a[r0 * inW + q0] + s_a[r0 * inW + q1]) + (s_a[r1 * inW + q0] + s_a[r1 * inW + q1])) * 0.25f;
        b_half[o] = ((s_b[r0 * inW + q0] + s_b[r0 * inW + q1]) + (s_b[r1 * inW + q0] + s_b[r1 * inW + q1])) * 0.25f;
      }
    }

    // along x: the five products of every staged row, fp64
    for (int e = threadIdx.x; e < plane; e += kThreads) {
      const int ry = e / kSsimTileF, f = e - ry * kSsimTileF;
      const float* pa = s_a + ry * inW + f;
      const float* pb = s_b + ry * inW + f;
      double m1 = 0.0, m2 = 0.0, aa = 0.0, bb = 0.0, ab = 0.0;
#pragma unroll
      for (int k = 0; k < kSsimMaxWindow; ++k) {
        if (k < S) {
          const double da = (double)pa[k * C], db = (double)pb[k * C];
          const double ga = win.g[k] * da, gb = win.g[k] * db;
          m1 += ga;
          m2 += gb;
          aa = fma(ga, da, aa);
          bb = fma(gb, db, bb);
          ab = fma(ga, db, ab);
        }
      }
      s_x[e] = m1;
      s_x[plane + e] = m2;
      s_x[2 * plane + e] = aa;
      s_x[3 * plane + e] = bb;
      s_x[4 * plane + e] = ab;
    }
    __syncthreads();

    // along y, then the pixelwise map
    double sum_ssim = 0.0, sum_cs = 0.0;
    for (int e = threadIdx.x; e < kSsimTy * kSsimTileF; e += kThreads) {
      const int oy = e / kSsimTileF, f = e - oy * kSsimTileF;
      if (y0 + oy >= Hm || f0 + f >= Fm) continue;
      const double* p = s_x + e;
      double m1 = 0.0, m2 = 0.0, aa = 0.0, bb = 0.0, ab = 0.0;
#pragma unroll
      for (int k = 0; k < kSsimMaxWindow; ++k) {
        if (k < S) {
          const double g = win.g[k];
          const double* q = p + k * kSsimTileF;
          m1 = fma(g, q[0], m1);
          m2 = fma(g, q[plane], m2);
          aa = fma(g, q[2 * plane], aa);
          bb = fma(g, q[3 * plane], bb);
          ab = fma(g, q[4 * plane], ab);
        }
      }
      const double s11 = aa - m1 * m1, s22 = bb - m2 * m2, s12 = ab - m1 * m2;
      const double v1 = 2.0 * s12 + c2, v2 = s11 + s22 + c2;
      sum_cs += v1 / v2;
      sum_ssim += ((2.0 * m1 * m2 + c1) * v1) / ((m1 * m1 + m2 * m2 + c1) * v2);
    }
    const double r_ssim = ssim_block_sum(sum_ssim, s_red);
    const double r_cs = ssim_block_sum(sum_cs, s_red);
    if (threadIdx.x == 0) {
      part[2 * (size_t)blk] = r_ssim;
      part[2 * (size_t)blk + 1] = r_cs;
    }
  }
}

// ssim[n], cs[n] = (sum of pair n's `tiles` partials) / count: one wave per pair, lane t takes t, t + 64, ... in order
__global__ __launch_bounds__(64) void ssim_fold_kernel(const double* __restrict__ part, int64_t N, int tiles, double count,
                                                       double* __restrict__ ssim, double* __restrict__ cs) {
  for (int64_t n = blockIdx.x; n < N; n += gridDim.x) {
    const double* p = part + 2 * n * (size_t)tiles;
    double s = 0.0, c = 0.0;
    for (int t = threadIdx.x; t < tiles; t += 64) {
      s += p[2 * (size_t)t];
      c += p[2 * (size_t)t + 1];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      s += __shfl_xor(s, off, 64);
      c += __shfl_xor(c, off, 64);
    }
    if (threadIdx.x == 0) {
      ssim[n] = s / count;
      cs[n] = c / count;
    }
  }
}

inline int ssim_tiles_y(int H, int S) { return (H - S + 1 + kSsimTy - 1) / kSsimTy; }
inline int ssim_tiles_x(int W, int C, int S) { return (W - S + 1 + kSsimTileF / C - 1) / (kSsimTileF / C); }

inline size_t ssim_lds_bytes(int C, int S) {
  const size_t inH = kSsimTy + S - 1, inW = kSsimTileF + (S - 1) * C;
  return 5 * inH * kSsimTileF * sizeof(double) + 2 * inH * inW * sizeof(float);
}

}  // namespace

// The caller (t2i_capi.hip) has checked every extent: C in 1..4, 1 <= S <= min(11, H, W), N H W C < 2^31 (so the tile count,
// at most one tile per map element, fits 32 bits).

size_t ssim_scale_ws(int64_t N, int H, int W, int C, int S) {
  return ((size_t)N * ssim_tiles_y(H, S) * ssim_tiles_x(W, C, S) * 2 * sizeof(double) + 255) & ~(size_t)255;
}

hipError_t ssim_scale_launch(const float* a, const float* b, int64_t N, int H, int W, int C, const double* window, int S, double c1,
                             double c2, double* ssim, double* cs, float* a_half, float* b_half, void* ws, hipStream_t stream) {
  SsimWindow win;
  for (int k = 0; k < kSsimMaxWindow; ++k) win.g[k] = k < S ? window[k] : 0.0;
  const int tiles_y = ssim_tiles_y(H, S), tiles_x = ssim_tiles_x(W, C, S);
  const int tiles = tiles_y * tiles_x;
  double* part = static_cast<double*>(ws);
  const int64_t total = N * tiles;
  hipLaunchKernelGGL(ssim_scale_kernel, dim3((unsigned)min(total, kSsimMaxGrid)), dim3(kThreads), ssim_lds_bytes(C, S), stream, a, b, H, W,
                     C, S, win, c1, c2, tiles_x, tiles_y, (unsigned)total, part, a_half, b_half);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const double count = (double)(H - S + 1) * (double)(W - S + 1) * (double)C;
  hipLaunchKernelGGL(ssim_fold_kernel, dim3((unsigned)min(N, kSsimMaxGrid)), dim3(64), 0, stream, part, N, tiles, count, ssim, cs);
  return hipGetLastError();
}

}  // namespace t2i
