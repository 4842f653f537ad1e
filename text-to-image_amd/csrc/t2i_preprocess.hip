// t2i_preprocess.hip — the load-size image stores from decoded photographs (reference preprocess/utils.py transform:
// colorize, custom_crop, scipy.misc.imresize(float image, [S, S], 'bicubic')), for a ragged batch in one call.
//
// Every image of the batch has its own size, channel count and crop, so nothing here is indexed by a common [H, W]: an image
// is a descriptor (t2i_image_desc) into one packed byte buffer.  Colorize and crop are addressing: a grey image's single
// channel is read for all three output channels, the fourth channel of a 4-channel image is never read, and the crop is an
// offset into the stored rows.  Per image:
//   pp_rows_kernel     the running sum of the crops' heights: image n owns rows [row0[n], row0[n + 1]) of the intermediate, so the
//                      intermediate holds exactly the batch's rows and a tall image costs the others nothing;
//   pp_minmax_kernel   partial min / max of the crop (the channels that are read) per (image, slice of rows) — min and max do
//                      not depend on order, and there are no atomics, so the result is bitwise repeatable;
//   pp_lut_kernel      folds the partials and forms scipy's bytescale as a 256-entry table in fp64 (the float64 image only
//                      ever holds the integers 0 .. 255): lut[u] = uint8(trunc(clip((u - cmin) * (255.0 / cscale), 0, 255) + 0.5)),
//                      cscale = cmax - cmin or 1 when that is 0; also writes the crop's width and height for the next kernel;
//   pillow_tables_kernel   Pillow's precompute_coeffs + normalize_coeffs_8bpc (libImaging/Resample.c) for (crop width -> S) and
//                      (crop height -> S) in fp64, contraction off, in the operation order of evaluation/resize.py _tables —
//                      one thread per output index, the taps summed left to right.  The same kernel is t2i_pillow_tables;
//   pp_h_kernel        horizontal pass, the table applied on the load (the image's 256 bytes of table sit in LDS), into a uint8
//                      intermediate of [crop height, S, 3] per image;
//   pp_v_kernel        vertical pass into y [N, S, S, 3].  Both passes are clip8(2^21 + sum), as Pillow's.
// One thread per output byte in the two passes.  The horizontal pass has one row of workgroups per intermediate row (each finds
// its image in row0 by bisection, the same for the whole workgroup); the vertical pass one per (image, output row).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "t2i_internal.h"

namespace t2i {

namespace {

constexpr int kThreads = 256;
constexpr int kPrec = 22;                // Pillow PRECISION_BITS for 8-bit images (32 - 8 - 2)
constexpr int kSlices = 32;              // row slices of one image in the min / max pass

__device__ __forceinline__ int clip8(int v) {
  const int s = v >> kPrec;
  return s < 0 ? 0 : (s > 255 ? 255 : s);
}

// Pillow's bilinear_filter / bicubic_filter (a = -0.5), as evaluation/resize.py writes them
__device__ __forceinline__ double filter_value(int filter, double x) {
#pragma clang fp contract(off)
  x = fabs(x);
  if (filter == T2I_FILTER_BILINEAR) return x < 1.0 ? 1.0 - x : 0.0;
  const double a = -0.5;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

// taps of one axis: ceil(support) * 2 + 1 with support = filter support * max(in / out, 1)   (host and device, fp64)
__host__ __device__ inline int table_taps(int filter, int in_size, int out_size) {
  const double scale = (double)in_size / (double)out_size;
  const double filterscale = scale > 1.0 ? scale : 1.0;
  const double support = (filter == T2I_FILTER_BILINEAR ? 1.0 : 2.0) * filterscale;
  return (int)ceil(support) * 2 + 1;
}

// bounds [n, out, 2] and coeffs [n, out, kmax] of n axes; axis i resizes in_sizes[i] -> out_size.  An axis whose size is
// outside [1, T2I_PREPROCESS_MAX_SIDE] or whose tap count exceeds kmax gets empty rows (count 0, zero weights).
__global__ __launch_bounds__(kThreads) void pillow_tables_kernel(int filter, const int32_t* __restrict__ in_sizes, int64_t total,
                                                                 int out_size, int kmax, int32_t* __restrict__ bounds,
                                                                 int32_t* __restrict__ coeffs) {
#pragma clang fp contract(off)
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= total) return;
  const int64_t n = idx / out_size;
  const int xx = (int)(idx - n * out_size);
  const int in_size = in_sizes[n];
  int32_t* k = coeffs + idx * kmax;
  int xmin = 0, xmax = 0;
  if (in_size >= 1 && in_size <= T2I_PREPROCESS_MAX_SIDE && table_taps(filter, in_size, out_size) <= kmax) {
    const double scale = (double)in_size / (double)out_size;
    const double filterscale = scale > 1.0 ? scale : 1.0;
    const double support = (filter == T2I_FILTER_BILINEAR ? 1.0 : 2.0) * filterscale;
    const double ss = 1.0 / filterscale;
    const double center = ((double)xx + 0.5) * scale;
    xmin = (int)(center - support + 0.5);            // truncation toward zero, as the C cast in Pillow
    if (xmin < 0) xmin = 0;
    xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    if (xmax > kmax) xmax = kmax;                    // (cannot happen: xmax <= the tap count checked above)
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) ww += filter_value(filter, ((double)(x + xmin) - center + 0.5) * ss);
    for (int x = 0; x < xmax; ++x) {
      double w = filter_value(filter, ((double)(x + xmin) - center + 0.5) * ss);      // the same value as in the sum
      if (ww != 0.0) w = w / ww;
      k[x] = w < 0 ? (int32_t)(-0.5 + w * (double)(1 << kPrec)) : (int32_t)(0.5 + w * (double)(1 << kPrec));
    }
  }
  for (int x = xmax; x < kmax; ++x) k[x] = 0;
  bounds[2 * idx] = xmin;
  bounds[2 * idx + 1] = xmax;
}

// min / max over the workgroup: a butterfly across each wave64, then LDS across the waves.  Every thread returns the result.
__device__ __forceinline__ void block_minmax(int& lo, int& hi, int* s_lo, int* s_hi) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo = min(lo, __shfl_xor(lo, off, 64));
    hi = max(hi, __shfl_xor(hi, off, 64));
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
    lo = min(lo, s_lo[k]);
    hi = max(hi, s_hi[k]);
  }
}

// One workgroup: thread t sums the crop heights of its contiguous share of the images, the shares are scanned through LDS, and
// each thread writes its images' first rows.  row0[N] is the batch's row count.
__global__ __launch_bounds__(kThreads) void pp_rows_kernel(const t2i_image_desc* __restrict__ desc, int64_t N, int32_t* __restrict__ row0) {
  __shared__ int s_sum[kThreads];
  const int64_t per = (N + kThreads - 1) / kThreads;
  const int64_t beg = per * threadIdx.x < N ? per * threadIdx.x : N;
  const int64_t end = beg + per < N ? beg + per : N;
  int sum = 0;
  for (int64_t n = beg; n < end; ++n) sum += desc[n].y2 - desc[n].y1;
  s_sum[threadIdx.x] = sum;
  __syncthreads();
  int base = 0;
  for (int k = 0; k < (int)threadIdx.x; ++k) base += s_sum[k];
  for (int64_t n = beg; n < end; ++n) {
    row0[n] = base;
    base += desc[n].y2 - desc[n].y1;
  }
  if (threadIdx.x == kThreads - 1) row0[N] = base;
}

// Workgroup n * kSlices + slice reduces the crop rows slice, slice + kSlices, ... of image n over the channels that are read.
__global__ __launch_bounds__(kThreads) void pp_minmax_kernel(const uint8_t* __restrict__ packed, const t2i_image_desc* __restrict__ desc,
                                                             int32_t* __restrict__ part) {
  __shared__ int s_lo[kThreads / 64], s_hi[kThreads / 64];
  const int64_t n = blockIdx.x / kSlices;
  const int slice = blockIdx.x - (int)n * kSlices;
  const t2i_image_desc d = desc[n];
  const int C = d.channels, nch = C == 1 ? 1 : 3;
  const int cw = d.x2 - d.x1, ch = d.y2 - d.y1;
  const int row_elems = cw * nch;
  int lo = 255, hi = 0;
  for (int r = slice; r < ch; r += kSlices) {
    const uint8_t* row = packed + d.offset + ((size_t)(d.y1 + r) * d.width + d.x1) * C;
    for (int e = threadIdx.x; e < row_elems; e += kThreads) {
      const int px = e / nch, c = e - px * nch;
      const int v = row[(size_t)px * C + c];
      lo = min(lo, v);
      hi = max(hi, v);
    }
  }
  block_minmax(lo, hi, s_lo, s_hi);
  if (threadIdx.x == 0) {
    part[2 * (size_t)blockIdx.x] = lo;
    part[2 * (size_t)blockIdx.x + 1] = hi;
  }
}

// Workgroup n: thread u forms lut[n][u]; thread 0 also writes the crop's (width, height) as the table kernel's axis sizes.
__global__ __launch_bounds__(kThreads) void pp_lut_kernel(const t2i_image_desc* __restrict__ desc, const int32_t* __restrict__ part,
                                                          uint8_t* __restrict__ lut, int32_t* __restrict__ sizes) {
#pragma clang fp contract(off)
  const int64_t n = blockIdx.x;
  int lo = 255, hi = 0;
  for (int s = 0; s < kSlices; ++s) {                 // every thread folds the same 32 pairs: no barrier needed
    lo = min(lo, part[2 * (n * kSlices + s)]);
    hi = max(hi, part[2 * (n * kSlices + s) + 1]);
  }
  const double cmin = (double)lo;
  double cscale = (double)hi - cmin;
  if (cscale == 0.0) cscale = 1.0;
  const double scale = 255.0 / cscale;
  double b = ((double)(int)threadIdx.x - cmin) * scale;
  b = b < 0.0 ? 0.0 : (b > 255.0 ? 255.0 : b);
  lut[n * 256 + threadIdx.x] = (uint8_t)(int)(b + 0.5);
  if (threadIdx.x == 0) {
    sizes[2 * n] = desc[n].x2 - desc[n].x1;
    sizes[2 * n + 1] = desc[n].y2 - desc[n].y1;
  }
}

// tmp[row0[n] + iy, ox, c] = clip8(2^21 + sum_i lut[px(n, y1 + iy, x1 + xmin + i, c)] * xk[ox, i]); blockIdx.x is the intermediate row.
__global__ __launch_bounds__(kThreads) void pp_h_kernel(const uint8_t* __restrict__ packed, const t2i_image_desc* __restrict__ desc,
                                                        int64_t N, const int32_t* __restrict__ row0, const uint8_t* __restrict__ lut,
                                                        const int32_t* __restrict__ bounds, const int32_t* __restrict__ coeffs, int kmax,
                                                        int S, uint8_t* __restrict__ tmp) {
  __shared__ uint8_t s_lut[256];
  const int row = blockIdx.x;
  int64_t n = 0, hi = N;                              // the image with row0[n] <= row < row0[n + 1] (every crop has a row)
  while (hi - n > 1) {
    const int64_t mid = (n + hi) >> 1;
    if (row0[mid] <= row) n = mid; else hi = mid;
  }
  const t2i_image_desc d = desc[n];
  const int iy = row - row0[n];
  s_lut[threadIdx.x] = lut[n * 256 + threadIdx.x];
  __syncthreads();
  const int e = blockIdx.y * kThreads + threadIdx.x;
  if (e >= S * 3) return;
  const int ox = e / 3, c = e - 3 * ox;
  const int C = d.channels, cw = d.x2 - d.x1;
  const int32_t* xb = bounds + (2 * n) * (int64_t)S * 2;          // axis 2n: the image's columns
  const int32_t* xk = coeffs + ((2 * n) * (int64_t)S + ox) * kmax;
  const int x0 = xb[2 * ox];
  const int cnt = min(xb[2 * ox + 1], kmax);
  const uint8_t* src = packed + d.offset + ((size_t)(d.y1 + iy) * d.width + d.x1) * C + (C == 1 ? 0 : c);
  int acc = 1 << (kPrec - 1);
  for (int i = 0; i < cnt; ++i) {
    const int x = x0 + i;
    if (x < 0 || x >= cw) continue;
    acc += (int)s_lut[src[(size_t)x * C]] * xk[i];
  }
  tmp[(size_t)row * S * 3 + e] = (uint8_t)clip8(acc);
}

// y[n, oy, ox, c] = clip8(2^21 + sum_i tmp[row0[n] + ymin + i, ox, c] * yk[oy, i]); blockIdx.x is n * S + oy.
__global__ __launch_bounds__(kThreads) void pp_v_kernel(const int32_t* __restrict__ row0, const int32_t* __restrict__ bounds,
                                                        const int32_t* __restrict__ coeffs, int kmax, int S,
                                                        const uint8_t* __restrict__ tmp, uint8_t* __restrict__ y) {
  const int64_t n = blockIdx.x / S;
  const int oy = blockIdx.x - (int)n * S;
  const int e = blockIdx.y * kThreads + threadIdx.x;
  const int W3 = S * 3;
  if (e >= W3) return;
  const int ch = row0[n + 1] - row0[n];
  const int32_t* yb = bounds + (2 * n + 1) * (int64_t)S * 2;      // axis 2n + 1: the image's rows
  const int32_t* yk = coeffs + ((2 * n + 1) * (int64_t)S + oy) * kmax;
  const int y0 = yb[2 * oy];
  const int cnt = min(yb[2 * oy + 1], kmax);
  const uint8_t* col = tmp + (size_t)row0[n] * W3 + e;
  int acc = 1 << (kPrec - 1);
  for (int i = 0; i < cnt; ++i) {
    const int r = y0 + i;
    if (r < 0 || r >= ch) continue;
    acc += (int)col[(size_t)r * W3] * yk[i];
  }
  y[(size_t)blockIdx.x * W3 + e] = (uint8_t)clip8(acc);
}

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

struct Layout {
  size_t desc, row0, part, lut, sizes, bounds, coeffs, tmp, total;
  int kmax;
};

inline Layout layout(int64_t N, int64_t total_rows, int max_side, int S) {
  Layout L;
  L.kmax = table_taps(T2I_FILTER_BICUBIC, max_side, S);
  size_t o = 0;
  L.desc = o;   o += up256((size_t)N * sizeof(t2i_image_desc));
  L.row0 = o;   o += up256((size_t)(N + 1) * sizeof(int32_t));
  L.part = o;   o += up256((size_t)N * kSlices * 2 * sizeof(int32_t));
  L.lut = o;    o += up256((size_t)N * 256);
  L.sizes = o;  o += up256((size_t)N * 2 * sizeof(int32_t));
  L.bounds = o; o += up256((size_t)N * 2 * S * 2 * sizeof(int32_t));
  L.coeffs = o; o += up256((size_t)N * 2 * S * L.kmax * sizeof(int32_t));
  L.tmp = o;    o += up256((size_t)total_rows * S * 3);
  L.total = o;
  return L;
}

}  // namespace

int pillow_table_taps(int filter, int in_size, int out_size) { return table_taps(filter, in_size, out_size); }

hipError_t pillow_tables_launch(int filter, const int32_t* in_sizes, int64_t N, int out_size, int32_t* bounds, int32_t* coeffs,
                                int kmax, hipStream_t stream) {
  const int64_t total = N * out_size;
  hipLaunchKernelGGL(pillow_tables_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, filter,
                     in_sizes, total, out_size, kmax, bounds, coeffs);
  return hipGetLastError();
}

size_t preprocess_images_ws(int64_t N, int64_t total_rows, int max_side, int S) { return layout(N, total_rows, max_side, S).total; }

// The caller (t2i_capi.hip) has checked every descriptor against the packed buffer and the limits of the header: total_rows (the
// sum of the crops' heights) and N * S fit in int32; max_side is the batch's largest crop side.  desc is a HOST array.  It is
// copied into the head of the workspace on the stream, the kernels are enqueued behind the copy, and the call then waits for the
// copy alone (an event recorded right after it), so the caller may reuse the array on return while the kernels still run.
hipError_t preprocess_images_launch(const uint8_t* packed, const t2i_image_desc* desc, int64_t N, int64_t total_rows, int max_side,
                                    int S, uint8_t* y, void* ws, hipStream_t stream) {
  const Layout L = layout(N, total_rows, max_side, S);
  uint8_t* base = static_cast<uint8_t*>(ws);
  t2i_image_desc* d_desc = reinterpret_cast<t2i_image_desc*>(base + L.desc);
  int32_t* row0 = reinterpret_cast<int32_t*>(base + L.row0);
  int32_t* part = reinterpret_cast<int32_t*>(base + L.part);
  uint8_t* lut = base + L.lut;
  int32_t* sizes = reinterpret_cast<int32_t*>(base + L.sizes);
  int32_t* bounds = reinterpret_cast<int32_t*>(base + L.bounds);
  int32_t* coeffs = reinterpret_cast<int32_t*>(base + L.coeffs);
  uint8_t* tmp = base + L.tmp;
  hipEvent_t copied;
  hipError_t e = hipEventCreateWithFlags(&copied, hipEventDisableTiming);
  if (e != hipSuccess) return e;
  e = hipMemcpyAsync(d_desc, desc, (size_t)N * sizeof(t2i_image_desc), hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) e = hipEventRecord(copied, stream);
  const bool recorded = e == hipSuccess;
  const int gx = (S * 3 + kThreads - 1) / kThreads;
  if (e == hipSuccess) {
    hipLaunchKernelGGL(pp_rows_kernel, dim3(1), dim3(kThreads), 0, stream, d_desc, N, row0);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(pp_minmax_kernel, dim3((unsigned)(N * kSlices)), dim3(kThreads), 0, stream, packed, d_desc, part);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(pp_lut_kernel, dim3((unsigned)N), dim3(kThreads), 0, stream, d_desc, part, lut, sizes);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = pillow_tables_launch(T2I_FILTER_BICUBIC, sizes, 2 * N, S, bounds, coeffs, L.kmax, stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(pp_h_kernel, dim3((unsigned)total_rows, gx), dim3(kThreads), 0, stream, packed, d_desc, N, row0, lut, bounds,
                       coeffs, L.kmax, S, tmp);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(pp_v_kernel, dim3((unsigned)(N * S), gx), dim3(kThreads), 0, stream, row0, bounds, coeffs, L.kmax, S, tmp, y);
    e = hipGetLastError();
  }
  if (recorded) {
    const hipError_t w = hipEventSynchronize(copied);
    if (e == hipSuccess) e = w;
  }
  hipEventDestroy(copied);
  return e;
}

}  // namespace t2i
