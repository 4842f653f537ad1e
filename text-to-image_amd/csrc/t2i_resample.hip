// t2i_resample.hip — anti-aliased resampling: upsample by zero insertion, pad or crop, FIR filter, decimate (the `upfirdn2d` of Karras
// et al. 2019 with the low-pass taps of Zhang 2019; the reference resamples by nearest x2 and the 2x2 mean only).  DESIGN.md section 4.41.
//
// Per axis, for x of extent H, taps f[0..n), factors u, d in {1, 2}, pads p0, p1 (negative pads crop) and z[j] = x[j / u] where
// 0 <= j < H u and u divides j, else 0:
//
//   Ho = floor((H u + p0 + p1 - n) / d) + 1        y[o] = sum_{t = 0}^{n - 1} w[t] z[o d + t - p0],    w[t] = g[n - 1 - t],  g = f or f reversed
//
// applied along H and along W of x [B,H,W,C] with the same taps.  The entry reverses the taps on the host (w above), so the kernel
// correlates.  The adjoint of the operator is the operator itself with (u, d, p0, flip) -> (d, u, n - 1 - p0, !flip) and the p1 that
// returns H: one kernel family serves the forward, its backward and the backward of that.
//
//   upfirdn2d_kernel<U, D, V>   A workgroup of 256 threads computes a tile of kTile x kTile outputs of one sample for a chunk of CC
//       channels.  Stage: the input pixels the tile's taps can meet — IH x IW of them, IH = ((kTile - 1) D + n - 1) / U + 1, first
//       pixel ceil((o0 D - p0) / U) — are read once from memory into LDS, channels innermost (coalesced: lanes run along the channels,
//       then along W), zeros where the window leaves the image.  Only real samples are staged: the zeros that U = 2 inserts exist
//       nowhere.  Compute: a thread owns one output pixel x V channels at a time and applies the taps directly in two dimensions from
//       LDS, rows outer, columns inner: row = sum_s w[s] x[.., s] (ascending s, fma), y = sum_t w[t] row_t (ascending t, fma).
//       Polyphase: with U = 2 an output whose window starts at an odd z reads taps 1, 3, 5, .. and one that starts at an even z taps
//       0, 2, 4, ..: ceil(n / 2) or floor(n / 2) of them per axis, each on a stored sample.
//       V = 4: 16-byte loads, LDS accesses and stores (C % 4 == 0, x and y 16-byte aligned); V = 1: the scalar form (the fade-in's C = 3,
//       a misaligned base).  The pixel stride in LDS is CC + V floats: one access width of padding, so that pixels D apart do not
//       start on the same bank for the power-of-two chunks.  Lanes are dealt to (pixel, vector) by shift and mask over the power of
//       two that covers the chunk's vectors, and a staged pixel's row comes from a multiplication by 1 / IW: no integer division by a
//       run-time value in either loop.
//       Direct 2-D taps instead of two 1-D passes through LDS: one barrier and no intermediate image; the LDS traffic this costs (at most
//       n^2 / U^2 reads of V floats per output) stays several times below what the memory system needs for the same output, see DESIGN.
// The taps travel in the kernel's argument block and are copied to LDS by the first threads (a lane's tap index depends on its
// output's parity): no device table, so the call captures into a hipGraph.  Tiles are numbered chunk-fastest, then along W, H, B, and
// a grid of at most kMaxBlocks workgroups walks them with a stride: no grid dimension is derived from B.  No atomics, every output one
// fixed-order sum of its own: calls repeat bit for bit and a sample's bits do not depend on its batch.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>

#include "t2i_internal.h"

namespace t2i {
namespace {

constexpr int kThreads = 256;
constexpr int kTile = T2I_UPFIRDN_TILE;              // outputs per tile and axis
constexpr int kMaxTaps = T2I_UPFIRDN_MAX_TAPS;
constexpr int kMaxPad = 32768;
constexpr int kMaxBlocks = 65535;                    // workgroups of one launch; the tiles beyond are reached by the stride
constexpr size_t kLdsCap = 32 << 10;                 // bytes of LDS per workgroup, at most: the chunk is halved until the window fits (measured: DESIGN 4.41)
constexpr int kChunkVec = 64, kChunkScalar = 32;     // channels per workgroup, at most

int launched(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return T2I_OK;
  set_error("%s: %s", what, hipGetErrorString(e));
  return T2I_ERR_LAUNCH;
}

struct UfdParams {
  const float* x;
  float* y;
  int B, H, W, C, Ho, Wo;
  int n, p0;
  int CC, IH, IW;                 // channels per chunk; staged input pixels per axis
  int lv_shift;                   // lanes per pixel = 1 << lv_shift, the power of two covering CC / V: a lane's vector is e & mask, its pixel e >> shift
  float inv_iw;                   // 1 / IW: a staged pixel's row is (int)((px + 0.5) * inv_iw), exact for the few hundred pixels of a window
  int chunks, tiles_x, tiles_y;
  long long total;                // chunks * tiles_x * tiles_y * B
  float w[kMaxTaps];              // w[t] multiplies z[o d + t - p0]
};

template <int V> struct Vec;
template <> struct Vec<4> {
  typedef float4 T;
  static __device__ __forceinline__ T zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
  static __device__ __forceinline__ T fma(float a, T b, T c) { return make_float4(fmaf(a, b.x, c.x), fmaf(a, b.y, c.y), fmaf(a, b.z, c.z), fmaf(a, b.w, c.w)); }
};
template <> struct Vec<1> {
  typedef float T;
  static __device__ __forceinline__ T zero() { return 0.f; }
  static __device__ __forceinline__ T fma(float a, T b, T c) { return fmaf(a, b, c); }
};

__host__ __device__ inline long long ceil_div_ll(long long a, int b) {      // b in {1, 2}
  return b == 1 ? a : ((a + 1) >> 1);                                      // (arithmetic shift: floor((a + 1) / 2) = ceil(a / 2))
}

template <int U, int D, int V>
__global__ __launch_bounds__(kThreads) void upfirdn2d_kernel(const UfdParams P) {
  typedef typename Vec<V>::T T;
  extern __shared__ float4 smem4[];                    // 16-byte aligned: [8 taps][IH * IW pixels of CC + V floats]
  float* s_w = reinterpret_cast<float*>(smem4);
  float* tile = s_w + kMaxTaps;
  const int tid = threadIdx.x;
  if (tid < kMaxTaps) s_w[tid] = tid < P.n ? P.w[tid] : 0.f;
  const int CCP = P.CC + V;
  const int n = P.n;
  for (long long id = blockIdx.x; id < P.total; id += gridDim.x) {
    const int ch = (int)(id % P.chunks);
    long long r = id / P.chunks;
    const int tx = (int)(r % P.tiles_x); r /= P.tiles_x;
    const int ty = (int)(r % P.tiles_y);
    const int b = (int)(r / P.tiles_y);
    const int c0 = ch * P.CC;
    const int nvec = (min(P.CC, P.C - c0)) / V;        // (V = 4: C and CC are multiples of 4)
    const int oy0 = ty * kTile, ox0 = tx * kTile;
    // z index of the tile's first window, the first input pixel that can meet it, and the window's offset from that pixel (0 or -1)
    const long long jy0 = (long long)oy0 * D - P.p0, jx0 = (long long)ox0 * D - P.p0;
    const long long iy0 = ceil_div_ll(jy0, U), ix0 = ceil_div_ll(jx0, U);
    const int rely = (int)(jy0 - iy0 * U), relx = (int)(jx0 - ix0 * U);
    // ---- stage the input window: IH x IW pixels x nvec vectors, zeros outside the image
    const int lv_mask = (1 << P.lv_shift) - 1;
    const int items = (P.IH * P.IW) << P.lv_shift;
    for (int e = tid; e < items; e += kThreads) {
      const int cv = e & lv_mask, px = e >> P.lv_shift;
      if (cv >= nvec) continue;
      const int ly = (int)(((float)px + 0.5f) * P.inv_iw), lx = px - ly * P.IW;
      const long long iy = iy0 + ly, ix = ix0 + lx;
      T v = Vec<V>::zero();
      if (iy >= 0 && iy < P.H && ix >= 0 && ix < P.W)
        v = *reinterpret_cast<const T*>(P.x + (((size_t)b * P.H + (size_t)iy) * P.W + (size_t)ix) * P.C + c0 + cv * V);
      *reinterpret_cast<T*>(tile + (ly * P.IW + lx) * CCP + cv * V) = v;
    }
    __syncthreads();
    // ---- one output pixel x V channels per thread and round
    const int outs = (kTile * kTile) << P.lv_shift;
    for (int e = tid; e < outs; e += kThreads) {
      const int cv = e & lv_mask, o = e >> P.lv_shift;
      const int lox = o % kTile, loy = o / kTile;
      const int oy = oy0 + loy, ox = ox0 + lox;
      if (cv >= nvec || oy >= P.Ho || ox >= P.Wo) continue;
      const int by = rely + loy * D, bx = relx + lox * D;          // window start relative to the staged origin, in z units (>= -1)
      const int ty0 = U == 2 ? (by & 1) : 0, tx0 = U == 2 ? (bx & 1) : 0;
      const float* col = tile + cv * V;
      T acc = Vec<V>::zero();
      for (int t = ty0; t < n; t += U) {
        const int ly = U == 2 ? (by + t) >> 1 : by + t;
        const float* rowp = col + ly * P.IW * CCP;
        T row = Vec<V>::zero();
        for (int s = tx0; s < n; s += U) {
          const int lx = U == 2 ? (bx + s) >> 1 : bx + s;
          row = Vec<V>::fma(s_w[s], *reinterpret_cast<const T*>(rowp + lx * CCP), row);
        }
        acc = Vec<V>::fma(s_w[t], row, acc);
      }
      *reinterpret_cast<T*>(P.y + (((size_t)b * P.Ho + oy) * P.Wo + ox) * P.C + c0 + cv * V) = acc;
    }
    __syncthreads();                                   // the next tile overwrites the window
  }
}

template <int V>
void launch_ud(int u, int d, unsigned blocks, size_t lds, hipStream_t st, const UfdParams& P) {
  if (u == 1 && d == 1) hipLaunchKernelGGL((upfirdn2d_kernel<1, 1, V>), dim3(blocks), dim3(kThreads), lds, st, P);
  else if (u == 2 && d == 1) hipLaunchKernelGGL((upfirdn2d_kernel<2, 1, V>), dim3(blocks), dim3(kThreads), lds, st, P);
  else if (u == 1 && d == 2) hipLaunchKernelGGL((upfirdn2d_kernel<1, 2, V>), dim3(blocks), dim3(kThreads), lds, st, P);
  else hipLaunchKernelGGL((upfirdn2d_kernel<2, 2, V>), dim3(blocks), dim3(kThreads), lds, st, P);
}

constexpr long long kMaxElems = 1ll << 31;

long long elements(long long a, long long b, long long c, long long d) {      // a b c d, or kMaxElems when that or more (factors in [1, 2^31))
  long long v = a * b;
  if (v >= kMaxElems) return kMaxElems;
  v *= c;
  if (v >= kMaxElems) return kMaxElems;
  v *= d;
  return v >= kMaxElems ? kMaxElems : v;
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + nb && b0 < a0 + na;
}

}  // namespace
}  // namespace t2i

using namespace t2i;

int32_t t2i_upfirdn2d_extent(int32_t H, int32_t u, int32_t d, int32_t p0, int32_t p1, int32_t n) {
  if (H < 1 || (u != 1 && u != 2) || (d != 1 && d != 2) || n < 1 || n > kMaxTaps) return 0;
  if (p0 < -kMaxPad || p0 > kMaxPad || p1 < -kMaxPad || p1 > kMaxPad) return 0;
  const long long span = (long long)H * u + p0 + p1 - n;
  if (span < 0) return 0;
  const long long Ho = span / d + 1;
  return Ho > INT_MAX ? 0 : (int32_t)Ho;
}

int t2i_upfirdn2d(const float* x, int32_t B, int32_t H, int32_t W, int32_t C, const float* taps, int32_t n, int32_t u, int32_t d,
                  int32_t p0, int32_t p1, int32_t flip, float* y, t2i_stream_t stream) {
  return t2i_upfirdn2d_axes(x, B, H, W, C, taps, n, u, d, p0, p1, p1, flip, y, stream);
}

int t2i_upfirdn2d_axes(const float* x, int32_t B, int32_t H, int32_t W, int32_t C, const float* taps, int32_t n, int32_t u, int32_t d,
                       int32_t p0, int32_t p1_h, int32_t p1_w, int32_t flip, float* y, t2i_stream_t stream) {
  const char* what = "t2i_upfirdn2d";
  if (!x || !y || !taps) { set_error("%s: bad argument (a NULL pointer)", what); return T2I_ERR_INVALID; }
  if (B < 1 || H < 1 || W < 1 || C < 1) {
    set_error("%s: bad argument (x [%d,%d,%d,%d]: every size must be at least 1)", what, (int)B, (int)H, (int)W, (int)C);
    return T2I_ERR_INVALID;
  }
  if (n < 1 || n > kMaxTaps) { set_error("%s: bad argument (n = %d taps, outside [1, %d])", what, (int)n, kMaxTaps); return T2I_ERR_INVALID; }
  if ((u != 1 && u != 2) || (d != 1 && d != 2)) {
    set_error("%s: bad argument (u = %d, d = %d: each must be 1 or 2)", what, (int)u, (int)d);
    return T2I_ERR_INVALID;
  }
  if (p0 < -kMaxPad || p0 > kMaxPad || p1_h < -kMaxPad || p1_h > kMaxPad || p1_w < -kMaxPad || p1_w > kMaxPad) {
    set_error("%s: bad argument (pads %d, %d / %d: at most %d in magnitude)", what, (int)p0, (int)p1_h, (int)p1_w, kMaxPad);
    return T2I_ERR_INVALID;
  }
  const int32_t Ho = t2i_upfirdn2d_extent(H, u, d, p0, p1_h, n), Wo = t2i_upfirdn2d_extent(W, u, d, p0, p1_w, n);
  if (Ho < 1 || Wo < 1) {
    set_error("%s: bad argument (a %dx%d map with u=%d d=%d pads %d,%d/%d and %d taps has no output)", what, (int)H, (int)W, (int)u, (int)d,
              (int)p0, (int)p1_h, (int)p1_w, (int)n);
    return T2I_ERR_INVALID;
  }
  const long long nx = elements(B, H, W, C), ny = elements(B, Ho, Wo, C);
  if (nx >= kMaxElems || ny >= kMaxElems) {
    set_error("%s: bad argument (x [%d,%d,%d,%d] or y [%d,%d,%d,%d] has 2^31 elements or more)", what, (int)B, (int)H, (int)W, (int)C, (int)B,
              (int)Ho, (int)Wo, (int)C);
    return T2I_ERR_INVALID;
  }
  if (overlap(x, (size_t)nx * 4, y, (size_t)ny * 4)) { set_error("%s: bad argument (x and y overlap)", what); return T2I_ERR_INVALID; }
  UfdParams P;
  for (int t = 0; t < kMaxTaps; ++t) P.w[t] = 0.f;
  for (int t = 0; t < n; ++t) {
    const float g = flip ? taps[n - 1 - t] : taps[t];            // g = f, or f reversed
    if (!isfinite(g)) { set_error("%s: bad argument (tap %d is not finite)", what, flip ? n - 1 - t : t); return T2I_ERR_INVALID; }
    P.w[n - 1 - t] = g;                                          // w[t] = g[n - 1 - t]
  }
  const bool vec = (C % 4 == 0) && !((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15);
  const int V = vec ? 4 : 1;
  P.x = x; P.y = y; P.B = B; P.H = H; P.W = W; P.C = C; P.Ho = Ho; P.Wo = Wo; P.n = n; P.p0 = p0;
  P.IH = P.IW = ((kTile - 1) * d + n - 1) / u + 1;
  int CC = C < (vec ? kChunkVec : kChunkScalar) ? C : (vec ? kChunkVec : kChunkScalar);
  const size_t px = (size_t)P.IH * P.IW * 4;
  while (CC > V && px * (CC + V) + kMaxTaps * 4 > kLdsCap) CC = (CC / 2 + V - 1) / V * V;
  P.CC = CC;
  P.lv_shift = 0;
  while ((V << P.lv_shift) < CC) ++P.lv_shift;
  P.inv_iw = 1.0f / (float)P.IW;
  P.chunks = (C + CC - 1) / CC;
  P.tiles_x = (Wo + kTile - 1) / kTile;
  P.tiles_y = (Ho + kTile - 1) / kTile;
  P.total = (long long)P.chunks * P.tiles_x * P.tiles_y * B;     // at most ny < 2^31: a tile holds an output element
  const size_t lds = px * (CC + V) + kMaxTaps * 4;
  const unsigned blocks = (unsigned)(P.total < kMaxBlocks ? P.total : kMaxBlocks);
  if (vec) launch_ud<4>(u, d, blocks, lds, (hipStream_t)stream, P);
  else launch_ud<1>(u, d, blocks, lds, (hipStream_t)stream, P);
  return launched(what);
}
