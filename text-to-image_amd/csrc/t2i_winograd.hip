// t2i_winograd.hip — Winograd F(2x2, 3x3) for the 3x3 stride-1 SAME convolutions with many channels on few pixels
// (critic 4x4 maps with 512-1152 channels, generator 8x8x512 / 16x16x256): 2.25x fewer multiply-adds than the direct
// implicit GEMM at the price of three HBM-bound transform passes, which only pays when channels >> pixels per image.
//   y = A^T [ (G g G^T) (.) (B^T d B) ] A        per 2x2 output tile, 4x4 input patch d (pad 1), 3x3 filter g
//   U[xi][k][n]   = (G g G^T)[xi]      filter transform, once per call          wino_filter_kernel
//   V[xi][t][k]   = (B^T d B)[xi]      input transform, t = (b, ty, tx)         wino_input_kernel
//   M[xi][t][n]   = V[xi] * U[xi]      16 independent [T x K] x [K x N] GEMMs in ONE launch of igemm_kernel (grid.z)
//   y[b,2ty+i,2tx+j,n] = (A^T M A)[i][j] + bias, activation                     wino_output_kernel
// Both conv_fwd and conv_bwd_data take this path: the input gradient of a 3x3 stride-1 SAME conv is the same
// correlation with the filter flipped and its channel axes swapped; it reads the forward filter image (wino_slot).
// fp32 throughout (the GEMM follows the descriptor's math mode); transforms use only +, - and *0.5.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>

#include <mutex>
#include <vector>

#include "t2i_internal.h"

namespace t2i {

// ------------------------------------------------------------------------------------------------------------------
// Transformed-filter cache (opt-in, t2i_filter_cache_attach + t2i_filter_cache_enable): U = G g G^T of a filter is the same
// for every conv that uses it until the filter changes — the critic's filters are used by up to six convs per step.  Entries
// are keyed by (filter pointer, transform kind, dims); their storage is carved out of a CALLER-OWNED arena.  An entry is reusable only from the launch context that
// filled it: eager launches reuse eager fills, launches captured into a graph reuse fills of the SAME capture (so every
// graph contains all the transforms it depends on).  t2i_adam_tf drops the entries inside the arena it updates; any other
// writer of filter memory must call t2i_filter_cache_invalidate (see include/t2i_hip.h).
// ------------------------------------------------------------------------------------------------------------------
struct FilterEntry {
  const float* w; int kind, Cin, Cout; float* U; size_t bytes; unsigned long long cap; hipStream_t stream; bool valid;
  hipStream_t cap_fill = nullptr;      // the stream that filled it lazily inside capture `cap`; nullptr = the batched refresh did
};
static std::mutex g_fc_mu;
static std::vector<FilterEntry> g_fc;
static int g_fc_on = 0;
static char* g_fc_buf = nullptr;      // caller-owned arena (t2i_filter_cache_attach); entries are carved from it in order
static size_t g_fc_cap = 0, g_fc_used = 0;

int filter_cache_attach(void* buf, size_t bytes) {
  std::lock_guard<std::mutex> lk(g_fc_mu);
  g_fc.clear();                       // entries of the previous arena point into memory the caller may now free
  g_fc_buf = reinterpret_cast<char*>(buf);
  g_fc_cap = bytes;
  g_fc_used = 0;
  return T2I_OK;
}

int filter_cache_enable(int on) {
  std::lock_guard<std::mutex> lk(g_fc_mu);
  const int prev = g_fc_on;
  g_fc_on = on ? 1 : 0;
  for (auto& e : g_fc) e.valid = false;
  return prev;
}

void filter_cache_invalidate(const void* p, size_t bytes) {
  std::lock_guard<std::mutex> lk(g_fc_mu);
  const char* lo = reinterpret_cast<const char*>(p);
  for (auto& e : g_fc) {
    const char* q = reinterpret_cast<const char*>(e.w);
    if (!p || (q >= lo && q < lo + bytes)) e.valid = false;
  }
}

size_t filter_cache_bytes() {
  std::lock_guard<std::mutex> lk(g_fc_mu);
  return g_fc_used;
}

// Returns the cache slot for this filter's transform (and whether it has to be filled), or nullptr when the caller
// should transform into its workspace as without the cache (cache off, no arena attached or arena full, a second stream).
// The library allocates nothing: slots are carved out of the caller's arena, never moved, and live until the next attach.
float* filter_cache_get(const float* w, int kind, int Cin, int Cout, size_t bytes, hipStream_t stream, bool* fill) {
  *fill = true;
  if (!g_fc_on) return nullptr;
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  unsigned long long id = 0;
  if (hipStreamGetCaptureInfo(stream, &st, &id) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  const unsigned long long cap = st == hipStreamCaptureStatusActive ? id + 1 : 0;
  std::lock_guard<std::mutex> lk(g_fc_mu);
  if (!g_fc_buf) return nullptr;
  FilterEntry* e = nullptr;
  for (auto& x : g_fc)
    if (x.w == w && x.kind == kind && x.Cin == Cin && x.Cout == Cout) { e = &x; break; }
  if (!e) {
    const size_t need = (bytes + 255) & ~(size_t)255;
    if (g_fc_used + need > g_fc_cap) return nullptr;          // arena full: this filter is transformed per call
    float* U = reinterpret_cast<float*>(g_fc_buf + g_fc_used);
    g_fc_used += need;
    g_fc.push_back(FilterEntry{w, kind, Cin, Cout, U, bytes, 0ull, stream, false, nullptr});
    e = &g_fc.back();
  }
  if (e->bytes < bytes) return nullptr;
  if (!cap && e->stream != stream) return nullptr;     // eager use from a second stream: no ordering with the fills / readers
  if (e->valid && e->cap == cap) {
    // inside a capture an image may be read from any stream IF it was filled by the batched refresh at the head of the graph
    // (cap_fill == nullptr: issued before the streams forked); an image filled lazily by one captured stream has no edge to the
    // other streams of the capture, so those transform into their own workspace instead (round-2 review: the one-graph
    // iteration reads the generator's images from the main and from the ahead stream)
    if (cap && e->cap_fill != nullptr && e->cap_fill != stream) return nullptr;
    *fill = false;
    return e->U;
  }
  e->valid = true; e->cap = cap; e->cap_fill = stream;
  return e->U;
}

static inline size_t al256(size_t n) { return (n + 255) & ~(size_t)255; }

static inline int wino_blocks(size_t n) {
  size_t b = (n + 255) / 256;
  if (b > 8192) b = 8192;
  return b < 1 ? 1 : (int)b;
}

// Store of one float4 of a transformed operand (V, Z: written once, streamed once by the batched GEMM).  -DT2I_NT_PLANES: nontemporal
// (experiment, profiles/r04_winograd_transform_bw.txt).
__device__ __forceinline__ void wst(float4* p, float4 v) {
#if defined(T2I_NT_PLANES)
  typedef float f4v __attribute__((ext_vector_type(4)));
  __builtin_nontemporal_store(__builtin_bit_cast(f4v, v), reinterpret_cast<f4v*>(p));
#else
  *p = v;
#endif
}

__device__ __forceinline__ float4 f4sub(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ __forceinline__ float4 f4add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// U[xi][ci][co] = (G g G^T)[xi] with g[r][c] = w[r][c][ci][co].  The input gradient needs the same transform of the flipped
// filter, which is this image with plane rows / columns 0 and 3 exchanged (wino_slot below), and the channel swap of the
// input-gradient conv is left to the GEMM, which reads U as [n = ci][k = co] — its K-inner B image: ONE image per filter.
// Reads and writes are both contiguous along co.
__device__ __forceinline__ void wino_filter_body(const float* __restrict__ w, int Cin, int Cout, float* __restrict__ U,
                                                 unsigned vb, unsigned nvb) {
  const int K = Cin, N = Cout;
  const size_t total = (size_t)K * N;
  for (size_t i = (size_t)vb * 256 + threadIdx.x; i < total; i += (size_t)nvb * 256) {
    const int n = (int)(i % N), k = (int)(i / N);
    const int ci = k, co = n;
    float g[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) g[r][c] = w[((size_t)(r * 3 + c) * Cin + ci) * Cout + co];
    float s[4][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      s[0][c] = g[0][c];
      s[1][c] = 0.5f * (g[0][c] + g[1][c] + g[2][c]);
      s[2][c] = 0.5f * (g[0][c] - g[1][c] + g[2][c]);
      s[3][c] = g[2][c];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float u0 = s[r][0], u1 = 0.5f * (s[r][0] + s[r][1] + s[r][2]), u2 = 0.5f * (s[r][0] - s[r][1] + s[r][2]), u3 = s[r][2];
      U[((size_t)(r * 4 + 0) * K + k) * N + n] = u0;
      U[((size_t)(r * 4 + 1) * K + k) * N + n] = u1;
      U[((size_t)(r * 4 + 2) * K + k) * N + n] = u2;
      U[((size_t)(r * 4 + 3) * K + k) * N + n] = u3;
    }
  }
}

__global__ __launch_bounds__(256) void wino_filter_kernel(const float* __restrict__ w, int Cin, int Cout, float* __restrict__ U) {
  wino_filter_body(w, Cin, Cout, U, blockIdx.x, gridDim.x);
}

// Plane slot of tile position (r, c).  The input gradient of a 3x3 stride-1 conv is the same correlation with the filter flipped,
// and G flip(g) G^T is U with rows / columns 0 and 3 exchanged (rows 1 and 2 of G are symmetric in g): instead of keeping a
// second filter image, the input-gradient call stores V[xi] (and finds M[xi]) in the slot of the forward position whose U it
// needs — the batched GEMM then runs over the FORWARD image with uniform strides.
__device__ __forceinline__ int wino_slot(int r, int c, int flip) {
  const int rr = (flip && (r == 0 || r == 3)) ? 3 - r : r, cc = (flip && (c == 0 || c == 3)) ? 3 - c : c;
  return rr * 4 + cc;
}

// V[xi][t][c]: one thread = one tile x 4 channels
// plane_T: tiles per plane of V (>= T; > T when this call fills only a range of a larger batch's planes: x and V then point at that range)
__global__ __launch_bounds__(256) void wino_input_kernel(const float* __restrict__ x, int H, int W, int C, int Th, int Tw,
                                                         size_t T, float* __restrict__ V, int flip, size_t plane_T) {
  const int C4 = C >> 2;
  const size_t total = T * C4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % C4);
    const size_t t = i / C4;
    const int tx = (int)(t % Tw);
    const int ty = (int)((t / Tw) % Th);
    const size_t b = t / ((size_t)Tw * Th);
    float4 d[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ih = 2 * ty - 1 + r;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int iw = 2 * tx - 1 + c;
        d[r][c] = ((unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W)
                      ? reinterpret_cast<const float4*>(x + ((b * H + ih) * W + iw) * C)[c4]
                      : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    float4 tt[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      tt[0][c] = f4sub(d[0][c], d[2][c]);
      tt[1][c] = f4add(d[1][c], d[2][c]);
      tt[2][c] = f4sub(d[2][c], d[1][c]);
      tt[3][c] = f4sub(d[1][c], d[3][c]);
    }
    float4* o = reinterpret_cast<float4*>(V) + t * C4 + c4;
    const size_t plane = plane_T * C4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      wst(&o[(size_t)wino_slot(r, 0, flip) * plane], f4sub(tt[r][0], tt[r][2]));
      wst(&o[(size_t)wino_slot(r, 1, flip) * plane], f4add(tt[r][1], tt[r][2]));
      wst(&o[(size_t)wino_slot(r, 2, flip) * plane], f4sub(tt[r][2], tt[r][1]));
      wst(&o[(size_t)wino_slot(r, 3, flip) * plane], f4sub(tt[r][1], tt[r][3]));
    }
  }
}

// y[b, 2ty+i, 2tx+j, n] = act((A^T M A)[i][j] + bias[n]): one thread = one tile x 4 output channels
__global__ __launch_bounds__(256) void wino_output_kernel(const float* __restrict__ Mx, const float* __restrict__ bias, int H,
                                                          int W, int N, int Th, int Tw, size_t T, int act, float alpha,
                                                          float* __restrict__ y, int flip) {
  const int N4 = N >> 2;
  const size_t total = T * N4;
  const size_t plane = T * N4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int n4 = (int)(i % N4);
    const size_t t = i / N4;
    const int tx = (int)(t % Tw);
    const int ty = (int)((t / Tw) % Th);
    const size_t b = t / ((size_t)Tw * Th);
    const float4* m = reinterpret_cast<const float4*>(Mx) + t * N4 + n4;
    float4 z[2][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float4 m0 = m[(size_t)wino_slot(0, c, flip) * plane], m1 = m[(size_t)wino_slot(1, c, flip) * plane],
                   m2 = m[(size_t)wino_slot(2, c, flip) * plane], m3 = m[(size_t)wino_slot(3, c, flip) * plane];
      z[0][c] = f4add(f4add(m0, m1), m2);
      z[1][c] = f4sub(f4sub(m1, m2), m3);
    }
    const float4 bs = bias ? reinterpret_cast<const float4*>(bias)[n4] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      float4 y0 = f4add(f4add(f4add(z[r][0], z[r][1]), z[r][2]), bs);
      float4 y1 = f4add(f4sub(f4sub(z[r][1], z[r][2]), z[r][3]), bs);
      y0.x = apply_act(y0.x, act, alpha); y0.y = apply_act(y0.y, act, alpha); y0.z = apply_act(y0.z, act, alpha); y0.w = apply_act(y0.w, act, alpha);
      y1.x = apply_act(y1.x, act, alpha); y1.y = apply_act(y1.y, act, alpha); y1.z = apply_act(y1.z, act, alpha); y1.w = apply_act(y1.w, act, alpha);
      float4* o = reinterpret_cast<float4*>(y + ((b * H + 2 * ty + r) * W + 2 * tx) * N) + n4;
      o[0] = y0;
      o[N4] = y1;
    }
  }
}

static int wino_min_channels() { return tuning().winograd_minc; }

bool winograd_eligible(const t2i_conv_desc& d, bool bwd_data) {
  if (!tuning().winograd || d.math != T2I_MATH_F32) return false;     // bf16 math: the direct kernel is operand-stream bound, 16 GEMMs would stream 4x more
  if (!(d.KH == 3 && d.KW == 3 && d.SH == 1 && d.SW == 1 && d.pad_t == 1 && d.pad_l == 1 && d.Ho == d.H && d.Wo == d.W)) return false;
  if ((d.H & 1) || (d.W & 1) || (d.Cin % 32) || (d.Cout % 32)) return false;
  // pays when the GEMM work dominates the three transform passes: many channels on small maps
  const int cmin = d.Cin < d.Cout ? d.Cin : d.Cout;
  const int maxhw = tuning().winograd_maxhw;
  if (cmin < wino_min_channels() || (int64_t)d.H * d.W > maxhw) return false;
  // ... and the 16 GEMMs are big enough to fill the chip (winograd_minwork, 5e7).  Measured at B=64 with the filter images cached
  // and the persistent batched GEMM: 4x4x256->512, T*K*N = 3.4e7, would gain 15 % (5 us) in all three primitives — but it is the
  // critic layer the x_hat pass runs at B=64, and with it on the Winograd path D(x_hat) of the full-width step moves from 7e-6 to
  // 1.1e-5 of the float64 oracle, past SURVEY 8(c)'s 1e-5: parity first, the threshold stays.  4x4x256->256 and 8x8x128->128
  // (1.7e7) gain 5 % / lose 18 % forward and lose in the filter gradient.
  // Round 6: the stacked critic pass runs that layer on 4B = 256 images (T*K*N = 1.3e8), so it IS on the Winograd form there.  Re-measured
  // with the error split per network (tests/test_step_b64_gpu.py::_critic_alone, B = 64): D(x_hat) of the critic alone 4.7e-6 with it on
  // Winograd / 3.8e-6 with a per-image threshold keeping it direct (paired form 5.1e-6 / 5.7e-6), the chain G -> x_hat -> D 8.7e-6 / 9.0e-6
  // — the 7e-6 -> 1.1e-5 of round 4 was G's error pushed through the critic landing on either side of 1e-5 by the summation order, not this
  // layer's form.  The per-image threshold cost 0.85 % of the iteration and bought no parity margin: not kept.
  const int64_t T = (int64_t)d.B * (d.H / 2) * (d.W / 2);
  return T * d.Cin * d.Cout >= (int64_t)tuning().winograd_minwork;
}

// The filter gradient's 16 GEMMs are [Cin, T] x [T, Cout]: their tile count does not grow with the batch, and 128 x 128
// channels (64 tiles of 64x64 in all) leave the chip three quarters empty (8x8x128->128 at B=192: 85 us against 43 us for the
// direct GEMM).  From 128 x 512 on (256 tiles) the Winograd form wins again (8x8x128->512: 52.6 -> 47.2 us at B=64).
bool winograd_filter_eligible(const t2i_conv_desc& d) {
  return winograd_eligible(d, false) && (int64_t)d.Cin * d.Cout >= 65536;
}

static void wino_dims(const t2i_conv_desc& d, bool bwd, size_t* T, int* K, int* N) {
  *T = (size_t)d.B * (d.H / 2) * (d.W / 2);
  *K = bwd ? d.Cout : d.Cin;
  *N = bwd ? d.Cin : d.Cout;
}

size_t winograd_ws(const t2i_conv_desc& d, bool bwd) {
  size_t T; int K, N;
  wino_dims(d, bwd, &T, &K, &N);
  return al256((size_t)16 * K * N * 4) + al256(16 * T * K * 4) + al256(16 * T * N * 4);
}

int winograd_conv(const t2i_conv_desc& d, bool bwd, const float* in, const float* w, const float* bias, float* out, int act,
                  float alpha, void* ws, size_t ws_bytes, hipStream_t stream, float* Vkeep) {
  size_t T; int K, N;
  wino_dims(d, bwd, &T, &K, &N);
  if (!ws || ws_bytes < winograd_ws(d, bwd) || (reinterpret_cast<uintptr_t>(ws) & 15)) {
    set_error("winograd conv: workspace %zu B < %zu B required (or misaligned)", ws_bytes, winograd_ws(d, bwd));
    return T2I_ERR_WORKSPACE;
  }
  char* base = reinterpret_cast<char*>(ws);
  float* U = reinterpret_cast<float*>(base);
  float* V = Vkeep ? Vkeep : reinterpret_cast<float*>(base + al256((size_t)16 * K * N * 4));      // Vkeep: the caller keeps the input transform
  float* Mx = reinterpret_cast<float*>(base + al256((size_t)16 * K * N * 4) + al256(16 * T * K * 4));
  const int Th = d.H / 2, Tw = d.W / 2;
  bool fill = true;
  // ONE image per filter (kind 0) serves both directions: the input gradient permutes its V / M plane slots instead (wino_slot)
  if (float* Uc = filter_cache_get(w, 0, d.Cin, d.Cout, (size_t)16 * K * N * 4, stream, &fill)) U = Uc;
  if (fill)
    hipLaunchKernelGGL(wino_filter_kernel, dim3(wino_blocks((size_t)K * N)), dim3(256), 0, stream, w, d.Cin, d.Cout, U);
  hipLaunchKernelGGL(wino_input_kernel, dim3(wino_blocks(T * (K / 4))), dim3(256), 0, stream, in, d.H, d.W, K, Th, Tw, T, V, bwd ? 1 : 0, T);
  t2i_conv_desc gd = d;                // the 16 GEMMs as a batch of 1x1 convolutions over T "pixels" (fwd) / their input gradient (bwd)
  gd.B = (int32_t)T; gd.H = gd.W = gd.Ho = gd.Wo = 1; gd.KH = gd.KW = gd.SH = gd.SW = 1; gd.pad_t = gd.pad_l = 0;   // Cin, Cout as in d
  const int rc = run_batched_gemm(gd, bwd ? MODE_BWD_DATA : MODE_FWD, 16, V, U, Mx, (int64_t)T * K, (int64_t)d.Cin * d.Cout, (int64_t)T * N, stream, "winograd gemm");
  if (rc != T2I_OK) return rc;
  hipLaunchKernelGGL(wino_output_kernel, dim3(wino_blocks(T * (N / 4))), dim3(256), 0, stream, Mx, bias, d.H, d.W, N, Th, Tw, T, act, alpha, out,
                     bwd ? 1 : 0);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error("winograd conv: %s", hipGetErrorString(e)); return T2I_ERR_LAUNCH; }
  return T2I_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Filter gradient:  dw = G^T [ (B^T d B) (.) (A dy A^T) ] G  summed over tiles — the adjoint of the forward identity.
//   V[xi][t][ci] = B^T d B        (the forward's input transform)
//   Z[xi][t][co] = A dy A^T       wino_dy_kernel (2x2 output-gradient tile -> 4x4)
//   P[xi][ci][co] = sum_t V[xi][t][ci] Z[xi][t][co]     16 batched filter-gradient GEMMs (reduction over tiles)
//   dw[r][c][ci][co] (+)= (G^T P G)[r][c]               wino_dw_kernel
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void wino_dy_kernel(const float* __restrict__ dy, int H, int W, int N, int Th, int Tw, size_t T,
                                                      float* __restrict__ Z) {
  const int N4 = N >> 2;
  const size_t total = T * N4, plane = T * N4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int n4 = (int)(i % N4);
    const size_t t = i / N4;
    const int tx = (int)(t % Tw);
    const int ty = (int)((t / Tw) % Th);
    const size_t b = t / ((size_t)Tw * Th);
    const float4* src = reinterpret_cast<const float4*>(dy + ((b * H + 2 * ty) * W + 2 * tx) * N) + n4;
    const float4 d00 = src[0], d01 = src[N4], d10 = src[(size_t)W * N4], d11 = src[(size_t)W * N4 + N4];
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    // s[r][j] = sum_i A[r][i] d[i][j],  A = [1 0; 1 1; 1 -1; 0 -1]
    const float4 s[4][2] = {{d00, d01}, {f4add(d00, d10), f4add(d01, d11)}, {f4sub(d00, d10), f4sub(d01, d11)}, {f4sub(zero, d10), f4sub(zero, d11)}};
    float4* o = reinterpret_cast<float4*>(Z) + t * N4 + n4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      wst(&o[(size_t)(r * 4 + 0) * plane], s[r][0]);
      wst(&o[(size_t)(r * 4 + 1) * plane], f4add(s[r][0], s[r][1]));
      wst(&o[(size_t)(r * 4 + 2) * plane], f4sub(s[r][0], s[r][1]));
      wst(&o[(size_t)(r * 4 + 3) * plane], f4sub(zero, s[r][1]));
    }
  }
}

__device__ __forceinline__ float4 f4half(float4 a) { return make_float4(0.5f * a.x, 0.5f * a.y, 0.5f * a.z, 0.5f * a.w); }

__global__ __launch_bounds__(256) void wino_dw_kernel(const float* __restrict__ P, int Cin, int Cout, int accumulate,
                                                      float* __restrict__ dw) {
  const int N4 = Cout >> 2;
  const size_t total = (size_t)Cin * N4, plane = total;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const float4* p = reinterpret_cast<const float4*>(P) + i;
    float4 q[3][4];     // q[r][c'] = sum_rho GT[r][rho] P[rho][c'],  GT = [1 .5 .5 0; 0 .5 -.5 0; 0 .5 .5 1]
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float4 p0 = p[(size_t)(0 * 4 + c) * plane], p1 = p[(size_t)(1 * 4 + c) * plane], p2 = p[(size_t)(2 * 4 + c) * plane],
                   p3 = p[(size_t)(3 * 4 + c) * plane];
      const float4 hs = f4half(f4add(p1, p2)), hd = f4half(f4sub(p1, p2));
      q[0][c] = f4add(p0, hs);
      q[1][c] = hd;
      q[2][c] = f4add(hs, p3);
    }
    float4* o = reinterpret_cast<float4*>(dw) + i;        // dw [3][3][Cin][Cout]: tap plane stride = Cin*Cout/4
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const float4 hs = f4half(f4add(q[r][1], q[r][2])), hd = f4half(f4sub(q[r][1], q[r][2]));
      float4 w0 = f4add(q[r][0], hs), w1 = hd, w2 = f4add(hs, q[r][3]);
      if (accumulate) {
        w0 = f4add(w0, o[(size_t)(r * 3 + 0) * plane]); w1 = f4add(w1, o[(size_t)(r * 3 + 1) * plane]); w2 = f4add(w2, o[(size_t)(r * 3 + 2) * plane]);
      }
      wst(&o[(size_t)(r * 3 + 0) * plane], w0);
      wst(&o[(size_t)(r * 3 + 1) * plane], w1);
      wst(&o[(size_t)(r * 3 + 2) * plane], w2);
    }
  }
}

size_t winograd_filter_grad_ws(const t2i_conv_desc& d) {
  const size_t T = (size_t)d.B * (d.H / 2) * (d.W / 2);
  return al256(16 * T * d.Cin * 4) + al256(16 * T * d.Cout * 4) + al256((size_t)16 * d.Cin * d.Cout * 4);
}

// Vhave / valid_rows: the caller's kept input transform of x (planes of T tiles) and how many leading images of the batch it is current
// for (>= d.B: all): the tiles of the images behind are regenerated from x here, into the caller's planes
// plane_rows > d.B: Vhave's planes hold the tiles of plane_rows images (the transform of a larger, stacked batch whose LEADING d.B
// images are this call's x): the batched GEMM strides from plane to plane by that many tiles
int winograd_filter_grad(const t2i_conv_desc& d, const float* x, const float* dy, float* dw, int accumulate, void* ws, size_t ws_bytes,
                         hipStream_t stream, const float* Vhave, int valid_rows, int plane_rows) {
  const size_t T = (size_t)d.B * (d.H / 2) * (d.W / 2);
  const size_t Tp = (Vhave && plane_rows > d.B) ? (size_t)plane_rows * (d.H / 2) * (d.W / 2) : T;
  if (!ws || ws_bytes < winograd_filter_grad_ws(d) || (reinterpret_cast<uintptr_t>(ws) & 15)) {
    set_error("winograd filter gradient: workspace %zu B < %zu B required (or misaligned)", ws_bytes, winograd_filter_grad_ws(d));
    return T2I_ERR_WORKSPACE;
  }
  char* base = reinterpret_cast<char*>(ws);
  float* V = reinterpret_cast<float*>(base);
  float* Z = reinterpret_cast<float*>(base + al256(16 * T * d.Cin * 4));
  float* P = reinterpret_cast<float*>(base + al256(16 * T * d.Cin * 4) + al256(16 * T * d.Cout * 4));
  const int Th = d.H / 2, Tw = d.W / 2;
  if (Vhave) {
    V = const_cast<float*>(Vhave);          // the forward conv's input transform of this x, kept by the caller
    if (valid_rows < d.B) {
      const size_t t0 = (size_t)valid_rows * Th * Tw, Tr = T - t0;
      hipLaunchKernelGGL(wino_input_kernel, dim3(wino_blocks(Tr * (d.Cin / 4))), dim3(256), 0, stream, x + (size_t)valid_rows * d.H * d.W * d.Cin, d.H,
                         d.W, d.Cin, Th, Tw, Tr, V + t0 * d.Cin, 0, Tp);
    }
  } else hipLaunchKernelGGL(wino_input_kernel, dim3(wino_blocks(T * (d.Cin / 4))), dim3(256), 0, stream, x, d.H, d.W, d.Cin, Th, Tw, T, V, 0, T);
  hipLaunchKernelGGL(wino_dy_kernel, dim3(wino_blocks(T * (d.Cout / 4))), dim3(256), 0, stream, dy, d.H, d.W, d.Cout, Th, Tw, T, Z);
  t2i_conv_desc gd = d;
  gd.B = (int32_t)T; gd.H = gd.W = gd.Ho = gd.Wo = 1; gd.KH = gd.KW = gd.SH = gd.SW = 1; gd.pad_t = gd.pad_l = 0;
  const int rc = run_batched_gemm(gd, MODE_BWD_FILTER, 16, V, Z, P, (int64_t)Tp * d.Cin, (int64_t)T * d.Cout, (int64_t)d.Cin * d.Cout, stream,
                                  "winograd filter-gradient gemm");
  if (rc != T2I_OK) return rc;
  hipLaunchKernelGGL(wino_dw_kernel, dim3(wino_blocks((size_t)d.Cin * (d.Cout / 4))), dim3(256), 0, stream, P, d.Cin, d.Cout, accumulate, dw);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error("winograd filter gradient: %s", hipGetErrorString(e)); return T2I_ERR_LAUNCH; }
  return T2I_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// 4x4 stride-2 SAME convolutions (the critic trunk; the input gradient of the generator's deconvs) by Winograd F(2x2, 2x2):
// a k4 s2 conv is the sum over the 4 input phases (p,q) of a 2x2 stride-1 correlation,
//     y[oh][ow] = sum_{p,q} sum_{a,b} X_pq[oh+a][ow+b] w[2a+p][2b+q],    X_pq[r][c] = x[2r+p-1][2c+q-1],
// i.e. ONE 2x2 stride-1 conv over the space-to-depth image with 4*Cin channels.  F(2x2,2x2) computes a 2x2 output tile from
// a 3x3 patch with 9 multiplies instead of 16: 1.78x fewer multiply-adds.
//   V[xi][t][(p,q,ci)] = B^T X_pq B   (3x3 per phase; the 4 phases partition the tile's 6x6 input patch)   BT = [1 -1 0; 0 1 0; 0 -1 1]
//   U[xi][(p,q,ci)][co] = G g_pq G^T  (2x2 -> 3x3)                                                         G  = [1 0; 1 1; 0 1]
//   M[xi] = V[xi] * U[xi]             9 batched GEMMs [T x 4Cin] x [4Cin x Cout]
//   y tile = A^T M A + bias, act      (3x3 -> 2x2)                                                          AT = [1 1 0; 0 1 1]
// ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void wino2_filter_body(const float* __restrict__ w, int Cin, int Cout, float* __restrict__ U, unsigned vb, unsigned nvb) {
  const int N4 = Cout >> 2;
  const size_t total = (size_t)4 * Cin * N4;             // (phase, ci, co4)
  const size_t plane = (size_t)4 * Cin * N4;             // one xi plane of U, in float4
  for (size_t i = (size_t)vb * 256 + threadIdx.x; i < total; i += (size_t)nvb * 256) {
    const int n4 = (int)(i % N4);
    const int ci = (int)((i / N4) % Cin);
    const int ph = (int)(i / ((size_t)N4 * Cin));
    const int p = ph >> 1, q = ph & 1;
    float4 g[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
        g[a][b] = reinterpret_cast<const float4*>(w + ((size_t)((2 * a + p) * 4 + (2 * b + q)) * Cin + ci) * Cout)[n4];
    float4 s[3][2] = {{g[0][0], g[0][1]}, {f4add(g[0][0], g[1][0]), f4add(g[0][1], g[1][1])}, {g[1][0], g[1][1]}};
    float4* o = reinterpret_cast<float4*>(U) + ((size_t)ph * Cin + ci) * N4 + n4;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      wst(&o[(size_t)(r * 3 + 0) * plane], s[r][0]);
      wst(&o[(size_t)(r * 3 + 1) * plane], f4add(s[r][0], s[r][1]));
      wst(&o[(size_t)(r * 3 + 2) * plane], s[r][1]);
    }
  }
}

__global__ __launch_bounds__(256) void wino2_filter_kernel(const float* __restrict__ w, int Cin, int Cout, float* __restrict__ U) {
  wino2_filter_body(w, Cin, Cout, U, blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(256) void wino2_input_kernel(const float* __restrict__ x, int H, int W, int C, int Th, int Tw, size_t T,
                                                          float* __restrict__ V, size_t plane_T) {
  const int C4 = C >> 2;
  const size_t total = T * 4 * C4;                        // (tile, phase, ci4)
  const size_t plane = plane_T * 4 * C4;                  // (plane_T: see wino_input_kernel)
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % C4);
    const int ph = (int)((i / C4) & 3);
    const size_t t = i / ((size_t)4 * C4);
    const int p = ph >> 1, q = ph & 1;
    const int tx = (int)(t % Tw);
    const int ty = (int)((t / Tw) % Th);
    const size_t b = t / ((size_t)Tw * Th);
    float4 d[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int ih = 4 * ty - 1 + 2 * r + p;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int iw = 4 * tx - 1 + 2 * c + q;
        d[r][c] = ((unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W)
                      ? reinterpret_cast<const float4*>(x + ((b * H + ih) * W + iw) * C)[c4]
                      : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    float4 tt[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      tt[0][c] = f4sub(d[0][c], d[1][c]);
      tt[1][c] = d[1][c];
      tt[2][c] = f4sub(d[2][c], d[1][c]);
    }
    float4* o = reinterpret_cast<float4*>(V) + (t * 4 + ph) * C4 + c4;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      wst(&o[(size_t)(r * 3 + 0) * plane], f4sub(tt[r][0], tt[r][1]));
      wst(&o[(size_t)(r * 3 + 1) * plane], tt[r][1]);
      wst(&o[(size_t)(r * 3 + 2) * plane], f4sub(tt[r][2], tt[r][1]));
    }
  }
}

__global__ __launch_bounds__(256) void wino2_output_kernel(const float* __restrict__ Mx, const float* __restrict__ bias, int Ho, int Wo,
                                                           int N, int Th, int Tw, size_t T, int act, float alpha,
                                                           float* __restrict__ y) {
  const int N4 = N >> 2;
  const size_t total = T * N4, plane = T * N4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int n4 = (int)(i % N4);
    const size_t t = i / N4;
    const int tx = (int)(t % Tw);
    const int ty = (int)((t / Tw) % Th);
    const size_t b = t / ((size_t)Tw * Th);
    const float4* m = reinterpret_cast<const float4*>(Mx) + t * N4 + n4;
    float4 z[2][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float4 m0 = m[(size_t)(0 * 3 + c) * plane], m1 = m[(size_t)(1 * 3 + c) * plane], m2 = m[(size_t)(2 * 3 + c) * plane];
      z[0][c] = f4add(m0, m1);
      z[1][c] = f4add(m1, m2);
    }
    const float4 bs = bias ? reinterpret_cast<const float4*>(bias)[n4] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      float4 y0 = f4add(f4add(z[r][0], z[r][1]), bs);
      float4 y1 = f4add(f4add(z[r][1], z[r][2]), bs);
      y0.x = apply_act(y0.x, act, alpha); y0.y = apply_act(y0.y, act, alpha); y0.z = apply_act(y0.z, act, alpha); y0.w = apply_act(y0.w, act, alpha);
      y1.x = apply_act(y1.x, act, alpha); y1.y = apply_act(y1.y, act, alpha); y1.z = apply_act(y1.z, act, alpha); y1.w = apply_act(y1.w, act, alpha);
      float4* o = reinterpret_cast<float4*>(y + ((b * Ho + 2 * ty + r) * Wo + 2 * tx) * N) + n4;
      o[0] = y0;
      o[N4] = y1;
    }
  }
}

bool winograd_k4s2_eligible(const t2i_conv_desc& d, bool bwd_data) {
  const int minc = tuning().winograd_k4s2_minc;
  if (!tuning().winograd_k4s2 || d.math != T2I_MATH_F32) return false;
  if (!(d.KH == 4 && d.KW == 4 && d.SH == 2 && d.SW == 2 && d.pad_t == 1 && d.pad_l == 1)) return false;
  if ((d.H & 3) || (d.W & 3) || d.Ho * 2 != d.H || d.Wo * 2 != d.W) return false;          // 2x2 output tiles, no ragged edge
  if (bwd_data ? ((d.Cout % 32) || (d.Cin % 32)) : ((d.Cin % 8) || (d.Cout % 32))) return false;
  // the input-gradient form transforms dy once per output phase (9x its bytes through the workspace).  With one workgroup per
  // GEMM tile it only paid from 256 channels up (32x32x128->256 measured 13 % slower than the direct GEMM); with the persistent
  // batched GEMM (t2i_bgemm.hip) the 128-channel layers gain too (155 -> 143 us at B=64, 457 -> 422 us at B=192)
  const int minc_bwd = tuning().winograd_k4s2_bwd_minc;
  const int m = bwd_data ? minc_bwd : minc;
  if (!(d.Cin >= m && d.Cout >= m)) return false;
  // ... and only where the 9 (36) position GEMMs still fill the chip (round 5, profiles/r05_b8_winograd_threshold.txt): at 8 - 16 images per GPU
  // a layer has T = 64 - 1024 tiles, the batched launch 100 - 600 work items of 16 - 64 K-tiles each, and ONE direct GEMM with split-K wins by
  // 15 - 40 % (B = 8) or ties (B = 16); 8x8x512->1024 at B = 24 (T = 96: two M-tiles, the second half empty) loses 28 % while its siblings with
  // T = 384 / 1536 win 19 %.  Work = T * 4 Cin * Cout multiply-adds per position; items = 9 * M-tiles * N-tiles of the forward form.
  const int64_t T = (int64_t)d.B * (d.Ho / 2) * (d.Wo / 2);
  const int64_t items = 9 * ((T + 63) / 64) * ((d.Cout + 63) / 64);
  return T * 4 * d.Cin * d.Cout >= (int64_t)tuning().winograd_k4s2_minwork && items >= tuning().winograd_k4s2_minitems;
}

size_t winograd_k4s2_ws(const t2i_conv_desc& d) {
  const size_t T = (size_t)d.B * (d.Ho / 2) * (d.Wo / 2), K = (size_t)4 * d.Cin;
  return al256(9 * K * d.Cout * 4) + al256(9 * T * K * 4) + al256(9 * T * d.Cout * 4);
}

// The nine position GEMMs of an F(2x2,2x2) tile and its output transform as ONE work item (bgemm9_kernel, t2i_bgemm.hip): no M planes, no
// output-transform launch.  Taken when tuning().wino_fuse says so (1: only where phases x tiles still give >= wino_fuse_items items; 2: wherever
// the persistent kernel's operand conditions hold).  Returns T2I_OK after launching, or -1 if the caller should take the unfused path.
static int wino2_fused_gemm(int lay, int phases, size_t T, int N, int K, const float* V, const float* U, int64_t sa, int64_t sb, const float* bias,
                            float* out, int OH, int OW, int Th, int Tw, int sr, int act, float alpha, hipStream_t stream, const char* what,
                            const float* dy_raw = nullptr, int dHo = 0, int dWo = 0, int64_t dy_elems = 0) {
  // dy_raw != NULL (input gradient): the loader transforms dy itself; V is not read (and need not have been written)
  const int mode = tuning().wino_fuse;
  if (!mode || !tuning().bgemm) return -1;
  // K-tiles of 32, an even number of them.  The loader transform pads an odd count with one K-tile that reads zeros through the range
  // check (acc + 0 * 0 = acc) and addresses dy by pixel, so it takes any T; the V-plane forms keep their conditions
  const int ntiles = dy_raw ? ((K + 31) / 32 + 1) & ~1 : (K + 31) / 32;
  const int64_t a_elems = dy_raw ? dy_elems : (int64_t)T * K, b_elems = (int64_t)N * K;
  if (dy_raw) V = dy_raw;       // (alignment / extent checks below apply to the operand actually read)
  if ((ntiles & 1) || (!dy_raw && (T & 3)) || (N & 3) || (K & 3) || (reinterpret_cast<uintptr_t>(V) & 15) || (reinterpret_cast<uintptr_t>(U) & 15) || (sa & 3) || (sb & 3) ||
      a_elems >= (1LL << 30) || b_elems >= (1LL << 30) || T >= (1u << 30))
    return -1;
  Bgemm9Params q;
  memset(&q, 0, sizeof(q));
  q.g.a = V; q.g.b = U; q.g.c = nullptr;
  q.g.M = (int32_t)T; q.g.N = N; q.g.K = K;
  q.g.tiles_m = (int32_t)((T + 63) / 64); q.g.tiles_n = (N + 63) / 64;
  { const int g = tuning().group_n; q.g.group_n = q.g.tiles_n < g ? q.g.tiles_n : g; if (q.g.group_n < 1) q.g.group_n = 1; }
  q.g.ntiles = ntiles;
  const int64_t items = (int64_t)phases * q.g.tiles_m * q.g.tiles_n;
  if (items >= (1LL << 30)) return -1;
  if (mode == 1) {
    // auto: enough items, AND they must fill whole rounds of the 512 resident workgroups (2 per CU): 1536 and 512 items win 16-19 % on the
    // 128 -> 256 input gradient, 768 items (1.5 rounds) lose 10 % on 256 -> 512 even with the loader transform (profiles/r05_winograd_fused.txt)
    const int64_t rounds = (items + 511) / 512;
    if (items < (int64_t)tuning().wino_fuse_items * (lay == 0 ? 4 : 1) || items * 100 < rounds * 512 * 85) return -1;
    // ... and with K = 1024 (32 K-tiles x 9 positions per item) the unfused position GEMMs are efficient on their own while a single
    // round of fused items has nothing to overlap its epilogue with: the 512 -> 1024 input gradient of the stacked critic pass
    // (256 images, 512 items) 405.7 us fused / 358.9 us unfused; 128 -> 256 (2048 items) 461.6 / 583.2, 256 -> 512 (1024) 428.2 / 425.8
    // (profiles/r06_stacked_pass.txt)
    if (K >= 1024 && rounds < 3) return -1;
  }
  q.g.items = (int32_t)items;
  q.g.sa = sa; q.g.sb = sb; q.g.sc = 0;
  q.g.a_bytes = (uint32_t)(a_elems * 4); q.g.b_bytes = (uint32_t)(b_elems * 4);
  q.bias = bias; q.out = out; q.OH = OH; q.OW = OW; q.Th = Th; q.Tw = Tw; q.sr = sr; q.act = act; q.alpha = alpha;
  q.dy = dy_raw; q.dHo = dHo; q.dWo = dWo;
  if (tuning().debug_plan) fprintf(stderr, "[t2i plan] %s: fused 9-position items, %d phases x %d x %d tiles, K=%d\n", what, phases, q.g.tiles_m, q.g.tiles_n, K);
  const hipError_t e = bgemm9_launch(lay, q, stream);
  if (e != hipSuccess) { set_error("%s: %s", what, hipGetErrorString(e)); return T2I_ERR_LAUNCH; }
  return T2I_OK;
}

int winograd_k4s2_fwd(const t2i_conv_desc& d, const float* x, const float* w, const float* bias, float* y, int act, float alpha,
                      void* ws, size_t ws_bytes, hipStream_t stream, float* Vkeep) {
  const size_t T = (size_t)d.B * (d.Ho / 2) * (d.Wo / 2), K = (size_t)4 * d.Cin;
  if (!ws || ws_bytes < winograd_k4s2_ws(d) || (reinterpret_cast<uintptr_t>(ws) & 15)) {
    set_error("winograd k4s2 conv: workspace %zu B < %zu B required (or misaligned)", ws_bytes, winograd_k4s2_ws(d));
    return T2I_ERR_WORKSPACE;
  }
  char* base = reinterpret_cast<char*>(ws);
  float* U = reinterpret_cast<float*>(base);
  float* V = Vkeep ? Vkeep : reinterpret_cast<float*>(base + al256(9 * K * d.Cout * 4));
  float* Mx = reinterpret_cast<float*>(base + al256(9 * K * d.Cout * 4) + al256(9 * T * K * 4));
  const int Th = d.Ho / 2, Tw = d.Wo / 2;
  bool fill = true;
  if (float* Uc = filter_cache_get(w, 2, d.Cin, d.Cout, (size_t)9 * 4 * d.Cin * d.Cout * 4, stream, &fill)) U = Uc;
  if (fill)
    hipLaunchKernelGGL(wino2_filter_kernel, dim3(wino_blocks((size_t)4 * d.Cin * (d.Cout / 4))), dim3(256), 0, stream, w, d.Cin, d.Cout, U);
  hipLaunchKernelGGL(wino2_input_kernel, dim3(wino_blocks(T * d.Cin)), dim3(256), 0, stream, x, d.H, d.W, d.Cin, Th, Tw, T, V, T);
  t2i_conv_desc gd = d;
  gd.B = (int32_t)T; gd.H = gd.W = gd.Ho = gd.Wo = 1; gd.Cin = (int32_t)K; gd.KH = gd.KW = gd.SH = gd.SW = 1; gd.pad_t = gd.pad_l = 0;
  {   // all nine positions + the output transform in one work item where that still fills the chip
    const int fr = wino2_fused_gemm(0, 1, T, d.Cout, (int)K, V, U, (int64_t)T * K, (int64_t)K * d.Cout, bias, y, d.Ho, d.Wo, Th, Tw, 1, act, alpha, stream,
                                    "winograd k4s2 fused gemm");
    if (fr != -1) return fr;
  }
  const int rc = run_batched_gemm(gd, MODE_FWD, 9, V, U, Mx, (int64_t)T * K, (int64_t)K * d.Cout, (int64_t)T * d.Cout, stream, "winograd k4s2 gemm");
  if (rc != T2I_OK) return rc;
  hipLaunchKernelGGL(wino2_output_kernel, dim3(wino_blocks(T * (d.Cout / 4))), dim3(256), 0, stream, Mx, bias, d.Ho, d.Wo, d.Cout, Th, Tw, T, act,
                     alpha, y);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error("winograd k4s2 conv: %s", hipGetErrorString(e)); return T2I_ERR_LAUNCH; }
  return T2I_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Input gradient of a 4x4 stride-2 SAME conv (= tf conv2d_transpose k4 s2: the generator's up-sampling layers) by the
// same F(2x2, 2x2): each output phase (ph, pw) of dx is a 2x2 stride-1 correlation of dy with the flipped sub-filter
//     dx[2q+ph][2r+pw][ci] = sum_{a,b,co} dy[q + oh_off - 1 + a][r + ow_off - 1 + b][co] * w[kh0 + 2(1-a)][kw0 + 2(1-b)][ci][co]
// (kh0 = 1 - ph, oh_off = ph for pad 1).  36 batched GEMMs (4 phases x 9 tile positions) [T x Cout] x [Cin x Cout]^T.
// ------------------------------------------------------------------------------------------------------------------
// Plane slot of (tile position (r, c), output phase phs) in V and M of the input-gradient form.  Output phase (ph, pw) correlates dy
// with the FLIPPED sub-filter of the forward conv's input phase (1 - ph, 1 - pw), and G flip(g) G^T is the forward image with rows /
// columns 0 and 2 exchanged — so the 36 matrices are exactly the forward image U[xi][(p, q)][ci][co] (kind 2) read as
// [ci][co] blocks at block index xi' * 4 + (3 - phs), xi' = (2 - r, 2 - c): V and M use that block index as their plane slot and the
// batched GEMM walks the forward image with a uniform stride of Cin * Cout.  No second filter image.
__device__ __forceinline__ int wino2b_slot(int r, int c, int phs) { return ((2 - r) * 3 + (2 - c)) * 4 + (3 - phs); }

__global__ __launch_bounds__(256) void wino2b_input_kernel(const float* __restrict__ dy, int Ho, int Wo, int C, int Th, int Tw, size_t T,
                                                           float* __restrict__ V) {
  const int C4 = C >> 2;
  const size_t total = T * 4 * C4;                        // (phase, tile, co4)
  const size_t plane = T * C4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % C4);
    const size_t t = (i / C4) % T;
    const int phs = (int)(i / ((size_t)C4 * T));
    const int ph = phs >> 1, pw = phs & 1;
    const int tx = (int)(t % Tw);
    const int ty = (int)((t / Tw) % Th);
    const size_t b = t / ((size_t)Tw * Th);
    float4 d[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int oh = 2 * ty + ph - 1 + r;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int ow = 2 * tx + pw - 1 + c;
        d[r][c] = ((unsigned)oh < (unsigned)Ho && (unsigned)ow < (unsigned)Wo)
                      ? reinterpret_cast<const float4*>(dy + ((b * Ho + oh) * Wo + ow) * C)[c4]
                      : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    float4 tt[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      tt[0][c] = f4sub(d[0][c], d[1][c]);
      tt[1][c] = d[1][c];
      tt[2][c] = f4sub(d[2][c], d[1][c]);
    }
    float4* o = reinterpret_cast<float4*>(V) + t * C4 + c4;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      wst(&o[(size_t)wino2b_slot(r, 0, phs) * plane], f4sub(tt[r][0], tt[r][1]));
      wst(&o[(size_t)wino2b_slot(r, 1, phs) * plane], tt[r][1]);
      wst(&o[(size_t)wino2b_slot(r, 2, phs) * plane], f4sub(tt[r][2], tt[r][1]));
    }
  }
}

__global__ __launch_bounds__(256) void wino2b_output_kernel(const float* __restrict__ Mx, const float* __restrict__ bias, int H, int W,
                                                            int N, int Th, int Tw, size_t T, int act, float alpha,
                                                            float* __restrict__ dx) {
  const int N4 = N >> 2;
  const size_t total = T * 4 * N4, plane = T * N4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int n4 = (int)(i % N4);
    const size_t t = (i / N4) % T;
    const int phs = (int)(i / ((size_t)N4 * T));
    const int ph = phs >> 1, pw = phs & 1;
    const int tx = (int)(t % Tw);
    const int ty = (int)((t / Tw) % Th);
    const size_t b = t / ((size_t)Tw * Th);
    const float4* m = reinterpret_cast<const float4*>(Mx) + t * N4 + n4;
    float4 z[2][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float4 m0 = m[(size_t)wino2b_slot(0, c, phs) * plane], m1 = m[(size_t)wino2b_slot(1, c, phs) * plane],
                   m2 = m[(size_t)wino2b_slot(2, c, phs) * plane];
      z[0][c] = f4add(m0, m1);
      z[1][c] = f4add(m1, m2);
    }
    const float4 bs = bias ? reinterpret_cast<const float4*>(bias)[n4] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      float4 y0 = f4add(f4add(z[r][0], z[r][1]), bs);
      float4 y1 = f4add(f4add(z[r][1], z[r][2]), bs);
      y0.x = apply_act(y0.x, act, alpha); y0.y = apply_act(y0.y, act, alpha); y0.z = apply_act(y0.z, act, alpha); y0.w = apply_act(y0.w, act, alpha);
      y1.x = apply_act(y1.x, act, alpha); y1.y = apply_act(y1.y, act, alpha); y1.z = apply_act(y1.z, act, alpha); y1.w = apply_act(y1.w, act, alpha);
      // q = 2*ty + r, columns r' = 2*tx, 2*tx+1  ->  pixels (2q+ph, 2r'+pw)
      const size_t ih = (size_t)2 * (2 * ty + r) + ph;
      float4* o0 = reinterpret_cast<float4*>(dx + ((b * H + ih) * W + (size_t)2 * (2 * tx) + pw) * N) + n4;
      float4* o1 = reinterpret_cast<float4*>(dx + ((b * H + ih) * W + (size_t)2 * (2 * tx + 1) + pw) * N) + n4;
      *o0 = y0;
      *o1 = y1;
    }
  }
}

size_t winograd_k4s2_bwd_ws(const t2i_conv_desc& d) {
  const size_t T = (size_t)d.B * (d.Ho / 2) * (d.Wo / 2);
  return al256((size_t)36 * d.Cin * d.Cout * 4) + al256(36 * T * d.Cout * 4) + al256(36 * T * d.Cin * 4);
}

int winograd_k4s2_bwd_data(const t2i_conv_desc& d, const float* dy, const float* w, const float* bias, float* dx, int act, float alpha,
                           void* ws, size_t ws_bytes, hipStream_t stream) {
  const size_t T = (size_t)d.B * (d.Ho / 2) * (d.Wo / 2);
  if (!ws || ws_bytes < winograd_k4s2_bwd_ws(d) || (reinterpret_cast<uintptr_t>(ws) & 15)) {
    set_error("winograd k4s2 input gradient: workspace %zu B < %zu B required (or misaligned)", ws_bytes, winograd_k4s2_bwd_ws(d));
    return T2I_ERR_WORKSPACE;
  }
  char* base = reinterpret_cast<char*>(ws);
  float* U = reinterpret_cast<float*>(base);
  float* V = reinterpret_cast<float*>(base + al256((size_t)36 * d.Cin * d.Cout * 4));
  float* Mx = reinterpret_cast<float*>(base + al256((size_t)36 * d.Cin * d.Cout * 4) + al256(36 * T * d.Cout * 4));
  const int Th = d.Ho / 2, Tw = d.Wo / 2;
  bool fill = true;
  if (float* Uc = filter_cache_get(w, 2, d.Cin, d.Cout, (size_t)36 * d.Cin * d.Cout * 4, stream, &fill)) U = Uc;      // the forward image
  if (fill)
    hipLaunchKernelGGL(wino2_filter_kernel, dim3(wino_blocks((size_t)4 * d.Cin * (d.Cout / 4))), dim3(256), 0, stream, w, d.Cin, d.Cout, U);
  if (tuning().wino_fuse_xf) {   // everything in one launch: dy -> (transform in the loader) -> 4 x 9 GEMMs -> (transform in the epilogue) -> dx
    const int fr = wino2_fused_gemm(1, 4, T, d.Cin, d.Cout, V, U, (int64_t)T * d.Cout, (int64_t)d.Cin * d.Cout, bias, dx, d.H, d.W, Th, Tw, 2, act, alpha, stream,
                                    "winograd k4s2 input-gradient fused gemm (loader transform)", dy, d.Ho, d.Wo, (int64_t)d.B * d.Ho * d.Wo * d.Cout);
    if (fr != -1) return fr;
  }
  hipLaunchKernelGGL(wino2b_input_kernel, dim3(wino_blocks(T * d.Cout)), dim3(256), 0, stream, dy, d.Ho, d.Wo, d.Cout, Th, Tw, T, V);
  t2i_conv_desc gd = d;
  gd.B = (int32_t)T; gd.H = gd.W = gd.Ho = gd.Wo = 1; gd.KH = gd.KW = gd.SH = gd.SW = 1; gd.pad_t = gd.pad_l = 0;
  {
    const int fr = wino2_fused_gemm(1, 4, T, d.Cin, d.Cout, V, U, (int64_t)T * d.Cout, (int64_t)d.Cin * d.Cout, bias, dx, d.H, d.W, Th, Tw, 2, act, alpha, stream,
                                    "winograd k4s2 input-gradient fused gemm");
    if (fr != -1) return fr;
  }
  const int rc = run_batched_gemm(gd, MODE_BWD_DATA, 36, V, U, Mx, (int64_t)T * d.Cout, (int64_t)d.Cin * d.Cout, (int64_t)T * d.Cin, stream,
                                  "winograd k4s2 input-gradient gemm");
  if (rc != T2I_OK) return rc;
  hipLaunchKernelGGL(wino2b_output_kernel, dim3(wino_blocks(T * d.Cin)), dim3(256), 0, stream, Mx, bias, d.H, d.W, d.Cin, Th, Tw, T, act, alpha, dx);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error("winograd k4s2 input gradient: %s", hipGetErrorString(e)); return T2I_ERR_LAUNCH; }
  return T2I_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Filter gradient of the 4x4 stride-2 conv through the same F(2x2,2x2) identity (adjoint of winograd_k4s2_fwd):
//   V[xi][t][(p,q,ci)] = B^T X_pq B                      (the forward's input transform)
//   Z[xi][t][co]       = A dy A^T, A = [1 0; 1 1; 0 1]   (2x2 output-gradient tile -> 3x3)
//   P[s][xi][(p,q,ci)][co] = sum_{t in chunk s} V Z      9*S batched filter-gradient GEMMs (S tile chunks fill the chip
//                                                        when 9 * tiles is below the CU count; summed in the last step)
//   dw[2a+p][2b+q][ci][co] (+)= (G^T P G)[a][b]
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void wino2_dy_kernel(const float* __restrict__ dy, int Ho, int Wo, int N, int Th, int Tw, size_t T,
                                                       float* __restrict__ Z) {
  const int N4 = N >> 2;
  const size_t total = T * N4, plane = T * N4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int n4 = (int)(i % N4);
    const size_t t = i / N4;
    const int tx = (int)(t % Tw);
    const int ty = (int)((t / Tw) % Th);
    const size_t b = t / ((size_t)Tw * Th);
    const float4* src = reinterpret_cast<const float4*>(dy + ((b * Ho + 2 * ty) * Wo + 2 * tx) * N) + n4;
    const float4 d00 = src[0], d01 = src[N4], d10 = src[(size_t)Wo * N4], d11 = src[(size_t)Wo * N4 + N4];
    const float4 s[3][2] = {{d00, d01}, {f4add(d00, d10), f4add(d01, d11)}, {d10, d11}};
    float4* o = reinterpret_cast<float4*>(Z) + t * N4 + n4;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      wst(&o[(size_t)(r * 3 + 0) * plane], s[r][0]);
      wst(&o[(size_t)(r * 3 + 1) * plane], f4add(s[r][0], s[r][1]));
      wst(&o[(size_t)(r * 3 + 2) * plane], s[r][1]);
    }
  }
}

__global__ __launch_bounds__(256) void wino2_dw_kernel(const float* __restrict__ P, int Cin, int Cout, int nslab, int accumulate,
                                                       float* __restrict__ dw) {
  const int N4 = Cout >> 2;
  const size_t total = (size_t)4 * Cin * N4;              // (phase, ci, co4) = one xi plane of P
  const size_t plane = total;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int n4 = (int)(i % N4);
    const int ci = (int)((i / N4) % Cin);
    const int ph = (int)(i / ((size_t)N4 * Cin));
    const int p = ph >> 1, q = ph & 1;
    float4 m[9];
#pragma unroll
    for (int xi = 0; xi < 9; ++xi) m[xi] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int sl = 0; sl < nslab; ++sl) {                  // P is [xi][slab][K][Cout]
      const float4* src = reinterpret_cast<const float4*>(P) + (size_t)sl * plane + i;
#pragma unroll
      for (int xi = 0; xi < 9; ++xi) m[xi] = f4add(m[xi], src[(size_t)xi * nslab * plane]);
    }
    float4 z[2][3];                                       // z[a][c] = sum_r G[r][a] m[r][c]
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      z[0][c] = f4add(m[0 * 3 + c], m[1 * 3 + c]);
      z[1][c] = f4add(m[1 * 3 + c], m[2 * 3 + c]);
    }
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      float4 g0 = f4add(z[a][0], z[a][1]), g1 = f4add(z[a][1], z[a][2]);
      float4* o0 = reinterpret_cast<float4*>(dw + ((size_t)((2 * a + p) * 4 + (0 + q)) * Cin + ci) * Cout) + n4;
      float4* o1 = reinterpret_cast<float4*>(dw + ((size_t)((2 * a + p) * 4 + (2 + q)) * Cin + ci) * Cout) + n4;
      if (accumulate) { g0 = f4add(g0, *o0); g1 = f4add(g1, *o1); }
      *o0 = g0;
      *o1 = g1;
    }
  }
}

static int wino2_slabs(const t2i_conv_desc& d, size_t T) {
  const size_t tiles = (size_t)((4 * d.Cin + 127) / 128) * ((d.Cout + 127) / 128) * 9;
  int S = 1;
  while (tiles * S < 256 && S < 8 && (T % (size_t)(2 * S)) == 0 && T / (2 * S) >= 256) S *= 2;
  return S;
}

size_t winograd_k4s2_filter_grad_ws(const t2i_conv_desc& d) {
  const size_t T = (size_t)d.B * (d.Ho / 2) * (d.Wo / 2), K = (size_t)4 * d.Cin;
  return al256(9 * T * K * 4) + al256(9 * T * d.Cout * 4) + al256((size_t)9 * wino2_slabs(d, T) * K * d.Cout * 4);
}

int winograd_k4s2_filter_grad(const t2i_conv_desc& d, const float* x, const float* dy, float* dw, int accumulate, void* ws, size_t ws_bytes,
                              hipStream_t stream, const float* Vhave, int valid_rows) {
  const size_t T = (size_t)d.B * (d.Ho / 2) * (d.Wo / 2), K = (size_t)4 * d.Cin;
  if (!ws || ws_bytes < winograd_k4s2_filter_grad_ws(d) || (reinterpret_cast<uintptr_t>(ws) & 15)) {
    set_error("winograd k4s2 filter gradient: workspace %zu B < %zu B required (or misaligned)", ws_bytes, winograd_k4s2_filter_grad_ws(d));
    return T2I_ERR_WORKSPACE;
  }
  const int S = wino2_slabs(d, T);
  char* base = reinterpret_cast<char*>(ws);
  float* V = reinterpret_cast<float*>(base);
  float* Z = reinterpret_cast<float*>(base + al256(9 * T * K * 4));
  float* P = reinterpret_cast<float*>(base + al256(9 * T * K * 4) + al256(9 * T * d.Cout * 4));
  const int Th = d.Ho / 2, Tw = d.Wo / 2;
  if (Vhave) {
    V = const_cast<float*>(Vhave);
    if (valid_rows < d.B) {                 // (see winograd_filter_grad)
      const size_t t0 = (size_t)valid_rows * Th * Tw, Tr = T - t0;
      hipLaunchKernelGGL(wino2_input_kernel, dim3(wino_blocks(Tr * d.Cin)), dim3(256), 0, stream, x + (size_t)valid_rows * d.H * d.W * d.Cin, d.H, d.W,
                         d.Cin, Th, Tw, Tr, V + t0 * K, T);
    }
  } else hipLaunchKernelGGL(wino2_input_kernel, dim3(wino_blocks(T * d.Cin)), dim3(256), 0, stream, x, d.H, d.W, d.Cin, Th, Tw, T, V, T);
  hipLaunchKernelGGL(wino2_dy_kernel, dim3(wino_blocks(T * (d.Cout / 4))), dim3(256), 0, stream, dy, d.Ho, d.Wo, d.Cout, Th, Tw, T, Z);
  t2i_conv_desc gd = d;
  gd.B = (int32_t)(T / S); gd.Cin = (int32_t)K; gd.H = gd.W = gd.Ho = gd.Wo = 1; gd.KH = gd.KW = gd.SH = gd.SW = 1; gd.pad_t = gd.pad_l = 0;
  const int rc = run_batched_gemm(gd, MODE_BWD_FILTER, 9 * S, V, Z, P, (int64_t)(T / S) * K, (int64_t)(T / S) * d.Cout, (int64_t)K * d.Cout, stream,
                                  "winograd k4s2 filter-gradient gemm");
  if (rc != T2I_OK) return rc;
  hipLaunchKernelGGL(wino2_dw_kernel, dim3(wino_blocks((size_t)4 * d.Cin * (d.Cout / 4))), dim3(256), 0, stream, P, d.Cin, d.Cout, S, accumulate, dw);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error("winograd k4s2 filter gradient: %s", hipGetErrorString(e)); return T2I_ERR_LAUNCH; }
  return T2I_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Batched refresh of the filter cache.  After an optimizer step every cached image of the arena it updated is stale; filled
// lazily they cost one small launch per (filter, kind) and iteration — ~60 launches of 5-8 us at the benchmark's widths,
// 0.4-0.5 ms of a 15 ms (fp32) / 8 ms (bf16) iteration.  t2i_filter_cache_refresh regenerates all of them in ONE launch
// (per 96 entries): the table of (filter, image, dims, kind, first block) rides in the kernel arguments, a workgroup finds
// its entry by bisection on the scalar unit and runs that kind's transform body on its share of the entry.
//   kind  0    U = G g G^T of a 3x3 filter (the input gradient reads the same image, wino_slot)  wino_filter_body
//   kind  2    F(2x2,2x2) images of the four 2x2 phase filters of a 4x4 stride-2 conv; its      wino2_filter_body
//              input gradient reads the same 36 [ci][co] blocks in another order (wino2b_slot)
//              (kinds 1 and 3, the separate input-gradient images of rounds 1-2, are gone: half the bytes per refresh)
//   kinds 4/5  bf16 K-inner images [tap][Cout][Cin] (per-tap transpose) / [tap][Cin][Cout]    wcast_body
// ------------------------------------------------------------------------------------------------------------------
typedef __bf16 bf16_t;

// One workgroup = a 64 (ci) x 64 (co) block of one tap through an LDS tile; vb enumerates (tap, ci block, co block).  The
// fp32 block is read once (float4 along co) and leaves as either or both bf16 images: `plain` [tap][Ci][Co] (4 consecutive
// co per 8-byte store) and `trans` [tap][Co][Ci] (4 consecutive ci per 8-byte store, read down the LDS tile's columns).
// Ragged edges (Ci or Co not a multiple of 64, or Co % 4 != 0) take the element-wise path.
constexpr int WC_T = 64;
__device__ __forceinline__ unsigned wc_pk2(float lo, float hi) {
  typedef float f2 __attribute__((ext_vector_type(2)));
  typedef __bf16 h2 __attribute__((ext_vector_type(2)));
  f2 v = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, h2));
}
__device__ __forceinline__ unsigned wcast_blocks(int Ci, int Co, int taps) {
  return (unsigned)(((Co + WC_T - 1) / WC_T) * ((Ci + WC_T - 1) / WC_T) * taps);
}
__device__ __forceinline__ void wcast_body(const float* __restrict__ w, int Ci, int Co, bf16_t* __restrict__ plain, bf16_t* __restrict__ trans,
                                           float (*tile)[WC_T + 1], unsigned vb) {
  const unsigned nbx = (Co + WC_T - 1) / WC_T, nby = (Ci + WC_T - 1) / WC_T;
  const int bx = vb % nbx, by = (vb / nbx) % nby, t = vb / (nbx * nby);
  const int ci0 = by * WC_T, co0 = bx * WC_T;
  const float* src = w + (size_t)t * Ci * Co;
  const size_t tap_off = (size_t)t * Ci * Co;
  const int tid = threadIdx.x;
  const bool full = (ci0 + WC_T <= Ci) && (co0 + WC_T <= Co) && (Co % 4 == 0) && (Ci % 4 == 0);
  if (full) {
    const int c4 = tid & 15, r = tid >> 4;            // 16 float4 per row, 16 rows per pass
#pragma unroll
    for (int j = 0; j < WC_T; j += 16) {
      const float4 v = *reinterpret_cast<const float4*>(src + (size_t)(ci0 + r + j) * Co + co0 + c4 * 4);
      tile[r + j][c4 * 4 + 0] = v.x; tile[r + j][c4 * 4 + 1] = v.y; tile[r + j][c4 * 4 + 2] = v.z; tile[r + j][c4 * 4 + 3] = v.w;
      if (plain)
        *reinterpret_cast<uint2*>(plain + tap_off + (size_t)(ci0 + r + j) * Co + co0 + c4 * 4) = make_uint2(wc_pk2(v.x, v.y), wc_pk2(v.z, v.w));
    }
    if (trans) {
      __syncthreads();
#pragma unroll
      for (int j = 0; j < WC_T; j += 16) {            // thread -> (co = r + j, 4 consecutive ci = c4 * 4 ..)
        const int co = r + j;
        *reinterpret_cast<uint2*>(trans + tap_off + (size_t)(co0 + co) * Ci + ci0 + c4 * 4) =
            make_uint2(wc_pk2(tile[c4 * 4 + 0][co], tile[c4 * 4 + 1][co]), wc_pk2(tile[c4 * 4 + 2][co], tile[c4 * 4 + 3][co]));
      }
    }
    return;
  }
  const int tx = tid & 63, ty = tid >> 6;             // 64 x 4
  for (int j = ty; j < WC_T; j += 4) {
    const int ci = ci0 + j, co = co0 + tx;
    const float v = (ci < Ci && co < Co) ? src[(size_t)ci * Co + co] : 0.f;
    tile[j][tx] = v;
    if (plain && ci < Ci && co < Co) plain[tap_off + (size_t)ci * Co + co] = (bf16_t)v;
  }
  if (trans) {
    __syncthreads();
    for (int j = ty; j < WC_T; j += 4) {
      const int co = co0 + j, ci = ci0 + tx;
      if (co < Co && ci < Ci) trans[tap_off + (size_t)co * Ci + ci] = (bf16_t)tile[tx][j];
    }
  }
}

__global__ __launch_bounds__(256) void wcast_kernel(const float* __restrict__ w, int Ci, int Co, int transpose, bf16_t* __restrict__ out) {
  __shared__ float tile[WC_T][WC_T + 1];
  wcast_body(w, Ci, Co, transpose ? nullptr : out, transpose ? out : nullptr, tile, blockIdx.x);
}

hipError_t wcast_launch(const float* w, int taps, int Ci, int Co, int transpose, void* out, hipStream_t stream) {
  const unsigned blocks = (unsigned)(((Co + WC_T - 1) / WC_T) * ((Ci + WC_T - 1) / WC_T) * taps);
  hipLaunchKernelGGL(wcast_kernel, dim3(blocks), dim3(256), 0, stream, w, Ci, Co, transpose, reinterpret_cast<bf16_t*>(out));
  return hipGetLastError();
}

struct RefreshItem { const float* w; void* U; void* U2; int32_t Cin, Cout, kind, taps; uint32_t block0, nblocks; };   // 48 bytes
constexpr int REFRESH_MAX = 80;
struct RefreshBatch { int32_t n, pad; RefreshItem it[REFRESH_MAX]; };                                                 // 3848 bytes of kernarg

__device__ __forceinline__ RefreshItem load_refresh_item(int idx) {
  RefreshItem r;
#if defined(__HIP_DEVICE_COMPILE__)
  typedef const __attribute__((address_space(4))) char* KernArg;
  typedef const __attribute__((address_space(4))) int32_t* Words;
  const Words src = (Words)((KernArg)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(RefreshBatch, it) + (size_t)idx * sizeof(RefreshItem));
  int32_t* dst = reinterpret_cast<int32_t*>(&r);
#pragma unroll
  for (int i = 0; i < (int)(sizeof(RefreshItem) / 4); ++i) dst[i] = src[i];
#else
  (void)idx;
  r = RefreshItem();
#endif
  return r;
}

__device__ __forceinline__ uint32_t load_refresh_block0(int idx) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef const __attribute__((address_space(4))) char* KernArg;
  typedef const __attribute__((address_space(4))) uint32_t* Words;
  return *(Words)((KernArg)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(RefreshBatch, it) + (size_t)idx * sizeof(RefreshItem) + offsetof(RefreshItem, block0));
#else
  (void)idx;
  return 0;
#endif
}

__global__ __launch_bounds__(256) void filter_refresh_kernel(RefreshBatch tb) {
  __shared__ float tile[WC_T][WC_T + 1];
  int lo = 0, hi = tb.n - 1;                       // last entry whose first block is <= blockIdx.x (uniform: scalar loads)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (load_refresh_block0(mid) <= blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const RefreshItem it = load_refresh_item(lo);
  const unsigned vb = blockIdx.x - it.block0;
  switch (it.kind) {
    case 0: wino_filter_body(it.w, it.Cin, it.Cout, reinterpret_cast<float*>(it.U), vb, it.nblocks); break;
    case 2: wino2_filter_body(it.w, it.Cin, it.Cout, reinterpret_cast<float*>(it.U), vb, it.nblocks); break;
    default:      // 4: transposed image in U; 5: plain image in U; 6: both (U transposed, U2 plain) from one read of the filter
      wcast_body(it.w, it.Cin, it.Cout, reinterpret_cast<bf16_t*>(it.kind == 5 ? it.U : it.U2), reinterpret_cast<bf16_t*>(it.kind == 5 ? nullptr : it.U), tile, vb);
      break;
  }
}

// Marks the entries refresh would regenerate as filled for the launch context, launching nothing: the caller vouches for the bytes
// (include/t2i_hip.h: t2i_filter_cache_assume).
int filter_cache_assume(const void* p, size_t bytes, hipStream_t stream) {
  if (!g_fc_on) return T2I_OK;
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  unsigned long long id = 0;
  if (hipStreamGetCaptureInfo(stream, &st, &id) != hipSuccess) { (void)hipGetLastError(); return T2I_OK; }
  const unsigned long long cap = st == hipStreamCaptureStatusActive ? id + 1 : 0;
  std::lock_guard<std::mutex> lk(g_fc_mu);
  if (!g_fc_buf) return T2I_OK;
  const char* lo = reinterpret_cast<const char*>(p);
  for (auto& e : g_fc) {
    const char* q = reinterpret_cast<const char*>(e.w);
    const size_t wbytes = (size_t)(e.kind == 0 ? 9 : e.kind == 2 ? 16 : (int)(e.bytes / ((size_t)e.Cin * e.Cout * 2))) * e.Cin * e.Cout * 4;
    if (p && !(q >= lo && q + wbytes <= lo + bytes)) continue;
    if (!cap && e.stream != stream) continue;
    e.valid = true; e.cap = cap; e.cap_fill = nullptr;
  }
  return T2I_OK;
}

// Regenerates every cache entry whose filter lies in [p, p + bytes) (p == NULL: every entry) and that this launch context may
// use (same rules as filter_cache_get), marking it valid for the context: eager launches after it, or the rest of the capture
// it was recorded into, find the images filled.
int filter_cache_refresh(const void* p, size_t bytes, hipStream_t stream) {
  if (!g_fc_on) return T2I_OK;
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  unsigned long long id = 0;
  if (hipStreamGetCaptureInfo(stream, &st, &id) != hipSuccess) { (void)hipGetLastError(); return T2I_OK; }
  const unsigned long long cap = st == hipStreamCaptureStatusActive ? id + 1 : 0;
  std::lock_guard<std::mutex> lk(g_fc_mu);
  if (!g_fc_buf) return T2I_OK;
  const char* lo = reinterpret_cast<const char*>(p);
  RefreshBatch tb;
  tb.n = 0; tb.pad = 0;
  uint32_t blocks = 0;
  auto flush = [&]() {
    if (tb.n > 0) hipLaunchKernelGGL(filter_refresh_kernel, dim3(blocks), dim3(256), 0, stream, tb);
    tb.n = 0; blocks = 0;
  };
  for (auto& e : g_fc) {
    const char* q = reinterpret_cast<const char*>(e.w);
    // the filter this entry was made of must lie INSIDE the caller's range: an entry left behind by a filter that no longer
    // exists (another model's arena, freed since) is never read again
    const size_t wbytes = (size_t)(e.kind == 0 ? 9 : e.kind == 2 ? 16 : (int)(e.bytes / ((size_t)e.Cin * e.Cout * 2))) * e.Cin * e.Cout * 4;
    if (p && !(q >= lo && q + wbytes <= lo + bytes)) continue;
    if (!cap && e.stream != stream) continue;
    if (e.valid && e.cap == cap) continue;          // already fresh in this context
    RefreshItem it;
    it.w = e.w; it.U = e.U; it.U2 = nullptr; it.Cin = e.Cin; it.Cout = e.Cout; it.kind = e.kind; it.taps = 0;
    size_t nb;
    if (e.kind == 0) nb = ((size_t)e.Cin * e.Cout + 255) / 256;
    else if (e.kind == 2) nb = ((size_t)4 * e.Cin * (e.Cout / 4) + 255) / 256;
    else {
      it.taps = (int32_t)(e.bytes / ((size_t)e.Cin * e.Cout * 2));
      nb = (size_t)((e.Cout + WC_T - 1) / WC_T) * ((e.Cin + WC_T - 1) / WC_T) * it.taps;
      // the other bf16 image of the same filter, if stale too: one read of the filter serves both
      for (auto& o : g_fc)
        if (&o != &e && o.w == e.w && o.kind == 9 - e.kind && o.Cin == e.Cin && o.Cout == e.Cout && o.bytes == e.bytes &&
            !(o.valid && o.cap == cap) && (cap || o.stream == stream)) {
          it.kind = 6;
          it.U = e.kind == 4 ? e.U : o.U;            // transposed image
          it.U2 = e.kind == 4 ? o.U : e.U;           // plain image
          o.valid = true; o.cap = cap; o.cap_fill = nullptr;
          break;
        }
    }
    if (e.kind <= 3 && nb > 2048) nb = 2048;        // the transform bodies stride over their entry
    it.block0 = blocks; it.nblocks = (uint32_t)nb;
    tb.it[tb.n++] = it;
    blocks += (uint32_t)nb;
    e.valid = true; e.cap = cap; e.cap_fill = nullptr;
    if (tb.n == REFRESH_MAX) flush();
  }
  flush();
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) { set_error("t2i_filter_cache_refresh: %s", hipGetErrorString(err)); return T2I_ERR_LAUNCH; }
  return T2I_OK;
}

}  // namespace t2i
