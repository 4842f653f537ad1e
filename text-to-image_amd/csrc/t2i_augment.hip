// t2i_augment.hip — differentiable augmentation of the images a critic sees (Zhao et al., "Differentiable Augmentation for
// Data-Efficient GAN Training", NeurIPS 2020; the reference has no such layer): per sample a colour transform (brightness offset,
// saturation blend with the pixel's channel mean, contrast blend with the sample's mean), an integer translation with zero padding
// and a rectangular cutout, all driven by one row of a float32 parameter table on the device.  The operator is affine in the image,
// so two kernels close it under differentiation of any order: the forward (with or without the brightness offset) and the adjoint.
// A colour policy needs one reduction per sample, the sample's sum: aug_partial_kernel leaves per-workgroup partials in the
// workspace in a fixed order and the apply kernels add a sample's partials themselves, in a fixed order too — two launches, no
// join launch, no atomics.  A sample is cut into workgroups by H, W and C alone, so its result is the same bits in whatever batch
// it sits, and calls repeat bit for bit.  Without colour each way is one launch.  The apply kernels give a thread whole pixels
// (C = 3 is the case that matters: 12-byte pixels under arbitrary shifts, a gather per pixel).  Two one-workgroup kernels feed them
// (Karras et al., "Training Generative Adversarial Networks with Limited Data", NeurIPS 2020): aug_draw_kernel fills a table from a
// Philox4x32-10 stream, applying each transform to a row with a probability p kept in device memory next to the seed and the call
// counter, and aug_observe_kernel steers p from the critic's outputs on real images.  The entry points (declared in
// include/t2i_hip.h) are at the end of this file: they validate and enqueue on the caller's stream — no allocation, no synchronisation.
#include <hip/hip_runtime.h>
#include <math.h>

#include "t2i_internal.h"

namespace t2i {
namespace {

constexpr int kThreads = 256;
constexpr int kQuads = 4;                            // 16-byte units of a sample that one thread of the partial-sum kernel adds
constexpr int kChunk = kThreads * kQuads * 4;        // floats of a sample per partial: depends on nothing but these constants
constexpr int kPixPerThread = 4;                     // the apply kernels' grid is sized for this many pixels per thread
constexpr int kMaxSide = 32768;
constexpr long long kMaxElems = (1ll << 30) - 16;    // include/t2i_hip.h: no tensor may exceed 2^30 - 16 elements

int launched(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return T2I_OK;
  set_error("%s: %s", what, hipGetErrorString(e));
  return T2I_ERR_LAUNCH;
}

struct AugRow {
  float b, s, c;
  int ty, tx, y0, y1, x0, x1;
};

// An integer-valued float of the table as an int in [-lim, lim]: whatever the table holds (NaN goes to -lim), every index formed from
// the result stays in int range, and every address is formed only after an explicit test against the image.
__device__ __forceinline__ int aug_geo(float v, int lim) { return (int)fminf(fmaxf(v, -(float)lim), (float)lim); }

// Row n of P [B, 9] = (b, s, c, ty, tx, y0, y1, x0, x1); the columns of a policy that is not in the mask read as the identity.
__device__ __forceinline__ AugRow aug_row(const float* __restrict__ P, int n, int H, int W, int policy) {
  const float* p = P + (size_t)n * 9;
  AugRow r;
  const bool col = policy & T2I_DIFFAUG_COLOR, tr = policy & T2I_DIFFAUG_TRANSLATION, cut = policy & T2I_DIFFAUG_CUTOUT;
  r.b = col ? p[0] : 0.f;
  r.s = col ? p[1] : 1.f;
  r.c = col ? p[2] : 1.f;
  r.ty = tr ? aug_geo(p[3], H) : 0;
  r.tx = tr ? aug_geo(p[4], W) : 0;
  r.y0 = cut ? aug_geo(p[5], H) : 0;
  r.y1 = cut ? aug_geo(p[6], H) : 0;
  r.x0 = cut ? aug_geo(p[7], W) : 0;
  r.x1 = cut ? aug_geo(p[8], W) : 0;
  return r;
}

__device__ __forceinline__ bool aug_in_rect(const AugRow& r, int y, int x) { return y >= r.y0 && y < r.y1 && x >= r.x0 && x < r.x1; }
__device__ __forceinline__ bool aug_inside(int y, int x, int H, int W) { return (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W; }

__device__ __forceinline__ float wave_sum(float a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);       // a butterfly: the same tree, hence the same bits, in every lane
  return a;
}

// part[n][blk] = the sum of chunk blk of sample n of x [B, per]; adj: of the masked, shifted cotangent instead — element (y, x, .)
// of g counts iff it lies outside the cutout rectangle and its destination (y - ty, x - tx) inside the image, which is the sum
// of g3[y, x, .] = g[y + ty, x + tx, .] over the image.  A thread adds kQuads groups of four neighbours as (v0 + v1) + (v2 + v3), read
// by one 16-byte load where the sample is 16-byte aligned and by four guarded loads otherwise: the same values in the same order.
__global__ __launch_bounds__(kThreads) void aug_partial_kernel(const float* __restrict__ x, const float* __restrict__ P, int H, int W, int per,
                                                                FastDiv div_c, FastDiv div_w, int policy, int adj, int nblk,
                                                                float* __restrict__ part) {
  const int n = blockIdx.y, blk = blockIdx.x;
  const float* xs = x + (size_t)n * per;
  AugRow r = {};
  if (adj) r = aug_row(P, n, H, W, policy);
  const bool vec = (reinterpret_cast<uintptr_t>(xs) & 15) == 0;           // (a chunk starts a multiple of 16 bytes into its sample)
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < kQuads; ++k) {
    const int i0 = blk * kChunk + (k * kThreads + (int)threadIdx.x) * 4;
    float v[4];
    if (vec && i0 + 3 < per) {
      const float4 q = *reinterpret_cast<const float4*>(xs + i0);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = i0 + e < per ? xs[i0 + e] : 0.f;
    }
    if (adj) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = i0 + e < per ? i0 + e : 0;
        const int pix = div_c.div(i), yy = div_w.div(pix), xx = pix - yy * W;
        const bool keep = !aug_in_rect(r, yy, xx) && aug_inside(yy - r.ty, xx - r.tx, H, W);
        v[e] = keep ? v[e] : 0.f;
      }
    }
    acc += (v[0] + v[1]) + (v[2] + v[3]);
  }
  acc = wave_sum(acc);
  __shared__ float wsum[kThreads / 64];
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[(size_t)n * nblk + blk] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// The sum of a sample's nblk partials, for the whole workgroup: lane l of the first wave adds partials l, l + 64, ... in that order,
// then the butterfly.  Every workgroup of every launch forms it the same way.
__device__ __forceinline__ float aug_sample_total(const float* __restrict__ part, int nblk) {
  __shared__ float tot;
  if (threadIdx.x < 64) {
    float a = 0.f;
    for (int j = threadIdx.x; j < nblk; j += 64) a += part[j];
    a = wave_sum(a);
    if (threadIdx.x == 0) tot = a;
  }
  __syncthreads();
  return tot;
}

// the two blends, in exactly the form k a + (1 - k) mean: k = 1 returns a bit for bit
__device__ __forceinline__ float aug_blend(float k, float a, float mean) { return k * a + (1.f - k) * mean; }

// y = T(x).  CT: the channel count when a pixel is kept in registers (3, 4), 0 = any C, the pixel read twice.
template <int CT>
__global__ __launch_bounds__(kThreads) void aug_fwd_kernel(const float* __restrict__ x, const float* __restrict__ P, int H, int W, int C,
                                                            FastDiv div_w, int policy, int offset, const float* __restrict__ part, int nblk,
                                                            float* __restrict__ y) {
  const int n = blockIdx.y, HW = H * W;
  const AugRow r = aug_row(P, n, H, W, policy);
  const bool col = policy & T2I_DIFFAUG_COLOR;
  const float b = offset ? r.b : 0.f, invc = 1.f / (float)C;
  float M = 0.f;                                                             // M(u2) = M(u) + b
  if (col) M = aug_sample_total(part + (size_t)n * nblk, nblk) / ((float)HW * (float)C) + b;
  const float* xs = x + (size_t)n * HW * C;
  float* ys = y + (size_t)n * HW * C;
  for (int p = blockIdx.x * kThreads + threadIdx.x; p < HW; p += gridDim.x * kThreads) {
    const int yy = div_w.div(p), xx = p - yy * W;
    const int sy = yy - r.ty, sx = xx - r.tx;
    const bool live = !aug_in_rect(r, yy, xx) && aug_inside(sy, sx, H, W);
    const float* src = xs + ((size_t)(live ? sy : 0) * W + (live ? sx : 0)) * C;
    float* dst = ys + (size_t)p * C;
    if (CT > 0) {
      float v[CT > 0 ? CT : 1];
#pragma unroll
      for (int e = 0; e < CT; ++e) v[e] = live ? src[e] : 0.f;
      if (col && live) {
        float m = 0.f;
#pragma unroll
        for (int e = 0; e < CT; ++e) { if (offset) v[e] += b; m += v[e]; }
        m *= invc;
#pragma unroll
        for (int e = 0; e < CT; ++e) v[e] = aug_blend(r.c, aug_blend(r.s, v[e], m), M);
      }
#pragma unroll
      for (int e = 0; e < CT; ++e) dst[e] = v[e];
    } else if (!live) {
      for (int e = 0; e < C; ++e) dst[e] = 0.f;
    } else if (!col) {
      for (int e = 0; e < C; ++e) dst[e] = src[e];
    } else {
      float m = 0.f;
      for (int e = 0; e < C; ++e) m += offset ? src[e] + b : src[e];
      m *= invc;
      for (int e = 0; e < C; ++e) dst[e] = aug_blend(r.c, aug_blend(r.s, offset ? src[e] + b : src[e], m), M);
    }
  }
}

// dx = A^T g: g3[y, x, :] = g[y + ty, x + tx, :] inside the image and outside the rectangle (at the source position), else 0; then
// the contrast blend with M(g3) and the saturation blend with the pixel mean (both self-adjoint), which also reach the pixels whose g3 is 0.
template <int CT>
__global__ __launch_bounds__(kThreads) void aug_adj_kernel(const float* __restrict__ g, const float* __restrict__ P, int H, int W, int C,
                                                            FastDiv div_w, int policy, const float* __restrict__ part, int nblk,
                                                            float* __restrict__ dx) {
  const int n = blockIdx.y, HW = H * W;
  const AugRow r = aug_row(P, n, H, W, policy);
  const bool col = policy & T2I_DIFFAUG_COLOR;
  const float invc = 1.f / (float)C;
  float M = 0.f;
  if (col) M = aug_sample_total(part + (size_t)n * nblk, nblk) / ((float)HW * (float)C);
  const float* gs = g + (size_t)n * HW * C;
  float* ds = dx + (size_t)n * HW * C;
  for (int p = blockIdx.x * kThreads + threadIdx.x; p < HW; p += gridDim.x * kThreads) {
    const int yy = div_w.div(p), xx = p - yy * W;
    const int sy = yy + r.ty, sx = xx + r.tx;
    const bool live = aug_inside(sy, sx, H, W) && !aug_in_rect(r, sy, sx);
    const float* src = gs + ((size_t)(live ? sy : 0) * W + (live ? sx : 0)) * C;
    float* dst = ds + (size_t)p * C;
    if (CT > 0) {
      float v[CT > 0 ? CT : 1];
#pragma unroll
      for (int e = 0; e < CT; ++e) v[e] = live ? src[e] : 0.f;
      if (col) {
        float m = 0.f;
#pragma unroll
        for (int e = 0; e < CT; ++e) { v[e] = aug_blend(r.c, v[e], M); m += v[e]; }
        m *= invc;
#pragma unroll
        for (int e = 0; e < CT; ++e) v[e] = aug_blend(r.s, v[e], m);
      }
#pragma unroll
      for (int e = 0; e < CT; ++e) dst[e] = v[e];
    } else if (!col) {
      for (int e = 0; e < C; ++e) dst[e] = live ? src[e] : 0.f;
    } else {
      float m = 0.f;
      for (int e = 0; e < C; ++e) m += aug_blend(r.c, live ? src[e] : 0.f, M);
      m *= invc;
      for (int e = 0; e < C; ++e) dst[e] = aug_blend(r.s, aug_blend(r.c, live ? src[e] : 0.f, M), m);
    }
  }
}

inline int aug_nblk(int32_t H, int32_t W, int32_t C) { return (int)(((long long)H * W * C + kChunk - 1) / kChunk); }

// shapes, pointers and the policy mask; the output may not overlap the input (the kernels gather)
bool aug_args_ok(const char* what, const float* in, const float* P, const float* out, int32_t B, int32_t H, int32_t W, int32_t C, int32_t policy) {
  const int32_t all = T2I_DIFFAUG_COLOR | T2I_DIFFAUG_TRANSLATION | T2I_DIFFAUG_CUTOUT;
  if (!in || !P || !out || B <= 0 || B > 65535 || H <= 0 || W <= 0 || H > kMaxSide || W > kMaxSide || C <= 0 ||
      (long long)B * H * W > kMaxElems / C || policy <= 0 || (policy & ~all)) {
    set_error("%s: bad argument (a NULL tensor, B=%d %dx%dx%d policy=%d; 1 <= B <= 65535, 1 <= H, W <= %d, policy a non-empty mask of "
              "T2I_DIFFAUG_*)", what, B, H, W, C, policy, kMaxSide);
    return false;
  }
  const uintptr_t a = reinterpret_cast<uintptr_t>(in), o = reinterpret_cast<uintptr_t>(out);
  const size_t bytes = (size_t)B * H * W * C * sizeof(float);
  if ((a & 3) || (o & 3) || (reinterpret_cast<uintptr_t>(P) & 3) || (a < o + bytes && o < a + bytes)) {
    set_error("%s: bad argument (a tensor not aligned to 4 bytes, or the output overlaps the input)", what);
    return false;
  }
  return true;
}

bool aug_ws_ok(const char* what, const void* ws, size_t ws_bytes, size_t need) {
  if (need == 0) return true;
  if (!ws || ws_bytes < need || (reinterpret_cast<uintptr_t>(ws) & 3)) {
    set_error("%s: workspace missing, misaligned or too small (%zu bytes, %zu needed)", what, ws ? ws_bytes : (size_t)0, need);
    return false;
  }
  return true;
}

inline dim3 aug_grid(int32_t B, int32_t H, int32_t W) {
  const long long per_block = (long long)kThreads * kPixPerThread;
  return dim3((unsigned)(((long long)H * W + per_block - 1) / per_block), (unsigned)B);
}

// ---- the parameter table drawn on the device, and the controller of its probability p (include/t2i_hip.h: t2i_diffaug_state) ----------

// Philox4x32-10 (Salmon et al., "Parallel Random Numbers: As Easy as 1, 2, 3", SC 2011): counter (c0, c1, c2, c3), key (k0, k1).
struct Philox4 { uint32_t w[4]; };

__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// the top 24 bits as a float in [0, 1): the conversion and the scaling by a power of two are both exact
__device__ __forceinline__ float aug_u01(uint32_t w) { return (float)(w >> 8) * 5.9604644775390625e-8f; }
// a uniform integer in [0, m), m >= 1
__device__ __forceinline__ int aug_below(uint32_t w, int m) { return (int)(((uint64_t)w * (uint32_t)m) >> 32); }

// Row i of call k of the table: three Philox blocks (colour, translation, cutout) with the counter (i, block, k_lo, k_hi) and the
// state's seed as the key.  A transform is applied iff it is in the policy and u(word 0 of its block) < p; otherwise its columns
// are the identity's, which the apply kernels return their sample under bit for bit.  Each float below is one rounding of an exact
// value (no product feeds a sum), so there is nothing to contract and a restatement in numpy gives the same bits.  One workgroup:
// every thread reads words 0-4 before the barrier, thread 0 writes the advanced counter (words 2, 3, one 8-byte store) after it.
__global__ __launch_bounds__(kThreads) void aug_draw_kernel(uint32_t* __restrict__ state, int n, int H, int W, int policy,
                                                             float* __restrict__ P) {
  const uint32_t k0 = state[0], k1 = state[1], klo = state[2], khi = state[3];
  const float p = __uint_as_float(state[4]);
  const bool col = policy & T2I_DIFFAUG_COLOR, tr = policy & T2I_DIFFAUG_TRANSLATION, cut = policy & T2I_DIFFAUG_CUTOUT;
  const int rh = (H + 4) / 8, rw = (W + 4) / 8;                       // int(size / 8 + 0.5)
  const int eh = (H + 1) / 2, ew = (W + 1) / 2;                       // int(size / 2 + 0.5)
  for (int i = threadIdx.x; i < n; i += kThreads) {
    float b = 0.f, s = 1.f, c = 1.f;
    int ty = 0, tx = 0, y0 = 0, y1 = 0, x0 = 0, x1 = 0;
    if (col) {
      const Philox4 r = philox4x32_10((uint32_t)i, 0u, klo, khi, k0, k1);
      if (aug_u01(r.w[0]) < p) {
        b = aug_u01(r.w[1]) - 0.5f;
        s = 2.f * aug_u01(r.w[2]);
        c = aug_u01(r.w[3]) + 0.5f;
      }
    }
    if (tr) {
      const Philox4 r = philox4x32_10((uint32_t)i, 1u, klo, khi, k0, k1);
      if (aug_u01(r.w[0]) < p) {
        ty = aug_below(r.w[1], 2 * rh + 1) - rh;
        tx = aug_below(r.w[2], 2 * rw + 1) - rw;
      }
    }
    if (cut) {
      const Philox4 r = philox4x32_10((uint32_t)i, 2u, klo, khi, k0, k1);
      if (aug_u01(r.w[0]) < p) {
        const int oy = aug_below(r.w[1], H - eh % 2 + 1) - eh / 2, ox = aug_below(r.w[2], W - ew % 2 + 1) - ew / 2;
        y0 = max(oy, 0); y1 = min(oy + eh, H);
        x0 = max(ox, 0); x1 = min(ox + ew, W);
      }
    }
    float* row = P + (size_t)i * 9;
    row[0] = b; row[1] = s; row[2] = c;
    row[3] = (float)ty; row[4] = (float)tx;
    row[5] = (float)y0; row[6] = (float)y1; row[7] = (float)x0; row[8] = (float)x1;
  }
  __syncthreads();
  if (threadIdx.x == 0) *reinterpret_cast<uint64_t*>(state + 2) = (((uint64_t)khi << 32) | klo) + 1ull;
}

// The sum of v over the workgroup, the same bits in every thread: the wave butterfly, then the four waves added in a fixed order
// (as aug_partial_kernel).  `slot` is 4 floats of shared memory of the caller's; two calls need two slots or a barrier between.
__device__ __forceinline__ float aug_block_sum(float v, float* slot) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
  __syncthreads();
  return (slot[0] + slot[1]) + (slot[2] + slot[3]);
}

// The controller (Karras et al., "Training Generative Adversarial Networks with Limited Data", NeurIPS 2020, section 3): the statistic
// r = E[sign(d_real - theta)] accumulated over `interval` calls, then p moved by acc_n / ramp towards r = target.  theta = 0
// (T2I_ADA_LOGIT, the publication's r_t) or the midpoint of the two batch means (T2I_ADA_MIDPOINT).  One workgroup; every sum in
// a fixed order: thread t adds elements t, t + 256, ..., then aug_block_sum.  The signs are small integers, exact in fp32.  Thread 0
// alone writes words 4-9; words 0-3 and 10-15 are not touched.
__global__ __launch_bounds__(kThreads) void aug_observe_kernel(uint32_t* __restrict__ state, const float* __restrict__ d_real,
                                                                const float* __restrict__ d_fake, int n, int mode, float target,
                                                                int interval, float ramp) {
  __shared__ float slots[3][kThreads / 64];
  float theta = 0.f;
  if (mode == T2I_ADA_MIDPOINT) {
    float sr = 0.f, sf = 0.f;
    for (int i = threadIdx.x; i < n; i += kThreads) { sr += d_real[i]; sf += d_fake[i]; }
    sr = aug_block_sum(sr, slots[0]);
    sf = aug_block_sum(sf, slots[1]);
    theta = 0.5f * (sr / (float)n + sf / (float)n);
  }
  float sg = 0.f;
  for (int i = threadIdx.x; i < n; i += kThreads) {
    const float d = d_real[i] - theta;
    sg += d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
  }
  sg = aug_block_sum(sg, slots[2]);
  if (threadIdx.x != 0) return;
  float p = __uint_as_float(state[4]);
  float acc_sign = __uint_as_float(state[5]) + sg, acc_n = __uint_as_float(state[6]) + (float)n;
  uint32_t calls = state[7] + 1u;
  if (calls >= (uint32_t)interval) {
    const float r = acc_sign / acc_n;
    const float step = acc_n / ramp;
    p = r > target ? p + step : (r < target ? p - step : p);
    p = fminf(fmaxf(p, 0.f), 1.f);
    state[4] = __float_as_uint(p);
    state[8] = __float_as_uint(r);
    state[9] = state[9] + 1u;
    acc_sign = 0.f; acc_n = 0.f; calls = 0u;
  }
  state[5] = __float_as_uint(acc_sign);
  state[6] = __float_as_uint(acc_n);
  state[7] = calls;
}

}  // namespace
}  // namespace t2i

using namespace t2i;

size_t t2i_diff_augment_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t C, int32_t policy) {
  if (B <= 0 || B > 65535 || H <= 0 || W <= 0 || H > kMaxSide || W > kMaxSide || C <= 0 || (long long)B * H * W > kMaxElems / C) return 0;
  if (policy <= 0 || !(policy & T2I_DIFFAUG_COLOR)) return 0;
  return (size_t)B * (size_t)aug_nblk(H, W, C) * sizeof(float);
}

int t2i_diff_augment_fwd(const float* x, const float* params, int32_t B, int32_t H, int32_t W, int32_t C, int32_t policy, int32_t offset,
                         float* y, void* ws, size_t ws_bytes, t2i_stream_t stream) {
  if (!aug_args_ok("t2i_diff_augment_fwd", x, params, y, B, H, W, C, policy)) return T2I_ERR_INVALID;
  if (!aug_ws_ok("t2i_diff_augment_fwd", ws, ws_bytes, t2i_diff_augment_workspace_bytes(B, H, W, C, policy))) return T2I_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const int nblk = aug_nblk(H, W, C);
  float* part = reinterpret_cast<float*>(ws);
  FastDiv div_c, div_w;
  div_c.set((uint32_t)C);
  div_w.set((uint32_t)W);
  if (policy & T2I_DIFFAUG_COLOR)
    hipLaunchKernelGGL(aug_partial_kernel, dim3((unsigned)nblk, (unsigned)B), dim3(kThreads), 0, st, x, params, H, W, H * W * C, div_c, div_w,
                       policy, 0, nblk, part);
  const dim3 grid = aug_grid(B, H, W);
  offset = offset ? 1 : 0;
  if (C == 3) hipLaunchKernelGGL(aug_fwd_kernel<3>, grid, dim3(kThreads), 0, st, x, params, H, W, C, div_w, policy, offset, part, nblk, y);
  else if (C == 4) hipLaunchKernelGGL(aug_fwd_kernel<4>, grid, dim3(kThreads), 0, st, x, params, H, W, C, div_w, policy, offset, part, nblk, y);
  else hipLaunchKernelGGL(aug_fwd_kernel<0>, grid, dim3(kThreads), 0, st, x, params, H, W, C, div_w, policy, offset, part, nblk, y);
  return launched("t2i_diff_augment_fwd");
}

int t2i_diff_augment_adj(const float* g, const float* params, int32_t B, int32_t H, int32_t W, int32_t C, int32_t policy, float* dx,
                         void* ws, size_t ws_bytes, t2i_stream_t stream) {
  if (!aug_args_ok("t2i_diff_augment_adj", g, params, dx, B, H, W, C, policy)) return T2I_ERR_INVALID;
  if (!aug_ws_ok("t2i_diff_augment_adj", ws, ws_bytes, t2i_diff_augment_workspace_bytes(B, H, W, C, policy))) return T2I_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const int nblk = aug_nblk(H, W, C);
  float* part = reinterpret_cast<float*>(ws);
  FastDiv div_c, div_w;
  div_c.set((uint32_t)C);
  div_w.set((uint32_t)W);
  if (policy & T2I_DIFFAUG_COLOR)
    hipLaunchKernelGGL(aug_partial_kernel, dim3((unsigned)nblk, (unsigned)B), dim3(kThreads), 0, st, g, params, H, W, H * W * C, div_c, div_w,
                       policy, 1, nblk, part);
  const dim3 grid = aug_grid(B, H, W);
  if (C == 3) hipLaunchKernelGGL(aug_adj_kernel<3>, grid, dim3(kThreads), 0, st, g, params, H, W, C, div_w, policy, part, nblk, dx);
  else if (C == 4) hipLaunchKernelGGL(aug_adj_kernel<4>, grid, dim3(kThreads), 0, st, g, params, H, W, C, div_w, policy, part, nblk, dx);
  else hipLaunchKernelGGL(aug_adj_kernel<0>, grid, dim3(kThreads), 0, st, g, params, H, W, C, div_w, policy, part, nblk, dx);
  return launched("t2i_diff_augment_adj");
}

int t2i_diff_augment_draw(void* state, int32_t n, int32_t H, int32_t W, int32_t policy, float* params_out, t2i_stream_t stream) {
  const int32_t all = T2I_DIFFAUG_COLOR | T2I_DIFFAUG_TRANSLATION | T2I_DIFFAUG_CUTOUT;
  if (!state || !params_out || n < 1 || n > 65535 || H < 1 || W < 1 || H > kMaxSide || W > kMaxSide || policy <= 0 || (policy & ~all)) {
    set_error("t2i_diff_augment_draw: bad argument (a NULL state or table, n=%d %dx%d policy=%d; 1 <= n <= 65535, 1 <= H, W <= %d, policy a "
              "non-empty mask of T2I_DIFFAUG_*)", n, H, W, policy, kMaxSide);
    return T2I_ERR_INVALID;
  }
  if ((reinterpret_cast<uintptr_t>(state) & 15) || (reinterpret_cast<uintptr_t>(params_out) & 3)) {
    set_error("t2i_diff_augment_draw: bad argument (the state is not aligned to 16 bytes or the table not to 4)");
    return T2I_ERR_INVALID;
  }
  hipLaunchKernelGGL(aug_draw_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, reinterpret_cast<uint32_t*>(state), n, H, W, policy,
                     params_out);
  return launched("t2i_diff_augment_draw");
}

int t2i_diffaug_observe(void* state, const float* d_real, const float* d_fake, int32_t n, int32_t mode, float target, int32_t interval,
                        float ramp_images, t2i_stream_t stream) {
  if (mode != T2I_ADA_LOGIT && mode != T2I_ADA_MIDPOINT) {
    set_error("t2i_diffaug_observe: bad argument (mode=%d; T2I_ADA_LOGIT or T2I_ADA_MIDPOINT)", mode);
    return T2I_ERR_INVALID;
  }
  if (!state || !d_real || (!d_fake && mode != T2I_ADA_LOGIT) || n < 1 || n > 65535) {
    set_error("t2i_diffaug_observe: bad argument (a NULL state or d_real, a NULL d_fake under T2I_ADA_MIDPOINT, n=%d; 1 <= n <= 65535)", n);
    return T2I_ERR_INVALID;
  }
  if (interval < 1 || !(ramp_images > 0.f) || !isfinite(ramp_images) || !(target > -1.f && target < 1.f)) {
    set_error("t2i_diffaug_observe: bad argument (interval=%d ramp_images=%g target=%g; interval >= 1, ramp_images positive and finite, "
              "-1 < target < 1)", interval, (double)ramp_images, (double)target);
    return T2I_ERR_INVALID;
  }
  if ((reinterpret_cast<uintptr_t>(state) & 15) || (reinterpret_cast<uintptr_t>(d_real) & 3) || (reinterpret_cast<uintptr_t>(d_fake) & 3)) {
    set_error("t2i_diffaug_observe: bad argument (the state is not aligned to 16 bytes or a logit vector not to 4)");
    return T2I_ERR_INVALID;
  }
  hipLaunchKernelGGL(aug_observe_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, reinterpret_cast<uint32_t*>(state), d_real,
                     mode == T2I_ADA_MIDPOINT ? d_fake : d_real, n, mode, target, interval, ramp_images);
  return launched("t2i_diffaug_observe");
}
