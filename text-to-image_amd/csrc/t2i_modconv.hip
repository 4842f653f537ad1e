// t2i_modconv.hip — what a weight-demodulated convolution (Karras et al., "Analyzing and Improving the Image Quality of StyleGAN", CVPR 2020;
// not in the reference) needs around the convolution itself.  DESIGN.md section 4.45.
//
// With s [B,Cin] the style scales and W [T,Cin,Cout] the shared filter (T = kh kw taps), the layer
//
//   y[b] = conv(x[b], W s[b,:] d[b,:]),   d[b,o] = rsqrt(sum_{t,i} (W[t,i,o] s[b,i])^2 + eps)
//
// factorises exactly into  d[b,o] conv(x[b] s[b,:], W)[.,.,o],  and d itself into  rsqrt(sum_i s[b,i]^2 q[i,o] + eps),  q[i,o] = sum_t W[t,i,o]^2.
// The convolution kernels stay as they are (they see a scaled input and no bias); this unit holds the rest:
//
//   demod_q_kernel          q[i,o] = sum_t W[t,i,o]^2, t ascending, a thread per (i, o)
//   demod_d_kernel          per (b, 64 outputs): 4 lanes take every 4th input channel in ascending order (fmaf), merged 0..3 -> d [B,Cout]
//   demod_ds_kernel         per (b, 4 inputs): ds[b,i] = 2 s[b,i] sum_o q[i,o] e[b,o], e = -d^3 gd / 2 formed in place; 64 lanes take every
//                           64th output, merged 0..63
//   demod_dw_kernel         a thread per (i, o): dq = sum_b s[b,i]^2 e[b,o] (b ascending), dW[t,i,o] (+)= 2 W[t,i,o] dq for every tap
//   modulate_kernel<V>      xs[b,r,c] = x[b,r,c] s[b,c]       (with the cotangent in place of x: the adjoint for dx)
//   mod_scale_kernel<V>     per-item sums of g x over the item's rows -> workspace [B chunks][1][C]
//   demod_act_kernel<V>     out = act(p),  p = fmaf(strength[c], noise[b,r], fmaf(d[b,c], c[b,r,c], bias[c]))   (the outer fmaf only with noise)
//   demod_act_bwd_kernel<V> recomputes p by the same two fmaf; gp = act'(p) g; dc = gp d; per-item sums of gp c, gp, gp noise ->
//                           workspace [B chunks][3][C] (only the wanted components are written and read)
//   modconv_sum_kernel      fixed-order sums of such partials: job b < B: component 0 over the chunks of sample b -> [B,C]; job B: component
//                           1 over all B chunks partials -> [C]; job B + 1: component 2 likewise -> [C]
//
// and the backward of that backward (path-length regularisation differentiates the generator twice):
//
//   demod_act_bwd2_kernel<V> m = act'(p), p recomputed as above; gg = m (d vc + c vd), gc = m g vd, per-item sums of m g vc -> workspace
//                           [B chunks][1][C] (finished by modconv_sum_kernel -> gd [B,C]); every plane is read once
//   modulate2_kernel<V>     gg = s vx + x vs in one pass
//   demod_r_kernel          per (b, 64 outputs), demod_d_kernel's lanes: r = sum_i vs s q -> -d^3 r (to gd) and -3 d^2 gd r (to d)
//   demod_dw2_kernel        a thread per (i, o): dW[t,i,o] (+)= 4 W[t,i,o] sum_b vs[b,i] s[b,i] e[b,o], b ascending
//
// The tensor kernels use t2i_style.hip's item: (sample, chunk of 64 rows, tile of 64 channels), numbered tile-fastest, walked by a grid of at
// most 65535 workgroups of 256 threads with a stride; 16-byte accesses (V = 4) when C % 4 == 0 and the [B,R,C] tensors are 16-byte aligned,
// scalar ones otherwise.  No atomics; every sum's order depends on the shape alone and never on B, so a sample's results do not depend on its
// batch and calls repeat bit for bit; nothing is allocated, synchronised or read back: every launch can be captured.
#include <hip/hip_runtime.h>
#include <math.h>

#include "t2i_internal.h"

namespace t2i {
namespace {

constexpr int kThreads = 256;
constexpr int kChunk = T2I_MODCONV_CHUNK_ROWS;       // rows of a sample per item
constexpr int kTileC = 64;                           // channels per item
constexpr int kFinC = 16, kFinL = kThreads / kFinC;  // the finishing sums: channels per workgroup, lanes along the partials
constexpr int kDL = kThreads / kTileC;               // demod_d: lanes along the input channels (4)
constexpr int kDsRows = kThreads / 64;               // demod_ds: input channels per item (4), 64 lanes along the outputs each
constexpr int kMaxBlocks = 65535;
constexpr long long kMaxElems = 1ll << 31;

int launched(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return T2I_OK;
  set_error("%s: %s", what, hipGetErrorString(e));
  return T2I_ERR_LAUNCH;
}

template <int V> struct Lay {
  static constexpr int LX = kTileC / V, TY = kThreads / LX, RPT = kChunk / TY;      // V = 4: 16 x 16, 4 rows; V = 1: 64 x 4, 16 rows
};

struct ModParams {
  const float* x;          // x, or c of the epilogue
  const float* g;
  const float* s;          // modulate: [B,C] rows sstride apart; the epilogue: d [B,C] dense, or NULL (coefficient 1)
  const float* bias;       // [C] or NULL
  const float* noise;      // [B,R] or NULL
  const float* strength;   // [C] or NULL, with noise
  float* out;              // xs, out or dc (dc may be NULL)
  float* part;             // workspace partials
  const float* v;          // second order: the plane cotangent (vc of dc, vx of dx) or NULL
  const float* vrow;       // second order: the [B,C] cotangent (vd of dd, vs of ds), dense, or NULL
  float* out2;             // second order: gc or NULL
  long long R, items;
  int B, C, chunks, ctiles, act, sstride;
  int want_dd, want_dbias, want_dstrength;
  float alpha;
};

template <int V> __device__ __forceinline__ void load_v(const float* p, float (&v)[V]);
template <> __device__ __forceinline__ void load_v<4>(const float* p, float (&v)[4]) {
  const float4 t = *reinterpret_cast<const float4*>(p);
  v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
template <> __device__ __forceinline__ void load_v<1>(const float* p, float (&v)[1]) { v[0] = *p; }
template <int V> __device__ __forceinline__ void store_v(float* p, const float (&v)[V]);
template <> __device__ __forceinline__ void store_v<4>(float* p, const float (&v)[4]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
template <> __device__ __forceinline__ void store_v<1>(float* p, const float (&v)[1]) { *p = v[0]; }

// the pre-activation: the SAME fmaf sequence in the forward and in the backward (d = 1 and bias = 0 stand for the absent ones: exact)
__device__ __forceinline__ float pre_act(float c, float d, float bias, bool noisy, float s, float n) {
  const float p = fmaf(d, c, bias);
  return noisy ? fmaf(s, n, p) : p;
}
__device__ __forceinline__ float act_of(float p, int act, float alpha) {
  return act == T2I_ACT_NONE ? p : (p > 0.f ? p : (act == T2I_ACT_RELU ? 0.f : alpha * p));
}
__device__ __forceinline__ float dact_of(float p, int act, float alpha) {
  return act == T2I_ACT_NONE ? 1.f : (p > 0.f ? 1.f : (act == T2I_ACT_RELU ? 0.f : alpha));
}

struct Item { int b, ch, c0, nrows; long long row0; };

template <int V> __device__ __forceinline__ Item item_of(const ModParams& P, long long id, int tx) {
  Item it;
  const int ct = (int)(id % P.ctiles);
  const long long r = id / P.ctiles;
  it.ch = (int)(r % P.chunks);
  it.b = (int)(r / P.chunks);
  it.c0 = ct * kTileC + tx * V;
  const long long first = (long long)it.ch * kChunk;
  it.row0 = (long long)it.b * P.R + first;
  const long long left = P.R - first;
  it.nrows = left < kChunk ? (int)left : kChunk;
  return it;
}

// ---- the demodulation coefficients ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void demod_q_kernel(const float* W, int T, long long IO, float* q) {
  for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < IO; e += (long long)gridDim.x * kThreads) {
    float a = 0.f;
    for (int t = 0; t < T; ++t) { const float w = W[(size_t)t * IO + e]; a = fmaf(w, w, a); }
    q[e] = a;
  }
}

__global__ __launch_bounds__(kThreads) void demod_d_kernel(const float* q, const float* s, int sstride, int B, int Cin, int Cout, float eps,
                                                         float* d) {
  __shared__ float s_a[kDL][kTileC];
  const int tid = threadIdx.x, tx = tid % kTileC, ty = tid / kTileC;
  const int otiles = (Cout + kTileC - 1) / kTileC;
  const long long items = (long long)B * otiles;
  for (long long id = blockIdx.x; id < items; id += gridDim.x) {
    const int b = (int)(id / otiles), o = (int)(id % otiles) * kTileC + tx;
    float a = 0.f;
    if (o < Cout) {
      for (int i = ty; i < Cin; i += kDL) {
        const float sv = s[(size_t)b * sstride + i];
        a = fmaf(sv * sv, q[(size_t)i * Cout + o], a);
      }
    }
    s_a[ty][tx] = a;
    __syncthreads();
    if (ty == 0 && o < Cout) {
      a = 0.f;
      for (int t = 0; t < kDL; ++t) a += s_a[t][tx];
      d[(size_t)b * Cout + o] = rsqrtf(a + eps);
    }
    __syncthreads();
  }
}

__device__ __forceinline__ float e_of(float d, float gd) { return -0.5f * d * d * d * gd; }

__global__ __launch_bounds__(kThreads) void demod_ds_kernel(const float* gd, const float* d, const float* q, const float* s, int sstride, int B,
                                                          int Cin, int Cout, float* ds) {
  __shared__ float s_a[kDsRows][64];
  const int tid = threadIdx.x, tx = tid % 64, ty = tid / 64;
  const int groups = (Cin + kDsRows - 1) / kDsRows;
  const long long items = (long long)B * groups;
  for (long long id = blockIdx.x; id < items; id += gridDim.x) {
    const int b = (int)(id / groups), i = (int)(id % groups) * kDsRows + ty;
    float a = 0.f;
    if (i < Cin) {
      for (int o = tx; o < Cout; o += 64) a = fmaf(q[(size_t)i * Cout + o], e_of(d[(size_t)b * Cout + o], gd[(size_t)b * Cout + o]), a);
    }
    s_a[ty][tx] = a;
    __syncthreads();
    if (tx == 0 && i < Cin) {
      a = 0.f;
      for (int t = 0; t < 64; ++t) a += s_a[ty][t];
      ds[(size_t)b * Cin + i] = 2.0f * s[(size_t)b * sstride + i] * a;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kThreads) void demod_dw_kernel(const float* gd, const float* d, const float* s, int sstride, const float* W, int T,
                                                          int B, int Cin, int Cout, int accumulate, float* dW) {
  const long long IO = (long long)Cin * Cout;
  for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < IO; e += (long long)gridDim.x * kThreads) {
    const int i = (int)(e / Cout), o = (int)(e % Cout);
    float dq = 0.f;
    for (int b = 0; b < B; ++b) {
      const float sv = s[(size_t)b * sstride + i];
      dq = fmaf(sv * sv, e_of(d[(size_t)b * Cout + o], gd[(size_t)b * Cout + o]), dq);
    }
    dq *= 2.0f;
    for (int t = 0; t < T; ++t) {
      const float v = W[(size_t)t * IO + e] * dq;
      dW[(size_t)t * IO + e] = accumulate ? dW[(size_t)t * IO + e] + v : v;
    }
  }
}

// ---- the scale pass in front of the convolution ----------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(kThreads) void modulate_kernel(const ModParams P) {
  typedef Lay<V> L;
  const int tid = threadIdx.x, tx = tid % L::LX, ty = tid / L::LX;
  for (long long id = blockIdx.x; id < P.items; id += gridDim.x) {
    const Item it = item_of<V>(P, id, tx);
    if (it.c0 >= P.C) continue;                          // (V = 4: C % 4 == 0, so the four channels are inside together)
    float s[V];
#pragma unroll
    for (int j = 0; j < V; ++j) s[j] = P.s[(size_t)it.b * P.sstride + it.c0 + j];
#pragma unroll
    for (int k = 0; k < L::RPT; ++k) {
      const int lr = ty + k * L::TY;
      if (lr < it.nrows) {
        const long long row = it.row0 + lr;
        float v[V];
        load_v<V>(P.x + row * P.C + it.c0, v);
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] *= s[j];
        store_v<V>(P.out + row * P.C + it.c0, v);
      }
    }
  }
}

// the TY row lanes of an item's channel, summed in ascending order -> part[(b chunks + ch) ncomp + comp][c]
template <int TY>
__device__ __forceinline__ void item_sum(float (&lds)[TY][kTileC], int tid, int c, int C, float* out) {
  if (tid < kTileC && c < C) {
    float a = 0.f;
    for (int t = 0; t < TY; ++t) a += lds[t][tid];
    *out = a;
  }
}

template <int V>
__global__ __launch_bounds__(kThreads) void mod_scale_kernel(const ModParams P) {
  typedef Lay<V> L;
  __shared__ float s_a[L::TY][kTileC];
  const int tid = threadIdx.x, tx = tid % L::LX, ty = tid / L::LX;
  for (long long id = blockIdx.x; id < P.items; id += gridDim.x) {
    const Item it = item_of<V>(P, id, tx);
    float a[V];
#pragma unroll
    for (int j = 0; j < V; ++j) a[j] = 0.f;
    if (it.c0 < P.C) {
#pragma unroll
      for (int k = 0; k < L::RPT; ++k) {
        const int lr = ty + k * L::TY;
        if (lr < it.nrows) {
          const long long row = it.row0 + lr;
          float v[V], g[V];
          load_v<V>(P.x + row * P.C + it.c0, v);
          load_v<V>(P.g + row * P.C + it.c0, g);
#pragma unroll
          for (int j = 0; j < V; ++j) a[j] = fmaf(g[j], v[j], a[j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) s_a[ty][tx * V + j] = a[j];
    __syncthreads();
    const int c = it.c0 - tx * V + tid;                  // the tile's first channel + tid
    item_sum<L::TY>(s_a, tid, c, P.C, P.part + ((size_t)it.b * P.chunks + it.ch) * P.C + c);
    __syncthreads();                                     // the next item overwrites the LDS
  }
}

// ---- the epilogue behind the convolution -----------------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(kThreads) void demod_act_kernel(const ModParams P) {
  typedef Lay<V> L;
  const int tid = threadIdx.x, tx = tid % L::LX, ty = tid / L::LX;
  const bool noisy = P.noise != nullptr;
  for (long long id = blockIdx.x; id < P.items; id += gridDim.x) {
    const Item it = item_of<V>(P, id, tx);
    if (it.c0 >= P.C) continue;
    float d[V], bi[V], s[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int c = it.c0 + j;
      d[j] = P.s ? P.s[(size_t)it.b * P.C + c] : 1.0f;
      bi[j] = P.bias ? P.bias[c] : 0.f;
      s[j] = noisy ? P.strength[c] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < L::RPT; ++k) {
      const int lr = ty + k * L::TY;
      if (lr < it.nrows) {
        const long long row = it.row0 + lr;
        float v[V];
        load_v<V>(P.x + row * P.C + it.c0, v);
        const float nz = noisy ? P.noise[row] : 0.f;
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = act_of(pre_act(v[j], d[j], bi[j], noisy, s[j], nz), P.act, P.alpha);
        store_v<V>(P.out + row * P.C + it.c0, v);
      }
    }
  }
}

template <int V>
__global__ __launch_bounds__(kThreads) void demod_act_bwd_kernel(const ModParams P) {
  typedef Lay<V> L;
  __shared__ float s_a[L::TY][kTileC], s_b[L::TY][kTileC], s_n[L::TY][kTileC];
  const int tid = threadIdx.x, tx = tid % L::LX, ty = tid / L::LX;
  const bool noisy = P.noise != nullptr;
  for (long long id = blockIdx.x; id < P.items; id += gridDim.x) {
    const Item it = item_of<V>(P, id, tx);
    float sd[V], sb[V], sn[V];
#pragma unroll
    for (int j = 0; j < V; ++j) { sd[j] = 0.f; sb[j] = 0.f; sn[j] = 0.f; }
    if (it.c0 < P.C) {
      float d[V], bi[V], s[V];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const int c = it.c0 + j;
        d[j] = P.s ? P.s[(size_t)it.b * P.C + c] : 1.0f;
        bi[j] = P.bias ? P.bias[c] : 0.f;
        s[j] = noisy ? P.strength[c] : 0.f;
      }
#pragma unroll
      for (int k = 0; k < L::RPT; ++k) {
        const int lr = ty + k * L::TY;
        if (lr < it.nrows) {
          const long long row = it.row0 + lr;
          float v[V], g[V];
          load_v<V>(P.x + row * P.C + it.c0, v);
          load_v<V>(P.g + row * P.C + it.c0, g);
          const float nz = noisy ? P.noise[row] : 0.f;
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const float gp = dact_of(pre_act(v[j], d[j], bi[j], noisy, s[j], nz), P.act, P.alpha) * g[j];
            sd[j] = fmaf(gp, v[j], sd[j]);
            sb[j] += gp;
            sn[j] = fmaf(gp, nz, sn[j]);
            v[j] = gp * d[j];
          }
          if (P.out) store_v<V>(P.out + row * P.C + it.c0, v);
        }
      }
    }
    if (P.part) {                                        // (uniform over the launch, like the three wants)
#pragma unroll
      for (int j = 0; j < V; ++j) { s_a[ty][tx * V + j] = sd[j]; s_b[ty][tx * V + j] = sb[j]; s_n[ty][tx * V + j] = sn[j]; }
      __syncthreads();
      const int c = it.c0 - tx * V + tid;
      float* o = P.part + ((size_t)it.b * P.chunks + it.ch) * 3 * P.C + c;
      if (P.want_dd) item_sum<L::TY>(s_a, tid, c, P.C, o);
      if (P.want_dbias) item_sum<L::TY>(s_b, tid, c, P.C, o + P.C);
      if (P.want_dstrength) item_sum<L::TY>(s_n, tid, c, P.C, o + 2 * P.C);
      __syncthreads();
    }
  }
}

// part [B chunks][ncomp][C].  Job b < B: out_b[b,c] = sum over the chunks of sample b of component 0; job B: out_all1[c] = sum over all
// B chunks partials of component 1; job B + 1: out_all2[c] likewise of component 2.  A job whose output is NULL is skipped.  Lane ty owns the
// partials ty + kFinL k in four running sums (four loads in flight) joined in a fixed order; the kFinL lanes are then added in ascending order.
__global__ __launch_bounds__(kThreads) void modconv_sum_kernel(const float* part, int B, int chunks, int ncomp, int C, float* out_b,
                                                             float* out_all1, float* out_all2) {
  __shared__ float s_a[kFinL][kFinC];
  const int tid = threadIdx.x, tx = tid % kFinC, ty = tid / kFinC;
  const int ctiles = (C + kFinC - 1) / kFinC;
  const long long items = (long long)(B + 2) * ctiles;
  for (long long id = blockIdx.x; id < items; id += gridDim.x) {
    const int job = (int)(id / ctiles), c = (int)(id % ctiles) * kFinC + tx;
    float* out = job < B ? (out_b ? out_b + (size_t)job * C : nullptr) : (job == B ? out_all1 : out_all2);
    if (!out) continue;                                  // (uniform over the workgroup)
    const int comp = job < B ? 0 : job - B + 1;
    const int Pn = job < B ? chunks : B * chunks;
    const float* base = part + ((size_t)(job < B ? job : 0) * chunks * ncomp + comp) * C;
    const size_t one = (size_t)ncomp * C, step = (size_t)kFinL * one;
    float a = 0.f;
    if (c < C) {
      float a1 = 0.f, a2 = 0.f, a3 = 0.f;
      int p = ty;
      for (; p + 3 * kFinL < Pn; p += 4 * kFinL) {
        const float* q = base + (size_t)p * one + c;
        a += q[0]; a1 += q[step]; a2 += q[2 * step]; a3 += q[3 * step];
      }
      for (; p < Pn; p += kFinL) a += base[(size_t)p * one + c];
      a = (a + a1) + (a2 + a3);
    }
    s_a[ty][tx] = a;
    __syncthreads();
    if (ty == 0 && c < C) {
      a = 0.f;
      for (int t = 0; t < kFinL; ++t) a += s_a[t][tx];
      out[c] = a;
    }
    __syncthreads();
  }
}

// ---- the backward of the backward ------------------------------------------------------------------------------
// The epilogue: dc = m g d and dd = sum_r m g c are linear in g, c-and-d apart from m = act'(p), whose own derivative is zero almost
// everywhere.  Absent cotangents stand as zeros (exact: a product with 0 adds nothing), absent planes are not read.
template <int V>
__global__ __launch_bounds__(kThreads) void demod_act_bwd2_kernel(const ModParams P) {
  typedef Lay<V> L;
  __shared__ float s_a[L::TY][kTileC];
  const int tid = threadIdx.x, tx = tid % L::LX, ty = tid / L::LX;
  const bool noisy = P.noise != nullptr;
  for (long long id = blockIdx.x; id < P.items; id += gridDim.x) {
    const Item it = item_of<V>(P, id, tx);
    float sd[V];
#pragma unroll
    for (int j = 0; j < V; ++j) sd[j] = 0.f;
    if (it.c0 < P.C) {
      float d[V], bi[V], s[V], vd[V];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const int c = it.c0 + j;
        d[j] = P.s ? P.s[(size_t)it.b * P.C + c] : 1.0f;
        bi[j] = P.bias ? P.bias[c] : 0.f;
        s[j] = noisy ? P.strength[c] : 0.f;
        vd[j] = P.vrow ? P.vrow[(size_t)it.b * P.C + c] : 0.f;
      }
#pragma unroll
      for (int k = 0; k < L::RPT; ++k) {
        const int lr = ty + k * L::TY;
        if (lr < it.nrows) {
          const long long row = it.row0 + lr;
          float v[V], g[V], vc[V], gc[V];
          load_v<V>(P.x + row * P.C + it.c0, v);
          if (P.g) load_v<V>(P.g + row * P.C + it.c0, g);
          if (P.v) load_v<V>(P.v + row * P.C + it.c0, vc);
          const float nz = noisy ? P.noise[row] : 0.f;
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const float m = dact_of(pre_act(v[j], d[j], bi[j], noisy, s[j], nz), P.act, P.alpha);
            const float mg = P.g ? m * g[j] : 0.f;
            const float vcj = P.v ? vc[j] : 0.f;
            sd[j] = fmaf(mg, vcj, sd[j]);
            gc[j] = mg * vd[j];
            v[j] = m * fmaf(d[j], vcj, v[j] * vd[j]);
          }
          if (P.out) store_v<V>(P.out + row * P.C + it.c0, v);
          if (P.out2) store_v<V>(P.out2 + row * P.C + it.c0, gc);
        }
      }
    }
    if (P.part) {                                        // (uniform over the launch)
#pragma unroll
      for (int j = 0; j < V; ++j) s_a[ty][tx * V + j] = sd[j];
      __syncthreads();
      const int c = it.c0 - tx * V + tid;
      item_sum<L::TY>(s_a, tid, c, P.C, P.part + ((size_t)it.b * P.chunks + it.ch) * P.C + c);
      __syncthreads();
    }
  }
}

template <int V>
__global__ __launch_bounds__(kThreads) void modulate2_kernel(const ModParams P) {
  typedef Lay<V> L;
  const int tid = threadIdx.x, tx = tid % L::LX, ty = tid / L::LX;
  for (long long id = blockIdx.x; id < P.items; id += gridDim.x) {
    const Item it = item_of<V>(P, id, tx);
    if (it.c0 >= P.C) continue;
    float s[V], vs[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      s[j] = P.v ? P.s[(size_t)it.b * P.sstride + it.c0 + j] : 0.f;
      vs[j] = P.vrow ? P.vrow[(size_t)it.b * P.C + it.c0 + j] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < L::RPT; ++k) {
      const int lr = ty + k * L::TY;
      if (lr < it.nrows) {
        const long long row = it.row0 + lr;
        float x[V], vx[V];
        if (P.vrow) load_v<V>(P.x + row * P.C + it.c0, x);
        if (P.v) load_v<V>(P.v + row * P.C + it.c0, vx);
#pragma unroll
        for (int j = 0; j < V; ++j) x[j] = fmaf(s[j], P.v ? vx[j] : 0.f, (P.vrow ? x[j] : 0.f) * vs[j]);
        store_v<V>(P.out + row * P.C + it.c0, x);
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void demod_r_kernel(const float* vs, const float* s, int sstride, const float* q, const float* d,
                                                         const float* gd, int B, int Cin, int Cout, float* gg_d, float* gd_d) {
  __shared__ float s_a[kDL][kTileC];
  const int tid = threadIdx.x, tx = tid % kTileC, ty = tid / kTileC;
  const int otiles = (Cout + kTileC - 1) / kTileC;
  const long long items = (long long)B * otiles;
  for (long long id = blockIdx.x; id < items; id += gridDim.x) {
    const int b = (int)(id / otiles), o = (int)(id % otiles) * kTileC + tx;
    float a = 0.f;
    if (o < Cout) {
      for (int i = ty; i < Cin; i += kDL) a = fmaf(vs[(size_t)b * Cin + i] * s[(size_t)b * sstride + i], q[(size_t)i * Cout + o], a);
    }
    s_a[ty][tx] = a;
    __syncthreads();
    if (ty == 0 && o < Cout) {
      a = 0.f;
      for (int t = 0; t < kDL; ++t) a += s_a[t][tx];
      const float dv = d[(size_t)b * Cout + o], d2 = dv * dv;
      if (gg_d) gg_d[(size_t)b * Cout + o] = -(d2 * dv) * a;
      if (gd_d) gd_d[(size_t)b * Cout + o] = -3.0f * d2 * gd[(size_t)b * Cout + o] * a;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kThreads) void demod_dw2_kernel(const float* vs, const float* gd, const float* d, const float* s, int sstride,
                                                           const float* W, int T, int B, int Cin, int Cout, int accumulate, float* dW) {
  const long long IO = (long long)Cin * Cout;
  for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < IO; e += (long long)gridDim.x * kThreads) {
    const int i = (int)(e / Cout), o = (int)(e % Cout);
    float dq = 0.f;
    for (int b = 0; b < B; ++b)
      dq = fmaf(vs[(size_t)b * Cin + i] * s[(size_t)b * sstride + i], e_of(d[(size_t)b * Cout + o], gd[(size_t)b * Cout + o]), dq);
    dq *= 4.0f;
    for (int t = 0; t < T; ++t) {
      const float v = W[(size_t)t * IO + e] * dq;
      dW[(size_t)t * IO + e] = accumulate ? dW[(size_t)t * IO + e] + v : v;
    }
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + nb && b0 < a0 + na;
}

bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr) {
  return !((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15);
}

bool shape_ok(int32_t B, int64_t R, int32_t C) {
  return B >= 1 && R >= 1 && C >= 1 && R < kMaxElems && (long long)C * R < kMaxElems && (long long)C * R * B < kMaxElems;
}

// the checks of the [B,R,C] entries; fills the geometry of P
int geometry(const char* what, int32_t B, int64_t R, int32_t C, ModParams& P) {
  if (B < 1 || R < 1 || C < 1) {
    set_error("%s: bad argument (x [%d, %lld, %d]: every size must be at least 1)", what, (int)B, (long long)R, (int)C);
    return T2I_ERR_INVALID;
  }
  if (!shape_ok(B, R, C)) {
    set_error("%s: bad argument (x [%d, %lld, %d] has 2^31 elements or more)", what, (int)B, (long long)R, (int)C);
    return T2I_ERR_INVALID;
  }
  P.B = B; P.R = R; P.C = C; P.sstride = C;
  P.chunks = (int)((R + kChunk - 1) / kChunk);
  P.ctiles = (C + kTileC - 1) / kTileC;
  P.items = (long long)B * P.chunks * P.ctiles;          // at most one per element: < 2^31
  return T2I_OK;
}

int act_ok(const char* what, int act, float alpha, const float* noise, const float* strength, ModParams& P) {
  if (act != T2I_ACT_NONE && act != T2I_ACT_RELU && act != T2I_ACT_LRELU) {
    set_error("%s: bad argument (act %d: none, relu or lrelu)", what, act);
    return T2I_ERR_INVALID;
  }
  if (act == T2I_ACT_LRELU && !(alpha >= 0.f)) {
    set_error("%s: bad argument (lrelu slope %g: the derivative is read from the sign, which needs a slope >= 0)", what, (double)alpha);
    return T2I_ERR_INVALID;
  }
  if ((noise == nullptr) != (strength == nullptr)) {
    set_error("%s: bad argument (noise and strength come together or not at all)", what);
    return T2I_ERR_INVALID;
  }
  P.act = act; P.alpha = alpha; P.noise = noise; P.strength = strength;
  return T2I_OK;
}

int stride_ok(const char* what, int32_t style_stride, int32_t C, int32_t B) {
  if (style_stride < C) {
    set_error("%s: bad argument (style rows %d floats apart, below C = %d)", what, (int)style_stride, (int)C);
    return T2I_ERR_INVALID;
  }
  if ((long long)style_stride * B >= kMaxElems) {
    set_error("%s: bad argument (the style [%d rows, %d apart] spans 2^31 elements or more)", what, (int)B, (int)style_stride);
    return T2I_ERR_INVALID;
  }
  return T2I_OK;
}

int coef_shape_ok(const char* what, int32_t T, int32_t Cin, int32_t Cout, int32_t B, int32_t style_stride) {
  if (T < 1 || Cin < 1 || Cout < 1 || B < 1) {
    set_error("%s: bad argument (W [%d, %d, %d], B %d: every size must be at least 1)", what, (int)T, (int)Cin, (int)Cout, (int)B);
    return T2I_ERR_INVALID;
  }
  if ((long long)Cin * Cout >= kMaxElems || (long long)T * Cin * Cout >= kMaxElems || (long long)B * Cout >= kMaxElems) {
    set_error("%s: bad argument (W [%d, %d, %d] or d [%d, %d] has 2^31 elements or more)", what, (int)T, (int)Cin, (int)Cout, (int)B, (int)Cout);
    return T2I_ERR_INVALID;
  }
  return stride_ok(what, style_stride, Cin, B);
}

int workspace_ok(const char* what, const void* ws, size_t ws_bytes, size_t need) {
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 15) || ws_bytes < need) {
    set_error("%s: workspace is NULL, misaligned (16 bytes) or %zu bytes where %zu are needed", what, ws_bytes, need);
    return T2I_ERR_WORKSPACE;
  }
  return T2I_OK;
}

unsigned blocks_for(long long items) { return (unsigned)(items < kMaxBlocks ? items : kMaxBlocks); }

size_t partial_bytes(int32_t B, int64_t R, int32_t C, int ncomp) {
  if (!shape_ok(B, R, C)) return 0;
  const size_t chunks = (size_t)((R + kChunk - 1) / kChunk);
  return ((size_t)B * chunks * ncomp * (size_t)C * sizeof(float) + 255) & ~(size_t)255;
}

}  // namespace
}  // namespace t2i

using namespace t2i;

int32_t t2i_modconv_chunk_rows(void) { return kChunk; }

int t2i_demod_coef(const float* W, const float* s, int32_t style_stride, int32_t T, int32_t Cin, int32_t Cout, int32_t B, float eps, float* q,
                   float* d, t2i_stream_t stream) {
  const char* what = "t2i_demod_coef";
  if (!W || !s || !q || !d) { set_error("%s: bad argument (a NULL pointer)", what); return T2I_ERR_INVALID; }
  if (int rc = coef_shape_ok(what, T, Cin, Cout, B, style_stride)) return rc;
  if (!(eps >= 0.f) || !isfinite(eps)) { set_error("%s: bad argument (eps %g: finite and >= 0)", what, (double)eps); return T2I_ERR_INVALID; }
  const size_t wb = (size_t)T * Cin * Cout * 4, qb = (size_t)Cin * Cout * 4, db = (size_t)B * Cout * 4;
  const size_t sb = ((size_t)(B - 1) * style_stride + Cin) * 4;
  if (overlap(q, qb, W, wb) || overlap(q, qb, s, sb) || overlap(d, db, W, wb) || overlap(d, db, s, sb) || overlap(q, qb, d, db)) {
    set_error("%s: bad argument (q or d overlaps W, s or the other)", what);
    return T2I_ERR_INVALID;
  }
  const hipStream_t st = (hipStream_t)stream;
  const long long IO = (long long)Cin * Cout;
  hipLaunchKernelGGL(demod_q_kernel, dim3(blocks_for((IO + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, W, (int)T, IO, q);
  if (int rc = launched(what)) return rc;
  const long long items = (long long)B * ((Cout + kTileC - 1) / kTileC);
  hipLaunchKernelGGL(demod_d_kernel, dim3(blocks_for(items)), dim3(kThreads), 0, st, (const float*)q, s, (int)style_stride, (int)B, (int)Cin,
                     (int)Cout, eps, d);
  return launched(what);
}

int t2i_demod_coef_bwd(const float* gd, const float* d, const float* s, int32_t style_stride, const float* W, const float* q, int32_t T,
                       int32_t Cin, int32_t Cout, int32_t B, float* ds, float* dW, int32_t accumulate, t2i_stream_t stream) {
  const char* what = "t2i_demod_coef_bwd";
  if (!gd || !d || !s || (ds && !q) || (dW && !W)) { set_error("%s: bad argument (a NULL pointer)", what); return T2I_ERR_INVALID; }
  if (int rc = coef_shape_ok(what, T, Cin, Cout, B, style_stride)) return rc;
  const size_t wb = (size_t)T * Cin * Cout * 4, qb = (size_t)Cin * Cout * 4, db = (size_t)B * Cout * 4, dsb = (size_t)B * Cin * 4;
  const size_t sb = ((size_t)(B - 1) * style_stride + Cin) * 4;
  if ((ds && (overlap(ds, dsb, gd, db) || overlap(ds, dsb, d, db) || overlap(ds, dsb, s, sb) || overlap(ds, dsb, q, qb))) ||
      (dW && (overlap(dW, wb, gd, db) || overlap(dW, wb, d, db) || overlap(dW, wb, s, sb) || overlap(dW, wb, W, wb) ||
              (ds && overlap(dW, wb, ds, dsb)) || (q && overlap(dW, wb, q, qb))))) {
    set_error("%s: bad argument (ds or dW overlaps an input or the other)", what);
    return T2I_ERR_INVALID;
  }
  const hipStream_t st = (hipStream_t)stream;
  if (ds) {
    const long long items = (long long)B * ((Cin + kDsRows - 1) / kDsRows);
    hipLaunchKernelGGL(demod_ds_kernel, dim3(blocks_for(items)), dim3(kThreads), 0, st, gd, d, q, s, (int)style_stride, (int)B, (int)Cin,
                       (int)Cout, ds);
    if (int rc = launched(what)) return rc;
  }
  if (dW) {
    const long long IO = (long long)Cin * Cout;
    hipLaunchKernelGGL(demod_dw_kernel, dim3(blocks_for((IO + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, gd, d, s, (int)style_stride, W,
                       (int)T, (int)B, (int)Cin, (int)Cout, (int)accumulate, dW);
    if (int rc = launched(what)) return rc;
  }
  return T2I_OK;
}

int t2i_modulate(const float* x, const float* s, int32_t style_stride, int32_t B, int64_t R, int32_t C, float* xs, t2i_stream_t stream) {
  const char* what = "t2i_modulate";
  if (!x || !s || !xs) { set_error("%s: bad argument (a NULL pointer)", what); return T2I_ERR_INVALID; }
  ModParams P = {};
  if (int rc = geometry(what, B, R, C, P)) return rc;
  if (int rc = stride_ok(what, style_stride, C, B)) return rc;
  const size_t bytes = (size_t)B * (size_t)R * (size_t)C * 4;
  if (overlap(x, bytes, xs, bytes) || overlap(s, ((size_t)(B - 1) * style_stride + C) * 4, xs, bytes)) {
    set_error("%s: bad argument (xs overlaps x or s)", what);
    return T2I_ERR_INVALID;
  }
  P.x = x; P.s = s; P.sstride = style_stride; P.out = xs;
  const hipStream_t st = (hipStream_t)stream;
  if (C % 4 == 0 && aligned16(x, xs)) hipLaunchKernelGGL((modulate_kernel<4>), dim3(blocks_for(P.items)), dim3(kThreads), 0, st, P);
  else hipLaunchKernelGGL((modulate_kernel<1>), dim3(blocks_for(P.items)), dim3(kThreads), 0, st, P);
  return launched(what);
}

size_t t2i_modulate_bwd_scale_workspace_bytes(int32_t B, int64_t R, int32_t C) { return partial_bytes(B, R, C, 1); }

int t2i_modulate_bwd_scale(const float* g, const float* x, int32_t B, int64_t R, int32_t C, float* ds, void* ws, size_t ws_bytes,
                           t2i_stream_t stream) {
  const char* what = "t2i_modulate_bwd_scale";
  if (!g || !x || !ds) { set_error("%s: bad argument (a NULL pointer)", what); return T2I_ERR_INVALID; }
  ModParams P = {};
  if (int rc = geometry(what, B, R, C, P)) return rc;
  const size_t bytes = (size_t)B * (size_t)R * (size_t)C * 4;
  if (overlap(ds, (size_t)B * C * 4, g, bytes) || overlap(ds, (size_t)B * C * 4, x, bytes)) {
    set_error("%s: bad argument (ds overlaps g or x)", what);
    return T2I_ERR_INVALID;
  }
  if (int rc = workspace_ok(what, ws, ws_bytes, partial_bytes(B, R, C, 1))) return rc;
  P.x = x; P.g = g; P.part = static_cast<float*>(ws);
  const hipStream_t st = (hipStream_t)stream;
  if (C % 4 == 0 && aligned16(x, g)) hipLaunchKernelGGL((mod_scale_kernel<4>), dim3(blocks_for(P.items)), dim3(kThreads), 0, st, P);
  else hipLaunchKernelGGL((mod_scale_kernel<1>), dim3(blocks_for(P.items)), dim3(kThreads), 0, st, P);
  if (int rc = launched(what)) return rc;
  const long long fin = (long long)(B + 2) * ((C + kFinC - 1) / kFinC);
  hipLaunchKernelGGL(modconv_sum_kernel, dim3(blocks_for(fin)), dim3(kThreads), 0, st, (const float*)P.part, (int)B, P.chunks, 1, (int)C, ds,
                     static_cast<float*>(nullptr), static_cast<float*>(nullptr));
  return launched(what);
}

int t2i_demod_act(const float* c, const float* d, const float* bias, const float* noise, const float* strength, int32_t B, int64_t R, int32_t C,
                  int act, float alpha, float* out, t2i_stream_t stream) {
  const char* what = "t2i_demod_act";
  if (!c || !out) { set_error("%s: bad argument (a NULL pointer)", what); return T2I_ERR_INVALID; }
  ModParams P = {};
  if (int rc = geometry(what, B, R, C, P)) return rc;
  if (int rc = act_ok(what, act, alpha, noise, strength, P)) return rc;
  const size_t bytes = (size_t)B * (size_t)R * (size_t)C * 4;
  if (overlap(c, bytes, out, bytes) || (d && overlap(d, (size_t)B * C * 4, out, bytes)) || (bias && overlap(bias, (size_t)C * 4, out, bytes)) ||
      (noise && (overlap(noise, (size_t)B * R * 4, out, bytes) || overlap(strength, (size_t)C * 4, out, bytes)))) {
    set_error("%s: bad argument (out overlaps an input)", what);
    return T2I_ERR_INVALID;
  }
  P.x = c; P.s = d; P.bias = bias; P.out = out;
  const hipStream_t st = (hipStream_t)stream;
  if (C % 4 == 0 && aligned16(c, out)) hipLaunchKernelGGL((demod_act_kernel<4>), dim3(blocks_for(P.items)), dim3(kThreads), 0, st, P);
  else hipLaunchKernelGGL((demod_act_kernel<1>), dim3(blocks_for(P.items)), dim3(kThreads), 0, st, P);
  return launched(what);
}

size_t t2i_demod_act_bwd_workspace_bytes(int32_t B, int64_t R, int32_t C) { return partial_bytes(B, R, C, 3); }

int t2i_demod_act_bwd(const float* g, const float* c, const float* d, const float* bias, const float* noise, const float* strength, int32_t B,
                      int64_t R, int32_t C, int act, float alpha, float* dc, float* dd, float* dbias, float* dstrength, void* ws,
                      size_t ws_bytes, t2i_stream_t stream) {
  const char* what = "t2i_demod_act_bwd";
  if (!g || !c) { set_error("%s: bad argument (a NULL pointer)", what); return T2I_ERR_INVALID; }
  if (!dc && !dd && !dbias && !dstrength) { set_error("%s: bad argument (no output is wanted)", what); return T2I_ERR_INVALID; }
  ModParams P = {};
  if (int rc = geometry(what, B, R, C, P)) return rc;
  if (int rc = act_ok(what, act, alpha, noise, strength, P)) return rc;
  if (dstrength && !noise) { set_error("%s: bad argument (dstrength without noise)", what); return T2I_ERR_INVALID; }
  if (dd && !d) { set_error("%s: bad argument (dd without d)", what); return T2I_ERR_INVALID; }
  const size_t bytes = (size_t)B * (size_t)R * (size_t)C * 4;
  const float* ins[6] = {g, c, d, bias, noise, strength};
  const size_t inb[6] = {bytes, bytes, (size_t)B * C * 4, (size_t)C * 4, (size_t)B * R * 4, (size_t)C * 4};
  float* outs[4] = {dc, dd, dbias, dstrength};
  const size_t outb[4] = {bytes, (size_t)B * C * 4, (size_t)C * 4, (size_t)C * 4};
  for (int o = 0; o < 4; ++o) {
    if (!outs[o]) continue;
    for (int i = 0; i < 6; ++i)
      if (ins[i] && overlap(outs[o], outb[o], ins[i], inb[i])) { set_error("%s: bad argument (an output overlaps an input)", what); return T2I_ERR_INVALID; }
    for (int p = 0; p < o; ++p)
      if (outs[p] && overlap(outs[o], outb[o], outs[p], outb[p])) { set_error("%s: bad argument (two outputs overlap)", what); return T2I_ERR_INVALID; }
  }
  const bool sums = dd || dbias || dstrength;
  if (sums)
    if (int rc = workspace_ok(what, ws, ws_bytes, partial_bytes(B, R, C, 3))) return rc;
  P.x = c; P.g = g; P.s = d; P.bias = bias; P.out = dc;
  P.part = sums ? static_cast<float*>(ws) : nullptr;
  P.want_dd = dd != nullptr; P.want_dbias = dbias != nullptr; P.want_dstrength = dstrength != nullptr;
  const hipStream_t st = (hipStream_t)stream;
  if (C % 4 == 0 && aligned16(c, g, dc)) hipLaunchKernelGGL((demod_act_bwd_kernel<4>), dim3(blocks_for(P.items)), dim3(kThreads), 0, st, P);
  else hipLaunchKernelGGL((demod_act_bwd_kernel<1>), dim3(blocks_for(P.items)), dim3(kThreads), 0, st, P);
  if (int rc = launched(what)) return rc;
  if (!sums) return T2I_OK;
  const long long fin = (long long)(B + 2) * ((C + kFinC - 1) / kFinC);
  hipLaunchKernelGGL(modconv_sum_kernel, dim3(blocks_for(fin)), dim3(kThreads), 0, st, (const float*)P.part, (int)B, P.chunks, 3, (int)C, dd, dbias,
                     dstrength);
  return launched(what);
}

size_t t2i_demod_act_bwd2_workspace_bytes(int32_t B, int64_t R, int32_t C) { return partial_bytes(B, R, C, 1); }

int t2i_demod_act_bwd2(const float* g, const float* c, const float* d, const float* bias, const float* noise, const float* strength,
                       const float* vc, const float* vd, int32_t B, int64_t R, int32_t C, int act, float alpha, float* gg, float* gc, float* gd,
                       void* ws, size_t ws_bytes, t2i_stream_t stream) {
  const char* what = "t2i_demod_act_bwd2";
  if (!c) { set_error("%s: bad argument (a NULL pointer)", what); return T2I_ERR_INVALID; }
  if (!vc && !vd) { set_error("%s: bad argument (no cotangent: vc and vd are both NULL)", what); return T2I_ERR_INVALID; }
  if (!gg && !gc && !gd) { set_error("%s: bad argument (no output is wanted)", what); return T2I_ERR_INVALID; }
  ModParams P = {};
  if (int rc = geometry(what, B, R, C, P)) return rc;
  if (int rc = act_ok(what, act, alpha, noise, strength, P)) return rc;
  if (vd && !d) { set_error("%s: bad argument (vd without d: the coefficient 1 has no gradient)", what); return T2I_ERR_INVALID; }
  if (gc && !vd) { set_error("%s: bad argument (gc without vd)", what); return T2I_ERR_INVALID; }
  if (gd && (!vc || !d)) { set_error("%s: bad argument (gd without vc or without d)", what); return T2I_ERR_INVALID; }
  if ((gc || gd) && !g) { set_error("%s: bad argument (gc or gd without g)", what); return T2I_ERR_INVALID; }
  const size_t bytes = (size_t)B * (size_t)R * (size_t)C * 4, rowb = (size_t)B * C * 4;
  const float* ins[8] = {g, c, d, bias, noise, strength, vc, vd};
  const size_t inb[8] = {bytes, bytes, rowb, (size_t)C * 4, (size_t)B * R * 4, (size_t)C * 4, bytes, rowb};
  float* outs[3] = {gg, gc, gd};
  const size_t outb[3] = {bytes, bytes, rowb};
  for (int o = 0; o < 3; ++o) {
    if (!outs[o]) continue;
    for (int i = 0; i < 8; ++i)
      if (ins[i] && overlap(outs[o], outb[o], ins[i], inb[i])) { set_error("%s: bad argument (an output overlaps an input)", what); return T2I_ERR_INVALID; }
    for (int p = 0; p < o; ++p)
      if (outs[p] && overlap(outs[o], outb[o], outs[p], outb[p])) { set_error("%s: bad argument (two outputs overlap)", what); return T2I_ERR_INVALID; }
  }
  if (gd)
    if (int rc = workspace_ok(what, ws, ws_bytes, partial_bytes(B, R, C, 1))) return rc;
  P.x = c; P.g = (gc || gd) ? g : nullptr; P.s = d; P.bias = bias; P.v = vc; P.vrow = vd; P.out = gg; P.out2 = gc;
  P.part = gd ? static_cast<float*>(ws) : nullptr;
  const hipStream_t st = (hipStream_t)stream;
  if (C % 4 == 0 && aligned16(c, P.g, vc) && aligned16(gg, gc))
    hipLaunchKernelGGL((demod_act_bwd2_kernel<4>), dim3(blocks_for(P.items)), dim3(kThreads), 0, st, P);
  else hipLaunchKernelGGL((demod_act_bwd2_kernel<1>), dim3(blocks_for(P.items)), dim3(kThreads), 0, st, P);
  if (int rc = launched(what)) return rc;
  if (!gd) return T2I_OK;
  const long long fin = (long long)(B + 2) * ((C + kFinC - 1) / kFinC);
  hipLaunchKernelGGL(modconv_sum_kernel, dim3(blocks_for(fin)), dim3(kThreads), 0, st, (const float*)P.part, (int)B, P.chunks, 1, (int)C, gd,
                     static_cast<float*>(nullptr), static_cast<float*>(nullptr));
  return launched(what);
}

int t2i_modulate2(const float* s, int32_t style_stride, const float* vx, const float* x, const float* vs, int32_t B, int64_t R, int32_t C,
                  float* gg, t2i_stream_t stream) {
  const char* what = "t2i_modulate2";
  if (!gg) { set_error("%s: bad argument (a NULL pointer)", what); return T2I_ERR_INVALID; }
  if (!vx && !vs) { set_error("%s: bad argument (no cotangent: vx and vs are both NULL)", what); return T2I_ERR_INVALID; }
  if ((vx && !s) || (vs && !x)) { set_error("%s: bad argument (vx comes with s, vs with x)", what); return T2I_ERR_INVALID; }
  ModParams P = {};
  if (int rc = geometry(what, B, R, C, P)) return rc;
  if (vx)
    if (int rc = stride_ok(what, style_stride, C, B)) return rc;
  const size_t bytes = (size_t)B * (size_t)R * (size_t)C * 4;
  if ((vx && (overlap(vx, bytes, gg, bytes) || overlap(s, ((size_t)(B - 1) * style_stride + C) * 4, gg, bytes))) ||
      (vs && (overlap(x, bytes, gg, bytes) || overlap(vs, (size_t)B * C * 4, gg, bytes)))) {
    set_error("%s: bad argument (gg overlaps an input)", what);
    return T2I_ERR_INVALID;
  }
  P.s = s; P.sstride = vx ? style_stride : C; P.v = vx; P.x = vs ? x : nullptr; P.vrow = vs; P.out = gg;
  const hipStream_t st = (hipStream_t)stream;
  if (C % 4 == 0 && aligned16(P.x, vx, gg)) hipLaunchKernelGGL((modulate2_kernel<4>), dim3(blocks_for(P.items)), dim3(kThreads), 0, st, P);
  else hipLaunchKernelGGL((modulate2_kernel<1>), dim3(blocks_for(P.items)), dim3(kThreads), 0, st, P);
  return launched(what);
}

int t2i_demod_coef_bwd2(const float* vs, const float* gd, const float* d, const float* s, int32_t style_stride, const float* W, const float* q,
                        int32_t T, int32_t Cin, int32_t Cout, int32_t B, float* gg_d, float* gd_d, float* dW, int32_t accumulate,
                        t2i_stream_t stream) {
  const char* what = "t2i_demod_coef_bwd2";
  if (!vs || !gd || !d || !s || ((gg_d || gd_d) && !q) || (dW && !W)) { set_error("%s: bad argument (a NULL pointer)", what); return T2I_ERR_INVALID; }
  if (!gg_d && !gd_d && !dW) { set_error("%s: bad argument (no output is wanted)", what); return T2I_ERR_INVALID; }
  if (int rc = coef_shape_ok(what, T, Cin, Cout, B, style_stride)) return rc;
  if ((long long)B * Cin >= kMaxElems) { set_error("%s: bad argument (vs [%d, %d] has 2^31 elements or more)", what, (int)B, (int)Cin); return T2I_ERR_INVALID; }
  const size_t wb = (size_t)T * Cin * Cout * 4, qb = (size_t)Cin * Cout * 4, db = (size_t)B * Cout * 4, vb = (size_t)B * Cin * 4;
  const size_t sb = ((size_t)(B - 1) * style_stride + Cin) * 4;
  const float* ins[6] = {vs, gd, d, s, W, q};
  const size_t inb[6] = {vb, db, db, sb, wb, qb};
  float* outs[3] = {gg_d, gd_d, dW};
  const size_t outb[3] = {db, db, wb};
  for (int o = 0; o < 3; ++o) {
    if (!outs[o]) continue;
    for (int i = 0; i < 6; ++i)
      if (ins[i] && overlap(outs[o], outb[o], ins[i], inb[i])) { set_error("%s: bad argument (an output overlaps an input)", what); return T2I_ERR_INVALID; }
    for (int p = 0; p < o; ++p)
      if (outs[p] && overlap(outs[o], outb[o], outs[p], outb[p])) { set_error("%s: bad argument (two outputs overlap)", what); return T2I_ERR_INVALID; }
  }
  const hipStream_t st = (hipStream_t)stream;
  if (gg_d || gd_d) {
    const long long items = (long long)B * ((Cout + kTileC - 1) / kTileC);
    hipLaunchKernelGGL(demod_r_kernel, dim3(blocks_for(items)), dim3(kThreads), 0, st, vs, s, (int)style_stride, q, d, gd, (int)B, (int)Cin,
                       (int)Cout, gg_d, gd_d);
    if (int rc = launched(what)) return rc;
  }
  if (dW) {
    const long long IO = (long long)Cin * Cout;
    hipLaunchKernelGGL(demod_dw2_kernel, dim3(blocks_for((IO + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, vs, gd, d, s,
                       (int)style_stride, W, (int)T, (int)B, (int)Cin, (int)Cout, (int)accumulate, dW);
    if (int rc = launched(what)) return rc;
  }
  return T2I_OK;
}
