// t2i_incep_train.hip — the kernels of InceptionV3's fine-tuning step that are not convolutions or batch norms (reference
// models/inception/trainer.py: slim inception_v3(is_training=True) on the test split, loss = mean sparse softmax
// cross-entropy, RMSPropOptimizer(5e-5) over Mixed_7c + Logits):
//
//   pool_dropout_kernel     AvgPool_1a_8x8 of the Mixed_7c output [B, HW, D] -> PreLogits [B, D], then Dropout_1b:
//                           y = pre / keep * floor(keep + U) with U from Philox4x32-10 keyed by (seed, step) and counted by
//                           the element index, so a mask is a pure function of (seed, step, b, d).  The 0/1 mask is written
//                           out for the backward (and for tests).
//   head_fwd_kernel         one workgroup per row: logits = y W + b, softmax, the row's cross-entropy, whether argmax(softmax)
//                           (first maximum) hits the label, and dlogits = (softmax - onehot) / B.
//   head_bwd_kernel         one thread per PreLogits channel k: dW[k, :] = y[:, k]^T dlogits, dy[:, k] = dlogits W[k, :]^T;
//                           workgroup 0 also forms db and the batch means of loss and accuracy.  Every sum has one owner and
//                           a fixed order: no atomics, bitwise-repeatable.
//   pooled_grad_kernel      d(Mixed_7c branch outputs) from the PreLogits gradient: mask / keep * g / HW broadcast over the
//                           HW pixels, written straight into each branch's contiguous [B, HW, C_branch] tensor.
//   rmsprop_tf_kernel       tf.train.RMSPropOptimizer's ApplyRMSProp over a flat arena.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "t2i_internal.h"

namespace t2i {

namespace {

constexpr int kThreads = 256;
constexpr int kMaxScatterBranches = T2I_MAX_SCATTER_BRANCHES;

// One thread per 4 consecutive (b, d) elements (D % 4 == 0): the four uniforms of one Philox call (philox4x32_10: t2i_internal.h).
__global__ __launch_bounds__(kThreads) void pool_dropout_kernel(const float* __restrict__ x, int B, int HW, int D, float keep,
                                                                unsigned long long seed, unsigned long long step,
                                                                float* __restrict__ pre, float* __restrict__ mask,
                                                                float* __restrict__ y) {
#pragma clang fp contract(off)
  const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int64_t quads = (int64_t)B * D / 4;
  if (q >= quads) return;
  const int64_t i0 = q * 4;
  const int64_t b = i0 / D;
  const int d0 = (int)(i0 - b * D);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  const float* xb = x + b * (int64_t)HW * D + d0;
  for (int p = 0; p < HW; ++p) {                  // row-major taps, fp32 sum, then / count: t2i_pool2d's AVG arithmetic
    const float4 v = *reinterpret_cast<const float4*>(xb + (int64_t)p * D);
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  const float n = (float)HW;
  const float pv[4] = {acc.x / n, acc.y / n, acc.z / n, acc.w / n};
  unsigned r[4];
  philox4x32_10((unsigned)q, (unsigned)((unsigned long long)q >> 32), (unsigned)step, (unsigned)(step >> 32), (unsigned)seed,
                (unsigned)(seed >> 32), r);
  float mv[4], yv[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float u = (float)(r[e] >> 8) * (1.0f / 16777216.0f);        // [0, 1), 24 bits
    mv[e] = floorf(keep + u);                                          // tf.nn.dropout: floor(keep_prob + U)
    yv[e] = pv[e] / keep * mv[e];                                      // x / keep_prob * binary
  }
  *reinterpret_cast<float4*>(pre + i0) = make_float4(pv[0], pv[1], pv[2], pv[3]);
  *reinterpret_cast<float4*>(mask + i0) = make_float4(mv[0], mv[1], mv[2], mv[3]);
  *reinterpret_cast<float4*>(y + i0) = make_float4(yv[0], yv[1], yv[2], yv[3]);
}

// Workgroup b: row b of the head.  Each wavefront owns classes w, w + 4, ...; its 64 lanes split the D-long dot product and
// reduce by a fixed butterfly.  Row statistics on lane 0 of wavefront 0, classes in order.
// ws: dz [B, C] then rowloss [B], correct [B].
__global__ __launch_bounds__(kThreads) void head_fwd_kernel(const float* __restrict__ y, const float* __restrict__ W,
                                                            const float* __restrict__ bias, const int32_t* __restrict__ labels,
                                                            int B, int D, int C, float* __restrict__ logits,
                                                            float* __restrict__ prob, float* __restrict__ ws) {
  extern __shared__ float sm[];                   // y row [D], then logits [C]
  float* yr = sm;
  float* lg = sm + D;
  const int b = blockIdx.x;
  for (int k = threadIdx.x; k < D; k += kThreads) yr[k] = y[(int64_t)b * D + k];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c = wave; c < C; c += kThreads / 64) {
    float s = 0.f;
    for (int k = lane; k < D; k += 64) s = fmaf(yr[k], W[(int64_t)k * C + c], s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) lg[c] = s + bias[c];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float m = lg[0];
    for (int c = 1; c < C; ++c) m = fmaxf(m, lg[c]);
    const int lab = labels[b];
    int top = 0;
    while (top < C - 1 && lg[top] != m) ++top;                 // the first class at the maximum: its term of se is exactly 1
    // se = 1 + rest and prob[lab] - 1 = -others / se.  A confident row has se = 1 + (something far below 1): log(se) and
    // prob[lab] - 1 formed from the rounded se are good to eps absolutely, which is no relative accuracy at all in a loss or a
    // gradient of 1e-6; formed from the sums that leave the 1 out they are good relatively.
    float se = 0.f, rest = 0.f, others = 0.f;
    for (int c = 0; c < C; ++c) {
      const float e = expf(lg[c] - m);
      se += e;
      if (c != top) rest += e;
      if (c != lab) others += e;
    }
    float* dz = ws;
    float* rowloss = ws + (int64_t)B * C;
    float* correct = rowloss + B;
    int arg = 0;
    float best = -1.f;
    for (int c = 0; c < C; ++c) {
      const float p = expf(lg[c] - m) / se;
      logits[(int64_t)b * C + c] = lg[c];
      prob[(int64_t)b * C + c] = p;
      if (p > best) { best = p; arg = c; }                     // first maximum
      dz[(int64_t)b * C + c] = (c == lab ? -(others / se) : p) / (float)B;
    }
    rowloss[b] = log1pf(rest) - (lg[lab] - m);
    correct[b] = arg == lab ? 1.f : 0.f;
  }
}

// dz staged in LDS [B, C]; thread k owns column k of y / row k of W.
__global__ __launch_bounds__(kThreads) void head_bwd_kernel(const float* __restrict__ y, const float* __restrict__ W,
                                                            const float* __restrict__ ws, int B, int D, int C, float* __restrict__ dW,
                                                            int accumulate, float* __restrict__ db, float* __restrict__ dy,
                                                            float* __restrict__ loss, float* __restrict__ acc) {
  extern __shared__ float dz[];
  const int n = B * C;
  for (int i = threadIdx.x; i < n; i += kThreads) dz[i] = ws[i];
  __syncthreads();
  const int k = blockIdx.x * kThreads + threadIdx.x;
  if (k < D) {
    const float* wk = W + (int64_t)k * C;
    for (int b = 0; b < B; ++b) {
      float s = 0.f;
      for (int c = 0; c < C; ++c) s = fmaf(dz[b * C + c], wk[c], s);
      dy[(int64_t)b * D + k] = s;
    }
    for (int c = 0; c < C; ++c) {
      float s = 0.f;
      for (int b = 0; b < B; ++b) s = fmaf(y[(int64_t)b * D + k], dz[b * C + c], s);
      float* o = dW + (int64_t)k * C + c;
      *o = accumulate ? *o + s : s;
    }
  }
  if (blockIdx.x == 0) {
    for (int c = threadIdx.x; c < C; c += kThreads) {
      float s = 0.f;
      for (int b = 0; b < B; ++b) s += dz[b * C + c];
      db[c] = accumulate ? db[c] + s : s;
    }
    if (threadIdx.x == 0) {
      const float* rowloss = ws + n;
      const float* correct = rowloss + B;
      float l = 0.f, a = 0.f;
      for (int b = 0; b < B; ++b) { l += rowloss[b]; a += correct[b]; }
      *loss = l / (float)B;
      *acc = a / (float)B;
    }
  }
}

struct ScatterTable {
  float* out[kMaxScatterBranches];
  int32_t c0[kMaxScatterBranches];
  int32_t C[kMaxScatterBranches];
};

// grid.y = branch; one thread per 4 channels of one output pixel (every C_branch % 4 == 0, c0 % 4 == 0).
__global__ __launch_bounds__(kThreads) void pooled_grad_kernel(const float* __restrict__ g, const float* __restrict__ mask, int B, int HW,
                                                               int D, float keep, ScatterTable t) {
#pragma clang fp contract(off)
  const int br = blockIdx.y;
  const int Cb = t.C[br];
  const int CV = Cb / 4;
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= (int64_t)B * HW * CV) return;
  const int cv = (int)(idx % CV);
  const int64_t pix = idx / CV;
  const int64_t b = pix / HW;
  const int64_t src = b * D + t.c0[br] + cv * 4;
  const float4 gv = *reinterpret_cast<const float4*>(g + src);
  const float4 mv = *reinterpret_cast<const float4*>(mask + src);
  const float n = (float)HW;
  const float4 o = make_float4(gv.x * mv.x / keep / n, gv.y * mv.y / keep / n, gv.z * mv.z / keep / n, gv.w * mv.w / keep / n);
  *reinterpret_cast<float4*>(t.out[br] + pix * Cb + cv * 4) = o;
}

// TF ApplyRMSProp: ms += (g^2 - ms)(1 - rho); mom = momentum * mom + lr g / sqrt(ms + eps); w -= mom.
__global__ __launch_bounds__(kThreads) void rmsprop_tf_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ ms,
                                                              float* __restrict__ mom, size_t n, float lr, float rho, float momentum,
                                                              float eps) {
#pragma clang fp contract(off)
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) {
    const float gi = g[i];
    const float s = ms[i] + (gi * gi - ms[i]) * (1.f - rho);
    const float m = mom[i] * momentum + gi * lr / sqrtf(s + eps);
    ms[i] = s;
    mom[i] = m;
    w[i] = w[i] - m;
  }
}

}  // namespace

size_t softmax_ce_head_ws(int B, int C) { return ((size_t)B * C + 2 * (size_t)B) * sizeof(float); }

hipError_t pool_dropout_launch(const float* x, int B, int HW, int D, float keep, unsigned long long seed, unsigned long long step,
                               float* pre, float* mask, float* y, hipStream_t stream) {
  const int64_t quads = (int64_t)B * D / 4;
  hipLaunchKernelGGL(pool_dropout_kernel, dim3((unsigned)((quads + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, x, B, HW, D,
                     keep, seed, step, pre, mask, y);
  return hipGetLastError();
}

hipError_t softmax_ce_head_launch(const float* y, const float* W, const float* bias, const int32_t* labels, int B, int D, int C,
                                  float* logits, float* prob, float* loss, float* acc, float* dW, int accumulate, float* db, float* dy,
                                  void* ws, hipStream_t stream) {
  float* w = static_cast<float*>(ws);
  hipLaunchKernelGGL(head_fwd_kernel, dim3(B), dim3(kThreads), (size_t)(D + C) * sizeof(float), stream, y, W, bias, labels, B, D, C,
                     logits, prob, w);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(head_bwd_kernel, dim3((D + kThreads - 1) / kThreads), dim3(kThreads), (size_t)B * C * sizeof(float), stream, y, W,
                     w, B, D, C, dW, accumulate, db, dy, loss, acc);
  return hipGetLastError();
}

hipError_t pooled_grad_scatter_launch(const float* g, const float* mask, int B, int HW, int D, float keep, int n, float* const* outs,
                                      const int32_t* c0, const int32_t* Cb, hipStream_t stream) {
  ScatterTable t;
  int64_t most = 0;
  for (int i = 0; i < kMaxScatterBranches; ++i) {
    t.out[i] = i < n ? outs[i] : nullptr;
    t.c0[i] = i < n ? c0[i] : 0;
    t.C[i] = i < n ? Cb[i] : 4;
    if (i < n && (int64_t)B * HW * (Cb[i] / 4) > most) most = (int64_t)B * HW * (Cb[i] / 4);
  }
  hipLaunchKernelGGL(pooled_grad_kernel, dim3((unsigned)((most + kThreads - 1) / kThreads), n), dim3(kThreads), 0, stream, g, mask, B, HW, D,
                     keep, t);
  return hipGetLastError();
}

hipError_t rmsprop_tf_launch(float* w, const float* g, float* ms, float* mom, int64_t n, float lr, float rho, float momentum, float eps,
                             hipStream_t stream) {
  size_t nb = ((size_t)n + kThreads - 1) / kThreads;
  if (nb > 2048) nb = 2048;
  hipLaunchKernelGGL(rmsprop_tf_kernel, dim3((unsigned)(nb < 1 ? 1 : nb)), dim3(kThreads), 0, stream, w, g, ms, mom, (size_t)n, lr, rho,
                     momentum, eps);
  return hipGetLastError();
}

}  // namespace t2i
