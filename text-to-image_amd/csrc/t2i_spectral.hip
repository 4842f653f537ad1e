// t2i_spectral.hip — spectral normalisation of the kernels of an arena (Miyato et al., "Spectral Normalization for Generative
// Adversarial Networks", ICLR 2018; the reference has no such layer), as two entries that optim.AdamTF puts around its own launch
// (DESIGN.md section 4.40).  A normalised variable of shape [..., C] is the row-major matrix M [R, C] at `off` of the arena; its state
// is u [C], v [R] and sigma.  One power iteration:
//
//   t = M u;   v = t / max(|t|, 1e-12);   s = M^T v;   sigma = |s|;   u = s / max(sigma, 1e-12);   flat = raw / max(sigma, 1e-12)
//
// and the chain rule from G = dL/dW to dL/draw with u, v constant: (G - <G, W> v u^T) / sigma.
//
// The matrices are a ragged table: row s of a device table of T2I_SPECTRAL_COLS int64 is (off, R, C, u_off, v_off, part_off, iterate).
// A slot's region of the workspace: [items * C column partials][items partials of |t|^2][ceil(C / 64) partials of |s'|^2]; the
// gradient transform keeps its `items` partials of <G, W> at the head of the same region.
// The host wrapper builds and validates the table before it is uploaded (kernels.spectral_table); the kernels form addresses from it.
//   work items   A matrix is cut into runs of rb = sn_rows_per_item(R, C) rows (about 8192 elements, at most 2048 rows): the cut
//                depends on (R, C) alone.  The grids are (max items, slots); a workgroup whose item does not exist leaves at once.
//   sn_dot_kernel     per item the partial sum of G .* W (fp64 accumulation, a fixed tree), one float per item in the workspace
//   sn_grad_kernel    every workgroup adds its slot's partials (fp64, strided per thread, then the same fixed tree) and corrects its
//                     item of G in place
//   sn_rows_kernel    t = M u for the item's rows (a row per group of lanes, xor butterfly), kept in LDS and written to v, then the
//                     item's |t|^2 and its column sums of t[r] M[r, :] into the workspace: s' = M^T t, and s = s' / |t| needs no
//                     second pass over M
//   sn_cols_kernel    one workgroup per 64 columns of a slot: the items' column partials added in a fixed order (fp64), s' written
//                     to u, the block's sum of s'^2 into the workspace
//   sn_finish_kernel  one workgroup per slot: |t| and |s'| from the partials (fp64, fixed trees), sigma = |s'| / |t|, v = t / |t|,
//                     u = (s' / |t|) / sigma
//   sn_write_kernel   flat = raw / sigma inside the normalised slots, raw elsewhere (padding included: it is 0 in raw), over the whole
//                     arena with adam_tf_kernel's forward-only cursor; here the table selects a divisor and forms no address
// No atomics, every sum in a fixed order: calls repeat bit for bit, and a matrix gives the same bits whatever shares its table.
// Launches: t2i_spectral_grad 2, t2i_spectral_normalize 3 * iterations + 1.  The entries (include/t2i_hip.h) are at the end.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>

#include "t2i_internal.h"

namespace t2i {
namespace {

constexpr int kThreads = 256;
constexpr int kItemElems = 8192;                     // elements of a matrix per work item, at most
constexpr int kItemRows = 2048;                      // rows per work item, at most (t of an item lives in LDS)
constexpr int kColBlock = 64;                        // columns of a slot per workgroup of sn_cols_kernel
constexpr int kCols = T2I_SPECTRAL_COLS;
constexpr float kTiny = 1e-12f;

int launched(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return T2I_OK;
  set_error("%s: %s", what, hipGetErrorString(e));
  return T2I_ERR_LAUNCH;
}

__host__ __device__ inline int sn_rows_per_item(long long R, long long C) {
  long long rb = kItemElems / (C < 1 ? 1 : C);
  if (rb < 1) rb = 1;
  if (rb > kItemRows) rb = kItemRows;
  if (rb > R) rb = R;
  return (int)rb;
}

struct SnItem {
  long long off, R, C, u_off, v_off, part_off;
  int rb, items, r0, nr;       // rows per item, items of the slot, this item's first row and row count (0: no such item)
};

__device__ __forceinline__ SnItem sn_item(const long long* __restrict__ table, int s, int i) {
  const long long* row = table + (size_t)s * kCols;
  SnItem it;
  it.off = row[0]; it.R = row[1]; it.C = row[2]; it.u_off = row[3]; it.v_off = row[4]; it.part_off = row[5];
  it.rb = sn_rows_per_item(it.R, it.C);
  it.items = (int)((it.R + it.rb - 1) / it.rb);
  const long long r0 = (long long)i * it.rb;         // (i may belong to a larger slot of the grid: no int product before the test)
  const long long left = i < it.items ? it.R - r0 : 0;
  it.r0 = i < it.items ? (int)r0 : 0;
  it.nr = (int)(left < it.rb ? left : it.rb);
  return it;
}

// the sum of one double per thread, the same in every thread: a fixed tree through LDS
__device__ __forceinline__ double block_sum(double x, double* red) {
  __syncthreads();                                    // (red may still be read from the previous call)
  red[threadIdx.x] = x;
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(kThreads) void sn_dot_kernel(const float* __restrict__ g, const float* __restrict__ w,
                                                          const long long* __restrict__ table, float* __restrict__ part) {
  __shared__ double red[kThreads];
  const SnItem it = sn_item(table, blockIdx.y, blockIdx.x);
  if (it.nr <= 0) return;
  const long long base = it.off + (long long)it.r0 * it.C;
  const int n = it.nr * (int)it.C;                    // at most kItemElems
  double acc = 0.0;
  for (int e = threadIdx.x; e < n; e += kThreads) acc += (double)g[base + e] * (double)w[base + e];
  const double sum = block_sum(acc, red);
  if (threadIdx.x == 0) part[it.part_off + blockIdx.x] = (float)sum;
}

__global__ __launch_bounds__(kThreads) void sn_grad_kernel(float* __restrict__ g, const long long* __restrict__ table,
                                                           const float* __restrict__ u, const float* __restrict__ v,
                                                           const float* __restrict__ sigma, const float* __restrict__ part) {
  __shared__ double red[kThreads];
  const SnItem it = sn_item(table, blockIdx.y, blockIdx.x);
  if (it.nr <= 0) return;
  double d = 0.0;
  for (int j = threadIdx.x; j < it.items; j += kThreads) d += (double)part[it.part_off + j];
  d = block_sum(d, red);                               // the same tree in every workgroup of the slot
  const float dot = (float)d, sg = fmaxf(sigma[blockIdx.y], kTiny);
  const int C = (int)it.C, n = it.nr * C;
  float* gs = g + it.off + (long long)it.r0 * it.C;
  const float* us = u + it.u_off;
  const float* vs = v + it.v_off + it.r0;
  for (int e = threadIdx.x; e < n; e += kThreads) {
    const int r = e / C, c = e - r * C;
    gs[e] = (gs[e] - dot * vs[r] * us[c]) / sg;
  }
}

__global__ __launch_bounds__(kThreads) void sn_rows_kernel(const float* __restrict__ raw, const long long* __restrict__ table,
                                                           const float* __restrict__ u, float* __restrict__ v, float* __restrict__ part) {
  __shared__ float ts[kItemRows];
  __shared__ float red[kThreads];
  __shared__ double redd[kThreads];
  const long long* row = table + (size_t)blockIdx.y * kCols;
  if (!row[6]) return;
  const SnItem it = sn_item(table, blockIdx.y, blockIdx.x);
  if (it.nr <= 0) return;
  const int C = (int)it.C, nr = it.nr, tid = threadIdx.x;
  const float* M = raw + it.off + (long long)it.r0 * it.C;
  const float* us = u + it.u_off;
  // t[r] = M[r, :] . u: a row per group of L lanes (L the power of two that covers min(C, 64)), the lanes of a group added by an xor butterfly
  int L = 1;
  while (L < C && L < 64) L <<= 1;
  const int G = kThreads / L, grp = tid / L, lane = tid - grp * L;
  for (int r = grp; r < nr; r += G) {
    float acc = 0.f;
    for (int c = lane; c < C; c += L) acc = fmaf(M[r * C + c], us[c], acc);
    for (int m = L >> 1; m > 0; m >>= 1) acc += __shfl_xor(acc, m, L);
    if (lane == 0) ts[r] = acc;
  }
  __syncthreads();
  float* vout = v + it.v_off + it.r0;
  double tq = 0.0;
  for (int r = tid; r < nr; r += kThreads) {
    vout[r] = ts[r];
    tq += (double)ts[r] * (double)ts[r];
  }
  tq = block_sum(tq, redd);
  if (tid == 0) part[it.part_off + (long long)it.items * it.C + blockIdx.x] = (float)tq;      // the item's share of |t|^2
  // the item's column sums of t[r] M[r, c]: P row groups next to L2 columns, the groups added in ascending order
  int L2 = 1;
  while (L2 < C && L2 < kThreads) L2 <<= 1;
  const int P = kThreads / L2, p = tid / L2, c0 = tid - p * L2;
  float* out = part + it.part_off + (long long)blockIdx.x * it.C;
  for (int cb = 0; cb < C; cb += L2) {
    const int c = cb + c0;
    float acc = 0.f;
    if (c < C)
      for (int r = p; r < nr; r += P) acc = fmaf(ts[r], M[r * C + c], acc);
    red[tid] = acc;
    __syncthreads();
    if (p == 0 && c < C) {
      double sum = 0.0;
      for (int q = 0; q < P; ++q) sum += (double)red[q * L2 + c0];
      out[c] = (float)sum;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kThreads) void sn_cols_kernel(const long long* __restrict__ table, float* __restrict__ u, float* __restrict__ part) {
  __shared__ double red[kThreads];
  const long long* row = table + (size_t)blockIdx.y * kCols;
  if (!row[6]) return;
  const SnItem it = sn_item(table, blockIdx.y, 0);
  const long long ncb = (it.C + kColBlock - 1) / kColBlock;
  if ((long long)blockIdx.x >= ncb) return;
  const int tid = threadIdx.x, q = tid / kColBlock, cl = tid - q * kColBlock;       // four groups of items next to 64 columns
  const long long c = (long long)blockIdx.x * kColBlock + cl;
  const float* ps = part + it.part_off;
  double sum = 0.0;
  if (c < it.C)
    for (int i = q; i < it.items; i += kThreads / kColBlock) sum += (double)ps[(long long)i * it.C + c];
  red[tid] = sum;
  __syncthreads();
  double sq = 0.0;
  if (q == 0 && c < it.C) {
    const double sc = ((red[cl] + red[kColBlock + cl]) + red[2 * kColBlock + cl]) + red[3 * kColBlock + cl];
    u[it.u_off + c] = (float)sc;                      // s' = M^T t, not yet divided by |t|
    sq = sc * sc;
  }
  sq = block_sum(sq, red);
  if (tid == 0) part[it.part_off + (long long)it.items * it.C + it.items + blockIdx.x] = (float)sq;
}

__global__ __launch_bounds__(kThreads) void sn_finish_kernel(const long long* __restrict__ table, float* __restrict__ u, float* __restrict__ v,
                                                             float* __restrict__ sigma, const float* __restrict__ part) {
  __shared__ double red[kThreads];
  const long long* row = table + (size_t)blockIdx.x * kCols;
  if (!row[6]) return;
  const SnItem it = sn_item(table, blockIdx.x, 0);
  const int tid = threadIdx.x;
  const long long ncb = (it.C + kColBlock - 1) / kColBlock;
  const float* tp = part + it.part_off + (long long)it.items * it.C;      // the items' |t|^2
  const float* sp = tp + it.items;                                        // the column blocks' |s'|^2
  double tt = 0.0, ss = 0.0;
  for (int i = tid; i < it.items; i += kThreads) tt += (double)tp[i];
  tt = block_sum(tt, red);
  for (long long j = tid; j < ncb; j += kThreads) ss += (double)sp[j];
  ss = block_sum(ss, red);
  const float tn = fmaxf((float)sqrt(tt), kTiny);
  const float sg = (float)(sqrt(ss) / (double)tn), sn = fmaxf(sg, kTiny);
  float* vs = v + it.v_off;
  float* us = u + it.u_off;
  for (long long r = tid; r < it.R; r += kThreads) vs[r] = vs[r] / tn;
  for (long long c = tid; c < it.C; c += kThreads) us[c] = (us[c] / tn) / sn;
  if (tid == 0) sigma[blockIdx.x] = sg;
}

__global__ __launch_bounds__(kThreads) void sn_write_kernel(float* __restrict__ flat, const float* __restrict__ raw, size_t n,
                                                            const long long* __restrict__ table, const float* __restrict__ sigma,
                                                            int n_slots) {
  extern __shared__ __align__(16) unsigned char sn_lds[];
  long long* s_beg = reinterpret_cast<long long*>(sn_lds);                    // [n_slots]
  long long* s_end = s_beg + n_slots;                                         // [n_slots]: the unpadded end
  float* s_sig = reinterpret_cast<float*>(s_end + n_slots);                   // [n_slots]
  for (int s = threadIdx.x; s < n_slots; s += blockDim.x) {
    const long long* row = table + (size_t)s * kCols;
    s_beg[s] = row[0];
    s_end[s] = row[0] + row[1] * row[2];
    s_sig[s] = fmaxf(sigma[s], kTiny);
  }
  __syncthreads();
  const size_t n4 = n >> 2, stride = (size_t)gridDim.x * blockDim.x;
  int cur = -1;
  long long cur_beg = 0, cur_end = 0;
  float sg = 1.f;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const long long e = (long long)(i << 2);
    if (e >= cur_end && cur < n_slots) {
      int lo = cur + 1, hi = n_slots;          // the first slot behind the cursor whose end lies above e; n_slots if none does
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (e < s_end[mid]) hi = mid; else lo = mid + 1;
      }
      cur = lo;
      if (cur < n_slots) { cur_beg = s_beg[cur]; cur_end = s_end[cur]; sg = s_sig[cur]; }
      else { cur_beg = LLONG_MAX; cur_end = LLONG_MAX; }
    }
    const float4 Rw = reinterpret_cast<const float4*>(raw)[i];
    float4 W;
    W.x = (e >= cur_beg && e < cur_end) ? Rw.x / sg : Rw.x;
    W.y = (e + 1 >= cur_beg && e + 1 < cur_end) ? Rw.y / sg : Rw.y;
    W.z = (e + 2 >= cur_beg && e + 2 < cur_end) ? Rw.z / sg : Rw.z;
    W.w = (e + 3 >= cur_beg && e + 3 < cur_end) ? Rw.w / sg : Rw.w;
    reinterpret_cast<float4*>(flat)[i] = W;
  }
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + nb && b0 < a0 + na;
}

struct SnBuf { const void* p; size_t bytes; uintptr_t mask; };     // mask: the alignment asked of p, minus 1

// what the two entries refuse alike; bufs: every buffer of the call, none of which may overlap another
bool sn_args_ok(const char* what, const SnBuf* bufs, int nbufs, int64_t n, const int64_t* table, int32_t n_slots, int32_t max_items,
                int32_t max_col_blocks, int64_t nu, int64_t nv, int64_t part_floats, const void* ws, size_t ws_bytes) {
  for (int i = 0; i < nbufs; ++i)
    if (!bufs[i].p) { set_error("%s: bad argument (a NULL pointer)", what); return false; }
  if (!table || !ws) { set_error("%s: bad argument (a NULL table or workspace)", what); return false; }
  if (n <= 0 || (n & 3) || nu <= 0 || (nu & 3) || nv <= 0 || (nv & 3) || n > (1ll << 40) || nu > n || nv > n) {
    set_error("%s: bad argument (n=%lld nu=%lld nv=%lld: positive multiples of 4, nu and nv at most n)", what, (long long)n, (long long)nu, (long long)nv);
    return false;
  }
  if (n_slots < 1 || n_slots > T2I_SPECTRAL_MAX_SLOTS) {
    set_error("%s: bad argument (n_slots = %d is outside [1, %d])", what, (int)n_slots, (int)T2I_SPECTRAL_MAX_SLOTS);
    return false;
  }
  if (max_items < 1 || max_items > T2I_SPECTRAL_MAX_ITEMS || (int64_t)max_items > n || max_col_blocks < 1 || max_col_blocks > T2I_SPECTRAL_MAX_ITEMS ||
      (int64_t)max_col_blocks > n || part_floats < 1 || part_floats > 4 * n + 8 * (int64_t)n_slots) {
    set_error("%s: bad argument (max_items=%d max_col_blocks=%d part_floats=%lld for an arena of %lld elements)", what, (int)max_items,
              (int)max_col_blocks, (long long)part_floats, (long long)n);
    return false;
  }
  for (int i = 0; i < nbufs; ++i)
    if (reinterpret_cast<uintptr_t>(bufs[i].p) & bufs[i].mask) {
      set_error("%s: bad argument (the arenas, u, v and the workspace must be 16-byte aligned, sigma 4-byte)", what);
      return false;
    }
  if ((reinterpret_cast<uintptr_t>(table) & 7) || (reinterpret_cast<uintptr_t>(ws) & 15)) {
    set_error("%s: bad argument (the table must be 8-byte aligned, the workspace 16-byte)", what);
    return false;
  }
  const size_t need = t2i_spectral_workspace_bytes(part_floats);
  if (ws_bytes < need) {
    set_error("%s: bad argument (workspace too small: %zu bytes, %zu needed)", what, ws_bytes, need);
    return false;
  }
  const SnBuf tb{table, (size_t)n_slots * kCols * 8, 7}, wb{ws, need, 15};
  for (int i = 0; i < nbufs; ++i) {
    for (int j = i + 1; j < nbufs; ++j)
      if (overlap(bufs[i].p, bufs[i].bytes, bufs[j].p, bufs[j].bytes)) { set_error("%s: bad argument (two buffers overlap)", what); return false; }
    if (overlap(bufs[i].p, bufs[i].bytes, tb.p, tb.bytes) || overlap(bufs[i].p, bufs[i].bytes, wb.p, wb.bytes)) {
      set_error("%s: bad argument (the table or the workspace overlaps a buffer)", what);
      return false;
    }
  }
  if (overlap(tb.p, tb.bytes, wb.p, wb.bytes)) { set_error("%s: bad argument (the table overlaps the workspace)", what); return false; }
  return true;
}

}  // namespace
}  // namespace t2i

using namespace t2i;

size_t t2i_spectral_workspace_bytes(int64_t part_floats) {
  if (part_floats < 1 || part_floats > (1ll << 42)) return 0;
  return ((size_t)part_floats * 4 + 255) / 256 * 256;
}

int t2i_spectral_grad(float* grad, const float* flat, int64_t n, const int64_t* table_dev, int32_t n_slots, int32_t max_items, const float* u,
                      int64_t nu, const float* v, int64_t nv, const float* sigma, int64_t part_floats, void* ws, size_t ws_bytes,
                      t2i_stream_t stream) {
  const char* what = "t2i_spectral_grad";
  const size_t nb = n > 0 ? (size_t)n * 4 : 0;
  const SnBuf bufs[] = {{grad, nb, 15}, {flat, nb, 15}, {u, nu > 0 ? (size_t)nu * 4 : 0, 15}, {v, nv > 0 ? (size_t)nv * 4 : 0, 15},
                        {sigma, n_slots > 0 ? (size_t)n_slots * 4 : 0, 3}};
  if (!sn_args_ok(what, bufs, 5, n, table_dev, n_slots, max_items, 1, nu, nv, part_floats, ws, ws_bytes)) return T2I_ERR_INVALID;
  const long long* table = reinterpret_cast<const long long*>(table_dev);
  float* part = reinterpret_cast<float*>(ws);
  const dim3 grid((unsigned)max_items, (unsigned)n_slots);
  hipLaunchKernelGGL(sn_dot_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, grad, flat, table, part);
  hipLaunchKernelGGL(sn_grad_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, grad, table, u, v, sigma, part);
  return launched(what);
}

int t2i_spectral_normalize(float* flat, const float* raw, int64_t n, const int64_t* table_dev, int32_t n_slots, int32_t max_items,
                           int32_t max_col_blocks, float* u, int64_t nu, float* v, int64_t nv, float* sigma, int32_t iterations,
                           int64_t part_floats, void* ws, size_t ws_bytes, t2i_stream_t stream) {
  const char* what = "t2i_spectral_normalize";
  const size_t nb = n > 0 ? (size_t)n * 4 : 0;
  const SnBuf bufs[] = {{flat, nb, 15}, {raw, nb, 15}, {u, nu > 0 ? (size_t)nu * 4 : 0, 15}, {v, nv > 0 ? (size_t)nv * 4 : 0, 15},
                        {sigma, n_slots > 0 ? (size_t)n_slots * 4 : 0, 3}};
  if (iterations < 0 || iterations > T2I_SPECTRAL_MAX_ITERATIONS) {
    set_error("%s: bad argument (iterations = %d is outside [0, %d])", what, (int)iterations, (int)T2I_SPECTRAL_MAX_ITERATIONS);
    return T2I_ERR_INVALID;
  }
  if (!sn_args_ok(what, bufs, 5, n, table_dev, n_slots, max_items, max_col_blocks, nu, nv, part_floats, ws, ws_bytes)) return T2I_ERR_INVALID;
  const long long* table = reinterpret_cast<const long long*>(table_dev);
  float* part = reinterpret_cast<float*>(ws);
  hipStream_t st = (hipStream_t)stream;
  filter_cache_invalidate(flat, nb);                   // transformed filters of this arena are stale from here on
  for (int k = 0; k < iterations; ++k) {
    hipLaunchKernelGGL(sn_rows_kernel, dim3((unsigned)max_items, (unsigned)n_slots), dim3(kThreads), 0, st, raw, table, u, v, part);
    hipLaunchKernelGGL(sn_cols_kernel, dim3((unsigned)max_col_blocks, (unsigned)n_slots), dim3(kThreads), 0, st, table, u, part);
    hipLaunchKernelGGL(sn_finish_kernel, dim3((unsigned)n_slots), dim3(kThreads), 0, st, table, u, v, sigma, part);
  }
  size_t blocks = (((size_t)n >> 2) + kThreads - 1) / kThreads;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(sn_write_kernel, dim3((unsigned)blocks), dim3(kThreads), (size_t)n_slots * 20, st, flat, raw, (size_t)n, table, sigma,
                     (int)n_slots);
  const int rc = launched(what);
  if (rc != T2I_OK || !tuning().cache_refresh) return rc;
  return filter_cache_refresh(flat, nb, st);
}
