// t2i_knn.hip — all-pairs squared distances between two fp32 feature sets Q [M, D] and R [N, D] with a selection epilogue: the
// k smallest per query (t2i_knn_dist2) or the number of candidates whose ball holds the query, with the nearest distance
// (t2i_ball_counts).  The M x N matrix never reaches memory.  evaluation/prdc.py (precision, recall, density, coverage) calls it.
//
//   d2(m, n) = max(|Q_m|^2 + |R_n|^2 - 2 Q_m.R_n, 0), all three sums in fp64 from the fp32 inputs widened exactly (their products
//   are exact in fp64: 24 + 24 bits), so every value lies within a derivable band of the true distance and the discrete results
//   (d2 <= r2, order statistics) can be tested for equality with a float64 restatement.
//
//   knn_norm_kernel   |row|^2 in fp64, one wave per row: lane t adds the squares t, t + 64, ... in order, a butterfly adds the lanes.
//   knn_core_kernel   One workgroup (4 waves) owns kT = 64 queries and walks tiles of kTC = 128 candidates over the WHOLE depth D
//                     (no split over D: every d2(m, n) is formed in one place, by one chain of v_mfma_f64_16x16x4_f64 over
//                     ascending d, whatever `segments` is).  Depth chunks of kKT floats of both tiles are widened to fp64 while they
//                     are staged in LDS (rows kKT + 2 doubles apart: the 32 lanes of a half wave read 32 different 8-byte bank
//                     pairs); the next chunk's global loads are in flight while the current one is multiplied.  The product is
//                     oriented CANDIDATES x QUERIES: the candidates are the A operand (rows), the queries the B operand
//                     (columns), so in the f64 C/D map (col = lane & 15, row = (lane >> 4) + 4 reg — not the f32 map) a lane's
//                     accumulators all belong to ONE query, lane & 15 of the wave's 16, and to the 32 candidates
//                     16 j + (lane >> 4) + 4 reg (j = 0..7, reg = 0..3) of the tile.  The lane keeps that query's running list of the
//                     kList = 8 smallest (or count and minimum) in registers: no cross-lane traffic in the candidate loop.  The four
//                     lane groups of a column merge once per workgroup through LDS, groups 0, 1, 2, 3 in that order.
//                     `segments` splits the candidate tiles so that few query tiles still fill the chip; segment s of query m
//                     leaves its list (or count and minimum) in the workspace.
//   knn_fold_kernel / ball_fold_kernel   one thread per query folds the segments in ascending order.
// Comparisons are written so that a NaN never enters a list or a count (v < worst, v <= r2); an unfilled slot holds +inf.
// No atomics: results are bitwise identical from call to call and for every value of `segments`.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "t2i_internal.h"

namespace t2i {

namespace {

constexpr int kThreads = 256;
constexpr int kT = 64;                                    // queries per workgroup
constexpr int kTC = 128;                                  // candidates per tile
constexpr int kNJ = kTC / 16;                             // 16-candidate blocks per tile: accumulators per lane
constexpr int kKT = 32;                                   // depth chunk staged at a time
constexpr int kLd = kKT + 2;                              // LDS row stride in doubles: 2 mod 32, see above
constexpr int kList = 8;                                  // T2I_KNN_MAX_K
constexpr int64_t kMaxGrid = 1 << 20;                     // workgroups per launch; a larger problem strides over its work items

typedef double double4_t __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(kThreads) void knn_norm_kernel(const float* __restrict__ x, int64_t rows, int D, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * (kThreads / 64)) {
    const float* p = x + (size_t)r * D;
    double s = 0.0;
    for (int d = lane; d < D; d += 64) {
      const double v = (double)p[d];
      s = fma(v, v, s);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) out[r] = s;
  }
}

// keeps L ascending; a NaN is never taken
__device__ __forceinline__ void knn_insert(double (&L)[kList], double v) {
  if (v < L[kList - 1]) {
    L[kList - 1] = v;
#pragma unroll
    for (int i = kList - 1; i > 0; --i) {
      const double lo = L[i - 1], hi = L[i];
      const bool sw = hi < lo;
      L[i - 1] = sw ? hi : lo;
      L[i] = sw ? lo : hi;
    }
  }
}

// 8 floats of row `row` (of `rows`) from depth d; zeros beyond the row count and beyond D
__device__ __forceinline__ void knn_load8(const float* __restrict__ x, int64_t row, int64_t rows, int D, int d, int vec, float (&v)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = 0.f;
  if (row >= rows) return;
  const float* p = x + (size_t)row * D + d;
  if (vec && d + 8 <= D) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    const float4 b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (d + i < D) v[i] = p[i];
  }
}

__device__ __forceinline__ void knn_store8(double* s, const float (&v)[8]) {
#pragma unroll
  for (int i = 0; i < 8; i += 2) *reinterpret_cast<double2*>(s + i) = make_double2((double)v[i], (double)v[i + 1]);
}

// kBall false: part_list[(seg M + m) kList + i] = the segment's kList smallest d2 of query m, ascending.
// kBall true:  part_cnt[seg M + m] = #{n in the segment: d2 <= r2[n]}, part_min[seg M + m] = the segment's smallest d2.
template <bool kBall>
__global__ __launch_bounds__(kThreads) void knn_core_kernel(const float* __restrict__ Q, int64_t M, const float* __restrict__ R, int64_t N,
                                                            int D, int vec, const double* __restrict__ qn, const double* __restrict__ rn,
                                                            const double* __restrict__ r2, int exclude_self, int segments, int64_t total,
                                                            double* __restrict__ part_list, int32_t* __restrict__ part_cnt,
                                                            double* __restrict__ part_min) {
  __shared__ __attribute__((aligned(16))) double s_q[kT * kLd];
  __shared__ __attribute__((aligned(16))) double s_r[kTC * kLd];
  __shared__ double s_rn[kTC];
  __shared__ double s_r2[kTC];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int col = lane & 15, grp = lane >> 4;
  const int ld_row = t >> 2, ld_d = (t & 3) * 8;            // staging: thread t brings 8 floats of row t / 4
  const int64_t ntiles = (N + kTC - 1) / kTC;

  for (int64_t blk = blockIdx.x; blk < total; blk += gridDim.x) {
    const int64_t qtile = blk / segments;
    const int seg = (int)(blk - qtile * segments);
    const int64_t q0 = qtile * kT;
    const int64_t t_begin = ntiles * seg / segments, t_end = ntiles * (seg + 1) / segments;
    const int64_t qi = q0 + 16 * wave + col;                // this lane's query
    const double qv = qi < M ? qn[qi] : 0.0;

    double L[kList];
#pragma unroll
    for (int i = 0; i < kList; ++i) L[i] = INFINITY;
    int32_t cnt = 0;
    double dmin = INFINITY;

    for (int64_t ct = t_begin; ct < t_end; ++ct) {
      const int64_t c0 = ct * kTC;
      double4_t acc[kNJ];
#pragma unroll
      for (int j = 0; j < kNJ; ++j) acc[j] = double4_t{0.0, 0.0, 0.0, 0.0};

      float fq[8], fr[kTC / kT][8];
      knn_load8(Q, q0 + ld_row, M, D, ld_d, vec, fq);
#pragma unroll
      for (int h = 0; h < kTC / kT; ++h) knn_load8(R, c0 + kT * h + ld_row, N, D, ld_d, vec, fr[h]);
      for (int d0 = 0; d0 < D; d0 += kKT) {
        __syncthreads();                                    // the previous chunk (and the previous tile's epilogue) is done with the LDS
        knn_store8(s_q + ld_row * kLd + ld_d, fq);
#pragma unroll
        for (int h = 0; h < kTC / kT; ++h) knn_store8(s_r + (kT * h + ld_row) * kLd + ld_d, fr[h]);
        if (d0 == 0 && t < kTC) {
          const int64_t c = c0 + t;
          s_rn[t] = c < N ? rn[c] : 0.0;
          if (kBall) s_r2[t] = c < N ? r2[c] : 0.0;
        }
        __syncthreads();
        if (d0 + kKT < D) {                                 // in flight while this chunk is multiplied
          knn_load8(Q, q0 + ld_row, M, D, d0 + kKT + ld_d, vec, fq);
#pragma unroll
          for (int h = 0; h < kTC / kT; ++h) knn_load8(R, c0 + kT * h + ld_row, N, D, d0 + kKT + ld_d, vec, fr[h]);
        }
        const double* pq = s_q + (16 * wave + col) * kLd + grp;
        const double* pr = s_r + col * kLd + grp;
#pragma unroll
        for (int kk = 0; kk < kKT; kk += 4) {
          const double b = pq[kk];
#pragma unroll
          for (int j = 0; j < kNJ; ++j) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(pr[16 * j * kLd + kk], b, acc[j], 0, 0, 0);
        }
      }

      // epilogue: acc[j][reg] is candidate 16 j + grp + 4 reg of the tile against query qi
#pragma unroll
      for (int j = 0; j < kNJ; ++j) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int lc = 16 * j + grp + 4 * reg;
          const int64_t c = c0 + lc;
          const double v = (qv + s_rn[lc]) - 2.0 * acc[j][reg];
          const double d2 = v < 0.0 ? 0.0 : v;              // (a NaN stays a NaN)
          const bool valid = c < N && !(exclude_self && c == qi);
          if (kBall) {
            if (valid) {
              cnt += d2 <= s_r2[lc] ? 1 : 0;
              dmin = d2 < dmin ? d2 : dmin;
            }
          } else {
            if (valid) knn_insert(L, d2);
          }
        }
      }
    }

    // the four lane groups of a column, merged by group 0 in the order 0, 1, 2, 3 (s_q as scratch: 256 x 8 doubles fit)
    __syncthreads();
    if (kBall) {
      s_q[t] = dmin;
      reinterpret_cast<int32_t*>(s_r)[t] = cnt;
    } else {
#pragma unroll
      for (int i = 0; i < kList; ++i) s_q[t * kList + i] = L[i];
    }
    __syncthreads();
    if (grp == 0 && qi < M) {
      const size_t o = (size_t)seg * (size_t)M + (size_t)qi;
      if (kBall) {
#pragma unroll
        for (int g = 1; g < 4; ++g) {
          const double m2 = s_q[t + 16 * g];
          cnt += reinterpret_cast<const int32_t*>(s_r)[t + 16 * g];
          dmin = m2 < dmin ? m2 : dmin;
        }
        part_cnt[o] = cnt;
        part_min[o] = dmin;
      } else {
#pragma unroll
        for (int g = 1; g < 4; ++g) {
#pragma unroll
          for (int i = 0; i < kList; ++i) knn_insert(L, s_q[(t + 16 * g) * kList + i]);
        }
#pragma unroll
        for (int i = 0; i < kList; ++i) part_list[o * kList + i] = L[i];
      }
    }
    __syncthreads();                                        // the scratch is read before the next work item stages into it
  }
}

__global__ __launch_bounds__(kThreads) void knn_fold_kernel(const double* __restrict__ part, int64_t M, int segments, int k,
                                                            double* __restrict__ out) {
  for (int64_t m = (int64_t)blockIdx.x * kThreads + threadIdx.x; m < M; m += (int64_t)gridDim.x * kThreads) {
    double L[kList];
#pragma unroll
    for (int i = 0; i < kList; ++i) L[i] = part[(size_t)m * kList + i];
    for (int s = 1; s < segments; ++s) {
      const double* p = part + ((size_t)s * (size_t)M + (size_t)m) * kList;
#pragma unroll
      for (int i = 0; i < kList; ++i) knn_insert(L, p[i]);
    }
#pragma unroll
    for (int i = 0; i < kList; ++i)
      if (i < k) out[(size_t)m * k + i] = L[i];
  }
}

__global__ __launch_bounds__(kThreads) void ball_fold_kernel(const int32_t* __restrict__ part_cnt, const double* __restrict__ part_min,
                                                             int64_t M, int segments, int32_t* __restrict__ count,
                                                             double* __restrict__ dmin) {
  for (int64_t m = (int64_t)blockIdx.x * kThreads + threadIdx.x; m < M; m += (int64_t)gridDim.x * kThreads) {
    int32_t c = 0;
    double v = INFINITY;
    for (int s = 0; s < segments; ++s) {
      const size_t o = (size_t)s * (size_t)M + (size_t)m;
      const double p = part_min[o];
      c += part_cnt[o];
      v = p < v ? p : v;
    }
    count[m] = c;
    dmin[m] = v;
  }
}

inline size_t al256(size_t n) { return (n + 255) & ~(size_t)255; }
inline int64_t tiles_of(int64_t n) { return (n + kT - 1) / kT; }
inline int64_t ctiles_of(int64_t n) { return (n + kTC - 1) / kTC; }

inline unsigned grid_for(int64_t items) { return (unsigned)(items < kMaxGrid ? items : kMaxGrid); }

inline hipError_t norms_launch(const float* x, int64_t rows, int D, double* out, hipStream_t stream) {
  hipLaunchKernelGGL(knn_norm_kernel, dim3(grid_for((rows + 3) / 4)), dim3(kThreads), 0, stream, x, rows, D, out);
  return hipGetLastError();
}

inline int vec_ok(const float* Q, const float* R, int D) {
  return (D % 4) == 0 && (reinterpret_cast<uintptr_t>(Q) & 15) == 0 && (reinterpret_cast<uintptr_t>(R) & 15) == 0;
}

}  // namespace

// segments = 0: enough segments for about four workgroups on each of 256 compute units, at most one per candidate tile and 64
int knn_auto_segments(int64_t M, int64_t N) {
  const int64_t qtiles = tiles_of(M), ntiles = ctiles_of(N);
  int64_t want = (1024 + qtiles - 1) / qtiles;
  if (want > ntiles) want = ntiles;
  if (want > 64) want = 64;
  return (int)(want < 1 ? 1 : want);
}

// The caller (t2i_capi.hip) has checked every extent; segments >= 1 here.
// workspace: |Q_m|^2 [M], |R_n|^2 [N], then the per-segment partials
size_t knn_dist2_ws(int64_t M, int64_t N, int segments) {
  return al256((size_t)M * 8) + al256((size_t)N * 8) + al256((size_t)segments * (size_t)M * kList * 8);
}

size_t ball_counts_ws(int64_t M, int64_t N, int segments) {
  return al256((size_t)M * 8) + al256((size_t)N * 8) + al256((size_t)segments * (size_t)M * 8) + al256((size_t)segments * (size_t)M * 4);
}

hipError_t knn_dist2_launch(const float* Q, int64_t M, const float* R, int64_t N, int D, int k, int exclude_self, int segments, double* out,
                            void* ws, hipStream_t stream) {
  char* w = static_cast<char*>(ws);
  double* qn = reinterpret_cast<double*>(w);
  double* rn = reinterpret_cast<double*>(w + al256((size_t)M * 8));
  double* part = reinterpret_cast<double*>(w + al256((size_t)M * 8) + al256((size_t)N * 8));
  hipError_t e = norms_launch(Q, M, D, qn, stream);
  if (e != hipSuccess) return e;
  e = norms_launch(R, N, D, rn, stream);
  if (e != hipSuccess) return e;
  const int64_t total = tiles_of(M) * segments;
  hipLaunchKernelGGL(knn_core_kernel<false>, dim3(grid_for(total)), dim3(kThreads), 0, stream, Q, M, R, N, D, vec_ok(Q, R, D), qn, rn,
                     (const double*)nullptr, exclude_self, segments, total, part, (int32_t*)nullptr, (double*)nullptr);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(knn_fold_kernel, dim3(grid_for((M + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, part, M, segments, k, out);
  return hipGetLastError();
}

hipError_t ball_counts_launch(const float* Q, int64_t M, const float* R, int64_t N, int D, const double* r2, int segments, int32_t* count,
                              double* dmin, void* ws, hipStream_t stream) {
  char* w = static_cast<char*>(ws);
  double* qn = reinterpret_cast<double*>(w);
  double* rn = reinterpret_cast<double*>(w + al256((size_t)M * 8));
  double* part_min = reinterpret_cast<double*>(w + al256((size_t)M * 8) + al256((size_t)N * 8));
  int32_t* part_cnt = reinterpret_cast<int32_t*>(w + al256((size_t)M * 8) + al256((size_t)N * 8) + al256((size_t)segments * (size_t)M * 8));
  hipError_t e = norms_launch(Q, M, D, qn, stream);
  if (e != hipSuccess) return e;
  e = norms_launch(R, N, D, rn, stream);
  if (e != hipSuccess) return e;
  const int64_t total = tiles_of(M) * segments;
  hipLaunchKernelGGL(knn_core_kernel<true>, dim3(grid_for(total)), dim3(kThreads), 0, stream, Q, M, R, N, D, vec_ok(Q, R, D), qn, rn, r2, 0,
                     segments, total, (double*)nullptr, part_cnt, part_min);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ball_fold_kernel, dim3(grid_for((M + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, part_cnt, part_min, M,
                     segments, count, dmin);
  return hipGetLastError();
}

}  // namespace t2i
