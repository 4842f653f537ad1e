// t2i_mmd.hip — the three kernel sums of the polynomial-kernel MMD^2 (the Kernel Inception distance of Binkowski et al. 2018) for S
// subsets of m rows of two fp32 feature sets X [NX, D] and Y [NY, D], named by index tables ix, iy [S, m]:
//
//   k(a, b) = (gamma a.b + coef0)^degree     P_xx = sum_{i<j} k(x_i, x_j)     P_yy likewise     S_xy = sum_{i,j} k(x_i, y_j)
//
// with i, j POSITIONS in the subset.  No m x m matrix and no gathered copy of a subset reaches memory.  evaluation/mmd.py calls it.
//
// Taken over from t2i_knn.hip (which stays as it is): the workgroup of 4 waves, the 64 x 128 tile walked over the WHOLE depth D in
// chunks of kKT floats widened to fp64 while they are staged in LDS (rows kKT + 2 doubles apart), the next chunk's global loads in
// flight while the current one is multiplied, one chain of v_mfma_f64_16x16x4_f64 over ascending d per pair, and the f64 C/D map
// (col = lane & 15, row = (lane >> 4) + 4 reg).  The tile's 128 columns j are the A operand, its 64 rows i the B operand, so
// acc[jb][reg] of a lane is the pair (i = 16 wave + (lane & 15), j = 16 jb + (lane >> 4) + 4 reg) of the tile.
// What differs:
//   work items   One workgroup per (subset, product, tile), the grid exactly their number.  Row tile ti of a symmetric product (xx, yy)
//                has the column tiles tj >= ti / 2 only: 128 tj + 127 > 64 ti is the condition for a tile to hold any pair i < j, so
//                tiles wholly below the diagonal are no work items.  Per subset: [xx tiles][yy tiles][xy tiles], row-major each.
//   loader       Row r of a tile is row ix[s, r] of X, read in place.  Positions beyond m and depths beyond D are zeros; an index
//                outside 0..N-1 is never turned into an address: its row is NaNs, so exactly the sums it belongs to are NaN.
//   epilogue     t = fma(gamma, dot, coef0), then degree - 1 multiplications by t; pairs with a position beyond m, and in a symmetric
//                product pairs with i >= j, are SELECTED away (a padded row has k = coef0^degree, not 0; a NaN is not multiplied by 0).
//                A lane adds its 32 values in ascending register order, a fixed xor butterfly adds the 64 lanes, the four waves go
//                through LDS and are added in the order 0, 1, 2, 3: one double per work item in the workspace.
//   mmd_fold_kernel   one thread per (subset, product) adds its tiles in ascending order into sums [S, 3].
// No atomics: results are bitwise identical from call to call.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "t2i_internal.h"

namespace t2i {

namespace {

constexpr int kThreads = 256;
constexpr int kT = 64;                                    // rows i per tile (B operand)
constexpr int kTC = 128;                                  // columns j per tile (A operand)
constexpr int kNJ = kTC / 16;                             // 16-column blocks per tile: accumulators per lane
constexpr int kKT = 32;                                   // depth chunk staged at a time
constexpr int kLd = kKT + 2;                              // LDS row stride in doubles: 2 mod 32

typedef double double4_t __attribute__((ext_vector_type(4)));

struct MmdGeom {
  int64_t nrt, nct;                                       // row and column tiles of one product
  int64_t wsym, wxy, wsub;                                // work items of a symmetric product, of xy, of one subset
};

// tiles of the symmetric product before row-tile pair a (rows 2a and 2a + 1 have nct - a tiles each)
__host__ __device__ inline int64_t mmd_before_pair(int64_t a, int64_t nct) { return 2 * a * nct - a * (a - 1); }

__host__ __device__ inline MmdGeom mmd_geom(int64_t m) {
  MmdGeom g;
  g.nrt = (m + kT - 1) / kT;
  g.nct = (m + kTC - 1) / kTC;
  const int64_t pairs = g.nrt / 2;
  g.wsym = mmd_before_pair(pairs, g.nct) + ((g.nrt & 1) ? g.nct - pairs : 0);
  g.wxy = g.nrt * g.nct;
  g.wsub = 2 * g.wsym + g.wxy;
  return g;
}

// item `rem` (0 <= rem < wsym) of a symmetric product -> (ti, tj), row-major over the kept tiles
__host__ __device__ inline void mmd_sym_tile(int64_t rem, int64_t nct, int64_t* ti, int64_t* tj) {
  const double b = 2.0 * (double)nct + 1.0;
  double disc = b * b - 4.0 * (double)rem;
  int64_t a = (int64_t)((b - sqrt(disc < 0.0 ? 0.0 : disc)) * 0.5);
  if (a < 0) a = 0;
  if (a > nct - 1) a = nct - 1;
  while (a > 0 && mmd_before_pair(a, nct) > rem) --a;      // (the square root is a guess: these two loops make it exact)
  while (a + 1 < nct && mmd_before_pair(a + 1, nct) <= rem) ++a;
  const int64_t r = rem - mmd_before_pair(a, nct), cnt = nct - a;
  const int64_t odd = r >= cnt ? 1 : 0;
  *ti = 2 * a + odd;
  *tj = a + (r - odd * cnt);
}

// where a tile row comes from: p the row in its set, or nullptr with nan = 0 (a position beyond m: zeros) or 1 (an index out of range)
struct MmdRow {
  const float* p;
  int nan;
};

__device__ __forceinline__ MmdRow mmd_row(const float* __restrict__ x, int64_t rows, int D, const int32_t* __restrict__ idx, int64_t pos,
                                          int64_t m) {
  MmdRow r = {nullptr, 0};
  if (pos < m) {
    const int32_t i = idx[pos];
    if (i >= 0 && (int64_t)i < rows) r.p = x + (size_t)i * (size_t)D;
    else r.nan = 1;
  }
  return r;
}

// 8 floats of the row from depth d; zeros beyond D
__device__ __forceinline__ void mmd_load8(const MmdRow& r, int D, int d, int vec, float (&v)[8]) {
  const float fill = r.nan ? __builtin_nanf("") : 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = fill;
  if (!r.p) return;
  const float* p = r.p + d;
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

__device__ __forceinline__ void mmd_store8(double* s, const float (&v)[8]) {
#pragma unroll
  for (int i = 0; i < 8; i += 2) *reinterpret_cast<double2*>(s + i) = make_double2((double)v[i], (double)v[i + 1]);
}

// part[blockIdx.x] = the masked sum of k over this work item's tile.  Three waves per SIMD (three workgroups per CU, what the LDS admits):
// the compiler's default allocation leaves two; measured 15.25 against 17.32 ms at 100 subsets of 1000 x 2048, the same bits.
__global__ __launch_bounds__(kThreads, 3) void mmd_core_kernel(const float* __restrict__ X, int64_t NX, const float* __restrict__ Y, int64_t NY,
                                                            int D, int vec, const int32_t* __restrict__ ix, const int32_t* __restrict__ iy,
                                                            int64_t m, int degree, double gamma, double coef0, double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) double s_i[kT * kLd];
  __shared__ __attribute__((aligned(16))) double s_j[kTC * kLd];
  __shared__ double s_wave[kThreads / 64];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int col = lane & 15, grp = lane >> 4;
  const int ld_row = t >> 2, ld_d = (t & 3) * 8;            // staging: thread t brings 8 floats of row t / 4

  // (subset, product, tile) of this workgroup
  const MmdGeom g = mmd_geom(m);
  const int64_t s = (int64_t)blockIdx.x / g.wsub;
  int64_t rem = (int64_t)blockIdx.x - s * g.wsub;
  const int prod = rem < g.wsym ? 0 : (rem < 2 * g.wsym ? 1 : 2);          // xx, yy, xy
  rem -= prod * g.wsym;
  int64_t ti, tj;
  if (prod < 2) {
    mmd_sym_tile(rem, g.nct, &ti, &tj);
  } else {
    ti = rem / g.nct;
    tj = rem - ti * g.nct;
  }
  const bool sym = prod < 2;
  const float* A = prod == 1 ? Y : X;                       // the set of the rows i
  const float* B = prod == 0 ? X : Y;                       // the set of the columns j
  const int64_t NA = prod == 1 ? NY : NX, NB = prod == 0 ? NX : NY;
  const int32_t* ia = (prod == 1 ? iy : ix) + (size_t)s * (size_t)m;
  const int32_t* ib = (prod == 0 ? ix : iy) + (size_t)s * (size_t)m;
  const int64_t i0 = ti * kT, j0 = tj * kTC;

  const MmdRow ri = mmd_row(A, NA, D, ia, i0 + ld_row, m);
  MmdRow rj[kTC / kT];
#pragma unroll
  for (int h = 0; h < kTC / kT; ++h) rj[h] = mmd_row(B, NB, D, ib, j0 + kT * h + ld_row, m);

  double4_t acc[kNJ];
#pragma unroll
  for (int j = 0; j < kNJ; ++j) acc[j] = double4_t{0.0, 0.0, 0.0, 0.0};

  float fi[8], fj[kTC / kT][8];
  mmd_load8(ri, D, ld_d, vec, fi);
#pragma unroll
  for (int h = 0; h < kTC / kT; ++h) mmd_load8(rj[h], D, ld_d, vec, fj[h]);
  for (int d0 = 0; d0 < D; d0 += kKT) {
    __syncthreads();                                        // the previous chunk is done with the LDS
    mmd_store8(s_i + ld_row * kLd + ld_d, fi);
#pragma unroll
    for (int h = 0; h < kTC / kT; ++h) mmd_store8(s_j + (kT * h + ld_row) * kLd + ld_d, fj[h]);
    __syncthreads();
    if (d0 + kKT < D) {                                     // in flight while this chunk is multiplied
      mmd_load8(ri, D, d0 + kKT + ld_d, vec, fi);
#pragma unroll
      for (int h = 0; h < kTC / kT; ++h) mmd_load8(rj[h], D, d0 + kKT + ld_d, vec, fj[h]);
    }
    const double* pi = s_i + (16 * wave + col) * kLd + grp;
    const double* pj = s_j + col * kLd + grp;
#pragma unroll
    for (int kk = 0; kk < kKT; kk += 4) {
      const double b = pi[kk];
#pragma unroll
      for (int j = 0; j < kNJ; ++j) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(pj[16 * j * kLd + kk], b, acc[j], 0, 0, 0);
    }
  }

  // epilogue: acc[j][reg] is the pair (i, jc): i this lane's row, jc = j0 + 16 j + grp + 4 reg
  const int64_t i = i0 + 16 * wave + col;
  double sum = 0.0;
#pragma unroll
  for (int j = 0; j < kNJ; ++j) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int64_t jc = j0 + 16 * j + grp + 4 * reg;
      const double tt = fma(gamma, acc[j][reg], coef0);
      double k = tt;
      for (int q = 1; q < degree; ++q) k *= tt;
      const bool valid = i < m && jc < m && (!sym || i < jc);
      sum += valid ? k : 0.0;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
  if (lane == 0) s_wave[wave] = sum;
  __syncthreads();
  if (t == 0) part[blockIdx.x] = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
}

__global__ __launch_bounds__(kThreads) void mmd_fold_kernel(const double* __restrict__ part, int64_t S, int64_t wsym, int64_t wxy,
                                                            double* __restrict__ sums) {
  const int64_t o = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (o >= 3 * S) return;
  const int64_t s = o / 3;
  const int prod = (int)(o - 3 * s);
  const double* p = part + s * (2 * wsym + wxy) + prod * wsym;
  const int64_t n = prod < 2 ? wsym : wxy;
  double v = 0.0;
  for (int64_t w = 0; w < n; ++w) v += p[w];
  sums[o] = v;
}

inline size_t al256(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace

// work items of one subset (the caller checks S * this against the cap); m >= 2
int64_t poly_mmd_items_per_subset(int64_t m) { return mmd_geom(m).wsub; }

// The caller (t2i_capi.hip) has checked every extent and the cap on the work items.
size_t poly_mmd_sums_ws(int64_t S, int64_t m) { return al256((size_t)S * (size_t)mmd_geom(m).wsub * 8); }

hipError_t poly_mmd_sums_launch(const float* X, int64_t NX, const float* Y, int64_t NY, int D, const int32_t* ix, const int32_t* iy, int64_t S,
                                int64_t m, int degree, double gamma, double coef0, double* sums, void* ws, hipStream_t stream) {
  const MmdGeom g = mmd_geom(m);
  double* part = static_cast<double*>(ws);
  const int vec = (D % 4) == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0 && (reinterpret_cast<uintptr_t>(Y) & 15) == 0;
  hipLaunchKernelGGL(mmd_core_kernel, dim3((unsigned)(S * g.wsub)), dim3(kThreads), 0, stream, X, NX, Y, NY, D, vec, ix, iy, m, degree, gamma,
                     coef0, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(mmd_fold_kernel, dim3((unsigned)((3 * S + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, part, S, g.wsym, g.wxy,
                     sums);
  return hipGetLastError();
}

}  // namespace t2i
