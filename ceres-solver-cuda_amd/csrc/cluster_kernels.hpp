// cluster_kernels.hpp -- CLUSTER_JACOBI (cse_schur_cluster_jacobi): the
// preconditioner M = blockdiag(M_g), M_g = S restricted to the cameras of
// cluster g (visibility_based_preconditioner.cc), factored M_g = L_g L_g^T and
// applied by a forward and a backward substitution.
//
// The cluster's cells come from the explicit complement's own kernels
// (schur_complement_kernels.hpp) over the cluster-filtered pair plan
// (cse::PlanSchurClusters): SchurPairChunkKernel<9, true> and
// SchurSparseFinishKernel store 81-double tiles, tile first_tile[g] +
// ClusterTile(i, j) = S(c_i, c_j) for the cluster's cameras c_i <= c_j, so
// every cell has the dense complement's bits.
//
// Read through its transpose, that tile IS the block (j, i) of the lower
// triangle: entry [a][b] of tile t = j (j + 1) / 2 + i is A(9 j + b, 9 i + a).
// Both kernels keep this layout, in global memory and in LDS (El below); the
// tile stride of 81 doubles is odd, so neighbouring tiles start on different
// banks.
//
//   ClusterFactorKernel  one workgroup per cluster, the cluster's tiles in
//       LDS: a blocked right-looking Cholesky over 9 x 9 tiles.  Per tile
//       column k: wave 0 factors the diagonal tile in registers (lane r holds
//       row r, column entries exchanged by shuffles); one thread per row
//       below solves its 9 entries against L_kk^T; every entry of the
//       trailing tiles (I, J), k < J <= I, takes its 9 products.  Plain FMA
//       in a fixed order; three workgroup barriers per tile column.  Stores L
//       and 1 / L_rr; on a pivot that is not positive and finite it raises the
//       status word and stores zeros, so that the apply adds zeros.
//       Optionally writes the unfactored M_g, dense row-major, both triangles.
//   ClusterApplyKernel   one workgroup per cluster loads L (once), 1 / L_rr and
//       the cluster's x segment into LDS; then wave 0 alone runs the block
//       forward and backward substitution (the 9 x 9 diagonal solves by
//       shuffles, the updates one row per lane) and y (+)= the result.  The
//       segment of camera c is at f index 9 c; a cluster's cameras need not
//       be contiguous.
// No atomics, no cross-workgroup ordering but the kernel boundaries.
//
// CLUSTER_TRIDIAGONAL (cse_schur_cluster_tridiagonal) keeps the blocks between
// the clusters of a forest's edges too: TridiagonalFactorKernel and
// TridiagonalApplyKernel, described where they stand below.
//
// schur_operators.hip alone includes this.
#ifndef CSE_CLUSTER_KERNELS_HPP_
#define CSE_CLUSTER_KERNELS_HPP_

#include "plan.hpp"
#include "schur_kernels.hpp"

namespace cse {

constexpr int kClusterThreads = 256;
constexpr int kClusterMaxTiles = kSchurMaxClusterCameras * (kSchurMaxClusterCameras + 1) / 2;

struct ClusterArgs {
  const int32_t* camera_begin;  // [clusters + 1] into cameras
  const int32_t* cameras;       // camera indices, ascending inside a cluster
  const int64_t* first_tile;    // [clusters + 1]
  const int64_t* value_begin;   // [clusters + 1]: M_g's offset in matrices
  const double* tiles;          // the unfactored tiles
  double* factor;               // L, the same tiles
  double* inv_diag;             // [9 cameras]: 1 / L_rr at 9 camera_begin[g] + r
  double* matrices;             // may be null
  int* status;
};

// LDS of a cluster of nc cameras, in bytes.  Factor: the tiles, 1 / L_rr, the
// flag word and the (I, J) of a packed tile index.  Apply: the tiles, the
// vector and 1 / L_rr.
constexpr size_t ClusterFactorLds(int64_t nc) {
  return (size_t)(nc * (nc + 1) / 2 * 81 + 9 * nc + 1) * sizeof(double) + 2 * kClusterMaxTiles;
}
constexpr size_t ClusterApplyLds(int64_t nc) {
  return (size_t)(nc * (nc + 1) / 2 * 81 + 18 * nc) * sizeof(double);
}
static_assert(ClusterFactorLds(kSchurMaxClusterCameras) <= 160 * 1024, "one cluster in one workgroup's LDS");

// Entry (r, c) of lower-triangle block t: row r of block row I, column c of
// block column J.
template <int S0>
__device__ __forceinline__ int El(int t, int r, int c) {
  return t * (S0 * S0) + c * S0 + r;
}

__device__ __forceinline__ void ClusterWaveSync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// Tile columns [0, ncols) of the blocked right-looking Cholesky of the nc x nc
// tile triangle T: ClusterFactorKernel's loop, restated for
// TridiagonalFactorKernel (ncols = nc would factor the triangle whole).  With
// ncols < nc the tiles (I, J), ncols <= J <= I, are left holding the Schur
// complement of the leading ncols tile columns: one step of the block
// tridiagonal factor.  Ends on a workgroup barrier.  ClusterFactorKernel keeps
// its own copy of the loop: compiled through this helper its instruction
// stream changed (1052 -> 1050 instructions, 74 -> 76 VGPRs).
template <int S0>
__device__ __forceinline__ void ClusterFactorColumns(double* T, double* inv, int* flag, const unsigned char* tile_i,
                                                     const unsigned char* tile_j, int tid, int nc, int ncols) {
  constexpr int kB = S0 * S0;
  for (int k = 0; k < ncols; ++k) {
    const int tkk = k * (k + 1) / 2 + k;
    // 1. The diagonal tile, by wave 0 in registers: lane r holds row r.
    if (tid < kWave) {
      const int r = tid < S0 ? tid : S0 - 1;
      double row[S0];
#pragma unroll
      for (int c = 0; c < S0; ++c) row[c] = T[El<S0>(tkk, r, c)];
      bool ok = true;
      double my_inv = 0.0;
#pragma unroll
      for (int c = 0; c < S0; ++c) {
        const double piv = __shfl(row[c], c);
        ok = ok && PivotOk(piv);
        const double l = sqrt(piv);
        const double iv = 1.0 / l;
        const double lc = r == c ? l : row[c] * iv;  // L[r][c], r >= c
        row[c] = lc;
        if (r == c) my_inv = iv;
#pragma unroll
        for (int j = c + 1; j < S0; ++j) {
          const double ljc = __shfl(lc, j);
          row[j] -= lc * ljc;  // used where r >= j alone
        }
      }
      if (tid < S0) {
#pragma unroll
        for (int c = 0; c < S0; ++c) T[El<S0>(tkk, r, c)] = c <= r ? row[c] : 0.0;
        inv[S0 * k + r] = my_inv;
      }
      if (!ok && tid == 0) *flag = 1;
    }
    __syncthreads();
    // 2. The panel: row r of block (I, k), I > k, solved against L_kk^T.
    if (tid < S0 * (nc - k - 1)) {
      const int I = k + 1 + tid / S0, r = tid % S0;
      const int t = I * (I + 1) / 2 + k;
      double x[S0];
#pragma unroll
      for (int c = 0; c < S0; ++c) {
        double v = T[El<S0>(t, r, c)];
#pragma unroll
        for (int j = 0; j < c; ++j) v -= x[j] * T[El<S0>(tkk, c, j)];
        x[c] = v * inv[S0 * k + c];
      }
#pragma unroll
      for (int c = 0; c < S0; ++c) T[El<S0>(t, r, c)] = x[c];
    }
    __syncthreads();
    // 3. The trailing tiles (I, J), k < J <= I: A_IJ -= L_Ik L_Jk^T.
    const int m = nc - k - 1;
    const int total = m * (m + 1) / 2 * kB;
    for (int idx = tid; idx < total; idx += kClusterThreads) {
      const int q = idx / kB, e = idx - q * kB;
      const int I = k + 1 + tile_i[q], J = k + 1 + tile_j[q];
      const int c = e / S0, r = e - c * S0;
      const int tik = I * (I + 1) / 2 + k, tjk = J * (J + 1) / 2 + k;
      const int at = El<S0>(I * (I + 1) / 2 + J, r, c);
      double v = T[at];
#pragma unroll
      for (int t = 0; t < S0; ++t) v -= T[El<S0>(tik, r, t)] * T[El<S0>(tjk, c, t)];
      T[at] = v;
    }
    __syncthreads();
  }
}

template <int S0>
__global__ __launch_bounds__(kClusterThreads) void ClusterFactorKernel(const ClusterArgs a) {
  constexpr int kB = S0 * S0;
  extern __shared__ double cluster_lds[];
  const int tid = threadIdx.x;
  const int g = blockIdx.x;
  const int cam0 = a.camera_begin[g];
  const int nc = a.camera_begin[g + 1] - cam0;
  const int n = S0 * nc;
  const int ntiles = nc * (nc + 1) / 2;
  double* T = cluster_lds;
  double* inv = T + ntiles * kB;
  int* flag = reinterpret_cast<int*>(inv + n);
  unsigned char* tile_i = reinterpret_cast<unsigned char*>(inv + n + 1);
  unsigned char* tile_j = tile_i + kClusterMaxTiles;
  const int64_t tile0 = a.first_tile[g];
  if (tid == 0) *flag = 0;
  if (tid < ntiles) {
    int I = 0;
    while ((I + 1) * (I + 2) / 2 <= tid) ++I;
    tile_i[tid] = (unsigned char)I;
    tile_j[tid] = (unsigned char)(tid - I * (I + 1) / 2);
  }
  for (int idx = tid; idx < ntiles * kB; idx += kClusterThreads) T[idx] = a.tiles[tile0 * kB + idx];
  __syncthreads();
  if (a.matrices) {
    // Tile (J <= I) entry [e / S0][e % S0] = M(S0 J + e / S0, S0 I + e % S0),
    // and its mirror; a diagonal tile holds both triangles already.
    double* M = a.matrices + a.value_begin[g];
    for (int idx = tid; idx < ntiles * kB; idx += kClusterThreads) {
      const int t = idx / kB, e = idx - t * kB;
      const int I = tile_i[t], J = tile_j[t];
      const int row = S0 * J + e / S0, col = S0 * I + e % S0;
      const double v = T[idx];
      M[(int64_t)row * n + col] = v;
      if (I != J) M[(int64_t)col * n + row] = v;
    }
    // Every read of the unfactored T before wave 0 writes L into tile 0
    // (a.matrices is a kernel argument: the branch is uniform).
    __syncthreads();
  }
  for (int k = 0; k < nc; ++k) {
    const int tkk = k * (k + 1) / 2 + k;
    // 1. The diagonal tile, by wave 0 in registers: lane r holds row r.
    if (tid < kWave) {
      const int r = tid < S0 ? tid : S0 - 1;
      double row[S0];
#pragma unroll
      for (int c = 0; c < S0; ++c) row[c] = T[El<S0>(tkk, r, c)];
      bool ok = true;
      double my_inv = 0.0;
#pragma unroll
      for (int c = 0; c < S0; ++c) {
        const double piv = __shfl(row[c], c);
        ok = ok && PivotOk(piv);
        const double l = sqrt(piv);
        const double iv = 1.0 / l;
        const double lc = r == c ? l : row[c] * iv;  // L[r][c], r >= c
        row[c] = lc;
        if (r == c) my_inv = iv;
#pragma unroll
        for (int j = c + 1; j < S0; ++j) {
          const double ljc = __shfl(lc, j);
          row[j] -= lc * ljc;  // used where r >= j alone
        }
      }
      if (tid < S0) {
#pragma unroll
        for (int c = 0; c < S0; ++c) T[El<S0>(tkk, r, c)] = c <= r ? row[c] : 0.0;
        inv[S0 * k + r] = my_inv;
      }
      if (!ok && tid == 0) *flag = 1;
    }
    __syncthreads();
    // 2. The panel: row r of block (I, k), I > k, solved against L_kk^T.
    if (tid < S0 * (nc - k - 1)) {
      const int I = k + 1 + tid / S0, r = tid % S0;
      const int t = I * (I + 1) / 2 + k;
      double x[S0];
#pragma unroll
      for (int c = 0; c < S0; ++c) {
        double v = T[El<S0>(t, r, c)];
#pragma unroll
        for (int j = 0; j < c; ++j) v -= x[j] * T[El<S0>(tkk, c, j)];
        x[c] = v * inv[S0 * k + c];
      }
#pragma unroll
      for (int c = 0; c < S0; ++c) T[El<S0>(t, r, c)] = x[c];
    }
    __syncthreads();
    // 3. The trailing tiles (I, J), k < J <= I: A_IJ -= L_Ik L_Jk^T.
    const int m = nc - k - 1;
    const int total = m * (m + 1) / 2 * kB;
    for (int idx = tid; idx < total; idx += kClusterThreads) {
      const int q = idx / kB, e = idx - q * kB;
      const int I = k + 1 + tile_i[q], J = k + 1 + tile_j[q];
      const int c = e / S0, r = e - c * S0;
      const int tik = I * (I + 1) / 2 + k, tjk = J * (J + 1) / 2 + k;
      const int at = El<S0>(I * (I + 1) / 2 + J, r, c);
      double v = T[at];
#pragma unroll
      for (int t = 0; t < S0; ++t) v -= T[El<S0>(tik, r, t)] * T[El<S0>(tjk, c, t)];
      T[at] = v;
    }
    __syncthreads();
  }
  const bool bad = *flag != 0;
  for (int idx = tid; idx < ntiles * kB; idx += kClusterThreads) a.factor[tile0 * kB + idx] = bad ? 0.0 : T[idx];
  for (int idx = tid; idx < n; idx += kClusterThreads) a.inv_diag[S0 * cam0 + idx] = bad ? 0.0 : inv[idx];
  if (bad && tid == 0) *a.status = 1;
}

// The block forward and backward substitution with the factor tiles T of one
// cluster of nc cameras, by one wave, in place on v: ClusterApplyKernel's two
// loops, restated for TridiagonalApplyKernel, which runs them once per path
// step (ClusterApplyKernel keeps its own copy for the same reason as above:
// 575 -> 573 instructions through the helpers).  r = min(lane, S0 - 1).
template <int S0>
__device__ __forceinline__ void ClusterSubstituteForward(const double* T, double* v, const double* inv, int nc,
                                                         int n, int lane, int r) {
  for (int k = 0; k < nc; ++k) {
    const int tkk = k * (k + 1) / 2 + k;
    {
      double xr = v[S0 * k + r], mine = 0.0;
      const double ir = inv[S0 * k + r];
      double l[S0];
#pragma unroll
      for (int c = 0; c < S0; ++c) l[c] = T[El<S0>(tkk, r, c)];
#pragma unroll
      for (int c = 0; c < S0; ++c) {
        const double wc = __shfl(xr * ir, c);
        if (r > c) xr -= l[c] * wc;
        if (r == c) mine = wc;
      }
      if (lane < S0) v[S0 * k + r] = mine;
    }
    ClusterWaveSync();
    for (int row = S0 * (k + 1) + lane; row < n; row += kWave) {
      const int I = row / S0, rr = row - I * S0;
      const int t = I * (I + 1) / 2 + k;
      double s = v[row];
#pragma unroll
      for (int c = 0; c < S0; ++c) s -= T[El<S0>(t, rr, c)] * v[S0 * k + c];
      v[row] = s;
    }
    ClusterWaveSync();
  }
}

template <int S0>
__device__ __forceinline__ void ClusterSubstituteBackward(const double* T, double* v, const double* inv, int nc,
                                                          int lane, int r) {
  for (int k = nc - 1; k >= 0; --k) {
    const int tkk = k * (k + 1) / 2 + k;
    {
      double xr = v[S0 * k + r], mine = 0.0;
      const double ir = inv[S0 * k + r];
      double l[S0];
#pragma unroll
      for (int c = 0; c < S0; ++c) l[c] = T[El<S0>(tkk, c, r)];  // L[c][r]
#pragma unroll
      for (int c = S0 - 1; c >= 0; --c) {
        const double zc = __shfl(xr * ir, c);
        if (r < c) xr -= l[c] * zc;
        if (r == c) mine = zc;
      }
      if (lane < S0) v[S0 * k + r] = mine;
    }
    ClusterWaveSync();
    for (int row = lane; row < S0 * k; row += kWave) {
      const int J = row / S0, rr = row - J * S0;
      const int t = k * (k + 1) / 2 + J;
      double s = v[row];
#pragma unroll
      for (int c = 0; c < S0; ++c) s -= T[El<S0>(t, c, rr)] * v[S0 * k + c];
      v[row] = s;
    }
    ClusterWaveSync();
  }
}

template <int S0>
__global__ __launch_bounds__(kClusterThreads) void ClusterApplyKernel(const ClusterArgs a, const double* x,
                                                                      double* y, int accumulate) {
  constexpr int kB = S0 * S0;
  extern __shared__ double cluster_lds[];
  const int tid = threadIdx.x;
  const int g = blockIdx.x;
  const int cam0 = a.camera_begin[g];
  const int nc = a.camera_begin[g + 1] - cam0;
  const int n = S0 * nc;
  const int ntiles = nc * (nc + 1) / 2;
  double* T = cluster_lds;
  double* v = T + ntiles * kB;
  double* inv = v + n;
  const int64_t tile0 = a.first_tile[g];
  for (int idx = tid; idx < ntiles * kB; idx += kClusterThreads) T[idx] = a.factor[tile0 * kB + idx];
  for (int idx = tid; idx < n; idx += kClusterThreads) {
    v[idx] = x[(int64_t)S0 * a.cameras[cam0 + idx / S0] + idx % S0];
    inv[idx] = a.inv_diag[S0 * cam0 + idx];
  }
  __syncthreads();
  if (tid >= kWave) return;  // the substitutions are one wave's
  const int lane = tid;
  const int r = lane < S0 ? lane : S0 - 1;
  // L w = x, block column by block column.
  for (int k = 0; k < nc; ++k) {
    const int tkk = k * (k + 1) / 2 + k;
    {
      double xr = v[S0 * k + r], mine = 0.0;
      const double ir = inv[S0 * k + r];
      double l[S0];
#pragma unroll
      for (int c = 0; c < S0; ++c) l[c] = T[El<S0>(tkk, r, c)];
#pragma unroll
      for (int c = 0; c < S0; ++c) {
        const double wc = __shfl(xr * ir, c);
        if (r > c) xr -= l[c] * wc;
        if (r == c) mine = wc;
      }
      if (lane < S0) v[S0 * k + r] = mine;
    }
    ClusterWaveSync();
    for (int row = S0 * (k + 1) + lane; row < n; row += kWave) {
      const int I = row / S0, rr = row - I * S0;
      const int t = I * (I + 1) / 2 + k;
      double s = v[row];
#pragma unroll
      for (int c = 0; c < S0; ++c) s -= T[El<S0>(t, rr, c)] * v[S0 * k + c];
      v[row] = s;
    }
    ClusterWaveSync();
  }
  // L^T z = w, from the last block column up.
  for (int k = nc - 1; k >= 0; --k) {
    const int tkk = k * (k + 1) / 2 + k;
    {
      double xr = v[S0 * k + r], mine = 0.0;
      const double ir = inv[S0 * k + r];
      double l[S0];
#pragma unroll
      for (int c = 0; c < S0; ++c) l[c] = T[El<S0>(tkk, c, r)];  // L[c][r]
#pragma unroll
      for (int c = S0 - 1; c >= 0; --c) {
        const double zc = __shfl(xr * ir, c);
        if (r < c) xr -= l[c] * zc;
        if (r == c) mine = zc;
      }
      if (lane < S0) v[S0 * k + r] = mine;
    }
    ClusterWaveSync();
    for (int row = lane; row < S0 * k; row += kWave) {
      const int J = row / S0, rr = row - J * S0;
      const int t = k * (k + 1) / 2 + J;
      double s = v[row];
#pragma unroll
      for (int c = 0; c < S0; ++c) s -= T[El<S0>(t, c, rr)] * v[S0 * k + c];
      v[row] = s;
    }
    ClusterWaveSync();
  }
  for (int row = lane; row < n; row += kWave) {
    const int64_t at = (int64_t)S0 * a.cameras[cam0 + row / S0] + row % S0;
    y[at] = accumulate ? y[at] + v[row] : v[row];
  }
}

// ---------------------------------------------------------------------------
// CLUSTER_TRIDIAGONAL (cse_schur_cluster_tridiagonal; cse::PlanSchurTridiagonal)
// ---------------------------------------------------------------------------
// M keeps S's blocks inside a cluster and between the two clusters of a forest
// edge; every tree of the forest is a path, and along a path g_0, g_1, .. M is
// block tridiagonal: M = L L^T with
//     A_0 = M_00;   L_kk L_kk^T = A_k;   L_{k+1,k} = M_{k+1,k} L_kk^-T;
//     A_{k+1} = M_{k+1,k+1} - L_{k+1,k} L_{k+1,k}^T.
// One step is the first n_k tile columns of ClusterFactorKernel's Cholesky on
// the combined triangle [[A_k, .], [M_{k+1,k}, M_{k+1,k+1}]] of n_k + n_{k+1}
// <= kSchurMaxClusterCameras cameras (ClusterFactorColumns): what it leaves in
// the trailing triangle is A_{k+1}.
//
//   TridiagonalFactorKernel  one workgroup per path walks it: load the edge's
//       rectangle and the next cluster's triangle behind A_k, run the step,
//       store L_kk, 1 / L_rr and the panel L_{k+1,k}, move the trailing triangle
//       to the front.  L goes to `factor`: the unfactored tiles stay.  Launched
//       twice.  The first pass factors M as it is; a pivot that is not positive
//       raises *failed.  The second ("scaled") pass returns at once when *failed
//       is clear; otherwise EVERY path is factored again with its edges'
//       rectangles multiplied by 0.5 on load (visibility_based_preconditioner.cc:
//       340-357 scales all off-diagonal cells), and a pivot that fails now
//       zeroes the path's factor and raises the status word.
//   TridiagonalApplyKernel   one workgroup per path: forward w_k = L_kk^-1 (x_k -
//       L_{k,k-1} w_{k-1}) with w kept in `scratch` (a path's vector need not fit
//       in LDS), backward z_k = L_kk^-T (w_k - L_{k+1,k}^T z_{k+1}), y (+)= z.
//       The step's tiles are streamed into LDS by the whole workgroup; wave 0
//       runs the substitutions (ClusterApplyKernel's).  x is read whole before
//       y is written: they may be one buffer.
// A rectangle's tile holds S(min, max) of its two cameras (plan.hpp): where the
// first cluster's camera is the larger one the tile is read transposed.  A
// panel tile (j of the later cluster, i of the earlier one, in path order) is
// stored at edge_tile[e] + j n_earlier + i in the LDS layout El.
struct TridiagonalArgs {
  const int32_t* camera_begin;  // [clusters + 1] into cameras
  const int32_t* cameras;
  const int64_t* first_tile;    // [clusters + 1]
  const int64_t* value_begin;   // [clusters + 1]
  const int32_t* edges;         // [edges][2]
  const int64_t* edge_tile;     // [edges + 1]
  const int64_t* edge_value;    // [edges + 1]
  const int32_t* path_begin;    // [paths + 1]
  const int32_t* path_cluster;
  const int32_t* path_edge;     // 2 e + flip, -1 at a path's end
  const double* tiles;
  double* factor;
  double* inv_diag;  // 1 / L_rr at 9 camera_begin[g] + r
  double* matrices;  // may be null
  double* scratch;   // [f columns]: the forward sweep's w
  int* failed;       // a pivot failed in the first pass
  int* status;
  int max_step;      // the launch's LDS holds a triangle of this many cameras
};

constexpr size_t TridiagonalApplyLds(int64_t ns) {
  return (size_t)(ns * (ns + 1) / 2 * 81 + 27 * ns) * sizeof(double);
}
static_assert(TridiagonalApplyLds(kSchurMaxClusterCameras) <= 160 * 1024, "one step in one workgroup's LDS");

template <int S0>
__global__ __launch_bounds__(kClusterThreads) void TridiagonalFactorKernel(const TridiagonalArgs a, int scaled) {
  constexpr int kB = S0 * S0;
  extern __shared__ double cluster_lds[];
  if (scaled && *a.failed == 0) return;  // the whole workgroup
  const int tid = threadIdx.x;
  const int q0 = a.path_begin[blockIdx.x], q1 = a.path_begin[blockIdx.x + 1];
  const int max_tiles = a.max_step * (a.max_step + 1) / 2;
  double* T = cluster_lds;
  double* inv = T + max_tiles * kB;
  int* flag = reinterpret_cast<int*>(inv + S0 * a.max_step);
  unsigned char* tile_i = reinterpret_cast<unsigned char*>(inv + S0 * a.max_step + 1);
  unsigned char* tile_j = tile_i + kClusterMaxTiles;
  if (tid == 0) *flag = 0;
  if (tid < max_tiles) {
    int I = 0;
    while ((I + 1) * (I + 2) / 2 <= tid) ++I;
    tile_i[tid] = (unsigned char)I;
    tile_j[tid] = (unsigned char)(tid - I * (I + 1) / 2);
  }
  __syncthreads();
  if (a.matrices && !scaled) {
    // The unscaled, unfactored cells from the tiles in global memory: the
    // path's cluster matrices (ClusterFactorKernel's layout) and S[g, h] of
    // its edges, dense row-major, g and h as the edge was given.
    for (int q = q0; q < q1; ++q) {
      const int g = a.path_cluster[q];
      const int nc = a.camera_begin[g + 1] - a.camera_begin[g], n = S0 * nc;
      const double* src = a.tiles + a.first_tile[g] * kB;
      double* M = a.matrices + a.value_begin[g];
      for (int idx = tid; idx < nc * (nc + 1) / 2 * kB; idx += kClusterThreads) {
        const int t = idx / kB, e = idx - t * kB;
        const int I = tile_i[t], J = tile_j[t];
        const int row = S0 * J + e / S0, col = S0 * I + e % S0;
        const double v = src[idx];
        M[(int64_t)row * n + col] = v;
        if (I != J) M[(int64_t)col * n + row] = v;
      }
      if (a.path_edge[q] < 0) continue;
      const int e = a.path_edge[q] >> 1;
      const int eg = a.edges[2 * e], eh = a.edges[2 * e + 1];
      const int cg = a.camera_begin[eg], ch = a.camera_begin[eh];
      const int ng = a.camera_begin[eg + 1] - cg, nh = a.camera_begin[eh + 1] - ch;
      const double* rect = a.tiles + a.edge_tile[e] * kB;
      double* R = a.matrices + a.edge_value[e];
      for (int idx = tid; idx < ng * nh * kB; idx += kClusterThreads) {
        const int t = idx / kB, el = idx - t * kB;
        const int i = t / nh, j = t - i * nh;
        const bool direct = a.cameras[cg + i] < a.cameras[ch + j];  // the tile is S(g's, h's)
        const int ra = direct ? el / S0 : el % S0, cb = direct ? el % S0 : el / S0;
        R[(int64_t)(S0 * i + ra) * (S0 * nh) + S0 * j + cb] = rect[idx];
      }
    }
  }
  int g = a.path_cluster[q0];
  int n1 = a.camera_begin[g + 1] - a.camera_begin[g];
  for (int idx = tid; idx < n1 * (n1 + 1) / 2 * kB; idx += kClusterThreads) T[idx] = a.tiles[a.first_tile[g] * kB + idx];
  for (int q = q0; q < q1; ++q) {
    const int pe = a.path_edge[q];
    const int e = pe >> 1;
    int h = -1, n2 = 0;
    if (pe >= 0) {
      h = a.path_cluster[q + 1];
      const int c1 = a.camera_begin[g], c2 = a.camera_begin[h];
      n2 = a.camera_begin[h + 1] - c2;
      const bool flip = (pe & 1) != 0;  // g is the edge's second cluster
      const double* rect = a.tiles + a.edge_tile[e] * kB;
      const double scale = scaled ? 0.5 : 1.0;
      // Block (n1 + j, i) of the combined triangle: rows of h's camera j,
      // columns of g's camera i; El = S(g's, h's)[c][r] at c S0 + r.
      for (int idx = tid; idx < n1 * n2 * kB; idx += kClusterThreads) {
        const int t = idx / kB, el = idx - t * kB;
        const int j = t / n1, i = t - j * n1;
        const int src_tile = flip ? j * n1 + i : i * n2 + j;
        const bool direct = a.cameras[c1 + i] < a.cameras[c2 + j];  // the tile is S(g's, h's)
        const int src_el = direct ? el : (el % S0) * S0 + el / S0;
        const int I = n1 + j;
        T[(I * (I + 1) / 2 + i) * kB + el] = scale * rect[src_tile * kB + src_el];
      }
      const double* tri = a.tiles + a.first_tile[h] * kB;
      for (int idx = tid; idx < n2 * (n2 + 1) / 2 * kB; idx += kClusterThreads) {
        const int t = idx / kB, el = idx - t * kB;
        const int I = n1 + tile_i[t], J = n1 + tile_j[t];
        T[(I * (I + 1) / 2 + J) * kB + el] = tri[idx];
      }
    }
    __syncthreads();
    ClusterFactorColumns<S0>(T, inv, flag, tile_i, tile_j, tid, n1 + n2, n1);
    for (int idx = tid; idx < n1 * (n1 + 1) / 2 * kB; idx += kClusterThreads)
      a.factor[a.first_tile[g] * kB + idx] = T[idx];
    for (int idx = tid; idx < S0 * n1; idx += kClusterThreads) a.inv_diag[S0 * a.camera_begin[g] + idx] = inv[idx];
    if (pe >= 0) {
      double* panel = a.factor + a.edge_tile[e] * kB;
      for (int idx = tid; idx < n1 * n2 * kB; idx += kClusterThreads) {
        const int t = idx / kB, el = idx - t * kB;
        const int j = t / n1, i = t - j * n1;
        const int I = n1 + j;
        panel[idx] = T[(I * (I + 1) / 2 + i) * kB + el];
      }
      __syncthreads();  // the panel is read before the move overwrites it
      // The trailing triangle A_h to the front.  A destination index is never
      // above its source and both ascend, so per batch of one entry a thread a
      // barrier between the reads and the writes is enough.
      const int total = n2 * (n2 + 1) / 2 * kB;
      for (int base = 0; base < total; base += kClusterThreads) {
        const int idx = base + tid;
        double v = 0.0;
        if (idx < total) {
          const int t = idx / kB, el = idx - t * kB;
          const int I = n1 + tile_i[t], J = n1 + tile_j[t];
          v = T[(I * (I + 1) / 2 + J) * kB + el];
        }
        __syncthreads();
        if (idx < total) T[idx] = v;
      }
      g = h;
      n1 = n2;
    }
  }
  __syncthreads();
  if (*flag == 0) return;
  if (!scaled) {
    if (tid == 0) *a.failed = 1;
    return;
  }
  // Not positive definite even with halved edges: the path's factor is zeroed,
  // so its apply adds zeros, and the status word says so.
  for (int q = q0; q < q1; ++q) {
    const int c = a.path_cluster[q];
    const int c0 = a.camera_begin[c], nc = a.camera_begin[c + 1] - c0;
    for (int idx = tid; idx < nc * (nc + 1) / 2 * kB; idx += kClusterThreads) a.factor[a.first_tile[c] * kB + idx] = 0.0;
    for (int idx = tid; idx < S0 * nc; idx += kClusterThreads) a.inv_diag[S0 * c0 + idx] = 0.0;
    if (a.path_edge[q] < 0) continue;
    const int e = a.path_edge[q] >> 1;
    const int cells = (int)(a.edge_tile[e + 1] - a.edge_tile[e]) * kB;
    for (int idx = tid; idx < cells; idx += kClusterThreads) a.factor[a.edge_tile[e] * kB + idx] = 0.0;
  }
  if (tid == 0) *a.status = 1;
}

template <int S0>
__global__ __launch_bounds__(kClusterThreads) void TridiagonalApplyKernel(const TridiagonalArgs a, const double* x,
                                                                          double* y, int accumulate) {
  constexpr int kB = S0 * S0;
  extern __shared__ double cluster_lds[];
  const int tid = threadIdx.x;
  const int q0 = a.path_begin[blockIdx.x], q1 = a.path_begin[blockIdx.x + 1];
  const int max_tiles = a.max_step * (a.max_step + 1) / 2;
  double* T = cluster_lds;               // L_kk, then the step's panel
  double* v = T + max_tiles * kB;        // the step's segment
  double* other = v + S0 * a.max_step;   // the neighbour's: w_{k-1} or z_{k+1}
  double* inv = other + S0 * a.max_step;
  const int lane = tid;
  const int r = lane < S0 ? lane : S0 - 1;
  int np = 0;  // cameras of the neighbour
  // Forward: w_k = L_kk^-1 (x_k - L_{k,k-1} w_{k-1}).
  for (int q = q0; q < q1; ++q) {
    const int g = a.path_cluster[q];
    const int cam0 = a.camera_begin[g];
    const int nc = a.camera_begin[g + 1] - cam0, n = S0 * nc;
    const int ntiles = nc * (nc + 1) / 2;
    double* P = T + ntiles * kB;
    for (int idx = tid; idx < ntiles * kB; idx += kClusterThreads) T[idx] = a.factor[a.first_tile[g] * kB + idx];
    if (q > q0) {
      const double* panel = a.factor + a.edge_tile[a.path_edge[q - 1] >> 1] * kB;
      for (int idx = tid; idx < nc * np * kB; idx += kClusterThreads) P[idx] = panel[idx];
    }
    for (int idx = tid; idx < n; idx += kClusterThreads) {
      v[idx] = x[(int64_t)S0 * a.cameras[cam0 + idx / S0] + idx % S0];
      inv[idx] = a.inv_diag[S0 * cam0 + idx];
    }
    __syncthreads();
    if (tid < kWave) {
      if (q > q0) {
        for (int row = lane; row < n; row += kWave) {
          const int j = row / S0, rr = row - j * S0;
          double s = v[row];
          for (int i = 0; i < np; ++i) {
#pragma unroll
            for (int c = 0; c < S0; ++c) s -= P[El<S0>(j * np + i, rr, c)] * other[S0 * i + c];
          }
          v[row] = s;
        }
        ClusterWaveSync();
      }
      ClusterSubstituteForward<S0>(T, v, inv, nc, n, lane, r);
      for (int row = lane; row < n; row += kWave) {
        other[row] = v[row];
        if (q + 1 < q1) a.scratch[(int64_t)S0 * a.cameras[cam0 + row / S0] + row % S0] = v[row];
      }
    }
    np = nc;
    __syncthreads();
  }
  // Backward: z_k = L_kk^-T (w_k - L_{k+1,k}^T z_{k+1}).  The last cluster's
  // L_kk, 1 / L_rr and w are still in LDS.
  for (int q = q1 - 1; q >= q0; --q) {
    const int g = a.path_cluster[q];
    const int cam0 = a.camera_begin[g];
    const int nc = a.camera_begin[g + 1] - cam0, n = S0 * nc;
    const int ntiles = nc * (nc + 1) / 2;
    double* P = T + ntiles * kB;
    if (q < q1 - 1) {
      for (int idx = tid; idx < ntiles * kB; idx += kClusterThreads) T[idx] = a.factor[a.first_tile[g] * kB + idx];
      const double* panel = a.factor + a.edge_tile[a.path_edge[q] >> 1] * kB;
      for (int idx = tid; idx < nc * np * kB; idx += kClusterThreads) P[idx] = panel[idx];
      for (int idx = tid; idx < n; idx += kClusterThreads) {
        v[idx] = a.scratch[(int64_t)S0 * a.cameras[cam0 + idx / S0] + idx % S0];
        inv[idx] = a.inv_diag[S0 * cam0 + idx];
      }
      __syncthreads();
    }
    if (tid < kWave) {
      if (q < q1 - 1) {
        // Panel tile (j of the later cluster, i of this one) is at j nc + i.
        for (int row = lane; row < n; row += kWave) {
          const int i = row / S0, c = row - i * S0;
          double s = v[row];
          for (int j = 0; j < np; ++j) {
#pragma unroll
            for (int rr = 0; rr < S0; ++rr) s -= P[El<S0>(j * nc + i, rr, c)] * other[S0 * j + rr];
          }
          v[row] = s;
        }
        ClusterWaveSync();
      }
      ClusterSubstituteBackward<S0>(T, v, inv, nc, lane, r);
      for (int row = lane; row < n; row += kWave) {
        other[row] = v[row];
        const int64_t at = (int64_t)S0 * a.cameras[cam0 + row / S0] + row % S0;
        y[at] = accumulate ? y[at] + v[row] : v[row];
      }
    }
    np = nc;
    __syncthreads();
  }
}

}  // namespace cse

#endif  // CSE_CLUSTER_KERNELS_HPP_
