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

}  // namespace cse

#endif  // CSE_CLUSTER_KERNELS_HPP_
