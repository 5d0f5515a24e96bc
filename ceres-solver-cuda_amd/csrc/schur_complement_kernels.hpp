// schur_complement_kernels.hpp -- the explicit Schur complement: the dense
// reduced camera matrix S that SchurEliminator::Eliminate forms for
// DENSE_SCHUR (internal/ceres/schur_eliminator_impl.h, schur_complement_
// solver.cc), from the Jacobian values, D and the per-point inverses M_p that
// cse_schur_init bound and computed (schur_kernels.hpp).
//
// With Q_bb' = delta_bb' I - E_b M_p E_b'^T (2 x 2) for two residual blocks b,
// b' of one e block p, the block of S at (f block c, f block c') is
//     S(c, c') = delta_cc' D_c^2 + sum over the pairs (b, b') with
//                f(b) = c, f(b') = c' of  F_b^T Q_bb' F_b'.
// The host plan (cse::PlanSchurPairs, plan.hpp) lists the pairs of every
// non-zero block of the upper triangle, block by block, and cuts each
// block's list into work chunks of at most kSchurPairChunk pairs.
//
//   SchurPairChunkKernel   one wave per chunk: the chunk's sum as ONE matrix
//       product C (16 x 16) += A^T B over two rows per pair, A = [F_b rows]
//       and B = [rows of Q_bb' F_b'] (9 of 16 columns each), on the matrix
//       cores as SchurCameraPassKernel: per slab of 32 pairs each lane
//       gathers one row of one pair into the wave's LDS slab, then
//       v_mfma_f64_16x16x4_f64 takes the slab's rows four at a time.  The
//       9 x 9 sum goes to partial[chunk].
//   SchurPairFinishKernel  one thread per entry of a block: its chunk
//       partials added in chunk order, D^2 on the diagonal, and the value
//       stored at (c, c') and at its mirror (c', c) -- a diagonal block
//       from its upper triangle alone -- so S is symmetric bit for bit.
// No atomics; every sum runs in the plan's order: bit-identical run to run.
// The caller zeroes S first (blocks of f blocks that share no e block) and
// writes D^2 on the diagonal (f blocks without residual blocks).
#ifndef CSE_SCHUR_COMPLEMENT_KERNELS_HPP_
#define CSE_SCHUR_COMPLEMENT_KERNELS_HPP_

#include "plan.hpp"
#include "schur_kernels.hpp"

namespace cse {

struct SchurPairArgs {
  const int32_t* ids;      // [n][2]: f block, e block
  const double* jac;       // BlockSparseMatrix values
  int64_t f_base, e_base;  // cell of block i: F at f_base + 2 S0 i, E at e_base + 6 i
  int64_t f_col_base;      // f index of f block id: f_col_base + S0 id
  int64_t e_col_base;      // e column of e block id: e_col_base + 3 id
  int64_t e_cols;          // D[e_cols + k] scales f column k
  const double* D;         // may be null
  const double* ete_inv;   // M_p, packed upper triangle, at 2 * (e column of p)
  const int32_t *block_row, *block_col;      // [nblocks]
  const int64_t *pair_begin, *chunk_off;     // [nblocks + 1]
  const int32_t* chunk_block;                // [nchunks]
  const int32_t* pairs;                      // [npairs][2]
  int64_t nblocks, nchunks;
  double* partial;  // [nchunks][S0 * S0]
  double* S;        // row-major, leading dimension ld
  int64_t ld;
};

template <int S0>
__global__ __launch_bounds__(kBlockThreads) void SchurPairChunkKernel(const SchurPairArgs a) {
  static_assert(S0 <= 16, "A^T B in one 16 x 16 f64 tile");
  constexpr int kW = 2 * S0;        // doubles per LDS row: F_b row | (Q F_b') row
  constexpr int kSlab = kWave / 2;  // pairs per slab: one lane per row, two rows per pair
  constexpr int kRows = 2 * kSlab;
  typedef double v4d __attribute__((ext_vector_type(4)));
  __shared__ double slab_all[kWavesPerBlock][kRows * kW];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t q = (int64_t)blockIdx.x * kWavesPerBlock + wave;
  if (q >= a.nchunks) return;
  double* slab = slab_all[wave];
  const int64_t k = a.chunk_block[q];
  const int64_t p0 = a.pair_begin[k] + (q - a.chunk_off[k]) * kSchurPairChunk;
  const int64_t pe = a.pair_begin[k + 1];
  const int64_t p1 = p0 + kSchurPairChunk < pe ? p0 + kSchurPairChunk : pe;
  const int col = lane & 15, rsub = lane >> 4;
  const int bl = lane >> 1, h = lane & 1;  // pair of the slab, row of the pair
  v4d acc = {0.0, 0.0, 0.0, 0.0};
  for (int64_t ps = p0; ps < p1; ps += kSlab) {
    const int nb = (int)(p1 - ps < kSlab ? p1 - ps : kSlab);
    if (bl < nb) {
      const int64_t b = a.pairs[2 * (ps + bl)], b2 = a.pairs[2 * (ps + bl) + 1];
      const int id1 = a.ids[2 * b + 1];
      const double* m = a.ete_inv + 2 * (a.e_col_base + 3LL * id1);
      double M[6], E2[6], Eh[3];
#pragma unroll
      for (int t = 0; t < 6; ++t) M[t] = m[t];
      const double* e2 = a.jac + a.e_base + 6 * b2;
#pragma unroll
      for (int t = 0; t < 6; ++t) E2[t] = e2[t];
      const double* eh = a.jac + a.e_base + 6 * b + 3 * h;
#pragma unroll
      for (int t = 0; t < 3; ++t) Eh[t] = eh[t];
      // Row h of Q = delta I - E_b M E_b'^T.
      double me0[3], me1[3];
      SymMul3(M, E2, me0);
      SymMul3(M, E2 + 3, me1);
      const double d = b == b2 ? 1.0 : 0.0;
      const double q0 = (h == 0 ? d : 0.0) - (Eh[0] * me0[0] + Eh[1] * me0[1] + Eh[2] * me0[2]);
      const double q1 = (h == 1 ? d : 0.0) - (Eh[0] * me1[0] + Eh[1] * me1[1] + Eh[2] * me1[2]);
      const double* fh = a.jac + a.f_base + 2 * S0 * b + S0 * h;
      const double* f2 = a.jac + a.f_base + 2 * S0 * b2;
      double* r = slab + (2 * bl + h) * kW;
#pragma unroll
      for (int t = 0; t < S0; ++t) {
        r[t] = fh[t];
        r[S0 + t] = q0 * f2[t] + q1 * f2[S0 + t];
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    // A[m][k] = row k, column m of F_b; B[k][n] = row k, column n of Q F_b'.
    const int rows = 2 * nb;
#pragma unroll 4
    for (int s = 0; s < kRows / 4; ++s) {
      const int row = 4 * s + rsub;
      if (4 * s >= rows) break;
      const bool live = row < rows && col < S0;
      const double av = live ? slab[row * kW + col] : 0.0;
      const double bv = live ? slab[row * kW + S0 + col] : 0.0;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
  }
  // C[m][n]: m = lane / 16 + 4 r, n = lane % 16.
  double* out = a.partial + q * (S0 * S0);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int mm = rsub + 4 * r;
    if (mm < S0 && col < S0) out[mm * S0 + col] = acc[r];
  }
}

template <int S0>
__global__ __launch_bounds__(kBlockThreads) void SchurPairFinishKernel(const SchurPairArgs a) {
  const int64_t idx = (int64_t)blockIdx.x * kBlockThreads + threadIdx.x;
  const int64_t k = idx / (S0 * S0);
  if (k >= a.nblocks) return;
  const int e = (int)(idx - k * (S0 * S0));
  const int m = e / S0, n = e - m * S0;
  const int32_t c = a.block_row[k], c2 = a.block_col[k];
  if (c == c2 && m > n) return;  // a diagonal block: the upper triangle, mirrored
  double v = 0.0;
  for (int64_t q = a.chunk_off[k]; q < a.chunk_off[k + 1]; ++q) v += a.partial[q * (S0 * S0) + e];
  const int64_t row = a.f_col_base + (int64_t)S0 * c + m, cl = a.f_col_base + (int64_t)S0 * c2 + n;
  if (row == cl && a.D) {
    const double d = a.D[a.e_cols + row];
    v += d * d;
  }
  a.S[row * a.ld + cl] = v;
  a.S[cl * a.ld + row] = v;
}

// S[k][k] = D_f[k]^2: the diagonal of f blocks without residual blocks (the
// finish overwrites the others').
__global__ __launch_bounds__(kBlockThreads) void SchurDiagonalFillKernel(const double* D, int64_t off,
                                                                         double* S, int64_t ld,
                                                                         int64_t n) {
  const int64_t k = (int64_t)blockIdx.x * kBlockThreads + threadIdx.x;
  if (k >= n) return;
  const double d = D[off + k];
  S[k * ld + k] = d * d;
}

}  // namespace cse

#endif  // CSE_SCHUR_COMPLEMENT_KERNELS_HPP_
