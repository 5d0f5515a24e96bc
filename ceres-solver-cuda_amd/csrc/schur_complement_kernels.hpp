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
//
// The block-sparse output (cse::PlanSchurSparse: the 9 x 9 blocks of S's upper
// triangle as block-compressed rows, BlockRandomAccessSparseMatrix's cells):
//   SchurPairChunkKernel<S0, true> + SchurSparseFinishKernel   the same sums
//       stored block by block (cse_schur_complement_sparse);
//   SchurExplicitRowKernel + SchurExplicitColumnKernel   y = S x on those
//       blocks (cse_schur_explicit_multiply).
//
// schur_operators.hip owns the plain (non-template) kernel here
// (SchurDiagonalFillKernel): no other TU of the library includes this.
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
  // The block-sparse store (kSparse kernels) only: values[k][S0][S0] in the
  // structure's order (cse::SchurSparsePlan).
  const int32_t* sparse_of_plan;  // [nblocks]: the sparse block of a plan block
  const int32_t* plan_block;      // [sparse blocks]: the inverse, -1 = added diagonal
  const int32_t* sparse_col;      // [sparse blocks]: camera index
  const int32_t* finish;          // [nfinish]: the sparse blocks the finish writes
  int64_t nfinish;
  double* values;
};

// kSparse: the block-sparse store.  The chunk of a block with one chunk adds
// D^2 and stores the block's S0 x S0 doubles straight into values (a diagonal
// block from its upper triangle, both ways); the other chunks go to partial
// as in the dense store.
template <int S0, bool kSparse = false>
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
  if constexpr (kSparse) {
    if (a.chunk_off[k + 1] - a.chunk_off[k] == 1) {
      const int32_t c = a.block_row[k];
      const bool diagonal = c == a.block_col[k];
      double* out = a.values + (int64_t)a.sparse_of_plan[k] * (S0 * S0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int mm = rsub + 4 * r;
        if (mm >= S0 || col >= S0 || (diagonal && mm > col)) continue;
        double v = 0.0;  // the finish's sum of one partial
        v += acc[r];
        if (diagonal && mm == col && a.D) {
          const double d = a.D[a.e_cols + a.f_col_base + (int64_t)S0 * c + mm];
          v += d * d;
        }
        out[mm * S0 + col] = v;
        if (diagonal) out[col * S0 + mm] = v;
      }
      return;
    }
  }
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

// The block-sparse store's finish: one thread per entry of a listed block
// (several chunks, or a diagonal added for a camera without residual blocks:
// D^2 or zeros), SchurPairFinishKernel's sums written block by block.
template <int S0>
__global__ __launch_bounds__(kBlockThreads) void SchurSparseFinishKernel(const SchurPairArgs a) {
  const int64_t idx = (int64_t)blockIdx.x * kBlockThreads + threadIdx.x;
  const int64_t i = idx / (S0 * S0);
  if (i >= a.nfinish) return;
  const int e = (int)(idx - i * (S0 * S0));
  const int m = e / S0, n = e - m * S0;
  const int64_t kk = a.finish[i];
  const int64_t k = a.plan_block[kk];
  double* out = a.values + kk * (S0 * S0);
  if (k < 0) {
    double v = 0.0;
    if (m == n && a.D) {
      const double d = a.D[a.e_cols + (int64_t)S0 * a.sparse_col[kk] + m];
      v = d * d;
    }
    out[e] = v;
    return;
  }
  const int32_t c = a.block_row[k], c2 = a.block_col[k];
  if (c == c2 && m > n) return;  // a diagonal block: the upper triangle, mirrored
  double v = 0.0;
  for (int64_t q = a.chunk_off[k]; q < a.chunk_off[k + 1]; ++q) v += a.partial[q * (S0 * S0) + e];
  if (c == c2 && m == n && a.D) {
    const double d = a.D[a.e_cols + a.f_col_base + (int64_t)S0 * c + m];
    v += d * d;
  }
  out[e] = v;
  if (c == c2) out[n * S0 + m] = v;
}

// y = S x from the block-sparse upper triangle, every block read once, in
// two kernels; no atomics, every sum in a fixed order.
struct SchurExplicitArgs {
  const int64_t *row_begin, *col_begin;  // [C + 1]
  const int32_t* block_col;              // [blocks]
  const int32_t* col_block;              // [blocks - C]
  const double* values;                  // [blocks][S0 * S0]
  const double* x;
  double* y;
  int64_t C;
};

// SchurExplicitRowKernel: camera c's workgroup walks its ROW blocks alone, cut
// over the waves by SchurExplicitPer(row blocks).  Besides the row sums, each
// block S(c, c'), c' > c, leaves its column contribution S(c, c')^T x_c, S0
// doubles, in contrib[block]: per batch of kSchurExplicitBatch blocks the
// lanes put S[e] x[S0 c + e / S0] into the wave's LDS tile and lane (u, n) adds entries
// (0..S0, n) of block u in that order.  y = the row sums, per wave in wave
// order.  SchurExplicitColumnKernel then adds to y of camera c the
// contributions of its column blocks: slot s of kSchurExplicitSlots sums the
// list entries s, s + slots, .. in list order, thread i adds the slots in
// slot order.  Every block of values is read once.  x and y may not overlap
// (y_c is assigned while other workgroups read x).
constexpr int kSchurExplicitBatch = 7;  // blocks per batch: S0 lanes each in one wave

template <int S0>
__global__ __launch_bounds__(kSchurExplicitWaves* kWave) void SchurExplicitRowKernel(
    const SchurExplicitArgs a, double* contrib) {
  constexpr int kB = S0 * S0, kU = kSchurExplicitBatch;
  static_assert(kB > kWave && kB <= 2 * kWave, "two entries a lane");
  static_assert(kU * S0 <= kWave, "a lane per column sum of a batch");
  __shared__ double tile_all[kSchurExplicitWaves][kU * kB];
  __shared__ double sums[kSchurExplicitWaves][kB];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  double* tile = tile_all[wave];
  const int64_t c = blockIdx.x;
  const int64_t r0 = a.row_begin[c], nrow = a.row_begin[c + 1] - r0;
  const int64_t per = SchurExplicitPer(nrow);
  const int64_t lo = wave * per, hi = lo + per < nrow ? lo + per : nrow;
  const int e0 = lane, e1 = lane + kWave;
  const bool two = e1 < kB;
  const int n0 = e0 % S0, n1 = two ? e1 % S0 : 0, m0 = e0 / S0, m1 = two ? e1 / S0 : 0;
  const double xm0 = a.x[(int64_t)S0 * c + m0], xm1 = a.x[(int64_t)S0 * c + m1];
  const int tu = lane / S0, tn = lane - tu * S0;
  double ra = 0.0, rb = 0.0;
  for (int64_t base = lo; base < hi; base += kWave) {
    const int cnt = (int)(hi - base < kWave ? hi - base : kWave);
    const int my_cam = a.block_col[r0 + base + (lane < cnt ? lane : cnt - 1)];
    for (int g = 0; g < cnt; g += kU) {
      double v0[kU], v1[kU], x0[kU], x1[kU];
      const double* v[kU];
      const double* xc[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int i = g + u < cnt ? g + u : cnt - 1;  // past the end: the last block again, not used
        v[u] = a.values + (r0 + base + i) * kB;
        xc[u] = a.x + (int64_t)S0 * __builtin_amdgcn_readlane(my_cam, i);
        v0[u] = v[u][e0];
        x0[u] = xc[u][n0];
      }
      if (two) {
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          v1[u] = v[u][e1];
          x1[u] = xc[u][n1];
        }
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        if (g + u >= cnt) break;
        ra += v0[u] * x0[u];
        tile[u * kB + e0] = v0[u] * xm0;
        if (two) {
          rb += v1[u] * x1[u];
          tile[u * kB + e1] = v1[u] * xm1;
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_wave_barrier();
      // (the diagonal block, first of the row, has no column contribution)
      if (tu < kU && g + tu < cnt && base + g + tu > 0) {
        double s = 0.0;
#pragma unroll
        for (int m = 0; m < S0; ++m) s += tile[tu * kB + m * S0 + tn];
        contrib[(r0 + base + g + tu) * S0 + tn] = s;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_wave_barrier();
    }
  }
  sums[wave][e0] = ra;
  if (two) sums[wave][e1] = rb;
  __syncthreads();
  if (threadIdx.x < S0) {
    const int i = threadIdx.x;
    double y = 0.0;
    for (int w = 0; w < kSchurExplicitWaves; ++w) {
      double r = 0.0;
      for (int n = 0; n < S0; ++n) r += sums[w][i * S0 + n];
      y += r;
    }
    a.y[(int64_t)S0 * c + i] = y;
  }
}

template <int S0>
__global__ __launch_bounds__(kBlockThreads) void SchurExplicitColumnKernel(const SchurExplicitArgs a,
                                                                           const double* contrib) {
  constexpr int kSlots = kSchurExplicitSlots;
  static_assert(kSlots * S0 <= kBlockThreads, "a thread per slot and entry");
  __shared__ double part[kSlots][S0];
  const int64_t c = blockIdx.x;
  const int64_t t0 = a.col_begin[c], t1 = a.col_begin[c + 1];
  if (t0 == t1) return;  // the whole workgroup: y keeps its row sums
  const int s = threadIdx.x / S0, n = threadIdx.x - s * S0;
  if (s < kSlots) {
    double acc = 0.0;
#pragma unroll 4
    for (int64_t j = t0 + s; j < t1; j += kSlots) acc += contrib[(int64_t)a.col_block[j] * S0 + n];
    part[s][n] = acc;
  }
  __syncthreads();
  if (threadIdx.x < S0) {
    double r = 0.0;
    for (int q = 0; q < kSlots; ++q) r += part[q][threadIdx.x];
    a.y[(int64_t)S0 * c + threadIdx.x] += r;
  }
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
