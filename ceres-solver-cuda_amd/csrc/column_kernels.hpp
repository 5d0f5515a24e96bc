// column_kernels.hpp -- the plain kernels of cse_jacobian_squared_column_norm
// and cse_jacobian_scale_columns (SparseMatrix::SquaredColumnNorm and
// ScaleColumns, internal/ceres/sparse_matrix.h:81-87) on the Jacobian values
// in HBM.  linear_operators.hip's alone; the affine norm's template kernels
// are in operator_kernels.hpp.
//
// These kernels need a group's shape only (residuals, blocks, block sizes),
// never its functor, so they are written once over run-time shape values and
// serve the library's kinds and user kinds alike.
#ifndef CSE_COLUMN_KERNELS_HPP_
#define CSE_COLUMN_KERNELS_HPP_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host_shared.hpp"

namespace cse {

// One lane per residual block.  Table addressing (affine == 0) is the
// reference's WriteJacobians addressing, as MultiplyTableKernel's: row k of
// slot j at jac_offsets[jac_layout[block] + ...], constant blocks skipped,
// tangent_size columns.  Affine addressing (affine groups without a gradient
// plan; their tables are not uploaded): row k of slot j of block i at
// jac_base[j][k] + jac_stride[j] i, columns at delta_base[j] + sz[j] id.
struct ColumnBlockArgs {
  int64_t n;
  const int32_t* ids;  // [n][nb]
  int32_t nr, nb;
  int32_t sz[kMaxSlots];
  int32_t affine;
  // table addressing
  const PbDev* pbs;
  const int64_t* gindex;
  int64_t first;
  const int64_t* jac_layout;
  const int64_t* jac_offsets;
  // affine addressing (nb <= 2, nr <= 3)
  int64_t jac_base[2][3];
  int64_t jac_stride[2];
  int64_t delta_base[2];
};

// kScale: row[c] *= v[column] (v = the scale, jac written); else
// out[column] += row[c]^2 by FP64 atomics (out zero-filled by the host).
template <bool kScale>
__global__ __launch_bounds__(kBlockThreads) void ColumnBlockKernel(const ColumnBlockArgs a, double* jac,
                                                                   const double* scale, double* out) {
  const int64_t i = (int64_t)blockIdx.x * kBlockThreads + threadIdx.x;
  if (i >= a.n) return;
  int64_t q = 0;
  if (!a.affine) q = a.jac_layout[a.gindex ? a.gindex[i] : a.first + i];
  for (int j = 0; j < a.nb; ++j) {
    const int32_t id = a.ids[i * a.nb + j];
    int64_t col0;
    int cols = a.sz[j];
    if (a.affine) {
      col0 = a.delta_base[j] + (int64_t)cols * id;
    } else {
      const PbDev pb = a.pbs[id];
      if (pb.is_constant) continue;
      col0 = pb.delta_offset;
      cols = pb.tangent_size < cols ? pb.tangent_size : cols;
    }
    for (int k = 0; k < a.nr; ++k) {
      double* row = jac + (a.affine ? a.jac_base[j][k] + a.jac_stride[j] * i : a.jac_offsets[q++]);
      for (int c = 0; c < cols; ++c) {
        if constexpr (kScale)
          row[c] *= scale[col0 + c];
        else
          unsafeAtomicAdd(out + col0 + c, row[c] * row[c]);
      }
    }
  }
}

// ScaleColumns of an affine group as a stream: J once in, once out.  One wave
// per 64-block chunk, in the evaluator's chunk numbering.  Each lane loads its
// block's ids and its parameter blocks' scale values into the wave's LDS
// table (ntab doubles per block: 6 KiB per wave at 9 + 3).  The chunk's
// contiguous runs are then walked with 16-byte loads and stores, consecutive
// lanes on consecutive pieces:
//   BlockSparse: the F run (blocks x nr x s0 doubles) and the E run (x s1);
//   CompressedRow: one run of rows, blocks x nr x (s0 + s1), the table laid
//       out in the row's column order (tab_off = each slot's column).
// Element e of a run belongs to block e / cell and table entry
// run_tab + (e % cell) % s; both follow the lane's position by additions (no
// division in the loop).  A run whose first element is not 16-byte aligned
// is walked element by element (8-byte accesses, still coalesced), and an odd
// last element goes to lane 0; a ragged last chunk only shortens the runs.
struct ScaleStreamArgs {
  int64_t n;
  const int32_t* ids;  // [n][nb]
  int32_t nb;
  int32_t ntab;        // table doubles per block
  int32_t sz[2], tab_off[2];
  int64_t delta_base[2];
  int32_t nruns;
  int64_t run_base[2];  // first double of block 0's part of the run
  int32_t run_cell[2];  // doubles per block
  int32_t run_s[2];     // doubles per row
  int32_t run_tab[2];   // the row's first table entry
};

constexpr int kScaleUnroll = 3;  // divides the 9, 3 and 12 pieces per lane of the Snavely shapes

template <int kWPB>
__global__ __launch_bounds__(kWPB * kWave) void ScaleColumnsStreamKernel(const ScaleStreamArgs a, double* jac,
                                                                         const double* scale) {
  extern __shared__ double scale_tab[];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t nchunks = (a.n + kWave - 1) / kWave;
  const int64_t c = (int64_t)blockIdx.x * kWPB + wave;
  if (c >= nchunks) return;
  double* tab = scale_tab + wave * kWave * a.ntab;
  const int64_t i0 = c * kWave;
  const int nw = a.n - i0 < kWave ? (int)(a.n - i0) : kWave;
  if (lane < nw) {
    for (int j = 0; j < a.nb; ++j) {
      const int32_t id = a.ids[(i0 + lane) * a.nb + j];
      const double* src = scale + a.delta_base[j] + (int64_t)a.sz[j] * id;
      double* dst = tab + lane * a.ntab + a.tab_off[j];
      for (int k = 0; k < a.sz[j]; ++k) dst[k] = src[k];
    }
  }
  // The table is the wave's own: its LDS operations complete in order.
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
  typedef double v2d __attribute__((ext_vector_type(2)));
  for (int r = 0; r < a.nruns; ++r) {
    const int cell = a.run_cell[r], s = a.run_s[r];
    const double* row_tab = tab + a.run_tab[r];
    double* p = jac + a.run_base[r] + (int64_t)cell * i0;
    const int total = nw * cell;
    if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
      // Lane l takes pieces l, l + 64, ...: elements 2 l and 2 l + 1.
      int e = 2 * lane;
      int blk = e / cell, w = e - blk * cell, col = w % s;
      const int dblk = (2 * kWave) / cell, dw = (2 * kWave) % cell, dcol = (2 * kWave) % s;
      // The table entries of the lane's piece, and the step to its next one.
      auto entries = [&](int& i0, int& i1) {
        int blk1 = blk, col1 = col + 1;
        if (col1 == s) col1 = 0;
        if (w + 1 == cell) ++blk1;
        i0 = blk * a.ntab + col;
        i1 = blk1 * a.ntab + col1;
        blk += dblk;
        w += dw;
        if (w >= cell) {
          w -= cell;
          ++blk;
        }
        col += dcol;
        if (col >= s) col -= s;
      };
      // kScaleUnroll pieces per lane in flight: all their loads are issued
      // before the first store (a full chunk of the 2 x (9 + 3) shape is 9 F
      // and 3 E pieces per lane, of 2 x 12 CompressedRow rows 12).
      for (; e + 2 * kWave * (kScaleUnroll - 1) + 1 < total; e += 2 * kWave * kScaleUnroll) {
        v2d v[kScaleUnroll];
        int i0[kScaleUnroll], i1[kScaleUnroll];
#pragma unroll
        for (int u = 0; u < kScaleUnroll; ++u)
          v[u] = __builtin_nontemporal_load(reinterpret_cast<const v2d*>(p + e) + u * kWave);
#pragma unroll
        for (int u = 0; u < kScaleUnroll; ++u) entries(i0[u], i1[u]);
#pragma unroll
        for (int u = 0; u < kScaleUnroll; ++u) {
          v[u].x *= row_tab[i0[u]];
          v[u].y *= row_tab[i1[u]];
          __builtin_nontemporal_store(v[u], reinterpret_cast<v2d*>(p + e) + u * kWave);
        }
      }
      for (; e + 1 < total; e += 2 * kWave) {
        int i0, i1;
        entries(i0, i1);
        v2d v = *reinterpret_cast<const v2d*>(p + e);
        v.x *= row_tab[i0];
        v.y *= row_tab[i1];
        *reinterpret_cast<v2d*>(p + e) = v;
      }
      if ((total & 1) && lane == 0) p[total - 1] *= row_tab[(nw - 1) * a.ntab + s - 1];
    } else {
      int e = lane;
      int blk = e / cell, w = e - blk * cell, col = w % s;
      const int dblk = kWave / cell, dw = kWave % cell, dcol = kWave % s;
      for (; e < total; e += kWave) {
        p[e] *= row_tab[blk * a.ntab + col];
        blk += dblk;
        w += dw;
        if (w >= cell) {
          w -= cell;
          ++blk;
        }
        col += dcol;
        if (col >= s) col -= s;
      }
    }
  }
}

}  // namespace cse

#endif  // CSE_COLUMN_KERNELS_HPP_
