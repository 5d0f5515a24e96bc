// host_shared.hpp -- the constants and plain records that the host-only
// planner (plan.cpp) and the kernels both need.  Plain C++: no HIP include,
// nothing __device__.  kernel_common.hpp, operator_kernels.hpp and
// evaluate_kernel.hpp include it, so kernel TUs see the same names as before.
#ifndef CSE_HOST_SHARED_HPP_
#define CSE_HOST_SHARED_HPP_

#include <stdint.h>

namespace cse {

constexpr int kBlockThreads = 256;
constexpr int kWave = 64;
constexpr int kWavesPerBlock = kBlockThreads / kWave;
constexpr int kMaxSlots = 10;  // parameter blocks per residual block (table path)

// Device copy of a parameter block (table path).  plus_jacobian_offset:
// >= 0 the explicit matrix, -1 none, kPlusJacobianQuaternion the
// CSE_MANIFOLD_QUATERNION_EUCLIDEAN manifold (built in registers).
constexpr int64_t kPlusJacobianQuaternion = -2;
struct PbDev {
  int64_t state_offset;
  int64_t delta_offset;
  int64_t plus_jacobian_offset;
  int32_t tangent_size;
  int32_t is_constant;
};

// Row stride (doubles) of the repacked slot-0 table that the LDS-DMA gather
// reads: the block's size rounded up to 16 bytes and then to a power of two
// up to 128 bytes, so that no row straddles a 128-byte L2 line (16 doubles
// for the 9-double BAL camera).  Each DMA instruction then touches one line
// per row instead of 1.5 on average: the residual-only evaluation of
// problem-13682 went from 0.487 to 0.420 ms (profiles/round2/s4e).
constexpr int PackedRowDoubles(int s) {
  const int p = (s + 1) & ~1;
  return p <= 2 ? 2 : p <= 4 ? 4 : p <= 8 ? 8 : p <= 16 ? 16 : p;
}

// Parameter blocks with many blocks (cameras): their block lists are cut
// into chunks of at most kGradChunk blocks, one wave per chunk
// (GradientLanesKernel), and GradientChunkReduceKernel adds each parameter
// block's chunk partials in order.  Deterministic, no atomics.  (An
// element-per-lane variant that reads whole cells per instruction measured
// 3-10 % slower: the random cells and residual pairs cost whole lines
// either way.)
constexpr int kGradChunk = 512;

// Program::Plus for manifold-free blocks: runs of consecutive state entries
// whose delta offset is a constant shift away (one run for a BAL problem).
struct PlusRun {
  int64_t state_begin;
  int64_t length;
  int64_t delta_shift;  // delta index = state index - delta_shift
};

// A CSE_MANIFOLD_QUATERNION_EUCLIDEAN block of Program::Plus
// (QuaternionPlusKernel, one block per thread).
struct QuatPlusBlock {
  int64_t state_offset;
  int64_t delta_offset;
  int32_t size;
  int32_t pad;
};

// One non-constant parameter block of cse_cgnr_init's block-Jacobi
// preconditioner (PlanCgnrBlocks in plan.cpp): its tangent_size x tangent_size
// row-major block starts at value_offset of the packed values, as
// BlockCRSJacobiPreconditioner stores its blocks.
struct CgnrBlock {
  int64_t delta_offset;
  int64_t value_offset;
  int32_t tangent_size;
  int32_t pad;
};

// Largest block JACOBI takes (the affine path's slot limit).
constexpr int kCgnrMaxBlockColumns = 16;

// Flags of a table group's per-chunk store run record (BuildTableRuns in
// plan.cpp writes them, TableStores in evaluate_kernel.hpp reads them).
constexpr int kTableRunFlagResiduals = 1, kTableRunFlagBsm = 2, kTableRunFlagCrs = 4;

}  // namespace cse

#endif  // CSE_HOST_SHARED_HPP_
