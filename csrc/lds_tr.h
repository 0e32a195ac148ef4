// Transposing LDS reads (ds_read_b64_tr_b16) as inline assembly, for kernels that stream operands with LDS-DMA.
//
// The compiler's wait-count pass does not know which LDS bytes __builtin_amdgcn_ds_read_tr16_b64_v4i16 reads and
// drains every LDS-DMA in flight (s_waitcnt vmcnt(0)) before it, which serialises a DMA / MFMA pipeline: the wave
// waits for the stage it has just issued before it computes on the one that landed an iteration earlier. Reads
// issued through these helpers are invisible to that pass: the caller owns both waits. The stage read must have
// been retired by the caller's own `s_waitcnt vmcnt` + barrier, and the results are pending until the caller's own
// `s_waitcnt lgkmcnt(0)`.
#pragma once
#include "common.h"

// Rows r and r + 4 of one fragment where the second row sits a constant 1024 bytes behind the first (256-byte rows,
// slot function independent of bit 2 of the row).
template <int OFF>
__device__ __forceinline__ void tr_pair(unsigned addr, v4s& lo, v4s& hi) {
  asm volatile("ds_read_b64_tr_b16 %0, %2 offset:%3\n\tds_read_b64_tr_b16 %1, %2 offset:%4"
               : "=&v"(lo), "=&v"(hi)
               : "v"(addr), "n"(OFF), "n"(OFF + 1024)
               : "memory");
}

// Rows r and r + 4 at two lane addresses (slot function that depends on bit 2 of the row, as wswz in conv_igemm.hip).
template <int OFF>
__device__ __forceinline__ void tr_pair2(unsigned addr_lo, unsigned addr_hi, v4s& lo, v4s& hi) {
  asm volatile("ds_read_b64_tr_b16 %0, %2 offset:%4\n\tds_read_b64_tr_b16 %1, %3 offset:%4"
               : "=&v"(lo), "=&v"(hi)
               : "v"(addr_lo), "v"(addr_hi), "n"(OFF)
               : "memory");
}

__device__ __forceinline__ v8s tr_join(const v4s lo, const v4s hi) {
  return v8s{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

__device__ __forceinline__ unsigned lds_byte_addr(const void* p) {
  return (unsigned)(uintptr_t)(LDS_PTR(const void))(p);
}
