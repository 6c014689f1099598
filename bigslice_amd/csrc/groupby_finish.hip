// Finish of a K9 table straight into shuffle partitions: the used slots
// leave the table already grouped by partition id, so the compacted copy
// that k_groupby_compact writes and hash_partition re-reads never exists.
//
// The partition id of a slot is hash_row over its one int64 key with
// seed 0, % nparts: what hash_partition(..., 0) and hashing.hash_columns
// give, so every rank and every consumer agrees on it.  The table has
// cap + 1 slots; slot cap (the sentinel key's) is live iff flags[0].
//
// Three launches, ordered by the stream; no workgroup waits on another:
//   1. k_gbf_count    each workgroup owns a contiguous slot range and
//                     histograms its live slots by partition in LDS:
//                     hist[p][block].
//   2. k_gbf_offsets  one workgroup per partition: exclusive scan of its
//                     row of hist over the blocks, the partition's total,
//                     and (workgroup 0) the flags for the one readback.
//   3. k_gbf_write    re-reads the range, ranks each live slot inside its
//                     partition with an LDS cursor that starts at
//                     partition start + hist[p][block], and stores key
//                     and values there: each partition's rows of a block
//                     are one run.
//
// hist is partition-major so that the scan of step 2 reads consecutive
// counters.  The host picks the block count (gbf_blocks in ext.hip): at
// most GBF_THREADS, so that step 2 is one counter per thread.

#include <hip/hip_runtime.h>

#include "hashtable.h"

#define GBF_THREADS 512
#define GBF_WAVES (GBF_THREADS / 64)
#define GBF_MAX_PARTS 4096
#define GBF_SCAN_C (GBF_MAX_PARTS / GBF_THREADS)

struct FinishCols {
  ColDesc tab[MAX_COLS];
  MutColDesc out[MAX_COLS];
  int n;
};

__device__ __forceinline__ uint32_t gbf_part(int64_t k, uint32_t nparts) {
  return mm3_u64((uint64_t)k, 0u) % nparts;
}

// Calls f(slot, key) for every live slot of [start, end), end <= cap + 1.
// WIDE: two adjacent slots per 16-byte load (tkeys 16-byte aligned, start
// even), else one slot per load.
template <bool WIDE, typename F>
__device__ __forceinline__ void gbf_live_slots(const int64_t* tkeys,
                                               int64_t cap, bool sentinel,
                                               int64_t start, int64_t end,
                                               F f) {
  auto one = [&](int64_t i, int64_t k) {
    if (i < cap ? k != GB_SENTINEL : sentinel) f(i, k);
  };
  if constexpr (WIDE) {
    for (int64_t i = start + 2 * threadIdx.x; i < end;
         i += 2 * GBF_THREADS) {
      if (i + 1 < end) {
        const longlong2 two = *(const longlong2*)(tkeys + i);
        one(i, two.x);
        one(i + 1, two.y);
      } else {
        one(i, tkeys[i]);
      }
    }
  } else {
    for (int64_t i = start + threadIdx.x; i < end; i += GBF_THREADS)
      one(i, tkeys[i]);
  }
}

extern "C" __global__ __launch_bounds__(GBF_THREADS) void k_gbf_count(
    const int64_t* tkeys, int64_t cap, int64_t slots_per_block,
    uint32_t nparts, const int32_t* flags, uint32_t* hist) {
  __shared__ uint32_t lh[GBF_MAX_PARTS];
  for (uint32_t p = threadIdx.x; p < nparts; p += GBF_THREADS) lh[p] = 0;
  __syncthreads();
  const int64_t start = (int64_t)blockIdx.x * slots_per_block;
  const int64_t end = min(start + slots_per_block, cap + 1);
  const bool sentinel = flags[0] != 0;
  auto count = [&](int64_t, int64_t k) {
    atomicAdd(&lh[gbf_part(k, nparts)], 1u);
  };
  if (((uintptr_t)tkeys & 15) == 0)
    gbf_live_slots<true>(tkeys, cap, sentinel, start, end, count);
  else
    gbf_live_slots<false>(tkeys, cap, sentinel, start, end, count);
  __syncthreads();
  for (uint32_t p = threadIdx.x; p < nparts; p += GBF_THREADS)
    hist[(int64_t)p * gridDim.x + blockIdx.x] = lh[p];
}

// Exclusive scan of one value per thread over the workgroup; *total gets
// the sum.  wtmp: GBF_WAVES words of LDS.  Ends with a barrier.
__device__ __forceinline__ uint32_t gbf_block_scan(uint32_t x,
                                                   uint32_t* wtmp,
                                                   uint32_t* total) {
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  uint32_t run = x;  // inclusive wave scan
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t up = __shfl_up(run, off);
    if (lane >= off) run += up;
  }
  if (lane == 63) wtmp[w] = run;
  __syncthreads();
  uint32_t base = 0, all = 0;
  for (int w2 = 0; w2 < GBF_WAVES; ++w2) {
    if (w2 < w) base += wtmp[w2];
    all += wtmp[w2];
  }
  *total = all;
  __syncthreads();
  return base + run - x;
}

// host[0..nparts) = rows per partition, host[nparts] = sentinel_seen,
// host[nparts + 1] = overflow: what the one readback carries.
extern "C" __global__ __launch_bounds__(GBF_THREADS) void k_gbf_offsets(
    uint32_t* hist, uint32_t nblocks, uint32_t nparts, const int32_t* flags,
    uint32_t* totals, int64_t* host) {
  __shared__ uint32_t wtmp[GBF_WAVES];
  const uint32_t p = blockIdx.x;
  uint32_t* row = hist + (int64_t)p * nblocks;
  const bool ok = threadIdx.x < nblocks;
  const uint32_t x = ok ? row[threadIdx.x] : 0;
  uint32_t total;
  const uint32_t excl = gbf_block_scan(x, wtmp, &total);
  if (ok) row[threadIdx.x] = excl;
  if (threadIdx.x == 0) {
    totals[p] = total;
    host[p] = (int64_t)total;
    if (p == 0) {
      host[nparts] = flags[0];
      host[nparts + 1] = flags[1];
    }
  }
}

// A GroupTable's value columns are 4 or 8 bytes wide (the wrapper checks).
__device__ __forceinline__ void gbf_copy_elt(const MutColDesc& dst,
                                             int64_t di, const ColDesc& src,
                                             int64_t si) {
  if (elt_size(src.code) == 4)
    ((uint32_t*)dst.ptr)[di] = ((const uint32_t*)src.ptr)[si];
  else
    ((uint64_t*)dst.ptr)[di] = ((const uint64_t*)src.ptr)[si];
}

extern "C" __global__ __launch_bounds__(GBF_THREADS) void k_gbf_write(
    const int64_t* tkeys, int64_t cap, int64_t slots_per_block,
    uint32_t nparts, const int32_t* flags, const uint32_t* hist,
    const uint32_t* totals, FinishCols cols, int64_t* out_keys) {
  __shared__ uint32_t lcur[GBF_MAX_PARTS];
  __shared__ uint32_t wtmp[GBF_WAVES];
  // partition starts: exclusive scan of totals, GBF_SCAN_C adjacent
  // entries per thread
  uint32_t t[GBF_SCAN_C];
  uint32_t sum = 0;
#pragma unroll
  for (int j = 0; j < GBF_SCAN_C; ++j) {
    const uint32_t p = threadIdx.x * GBF_SCAN_C + j;
    t[j] = p < nparts ? totals[p] : 0;
    sum += t[j];
  }
  uint32_t unused;
  uint32_t run = gbf_block_scan(sum, wtmp, &unused);
#pragma unroll
  for (int j = 0; j < GBF_SCAN_C; ++j) {
    const uint32_t p = threadIdx.x * GBF_SCAN_C + j;
    if (p < nparts)
      lcur[p] = run + hist[(int64_t)p * gridDim.x + blockIdx.x];
    run += t[j];
  }
  __syncthreads();
  const int64_t start = (int64_t)blockIdx.x * slots_per_block;
  const int64_t end = min(start + slots_per_block, cap + 1);
  const bool sentinel = flags[0] != 0;
  auto put = [&](int64_t i, int64_t k) {
    const int64_t pos = atomicAdd(&lcur[gbf_part(k, nparts)], 1u);
    out_keys[pos] = k;
    for (int c = 0; c < cols.n; ++c)
      gbf_copy_elt(cols.out[c], pos, cols.tab[c], i);
  };
  if (((uintptr_t)tkeys & 15) == 0)
    gbf_live_slots<true>(tkeys, cap, sentinel, start, end, put);
  else
    gbf_live_slots<false>(tkeys, cap, sentinel, start, end, put);
}
