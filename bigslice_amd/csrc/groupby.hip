// K9: hash-aggregate group-by over device-resident columns.
//
// Role-parity with the reference's combiningFrame (exec/combiner.go:
// open-addressing, power-of-two capacity, grow x2 on pressure, seeded with
// hashSeed 0x9acb0442 so a previous partitioning step does not strip hash
// entropy).  The CDNA4 redesign: one pass of global-memory atomics into an
// open-addressing table in HBM/LLC; on table overflow the host doubles
// capacity and retries (the reference's rehash-x2, done batch-wise).
// Slot `cap` (one extra) is reserved for the sentinel key itself.

#include <hip/hip_runtime.h>

#include "hashtable.h"

#define THREADS 256

// Compaction: scan the table, appending used slots to the output arrays.
// Wave-aggregated cursor: one global atomicAdd per wave (64 lanes), not per
// element — a single hot counter saturates at ~88 atomics/us on this chip.
struct CompactCols {
  ColDesc tab[MAX_COLS];
  MutColDesc out[MAX_COLS];
  int n;
};

__device__ __forceinline__ void copy_elt(const MutColDesc& dst, int64_t di,
                                         const ColDesc& src, int64_t si) {
  switch (elt_size(src.code)) {
    case 1: ((uint8_t*)dst.ptr)[di] = ((const uint8_t*)src.ptr)[si]; break;
    case 2: ((uint16_t*)dst.ptr)[di] = ((const uint16_t*)src.ptr)[si]; break;
    case 4: ((uint32_t*)dst.ptr)[di] = ((const uint32_t*)src.ptr)[si]; break;
    default: ((uint64_t*)dst.ptr)[di] = ((const uint64_t*)src.ptr)[si];
  }
}

// Two-pass block-chunk compaction: each block owns a contiguous slot
// range; pass 1 counts its used slots (block reduce -> ONE cursor atomic
// per block), pass 2 writes them out at block_base + thread prefix.
// A single hot cursor saturates at ~88 atomics/us on this chip, so the
// atomic count must scale with blocks (~2k), not waves (~100k).
extern "C" __global__ void k_groupby_compact(
    const int64_t* tkeys, int64_t cap, int64_t slots_per_block,
    CompactCols cols, int64_t* out_keys, unsigned long long* cursor) {
  __shared__ uint32_t counts[THREADS];
  __shared__ unsigned long long block_base;
  int64_t start = (int64_t)blockIdx.x * slots_per_block;
  int64_t end = min(start + slots_per_block, cap);
  // pass 1: per-thread count over its strided slots
  uint32_t mine = 0;
  for (int64_t i = start + threadIdx.x; i < end; i += blockDim.x)
    mine += (tkeys[i] != GB_SENTINEL);
  counts[threadIdx.x] = mine;
  __syncthreads();
  // exclusive scan of per-thread counts (simple LDS scan, 256 wide)
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (int t = 0; t < (int)blockDim.x; ++t) {
      uint32_t c = counts[t];
      counts[t] = run;
      run += c;
    }
    block_base = run ? atomicAdd(cursor, (unsigned long long)run) : 0;
  }
  __syncthreads();
  // pass 2: write used slots at base + prefix
  int64_t pos = (int64_t)block_base + counts[threadIdx.x];
  for (int64_t i = start + threadIdx.x; i < end; i += blockDim.x) {
    int64_t k = tkeys[i];
    if (k == GB_SENTINEL) continue;
    out_keys[pos] = k;
    for (int c = 0; c < cols.n; ++c)
      copy_elt(cols.out[c], pos, cols.tab[c], i);
    ++pos;
  }
}

// Two-level insert for the single-int64-SUM shape (reference K10,
// exec/bigmachine.go:1144-1199 two-level combine): each workgroup first
// aggregates into a 1024-slot LDS table (16 KiB: small enough to keep
// full 32-wave/CU occupancy for the global-atomic path), absorbing hot
// keys entirely
// on-CU (LDS atomics), and only LDS-table misses and the end-of-block
// flush touch the global table.  At low key cardinality this removes
// the global atomic contention that serializes the one-level kernel
// (measured 4x); at high cardinality the LDS probe adds a small
// constant.
#define GB_LDS_SLOTS 1024

__device__ __forceinline__ void gb_global_insert_sum(
    int64_t k, long long v, int64_t* tkeys, long long* tab, uint64_t mask,
    int64_t cap, uint32_t seed, int32_t* sentinel_seen, int32_t* overflow,
    int64_t max_probes) {
  int64_t slot;
  if (k == GB_SENTINEL) {
    atomicOr(sentinel_seen, 1);
    slot = cap;
  } else {
    uint64_t h = mm3_u64((uint64_t)k, seed) & mask;
    if (gb_probe_claim(tkeys, h, mask, k, max_probes) == GB_FULL) {
      atomicOr(overflow, 1);
      return;
    }
    slot = (int64_t)h;
  }
  atomicAdd((unsigned long long*)&tab[slot], (unsigned long long)v);
}

// One row through the LDS table; returns false on LDS-table miss
// (caller falls back to the global table).
__device__ __forceinline__ bool gb_lds_try(int64_t k, long long v,
                                           long long* lk, long long* lv,
                                           uint32_t seed) {
  uint32_t h = mm3_u64((uint64_t)k, seed) & (GB_LDS_SLOTS - 1);
  for (int p = 0; p < 4; ++p) {  // short LDS probe chain
    long long cur = lk[h];
    if (cur == GB_SENTINEL) {
      long long prev = atomicCAS((unsigned long long*)&lk[h],
                                 (unsigned long long)GB_SENTINEL,
                                 (unsigned long long)k);
      cur = (prev == GB_SENTINEL) ? k : prev;
    }
    if (cur == k) {
      atomicAdd((unsigned long long*)&lv[h], (unsigned long long)v);
      return true;
    }
    h = (h + 1) & (GB_LDS_SLOTS - 1);
  }
  return false;
}

// Grid-stride geometry like the one-level kernel (the block-chunked
// variant measured 2.6x slower in the global-atomic regime); each
// block's LDS table aggregates its strided rows and flushes once.
extern "C" __global__ void k_groupby_insert_sum_i64_lds(
    const int64_t* keys, const int64_t* vals, int64_t n, int64_t* tkeys,
    long long* tab, int64_t cap, uint32_t seed, int32_t* sentinel_seen,
    int32_t* overflow, int64_t max_probes) {
  __shared__ long long lk[GB_LDS_SLOTS];
  __shared__ long long lv[GB_LDS_SLOTS];
  for (int i = threadIdx.x; i < GB_LDS_SLOTS; i += blockDim.x) {
    lk[i] = GB_SENTINEL;
    lv[i] = 0;
  }
  __syncthreads();
  uint64_t gmask = (uint64_t)cap - 1;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < n; i += stride) {
    int64_t k = keys[i];
    long long v = (long long)vals[i];
    if (k == GB_SENTINEL || !gb_lds_try(k, v, lk, lv, seed))
      gb_global_insert_sum(k, v, tkeys, tab, gmask, cap, seed,
                           sentinel_seen, overflow, max_probes);
  }
  __syncthreads();
  // flush the block's LDS table into the global one
  for (int i2 = threadIdx.x; i2 < GB_LDS_SLOTS; i2 += blockDim.x) {
    if (lk[i2] != GB_SENTINEL)
      gb_global_insert_sum(lk[i2], lv[i2], tkeys, tab, gmask, cap, seed,
                           sentinel_seen, overflow, max_probes);
  }
}

// Partition ids from table-slot high bits: the bucket id of the
// partitioned insert (groupby_part.hip), whose tests use this kernel
// as their oracle.
extern "C" __global__ void k_slot_pids(const int64_t* keys, int64_t n,
                                       int64_t cap, int32_t nparts,
                                       uint32_t seed, int32_t* pids) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  uint64_t mask = (uint64_t)cap - 1;
  uint64_t shift = 0;
  while (((uint64_t)cap >> shift) > (uint64_t)nparts) ++shift;
  for (; i < n; i += stride) {
    uint64_t h = mm3_u64((uint64_t)keys[i], seed) & mask;
    pids[i] = (int32_t)(h >> shift);
  }
}

extern "C" __global__ void k_groupby_insert(
    const int64_t* keys, int64_t n, ValCols vals, int64_t* tkeys,
    int64_t cap, uint32_t seed, int32_t* sentinel_seen, int32_t* overflow,
    int64_t max_probes) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  uint64_t mask = (uint64_t)cap - 1;
  for (; i < n; i += stride) {
    int64_t k = keys[i];
    int64_t slot;
    if (k == GB_SENTINEL) {
      // reserved extra slot
      if (atomicOr(sentinel_seen, 1) == 0) {}
      slot = cap;
    } else {
      uint64_t h = mm3_u64((uint64_t)k, seed) & mask;
      if (gb_probe_claim(tkeys, h, mask, k, max_probes) == GB_FULL) {
        atomicOr(overflow, 1);
        return;
      }
      slot = (int64_t)h;
    }
    for (int c = 0; c < vals.n; ++c)
      accum(vals.tab[c], slot, vals.src[c], i, vals.agg[c]);
  }
}

// Cardinality sample: the exact count of distinct keys among the first
// `rows` keys of a batch, by claiming each key in a scratch tag table of
// m >= 2 * rows slots (a power of two: the load never exceeds 0.5, so a
// chain bounded by m never reports GB_FULL).  state[0] ends at
// distinct - 1, the number GroupTable._read_sample expects; state[1] is
// the flag that lets the first sentinel-key row count once (such rows
// never enter the table).
extern "C" __global__ void k_gbs_init(int64_t* tags, int64_t m,
                                      int64_t* state) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {
    state[0] = -1;
    state[1] = 0;
  }
  const longlong2 empty = {GB_SENTINEL, GB_SENTINEL};
  for (; 2 * i < m; i += stride) *(longlong2*)(tags + 2 * i) = empty;
}

__device__ __forceinline__ uint32_t gbs_claim(int64_t k, int64_t* tags,
                                              uint64_t mask, int32_t* flag) {
  if (k == GB_SENTINEL)
    return *(volatile int32_t*)flag == 0 && atomicOr(flag, 1) == 0;
  uint64_t h = gbm_fmix64((uint64_t)k) & mask;
  return gb_probe_claim(tags, h, mask, k, (int64_t)mask + 1) == GB_CLAIMED;
}

// WIDE: two adjacent rows per 16-byte load (keys 16-byte aligned), else
// one row per load, as gbp_load_rows does.
template <bool WIDE>
__device__ __forceinline__ uint32_t gbs_count_rows(const int64_t* keys,
                                                   int64_t rows,
                                                   int64_t* tags,
                                                   uint64_t mask,
                                                   int32_t* flag) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t mine = 0;
  if constexpr (WIDE) {
    for (int64_t i = 2 * t; i < rows; i += 2 * stride) {
      if (i + 1 < rows) {
        const longlong2 two = *(const longlong2*)(keys + i);
        mine += gbs_claim(two.x, tags, mask, flag);
        mine += gbs_claim(two.y, tags, mask, flag);
      } else {
        mine += gbs_claim(keys[i], tags, mask, flag);
      }
    }
  } else {
    for (int64_t i = t; i < rows; i += stride)
      mine += gbs_claim(keys[i], tags, mask, flag);
  }
  return mine;
}

extern "C" __global__ __launch_bounds__(THREADS) void k_gbs_count(
    const int64_t* keys, int64_t rows, int64_t* tags, int64_t m,
    int64_t* state) {
  __shared__ uint32_t claimed;
  if (threadIdx.x == 0) claimed = 0;
  __syncthreads();
  const uint64_t mask = (uint64_t)m - 1;
  int32_t* flag = (int32_t*)(state + 1);
  const uint32_t mine =
      ((uintptr_t)keys & 15) == 0
          ? gbs_count_rows<true>(keys, rows, tags, mask, flag)
          : gbs_count_rows<false>(keys, rows, tags, mask, flag);
  if (mine) atomicAdd(&claimed, mine);
  __syncthreads();
  if (threadIdx.x == 0 && claimed)
    atomicAdd((unsigned long long*)state, (unsigned long long)claimed);
}
