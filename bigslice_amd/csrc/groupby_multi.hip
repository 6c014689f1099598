// K21: hash-aggregate group-by over a tuple of 2..MAX_KEY_COLS int64 key
// columns.
//
// A tuple is wider than any CAS, and a reader that met a half-published
// tuple would have to wait for its writer.  So the table is claimed by a
// 64-bit fingerprint of the tuple (the tag) and the insert is two
// launches; the launch boundary is the publication fence:
//
//   k_gbm_claim  probes `tags` like k_groupby_insert probes its keys and
//                records each row's slot; the thread whose CAS claimed a
//                slot stores its tuple into the key arrays (plain stores).
//   k_gbm_accum  reads the row's slot, compares the stored tuple (complete:
//                the claim launch has ended) with the row's, and
//                accumulates the value columns.  A mismatch means two
//                tuples share a tag: it sets the collision flag and skips
//                the row; the host then recomputes the result exactly.
//
// No thread waits for another.  Key values are unrestricted: only the tag
// can equal the empty marker, and such a tag is remapped to 0.  Slot `cap`
// of every array exists (so groupby_compact takes the table as it is) and
// is never used.
//
// Key storage is one int64[cap+1] array per column (SoA).  The kernels
// are templated on the column count so that every index into the
// by-value pointer arrays is a compile-time constant (no scratch); NK = 0
// is the generic form, unrolled to MAX_KEY_COLS under a `c < n` guard.

#include <hip/hip_runtime.h>

#include "hashtable.h"

struct MkCols {
  const int64_t* src[MAX_KEY_COLS];  // the batch's key columns
  int64_t* tab[MAX_KEY_COLS];        // the table's key arrays
  int n;
};

#define GBM_NO_SLOT 0xFFFFFFFFu

// One chaining step: the running hash is remixed with every column, so
// the fingerprint depends on the order of the columns.
__device__ __host__ __forceinline__ uint64_t gbm_step(uint64_t h,
                                                       uint64_t k) {
  return gbm_fmix64((h + GBM_GOLDEN) ^ k);
}

__device__ __host__ __forceinline__ int64_t gbm_tag(uint64_t h,
                                                     uint64_t fp_mask) {
  return gb_tag((int64_t)(h & fp_mask));
}

template <int NK>
__device__ __forceinline__ int64_t gbm_load_tuple(const MkCols& kc,
                                                  int64_t i, uint32_t seed,
                                                  uint64_t fp_mask,
                                                  int64_t (&k)[MAX_KEY_COLS]) {
  constexpr int N = NK ? NK : MAX_KEY_COLS;
  uint64_t h = seed;
#pragma unroll
  for (int c = 0; c < N; ++c) {
    if (NK || c < kc.n) {
      k[c] = kc.src[c][i];
      h = gbm_step(h, (uint64_t)k[c]);
    }
  }
  return gbm_tag(h, fp_mask);
}

template <int NK>
__global__ void k_gbm_fingerprint(MkCols kc, int64_t n, uint32_t seed,
                                  uint64_t fp_mask, int64_t* out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    int64_t k[MAX_KEY_COLS];
    out[i] = gbm_load_tuple<NK>(kc, i, seed, fp_mask, k);
  }
}

template <int NK>
__global__ void k_gbm_claim(MkCols kc, int64_t n, int64_t* tags,
                            int64_t cap, uint32_t seed, uint64_t fp_mask,
                            uint32_t* slots, int32_t* overflow,
                            int64_t max_probes) {
  constexpr int N = NK ? NK : MAX_KEY_COLS;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  uint64_t mask = (uint64_t)cap - 1;
  bool full = false;  // this thread overflowed: the host will regrow
  for (; i < n; i += stride) {
    if (full) {
      slots[i] = GBM_NO_SLOT;
      continue;
    }
    int64_t k[MAX_KEY_COLS];
    int64_t tag = gbm_load_tuple<NK>(kc, i, seed, fp_mask, k);
    uint64_t h = gbm_home(tag) & mask;
    const int r = gb_probe_claim(tags, h, mask, tag, max_probes);
    if (r == GB_CLAIMED) {
      // The slot is this thread's: publish the tuple.  Nobody reads it
      // before the launch ends.
#pragma unroll
      for (int c = 0; c < N; ++c)
        if (NK || c < kc.n) kc.tab[c][h] = k[c];
    } else if (r == GB_FULL) {
      atomicOr(overflow, 1);
      full = true;
    }
    slots[i] = full ? GBM_NO_SLOT : (uint32_t)h;
  }
}

template <int NK>
__global__ void k_gbm_accum(MkCols kc, int64_t n, ValCols vals,
                            const uint32_t* slots, int64_t cap,
                            int32_t* collision) {
  constexpr int N = NK ? NK : MAX_KEY_COLS;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    // GBM_NO_SLOT is above every capacity (the binding bounds cap by
    // 2^31), so one compare skips it and keeps every access in bounds.
    uint32_t s = slots[i];
    if ((uint64_t)s >= (uint64_t)cap) continue;
    bool same = true;
#pragma unroll
    for (int c = 0; c < N; ++c)
      if (NK || c < kc.n) same &= kc.tab[c][s] == kc.src[c][i];
    if (!same) {
      // Two tuples share a fingerprint.
      atomicOr(collision, 1);
      continue;
    }
    for (int c = 0; c < vals.n; ++c)
      accum(vals.tab[c], (int64_t)s, vals.src[c], i, vals.agg[c]);
  }
}
