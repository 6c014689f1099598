// K23: id dictionary — a device hash table from the 64-bit id of a string
// (BytesColumn.ids64) to the position of one exemplar row in an
// append-only list of strings.
//
// The conventions are K21's (groupby_multi.hip): caller-owned tensors,
// tags int64[cap+1] with GB_SENTINEL for an empty slot, ref int64[cap+1],
// cap a power of two, home slot gbm_fmix64(id + golden) & (cap-1), linear
// probing with a plain read before the CAS, a bound on the probe chain.
// An id equal to the empty marker is treated as id 0 in every kernel.
//
//   k_idd_claim   one row per thread.  The thread whose CAS claims a slot
//                 takes the next position p of the append list, records
//                 its row in newrows[p] and stores ref[slot] = base + p
//                 (plain stores: nothing reads ref before the launch
//                 ends).  The host then gathers the rows in newrows.
//   k_idd_lookup  position of every id, -1 when absent.  Read-only.
//   k_idd_rehash  moves a table into a larger one, one old slot per
//                 thread; ids are unique, so every probe ends in a claim.
//
// No thread waits for another: there is no spin loop.  A row whose probe
// chain reaches max_probes is left out and raises the overflow counter;
// the host regrows, rehashes and runs the claim over the same batch
// again, which finds the rows of the first run and appends only the rest.

#include <hip/hip_runtime.h>

#include "hashtable.h"

// counters of k_idd_claim, uint64[3]
#define IDD_NEW_ROWS 0
#define IDD_NEW_BYTES 1
#define IDD_OVERFLOW 2

__global__ void k_idd_claim(const int64_t* __restrict__ ids, int64_t n,
                            const int64_t* __restrict__ lens, int64_t* tags,
                            int64_t* __restrict__ ref, int64_t cap,
                            int64_t base, int64_t* __restrict__ newrows,
                            unsigned long long* counters,
                            int64_t max_probes) {
  const int lane = threadIdx.x & 63;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const uint64_t mask = (uint64_t)cap - 1;
  bool full = false;  // this thread overflowed: the host will regrow
  // The bound is the wave's first row, so the lanes of a wave make the
  // same number of trips and meet at the ballot below.
  for (int64_t w0 = i - lane; w0 < n; w0 += stride, i += stride) {
    bool claimed = false;
    uint64_t h = 0;
    if (i < n && !full) {
      const int64_t tag = gb_tag(ids[i]);
      h = gbm_home(tag) & mask;
      const int r = gb_probe_claim(tags, h, mask, tag, max_probes);
      claimed = (r == GB_CLAIMED);
      if (r == GB_FULL) {
        atomicOr(&counters[IDD_OVERFLOW], 1ull);
        full = true;
      }
    }
    // Wave-aggregated append: one returning atomic per wave and trip.
    const uint64_t m = __ballot(claimed);
    if (m == 0) continue;  // wave-uniform
    const int leader = __ffsll((unsigned long long)m) - 1;
    long long bytes = claimed ? (long long)lens[i] : 0;
    for (int off = 32; off; off >>= 1) bytes += __shfl_xor(bytes, off, 64);
    unsigned long long p0 = 0;
    if (lane == leader) {
      p0 = atomicAdd(&counters[IDD_NEW_ROWS],
                     (unsigned long long)__popcll(m));
      atomicAdd(&counters[IDD_NEW_BYTES], (unsigned long long)bytes);
    }
    p0 = __shfl(p0, leader, 64);
    if (claimed) {
      const int64_t p =
          (int64_t)p0 + __popcll(m & ((1ull << lane) - 1ull));
      // p < n: a row claims at most once and the counter starts at 0
      if (p < n) {
        newrows[p] = i;
        ref[h] = base + p;
      }
    }
  }
}

__global__ void k_idd_lookup(const int64_t* __restrict__ ids, int64_t n,
                             const int64_t* __restrict__ tags,
                             const int64_t* __restrict__ ref, int64_t cap,
                             int64_t* __restrict__ out, int64_t max_probes) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const uint64_t mask = (uint64_t)cap - 1;
  for (; i < n; i += stride) {
    const int64_t tag = gb_tag(ids[i]);
    uint64_t h = gbm_home(tag) & mask;
    int64_t pos = -1;
    // the claim places nothing beyond max_probes slots from home
    for (int64_t probes = 0; probes < max_probes; ++probes) {
      const int64_t cur = tags[h];
      if (cur == tag) {
        pos = ref[h];
        break;
      }
      if (cur == GB_SENTINEL) break;
      h = (h + 1) & mask;
    }
    out[i] = pos;
  }
}

__global__ void k_idd_rehash(const int64_t* __restrict__ old_tags,
                             const int64_t* __restrict__ old_ref,
                             int64_t old_cap, int64_t* new_tags,
                             int64_t* __restrict__ new_ref, int64_t new_cap,
                             int32_t* overflow, int64_t max_probes) {
  int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const uint64_t mask = (uint64_t)new_cap - 1;
  for (; s < old_cap; s += stride) {
    const int64_t tag = old_tags[s];
    if (tag == GB_SENTINEL) continue;
    uint64_t h = gbm_home(tag) & mask;
    // ids of a table are unique, so GB_FOUND cannot happen
    const int r = gb_probe_claim(new_tags, h, mask, tag, max_probes);
    if (r == GB_CLAIMED) new_ref[h] = old_ref[s];
    else if (r == GB_FULL) atomicOr(overflow, 1);
  }
}
