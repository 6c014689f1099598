// What the device hash tables share: groupby.hip (K9, keys; its global
// insert also serves the partitioned insert of groupby_part.hip),
// groupby_multi.hip (K21, tuple fingerprints) and iddict.hip (K23, string
// ids).
//
// A table is an int64 array of cap + 1 tags, cap a power of two, with
// GB_SENTINEL marking an empty slot; linear probing from a home slot,
// at most max_probes slots far.  Slot `cap` is never probed.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "columns.h"

// Sentinel marking an empty slot.  K9 accumulates rows whose key equals
// it in the reserved extra slot (index == capacity); K21 and K23 remap
// such a tag to 0 (gb_tag).
#define GB_SENTINEL 0x8000000000000000LL

__device__ __host__ __forceinline__ int64_t gb_tag(int64_t t) {
  return t == GB_SENTINEL ? 0 : t;
}

#define GBM_GOLDEN 0x9e3779b97f4a7c15ULL

// murmur3's 64-bit finalizer: a bijection of the 64-bit words.
__device__ __host__ __forceinline__ uint64_t gbm_fmix64(uint64_t h) {
  h ^= h >> 33;
  h *= 0xff51afd7ed558ccdULL;
  h ^= h >> 33;
  h *= 0xc4ceb9fe1a85ec53ULL;
  h ^= h >> 33;
  return h;
}

// Home slot (before masking) of a K21 / K23 tag.
__device__ __host__ __forceinline__ uint64_t gbm_home(int64_t tag) {
  return gbm_fmix64((uint64_t)tag + GBM_GOLDEN);
}

// The claim probe of every table.  h is the home slot on entry and the
// resolved slot on return.  Plain read first: once the table is warm most
// probes land on an already-claimed matching tag, and a load is far
// cheaper than an atomicCAS.  GB_FULL means the chain reached max_probes:
// the table is too loaded, and the caller raises its overflow flag so that
// the host grows x2 and re-inserts (reference combiner grow policy).
enum GbProbe : int { GB_FOUND, GB_CLAIMED, GB_FULL };

__device__ __forceinline__ int gb_probe_claim(int64_t* tags, uint64_t& h,
                                              uint64_t mask, int64_t tag,
                                              int64_t max_probes) {
  int64_t probes = 0;
  for (;;) {
    long long cur = ((volatile long long*)tags)[h];
    if (cur == tag) return GB_FOUND;
    if (cur == GB_SENTINEL) {
      long long prev = atomicCAS((unsigned long long*)&tags[h],
                                 (unsigned long long)GB_SENTINEL,
                                 (unsigned long long)tag);
      if (prev == GB_SENTINEL) return GB_CLAIMED;
      if (prev == tag) return GB_FOUND;
    }
    h = (h + 1) & mask;
    if (++probes >= max_probes) return GB_FULL;
  }
}

// Value columns of K9 and K21 and the accumulation into a resolved slot.
enum AggCode : int32_t { AGG_SUM = 0, AGG_MIN = 1, AGG_MAX = 2, AGG_PROD = 3 };

struct ValCols {
  ColDesc src[MAX_COLS];
  MutColDesc tab[MAX_COLS];
  int32_t agg[MAX_COLS];
  int n;
};

template <typename T, typename U>
__device__ __forceinline__ void cas_loop(T* addr, T v, int agg) {
  U* a = (U*)addr;
  U old = *a, assumed;
  do {
    assumed = old;
    T cur = __builtin_bit_cast(T, assumed);
    T nv;
    switch (agg) {
      case AGG_MIN: nv = v < cur ? v : cur; break;
      case AGG_MAX: nv = v > cur ? v : cur; break;
      default: nv = cur * v; break;
    }
    if (nv == cur) return;
    old = atomicCAS(a, assumed, __builtin_bit_cast(U, nv));
  } while (old != assumed);
}

__device__ __forceinline__ void accum(const MutColDesc& t, int64_t slot,
                                      const ColDesc& s, int64_t i,
                                      int agg) {
  switch (t.code) {
    case DT_I32: {
      int32_t v = ((const int32_t*)s.ptr)[i];
      int32_t* a = (int32_t*)t.ptr + slot;
      if (agg == AGG_SUM) atomicAdd((int*)a, (int)v);
      else if (agg == AGG_MIN) atomicMin((int*)a, (int)v);
      else if (agg == AGG_MAX) atomicMax((int*)a, (int)v);
      else cas_loop<int32_t, unsigned int>(a, v, agg);
      break;
    }
    case DT_I64: {
      int64_t v = ((const int64_t*)s.ptr)[i];
      int64_t* a = (int64_t*)t.ptr + slot;
      if (agg == AGG_SUM)
        atomicAdd((unsigned long long*)a, (unsigned long long)v);
      else
        cas_loop<int64_t, unsigned long long>(a, v, agg);
      break;
    }
    case DT_F32: {
      float v = ((const float*)s.ptr)[i];
      float* a = (float*)t.ptr + slot;
      if (agg == AGG_SUM) atomicAdd(a, v);
      else cas_loop<float, unsigned int>(a, v, agg);
      break;
    }
    case DT_F64: {
      double v = ((const double*)s.ptr)[i];
      double* a = (double*)t.ptr + slot;
      if (agg == AGG_SUM) atomicAdd(a, v);
      else cas_loop<double, unsigned long long>(a, v, agg);
      break;
    }
  }
}
