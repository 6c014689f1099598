// K24: byte-order ranks of the rows of a BYTES column by prefix
// refinement — the two device passes of one refinement round.
//
// Round w looks at the bytes [7w, 7w+7) of every still-undecided row.
// Its key is one 64-bit word: those 7 bytes big-endian in the top 56
// bits, zero-padded past the row's end, and valid = clamp(len - 7w, 0, 7)
// in the low 8 bits.  As unsigned integers two keys order as the two rows
// do on that stretch (a row that ended is a prefix and sorts first), and
// equal keys with valid < 7 mean equal rows.  The key leaves with its top
// bit flipped, so the signed radix argsort gives the unsigned order.
//
//   k_bo_keys    keys of m selected rows, one row per thread, grid-stride.
//                offsets is absolute into data (a zero-copy slice works as
//                it is); a row index outside [0, n) has length 0.  The 7
//                bytes come from at most two aligned 8-byte loads and a
//                funnel shift.  An aligned word that is not wholly inside
//                data (its first or last one, or any word under corrupt
//                offsets) is put together byte by byte, each byte checked
//                against data_len: nothing outside data is read.
//   k_bo_refine  one pass over the active slots sorted by (grp, key):
//                head[j] = j where slot j starts a new (grp, key) group,
//                else 0 (an inclusive cummax then gives every slot its
//                head slot); stay[j] = slot j is tied with a neighbour
//                and its row still has bytes to look at (valid == 7).
//                A thread owns BO_ITEMS consecutive slots and compares
//                them in registers; its first and last pair go through
//                LDS to the neighbouring threads; the first and the last
//                thread of a tile load the one slot beyond the tile's
//                edge.  No workgroup waits on another.

#include <hip/hip_runtime.h>

#include <cstdint>

#define BO_BLOCK 256
#define BO_ITEMS 4
#define BO_TILE (BO_BLOCK * BO_ITEMS)  // slots per workgroup of k_bo_refine

// The aligned 8-byte word of data whose first byte has index i0 (which
// may be negative or past the end), little-endian; bytes outside
// [0, data_len) read as zero.
__device__ __forceinline__ uint64_t bo_word(const uint8_t* __restrict__ data,
                                            int64_t data_len, int64_t i0) {
  if (i0 >= 0 && i0 <= data_len - 8)
    return *reinterpret_cast<const uint64_t*>(data + i0);
  uint64_t v = 0;
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const int64_t s = i0 + b;
    if (s >= 0 && s < data_len) v |= (uint64_t)data[s] << (8 * b);
  }
  return v;
}

__global__ __launch_bounds__(BO_BLOCK) void k_bo_keys(
    const uint8_t* __restrict__ data, int64_t data_len,
    const int64_t* __restrict__ offsets, int64_t n,
    const int64_t* __restrict__ rows, int64_t m, int64_t w,
    int64_t* __restrict__ keys) {
  // data + i is 8-byte aligned iff (i + mis) % 8 == 0
  const int64_t mis = (int64_t)(reinterpret_cast<uintptr_t>(data) & 7);
  const int64_t skip = 7 * w;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m;
       j += stride) {
    const int64_t r = rows[j];
    int64_t beg = 0, len = 0;
    if (r >= 0 && r < n) {
      beg = offsets[r];
      len = offsets[r + 1] - beg;
    }
    int64_t left = len - skip;
    const int valid = left <= 0 ? 0 : (left >= 7 ? 7 : (int)left);
    uint64_t v = 0;
    if (valid > 0) {
      const int64_t q = beg + skip + mis;  // from the aligned-down base
      const int sh = (int)(q & 7);
      const int64_t i0 = (q - sh) - mis;   // index of the aligned word
      v = bo_word(data, data_len, i0) >> (8 * sh);
      if (sh + valid > 8)  // sh >= 2 here
        v |= bo_word(data, data_len, i0 + 8) << (64 - 8 * sh);
      v &= ~0ull >> (64 - 8 * valid);
    }
    // row byte 0 is the low byte of v; the eighth byte is masked off
    const uint64_t key = __builtin_bswap64(v) | (uint64_t)valid;
    keys[j] = (int64_t)(key ^ 0x8000000000000000ull);
  }
}

// grp, key: int64[m] sorted by (grp, key), 16-byte aligned.
__global__ __launch_bounds__(BO_BLOCK) void k_bo_refine(
    const int64_t* __restrict__ grp, const int64_t* __restrict__ key,
    int64_t m, int64_t* __restrict__ head, uint8_t* __restrict__ stay) {
  __shared__ int64_t s_first[2][BO_BLOCK];  // a thread's first (grp, key)
  __shared__ int64_t s_last[2][BO_BLOCK];   // and its last
  const int t = threadIdx.x;
  const int64_t j0 = (int64_t)blockIdx.x * BO_TILE + (int64_t)t * BO_ITEMS;
  int64_t g[BO_ITEMS], k[BO_ITEMS];
  if (j0 + BO_ITEMS <= m) {
    const longlong2* gp = reinterpret_cast<const longlong2*>(grp + j0);
    const longlong2* kp = reinterpret_cast<const longlong2*>(key + j0);
#pragma unroll
    for (int i = 0; i < BO_ITEMS / 2; ++i) {
      const longlong2 a = gp[i], b = kp[i];
      g[2 * i] = a.x; g[2 * i + 1] = a.y;
      k[2 * i] = b.x; k[2 * i + 1] = b.y;
    }
  } else {
#pragma unroll
    for (int i = 0; i < BO_ITEMS; ++i) {
      const bool in = j0 + i < m;
      g[i] = in ? grp[j0 + i] : 0;
      k[i] = in ? key[j0 + i] : 0;
    }
  }
  s_first[0][t] = g[0];
  s_first[1][t] = k[0];
  s_last[0][t] = g[BO_ITEMS - 1];
  s_last[1][t] = k[BO_ITEMS - 1];
  __syncthreads();
  // the slot before this thread's first and the one after its last
  int64_t pg = 0, pk = 0, ng = 0, nk = 0;
  if (t > 0) {
    pg = s_last[0][t - 1];
    pk = s_last[1][t - 1];
  } else if (j0 > 0 && j0 - 1 < m) {
    pg = grp[j0 - 1];
    pk = key[j0 - 1];
  }
  const int64_t jn = j0 + BO_ITEMS;
  if (t < BO_BLOCK - 1) {
    ng = s_first[0][t + 1];
    nk = s_first[1][t + 1];
  } else if (jn < m) {
    ng = grp[jn];
    nk = key[jn];
  }
  // h[i]: slot j0 + i is a head; h[BO_ITEMS]: so is the slot after
  bool h[BO_ITEMS + 1];
  h[0] = j0 == 0 || g[0] != pg || k[0] != pk;
#pragma unroll
  for (int i = 1; i < BO_ITEMS; ++i)
    h[i] = g[i] != g[i - 1] || k[i] != k[i - 1];
  h[BO_ITEMS] = g[BO_ITEMS - 1] != ng || k[BO_ITEMS - 1] != nk;
  // (a slot at or past m counts as a head: the last slot has no next)
#pragma unroll
  for (int i = 1; i <= BO_ITEMS; ++i)
    if (j0 + i >= m) h[i] = true;
  uint32_t packed = 0;
#pragma unroll
  for (int i = 0; i < BO_ITEMS; ++i) {
    const bool s = (!h[i] || !h[i + 1]) && (k[i] & 0xff) == 7;
    packed |= (s ? 1u : 0u) << (8 * i);
  }
  if (j0 + BO_ITEMS <= m) {
    longlong2* hp = reinterpret_cast<longlong2*>(head + j0);
#pragma unroll
    for (int i = 0; i < BO_ITEMS / 2; ++i) {
      longlong2 o;
      o.x = h[2 * i] ? j0 + 2 * i : 0;
      o.y = h[2 * i + 1] ? j0 + 2 * i + 1 : 0;
      hp[i] = o;
    }
    *reinterpret_cast<uint32_t*>(stay + j0) = packed;
  } else {
#pragma unroll
    for (int i = 0; i < BO_ITEMS; ++i) {
      if (j0 + i < m) {
        head[j0 + i] = h[i] ? j0 + i : 0;
        stay[j0 + i] = (uint8_t)(packed >> (8 * i));
      }
    }
  }
}
