// K22: run boundaries and lexicographic search over a tuple of int64 key
// columns, the two primitives the sort-merge cogroup needs beyond one
// key column.
//
// Run boundaries: rows are sorted lexicographically; row r starts a run
// iff r == 0 or ANY column differs from row r-1.  The compaction is the
// tokenizer's count / scan / write shape (K20), two launches with the
// scan of the per-tile counts between them, so no workgroup waits on
// another (k_runs_sorted's single pass pays for itself with a lookback
// spin; reading the keys a second time, L2-warm, costs well under one
// sort pass):
//   k_mruns_count  per tile, the number of flagged rows -> counts[tile]
//   (host side)    inclusive scan over tiles (1-D torch.cumsum)
//   k_mruns_write  recompute the flags, rank the flagged rows inside the
//                  tile, add the tile base, write starts and the tuples
//
// Geometry: a tile is MRUNS_TILE rows = MRUNS_SLABS slabs of MRUNS_BLOCK
// rows; in slab k thread t owns row base + k*MRUNS_BLOCK + t, so
// consecutive lanes hold consecutive rows and row r-1 is a wave shuffle.
// Lane 0 loads its real neighbour instead, which is also how the first
// row of a tile reaches into the previous tile.  Row order inside a tile
// is (slab, wave, lane).
//
// Lexicographic search: one query tuple per thread, a binary search over
// u sorted tuples, signed compare with column 0 first and a later column
// read only when the earlier ones are equal.
//
// All kernels are templated on the column count so that every index into
// the by-value pointer arrays is a compile-time constant (no scratch);
// NK = 0 is the generic form, unrolled to MAX_KEY_COLS under a `c < n`
// guard.

#include <hip/hip_runtime.h>

#include "columns.h"

#define MRUNS_BLOCK 256
#define MRUNS_SLABS 16
#define MRUNS_TILE (MRUNS_BLOCK * MRUNS_SLABS)  // 4096 rows
#define MRUNS_WAVES (MRUNS_BLOCK / 64)
#define MRUNS_SEGS (MRUNS_SLABS * MRUNS_WAVES)  // 64: one wave scans them

static_assert(MRUNS_SEGS == 64, "the segment scan is one wave wide");
static_assert(MRUNS_SLABS <= 32, "a thread's flags are bits of one word");

struct MrCols {
  const int64_t* src[MAX_KEY_COLS];  // sorted key columns
  int64_t* uniq[MAX_KEY_COLS];       // distinct tuples (write kernel)
  int n;
};

struct LexCols {
  const int64_t* sorted[MAX_KEY_COLS];
  const int64_t* query[MAX_KEY_COLS];
  int n;
};

// Slabs whose loads are issued together, ahead of the compare chain:
// J * columns 8-byte loads in flight per thread.
template <int NK>
struct MrunsBatch {
  static constexpr int J = NK == 2 ? 4 : (NK == 3 || NK == 4) ? 2 : 1;
};

// Boundary flags of this thread's rows in slabs k0 .. k0+J-1 of the tile
// at `base`, as bits 0 .. J-1.  Every lane of the wave must call it.
template <int NK>
__device__ __forceinline__ unsigned int mruns_flags(const MrCols& kc,
                                                    int64_t n, int64_t base,
                                                    int k0, int lane) {
  constexpr int N = NK ? NK : MAX_KEY_COLS;
  constexpr int J = MrunsBatch<NK>::J;
  int64_t cur[J][N], prev[J][N];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int64_t r = base + (int64_t)(k0 + j) * MRUNS_BLOCK + threadIdx.x;
#pragma unroll
    for (int c = 0; c < N; ++c) {
      cur[j][c] = 0;
      prev[j][c] = 0;
      if (NK || c < kc.n) {
        if (r < n) cur[j][c] = kc.src[c][r];
        if (lane == 0 && r > 0 && r < n) prev[j][c] = kc.src[c][r - 1];
      }
    }
  }
  unsigned int fb = 0;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int64_t r = base + (int64_t)(k0 + j) * MRUNS_BLOCK + threadIdx.x;
    bool differs = false;
#pragma unroll
    for (int c = 0; c < N; ++c) {
      if (NK || c < kc.n) {
        int64_t p = __shfl_up(cur[j][c], 1, 64);
        if (lane == 0) p = prev[j][c];
        differs |= cur[j][c] != p;
      }
    }
    const bool flag = (r < n) && (r == 0 || differs);
    fb |= flag ? (1u << j) : 0u;
  }
  return fb;
}

template <int NK>
__global__ __launch_bounds__(MRUNS_BLOCK) void k_mruns_count(
    MrCols kc, int64_t n, int64_t* __restrict__ counts) {
  constexpr int J = MrunsBatch<NK>::J;
  __shared__ unsigned int wsum[MRUNS_WAVES];
  const int64_t base = (int64_t)blockIdx.x * MRUNS_TILE;
  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  unsigned int cnt = 0;  // wave-uniform
#pragma unroll 1
  for (int k0 = 0; k0 < MRUNS_SLABS; k0 += J) {
    const unsigned int fb = mruns_flags<NK>(kc, n, base, k0, lane);
#pragma unroll
    for (int j = 0; j < J; ++j)
      cnt += (unsigned int)__popcll(__ballot((fb >> j) & 1u));
  }
  if (lane == 0) wsum[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned int sum = 0;
#pragma unroll
    for (int w = 0; w < MRUNS_WAVES; ++w) sum += wsum[w];
    counts[blockIdx.x] = (int64_t)sum;
  }
}

// incl: inclusive scan of counts over tiles.  The outputs hold `cap`
// entries (one per row is always enough); every store is checked
// against it.
template <int NK>
__global__ __launch_bounds__(MRUNS_BLOCK) void k_mruns_write(
    MrCols kc, int64_t n, const int64_t* __restrict__ incl, int64_t cap,
    int64_t* __restrict__ starts) {
  constexpr int N = NK ? NK : MAX_KEY_COLS;
  constexpr int J = MrunsBatch<NK>::J;
  __shared__ unsigned int seg[MRUNS_SEGS];  // slab-major (slab, wave)
  const int tile = blockIdx.x;
  const int64_t base = (int64_t)tile * MRUNS_TILE;
  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));

  unsigned int flags = 0;  // bit k: this thread's row of slab k
#pragma unroll 1
  for (int k0 = 0; k0 < MRUNS_SLABS; k0 += J) {
    const unsigned int fb = mruns_flags<NK>(kc, n, base, k0, lane);
    flags |= fb << k0;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const uint64_t b = __ballot((fb >> j) & 1u);
      if (lane == 0)
        seg[(k0 + j) * MRUNS_WAVES + wave] = (unsigned int)__popcll(b);
    }
  }
  __syncthreads();
  // exclusive scan of the 64 segment counts, in place, by wave 0
  if (wave == 0) {
    const unsigned int v = seg[lane];
    unsigned int incl_v = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned int up = (unsigned int)__shfl_up((int)incl_v, off, 64);
      if (lane >= off) incl_v += up;
    }
    seg[lane] = incl_v - v;
  }
  __syncthreads();
  const int64_t tb = tile > 0 ? incl[tile - 1] : 0;

#pragma unroll 1
  for (int k = 0; k < MRUNS_SLABS; ++k) {
    const bool flag = (flags >> k) & 1u;
    const uint64_t b = __ballot(flag);
    if (flag) {
      const int64_t r = base + (int64_t)k * MRUNS_BLOCK + threadIdx.x;
      const int64_t pos =
          tb + seg[k * MRUNS_WAVES + wave] + (unsigned int)__popcll(b & lt);
      if (pos < cap) {  // r < n: only rows inside the input are flagged
        starts[pos] = r;
#pragma unroll
        for (int c = 0; c < N; ++c)
          if (NK || c < kc.n) kc.uniq[c][pos] = kc.src[c][r];
      }
    }
  }
}

// out[i] = the lower (right == 0) or upper (right != 0) bound of query
// tuple i among the u sorted tuples, as torch.searchsorted defines them
// for scalars: the first position whose tuple is >= (lower) or > (upper)
// the query.  u == 0 gives 0.
template <int NK>
__global__ __launch_bounds__(256) void k_lex_search(
    LexCols kc, int64_t u, int64_t m, int right,
    int64_t* __restrict__ out) {
  constexpr int N = NK ? NK : MAX_KEY_COLS;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m;
       i += stride) {
    int64_t q[N];
#pragma unroll
    for (int c = 0; c < N; ++c) q[c] = (NK || c < kc.n) ? kc.query[c][i] : 0;
    int64_t lo = 0, hi = u;
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      int cmp = 0;  // sign of (sorted[mid] - q), first differing column
#pragma unroll
      for (int c = 0; c < N; ++c) {
        if ((NK || c < kc.n) && cmp == 0) {
          const int64_t v = kc.sorted[c][mid];
          cmp = v < q[c] ? -1 : (v > q[c] ? 1 : 0);
        }
      }
      if (right ? cmp <= 0 : cmp < 0) lo = mid + 1; else hi = mid;
    }
    out[i] = lo;
  }
}
