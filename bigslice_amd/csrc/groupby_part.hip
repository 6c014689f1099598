// K19: partitioned LDS pre-aggregation for the single-int64-SUM group-by.
//
// The one-pass insert (groupby.hip) pays one memory-side atomic per row.
// At mid cardinality (~1M keys, a few rows per key per batch) neither the
// 1024-slot LDS tier nor replication removes any of them.  This path
// makes duplicates of a key neighbours first, so a workgroup-private LDS
// table can absorb them and only ONE global atomic per distinct key per
// tile reaches the table:
//
//   1. k_gbp_hist     one workgroup per GROUP of G consecutive 4096-row
//                     tiles: LDS histogram of the group's bucket ids ->
//                     groups x B
//   2. k_gbp_offsets  column-wise exclusive scan of that matrix (in
//                     place) + per-bucket totals
//   3. k_gbp_scatter  one workgroup per group: bucket starts (scan of the
//                     totals) + its row of the matrix = a cursor per
//                     bucket, kept by the workgroup.  Tile by tile it
//                     re-reads the rows, reorders them by bucket in LDS,
//                     writes (key, value) as 16-byte pairs, each bucket's
//                     rows of the tile as one contiguous run at the
//                     cursor, and advances the cursor by the tile's count
//   4. k_gbp_aggregate fixed tiles of the partitioned buffer -> LDS hash
//                     table (LDS CAS + 64-bit LDS add) -> one
//                     gb_global_insert_sum per occupied LDS slot
//   4'. k_gbp_owned + k_gbp_cleanup replace 4 when a bucket's table slice
//                     fits in LDS: its owner updates the slice in LDS and
//                     stores it back, no global atomics ("Owned slices"
//                     below)
//
// Bucket id = high bits of the global table slot hash, so the rows of a
// bucket also share a table range.  The global table, its probing, the
// sentinel slot and the overflow flag are exactly those of groupby.hip:
// the LDS tables are private pre-aggregators only, and batches inserted
// by this path and by k_groupby_insert mix freely in one table.
//
// The bookkeeping is per group, not per tile: the matrix has tiles / G
// rows and the scatter never reads a per-tile offset.  G comes from the
// host (part_group_tiles in ext.hip: about two workgroups per CU, 1 for a
// 2M-row batch, 4 at 8M rows).
//
// No kernel waits on another workgroup; ordering is by launch.

#include <hip/hip_runtime.h>

#include "columns.h"

#define GBP_THREADS 512
// rows per histogram/scatter tile: 64 KiB of staged pairs, two
// workgroups per CU
#define GBP_SCATTER_ROWS 4096
// pairs per aggregate tile and slots of its LDS table (64 KiB: two
// workgroups per CU)
#define GBP_TILE_ROWS 8192
#define GBP_LDS_SLOTS 4096
#define GBP_LDS_BITS 12
#define GBP_LDS_PROBES 8
#define GBP_MAX_BUCKETS 1024

struct __attribute__((aligned(16))) GbPair {
  long long k;
  long long v;
};

// Sentinel-key rows go to bucket 0; the aggregate pass routes them to the
// reserved slot.
__device__ __forceinline__ uint32_t gbp_bucket(long long k, uint32_t seed,
                                               uint32_t mask,
                                               uint32_t shift) {
  if (k == GB_SENTINEL) return 0;
  return (mm3_u64((uint64_t)k, seed) & mask) >> shift;
}

// Tiles [t0, t1) of group g (G consecutive scatter tiles), clipped to the
// batch.
__device__ __forceinline__ void gbp_group_tiles(int64_t g, uint32_t G,
                                                int64_t ntiles, int64_t* t0,
                                                int64_t* t1) {
  *t0 = g * G;
  *t1 = min(*t0 + (int64_t)G, ntiles);
}

// Row of a tile (or histogram chunk) that register j of a thread holds.
// WIDE: a thread takes two adjacent rows per 16-byte load (the column
// must be 16-byte aligned; tiles start at even rows), else one row per
// load.
template <bool WIDE>
__device__ __forceinline__ uint32_t gbp_row(int j) {
  return WIDE ? (j >> 1) * 2 * GBP_THREADS + 2 * threadIdx.x + (j & 1)
              : j * GBP_THREADS + threadIdx.x;
}

// R rows of a column starting at row r (a multiple of the tile), rows
// below r1 only.
template <bool WIDE, int R>
__device__ __forceinline__ void gbp_load_rows(const int64_t* col, int64_t r,
                                              int64_t r1, long long (&x)[R]) {
  if constexpr (WIDE) {
#pragma unroll
    for (int j = 0; j < R; j += 2) {
      const int64_t i = r + gbp_row<true>(j);
      if (i + 1 < r1) {
        const longlong2 two = *(const longlong2*)(col + i);
        x[j] = two.x;
        x[j + 1] = two.y;
      } else if (i < r1) {
        x[j] = col[i];
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int64_t i = r + gbp_row<false>(j);
      if (i < r1) x[j] = col[i];
    }
  }
}

// keys per thread of one histogram chunk (one tile); the next chunk is
// in flight while the current one goes through the LDS atomics
#define GBP_HIST_C (GBP_SCATTER_ROWS / GBP_THREADS)

template <bool WIDE>
__device__ __forceinline__ void gbp_hist_rows(const int64_t* keys, int64_t r0,
                                              int64_t r1, uint32_t seed,
                                              uint32_t mask, uint32_t shift,
                                              uint32_t* lh) {
  constexpr int64_t CH = (int64_t)GBP_HIST_C * GBP_THREADS;
  long long k[GBP_HIST_C], kn[GBP_HIST_C];
  gbp_load_rows<WIDE>(keys, r0, r1, k);
  __syncthreads();  // lh is cleared
  for (int64_t r = r0; r < r1; r += CH) {
    const bool more = r + CH < r1;
    if (more) gbp_load_rows<WIDE>(keys, r + CH, r1, kn);
#pragma unroll
    for (int j = 0; j < GBP_HIST_C; ++j) {
      if (r + gbp_row<WIDE>(j) < r1)
        atomicAdd(&lh[gbp_bucket(k[j], seed, mask, shift)], 1u);
    }
    if (more) {
#pragma unroll
      for (int j = 0; j < GBP_HIST_C; ++j) k[j] = kn[j];
    }
  }
}

// One workgroup per group: all tiles of the group go into one LDS
// histogram, written as one row gsum[group][b].
extern "C" __global__ __launch_bounds__(GBP_THREADS) void k_gbp_hist(
    const int64_t* keys, int64_t n, int64_t ntiles, uint32_t G, uint32_t nb,
    uint32_t seed, uint32_t mask, uint32_t shift, uint32_t* gsum) {
  __shared__ uint32_t lh[GBP_MAX_BUCKETS];
  int64_t t0, t1;
  gbp_group_tiles(blockIdx.x, G, ntiles, &t0, &t1);
  const int64_t r0 = t0 * GBP_SCATTER_ROWS;
  const int64_t r1 = min(t1 * GBP_SCATTER_ROWS, n);
  for (uint32_t b = threadIdx.x; b < nb; b += GBP_THREADS) lh[b] = 0;
  if (((uintptr_t)keys & 15) == 0)
    gbp_hist_rows<true>(keys, r0, r1, seed, mask, shift, lh);
  else
    gbp_hist_rows<false>(keys, r0, r1, seed, mask, shift, lh);
  __syncthreads();
  uint32_t* row = gsum + (int64_t)blockIdx.x * nb;
  for (uint32_t b = threadIdx.x; b < nb; b += GBP_THREADS) row[b] = lh[b];
}

// In-place exclusive scan down each bucket column of the groups x B
// matrix (ntiles = its rows), plus the column totals.  One workgroup per
// 64 adjacent columns (a wave reads 64 consecutive counters of one row:
// coalesced); its 16 waves split the row axis, exchange chunk sums
// through LDS, then rewrite their chunk.  Loads are issued in groups of 8
// before the dependent stores so a chunk costs ~rows/128 round trips, not
// rows/16.
#define GBP_OFF_THREADS 1024
#define GBP_OFF_WAVES (GBP_OFF_THREADS / 64)

extern "C" __global__ __launch_bounds__(GBP_OFF_THREADS) void k_gbp_offsets(
    uint32_t* hist, int64_t ntiles, uint32_t nb, uint32_t* totals) {
  __shared__ uint32_t wsum[GBP_OFF_WAVES][64];
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const uint32_t col = blockIdx.x * 64 + lane;
  const bool ok = col < nb;
  const int64_t chunk = (ntiles + GBP_OFF_WAVES - 1) / GBP_OFF_WAVES;
  const int64_t t0 = min((int64_t)w * chunk, ntiles);
  const int64_t t1 = min(t0 + chunk, ntiles);
  uint32_t s = 0;
  if (ok) {
#pragma unroll 8
    for (int64_t t = t0; t < t1; ++t) s += hist[t * nb + col];
  }
  wsum[w][lane] = s;
  __syncthreads();
  uint32_t run = 0;
  for (int w2 = 0; w2 < w; ++w2) run += wsum[w2][lane];
  if (w == GBP_OFF_WAVES - 1 && ok) totals[col] = run + s;
  if (!ok) return;
  int64_t t = t0;
  for (; t + 8 <= t1; t += 8) {
    uint32_t v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = hist[(t + j) * nb + col];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      hist[(t + j) * nb + col] = run;
      run += v[j];
    }
  }
  for (; t < t1; ++t) {
    const uint32_t v = hist[t * nb + col];
    hist[t * nb + col] = run;
    run += v;
  }
}

// In-place exclusive scan of a[0..nb), nb <= 2 * GBP_THREADS, by the whole
// workgroup (two adjacent entries per thread).  Ends with a barrier.
__device__ __forceinline__ void gbp_block_scan(uint32_t* a, uint32_t nb,
                                               uint32_t* wtmp) {
  const uint32_t i0 = 2 * threadIdx.x;
  const uint32_t x0 = i0 < nb ? a[i0] : 0;
  const uint32_t x1 = i0 + 1 < nb ? a[i0 + 1] : 0;
  const uint32_t s = x0 + x1;
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  uint32_t run = s;  // inclusive wave scan
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t up = __shfl_up(run, off);
    if (lane >= off) run += up;
  }
  if (lane == 63) wtmp[w] = run;
  __syncthreads();
  uint32_t base = 0;
  for (int w2 = 0; w2 < w; ++w2) base += wtmp[w2];
  const uint32_t excl = base + run - s;
  if (i0 < nb) a[i0] = excl;
  if (i0 + 1 < nb) a[i0 + 1] = excl + x0;
  __syncthreads();
}

// The scan of one tile inside k_gbp_scatter.  lstart[b] = rows of bucket
// b in the tile -> their start in the staged tile, as gbp_block_scan
// does.  The thread that scans entries 2t and 2t+1 also keeps their
// cursors base0/base1 (where the next row of the bucket goes in `out`):
// it publishes delta[b] = cursor - start for the tile's stores, then
// moves the cursor past the tile's rows.  Ends with a barrier.
__device__ __forceinline__ void gbp_tile_scan(uint32_t* lstart,
                                              uint32_t* delta, uint32_t nb,
                                              uint32_t* wtmp,
                                              uint32_t* base0,
                                              uint32_t* base1) {
  const uint32_t i0 = 2 * threadIdx.x;
  const uint32_t x0 = i0 < nb ? lstart[i0] : 0;
  const uint32_t x1 = i0 + 1 < nb ? lstart[i0 + 1] : 0;
  const uint32_t s = x0 + x1;
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  uint32_t run = s;  // inclusive wave scan
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t up = __shfl_up(run, off);
    if (lane >= off) run += up;
  }
  if (lane == 63) wtmp[w] = run;
  __syncthreads();
  uint32_t wbase = 0;
  for (int w2 = 0; w2 < w; ++w2) wbase += wtmp[w2];
  const uint32_t excl = wbase + run - s;
  if (i0 < nb) {
    lstart[i0] = excl;
    delta[i0] = *base0 - excl;
    *base0 += x0;
  }
  if (i0 + 1 < nb) {
    lstart[i0 + 1] = excl + x0;
    delta[i0 + 1] = *base1 - (excl + x0);
    *base1 += x1;
  }
  __syncthreads();
}

#define GBP_SCATTER_R (GBP_SCATTER_ROWS / GBP_THREADS)

// The tiles [t0, t1) of one group: k_gbp_scatter below.
template <bool WIDE>
__device__ __forceinline__ void gbp_scatter_group(
    const int64_t* keys, const int64_t* vals, int64_t n, int64_t t0,
    int64_t t1, uint32_t nb, uint32_t seed, uint32_t mask, uint32_t shift,
    const uint32_t* grow, const uint32_t* totals, GbPair* out, GbPair* stage,
    uint32_t* lstart, uint32_t* delta, uint32_t* wtmp) {
  constexpr int R = GBP_SCATTER_R;
  long long k[R], v[R], kn[R], vn[R];
  uint32_t br[R];  // bucket << 16 | rank of the row inside its bucket
  // The small loads go first: loads return in order, and the scan below
  // should not wait for the tile's rows.
  const uint32_t i0 = 2 * threadIdx.x;
  const uint2 tot = i0 + 1 < nb ? *(const uint2*)(totals + i0)
                                : make_uint2(0, 0);
  const uint2 gs = i0 + 1 < nb ? *(const uint2*)(grow + i0)
                               : make_uint2(0, 0);
  gbp_load_rows<WIDE>(keys, t0 * GBP_SCATTER_ROWS, n, k);
  gbp_load_rows<WIDE>(vals, t0 * GBP_SCATTER_ROWS, n, v);
  if (i0 + 1 < nb) {  // nb is a power of two >= 2
    lstart[i0] = 0;
    lstart[i0 + 1] = 0;
    delta[i0] = tot.x;
    delta[i0 + 1] = tot.y;
  }
  __syncthreads();
  gbp_block_scan(delta, nb, wtmp);  // start of each bucket in `out`
  // cursors of buckets 2t and 2t+1: uint32 arithmetic wraps consistently
  // (n < 2^31)
  uint32_t base0 = i0 < nb ? delta[i0] + gs.x : 0;
  uint32_t base1 = i0 + 1 < nb ? delta[i0 + 1] + gs.y : 0;
  for (int64_t t = t0; t < t1; ++t) {
    const uint32_t cnt = (uint32_t)min((int64_t)GBP_SCATTER_ROWS,
                                       n - t * GBP_SCATTER_ROWS);
    if (t + 1 < t1) {
      gbp_load_rows<WIDE>(keys, (t + 1) * GBP_SCATTER_ROWS, n, kn);
      gbp_load_rows<WIDE>(vals, (t + 1) * GBP_SCATTER_ROWS, n, vn);
    }
#pragma unroll
    for (int j = 0; j < R; ++j) {
      if (gbp_row<WIDE>(j) < cnt) {
        const uint32_t b = gbp_bucket(k[j], seed, mask, shift);
        br[j] = (b << 16) | atomicAdd(&lstart[b], 1u);
      }
    }
    __syncthreads();
    gbp_tile_scan(lstart, delta, nb, wtmp, &base0, &base1);
#pragma unroll
    for (int j = 0; j < R; ++j) {
      if (gbp_row<WIDE>(j) < cnt) {
        GbPair pr;
        pr.k = k[j];
        pr.v = v[j];
        stage[lstart[br[j] >> 16] + (br[j] & 0xffffu)] = pr;
      }
    }
    __syncthreads();
    // lstart is free from here: clear it for the next tile
    for (uint32_t b = threadIdx.x; b < nb; b += GBP_THREADS) lstart[b] = 0;
    // destination of staged position p of bucket b = delta[b] + p
    for (uint32_t p = threadIdx.x; p < cnt; p += GBP_THREADS) {
      const GbPair pr = stage[p];
      const uint32_t b = gbp_bucket(pr.k, seed, mask, shift);
      const uint32_t d = delta[b] + p;
      if (d < n) out[d] = pr;  // always true; keeps a bad offset in bounds
    }
    if (t + 1 < t1) {
      __syncthreads();  // stage, delta and lstart go to the next tile
#pragma unroll
      for (int j = 0; j < R; ++j) {
        k[j] = kn[j];
        v[j] = vn[j];
      }
    }
  }
}

// One workgroup per group of G consecutive tiles.  gsum holds the scanned
// matrix (rows of each bucket in earlier groups), totals the rows per
// bucket; together they give the group's cursor into each bucket's
// segment, which then advances tile by tile without leaving the
// workgroup.  The next tile's rows are loaded while the current tile
// goes through LDS.  Consecutive groups are mapped to workgroups 8 apart
// so neighbouring runs of a bucket are written through the same XCD's L2
// and merge into whole lines there.
extern "C" __global__ __launch_bounds__(GBP_THREADS) void k_gbp_scatter(
    const int64_t* keys, const int64_t* vals, int64_t n, int64_t ntiles,
    uint32_t G, int64_t ngroups, uint32_t nb, uint32_t seed, uint32_t mask,
    uint32_t shift, const uint32_t* gsum, const uint32_t* totals,
    GbPair* out) {
  __shared__ GbPair stage[GBP_SCATTER_ROWS];
  __shared__ uint32_t lstart[GBP_MAX_BUCKETS];
  __shared__ uint32_t delta[GBP_MAX_BUCKETS];
  __shared__ uint32_t wtmp[GBP_THREADS / 64];
  const int64_t per_xcd = (ngroups + 7) / 8;
  const int64_t g = (int64_t)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
  if (g >= ngroups) return;
  int64_t t0, t1;
  gbp_group_tiles(g, G, ntiles, &t0, &t1);
  const uint32_t* grow = gsum + g * nb;
  if ((((uintptr_t)keys | (uintptr_t)vals) & 15) == 0)
    gbp_scatter_group<true>(keys, vals, n, t0, t1, nb, seed, mask, shift,
                            grow, totals, out, stage, lstart, delta, wtmp);
  else
    gbp_scatter_group<false>(keys, vals, n, t0, t1, nb, seed, mask, shift,
                             grow, totals, out, stage, lstart, delta, wtmp);
}

// One row through the tile's LDS table; false when the bounded probe
// chain is exhausted (caller goes to the global table).  The LDS index
// remixes the whole slot hash: rows of a tile share its bucket bits.
__device__ __forceinline__ bool gbp_lds_add(long long k, long long v,
                                            long long* lk, long long* lv,
                                            uint32_t seed) {
  uint32_t h = (mm3_u64((uint64_t)k, seed) * 0x9e3779b1u) >>
               (32 - GBP_LDS_BITS);
  for (int p = 0; p < GBP_LDS_PROBES; ++p) {
    long long cur = lk[h];
    if (cur == GB_SENTINEL) {
      const long long prev = atomicCAS((unsigned long long*)&lk[h],
                                       (unsigned long long)GB_SENTINEL,
                                       (unsigned long long)k);
      cur = (prev == GB_SENTINEL) ? k : prev;
    }
    if (cur == k) {
      atomicAdd((unsigned long long*)&lv[h], (unsigned long long)v);
      return true;
    }
    h = (h + 1) & (GBP_LDS_SLOTS - 1);
  }
  return false;
}

// Grid = ceil(n / GBP_TILE_ROWS) over fixed tiles of the partitioned
// buffer: a tile may span bucket boundaries and a skewed bucket spans
// many tiles, so no workgroup's work depends on the key distribution.
//
// CLEAN: the pass after k_gbp_owned.  todo[b] = (start, end) of the rows
// of bucket b that are still to be inserted (the front of its segment:
// what the owner did not reach plus what it spilled), so only rows i
// with i < end[bucket(i)] are live.  The tile works on [first, last), the
// hull of the intervals it meets: empty, it exits before it reads a pair
// or touches its LDS table; at most one row per thread (the usual case:
// a few spilled rows at the start of a segment), the rows go straight to
// the global table.
template <bool CLEAN>
__device__ __forceinline__ void gbp_aggregate_tile(
    const GbPair* pairs, int64_t n, int64_t* tkeys, long long* tab,
    int64_t cap, uint32_t seed, int32_t* sentinel_seen, int32_t* overflow,
    int64_t max_probes, const uint2* todo, uint32_t nb, uint32_t shift) {
  __shared__ long long lk[GBP_LDS_SLOTS];
  __shared__ long long lv[GBP_LDS_SLOTS];
  // CLEAN only; unused in k_gbp_aggregate, where the compiler drops them
  // (its LDS stays 65536 B in the kernel-resource-usage remark)
  __shared__ uint32_t lend[CLEAN ? GBP_MAX_BUCKETS : 1];
  __shared__ uint32_t hull[2];
  const uint64_t gmask = (uint64_t)cap - 1;
  const int64_t base = (int64_t)blockIdx.x * GBP_TILE_ROWS;
  int64_t first = base, last = n;
  if constexpr (CLEAN) {
    const uint32_t t0 = (uint32_t)base;  // n < 2^31
    const uint32_t t1 = (uint32_t)min(base + GBP_TILE_ROWS, n);
    if (threadIdx.x == 0) {
      hull[0] = t1;
      hull[1] = t0;
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < nb; b += GBP_THREADS) {
      const uint2 se = todo[b];
      lend[b] = se.y;
      if (se.y > se.x && se.x < t1 && se.y > t0) {
        atomicMin(&hull[0], max(se.x, t0));
        atomicMax(&hull[1], min(se.y, t1));
      }
    }
    __syncthreads();
    first = hull[0];
    last = hull[1];
    if (first >= last) return;
    if (last - first <= GBP_THREADS) {
      const int64_t i = first + threadIdx.x;
      if (i < last) {
        const GbPair pr = pairs[i];
        if (i < (int64_t)lend[gbp_bucket(pr.k, seed, (uint32_t)gmask, shift)])
          gb_global_insert_sum(pr.k, pr.v, tkeys, tab, gmask, cap, seed,
                               sentinel_seen, overflow, max_probes);
      }
      return;
    }
  }
  for (int s = threadIdx.x; s < GBP_LDS_SLOTS; s += GBP_THREADS) {
    lk[s] = GB_SENTINEL;
    lv[s] = 0;
  }
  __syncthreads();
  // G loads in flight per thread before the first LDS probe
  constexpr int G = 8;
  for (int j0 = 0; j0 < GBP_TILE_ROWS / GBP_THREADS; j0 += G) {
    if (CLEAN && first + j0 * GBP_THREADS >= last) break;
    GbPair pr[G];
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const int64_t i = first + (j0 + j) * GBP_THREADS + threadIdx.x;
      if (i < last) pr[j] = pairs[i];
    }
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const int64_t i = first + (j0 + j) * GBP_THREADS + threadIdx.x;
      bool live = i < last;
      if constexpr (CLEAN)
        live = live &&
               i < (int64_t)lend[gbp_bucket(pr[j].k, seed, (uint32_t)gmask,
                                            shift)];
      if (live && (pr[j].k == GB_SENTINEL ||
                   !gbp_lds_add(pr[j].k, pr[j].v, lk, lv, seed)))
        gb_global_insert_sum(pr[j].k, pr[j].v, tkeys, tab, gmask, cap, seed,
                             sentinel_seen, overflow, max_probes);
    }
  }
  __syncthreads();
  for (int s = threadIdx.x; s < GBP_LDS_SLOTS; s += GBP_THREADS) {
    const long long k = lk[s];
    if (k != GB_SENTINEL)
      gb_global_insert_sum(k, lv[s], tkeys, tab, gmask, cap, seed,
                           sentinel_seen, overflow, max_probes);
  }
}

extern "C" __global__ __launch_bounds__(GBP_THREADS) void k_gbp_aggregate(
    const GbPair* pairs, int64_t n, int64_t* tkeys, long long* tab,
    int64_t cap, uint32_t seed, int32_t* sentinel_seen, int32_t* overflow,
    int64_t max_probes) {
  gbp_aggregate_tile<false>(pairs, n, tkeys, tab, cap, seed, sentinel_seen,
                            overflow, max_probes, nullptr, 0, 0);
}

// ---------------------------------------------------------------------
// Owned slices.  Bucket b is the table range [b*S, (b+1)*S), S = cap / B.
// When S slots fit in LDS, the workgroup that owns bucket b loads that
// slice of the REAL table, runs the table's own linear probe on it with
// LDS atomics and stores it back with plain stores: no global atomic.
//
//   k_gbp_owned    grid = B.  At most GBP_OWN_LIMIT rows from the tail of
//                  segment b, so a heavy bucket costs its owner no more
//                  than a light one.  Rows it cannot place are compacted
//                  to the front of the region it consumed; clean[b] =
//                  rows of segment b, counted from its start, that are
//                  still to be inserted, todo[b] = that interval.
//   k_gbp_cleanup  the tiled aggregate above restricted to those
//                  intervals: the only global atomics left.
//
// Plain stores to a slice happen only in k_gbp_owned, by its owner;
// whatever may touch a foreign slice (a chain that leaves the range,
// the sentinel slot at cap, the rest of an oversize bucket) waits for
// the next launch, so no write-back races an atomic.
//
// A key lands in the slot gb_global_insert_sum would have chosen: the
// probe starts at slot_hash & (S-1) of the slice, walks linearly, claims
// the first empty slot, and gives up after max_probes slots.  A chain
// that reaches the end of the slice is spilled, not wrapped (for the
// last slice that is the table's wrap to slot 0).  The table never
// deletes, so a key that once spilled past its slice end and was stored
// in a later slice still finds every slot from its home to the slice end
// taken, and spills again: it is never stored twice.
#define GBP_OWN_LIMIT (2 * GBP_TILE_ROWS)
#define GBP_OWN_G 8
#define GBP_OWN_CHUNK (GBP_OWN_G * GBP_THREADS)

// One row through the owned slice; false = spill.  *won is set when the
// row claimed an empty slot.
__device__ __forceinline__ bool gbp_own_add(long long k, long long v,
                                            uint32_t l, long long* lk,
                                            long long* lv, uint32_t S,
                                            uint32_t max_probes,
                                            bool* won) {
  for (uint32_t p = 0;;) {
    long long cur = lk[l];
    if (cur == GB_SENTINEL) {
      const long long prev = atomicCAS((unsigned long long*)&lk[l],
                                       (unsigned long long)GB_SENTINEL,
                                       (unsigned long long)k);
      if (prev == GB_SENTINEL) *won = true;
      cur = (prev == GB_SENTINEL) ? k : prev;
    }
    if (cur == k) {
      atomicAdd((unsigned long long*)&lv[l], (unsigned long long)v);
      return true;
    }
    if (++l == S || ++p >= max_probes) return false;
  }
}

extern "C" __global__ __launch_bounds__(GBP_THREADS) void k_gbp_owned(
    GbPair* pairs, int64_t n, const uint32_t* totals, uint32_t nb,
    uint32_t S, int64_t* tkeys, long long* tab, uint32_t seed,
    int64_t max_probes, uint32_t* clean, uint2* todo) {
  extern __shared__ longlong2 gbp_own_lds[];  // S keys, then S sums
  __shared__ uint32_t seg[GBP_MAX_BUCKETS];
  __shared__ uint32_t wtmp[GBP_THREADS / 64];
  __shared__ uint32_t lwon, nspill;
  long long* lk = (long long*)gbp_own_lds;
  long long* lv = lk + S;
  const uint32_t b = blockIdx.x;
  const uint32_t total = totals[b];
  if (total == 0) {  // the slice stays untouched
    if (threadIdx.x == 0) {
      clean[b] = 0;
      todo[b] = make_uint2(0, 0);
    }
    return;
  }
  for (uint32_t i = threadIdx.x; i < nb; i += GBP_THREADS)
    seg[i] = totals[i];
  if (threadIdx.x == 0) {
    lwon = 0;
    nspill = 0;
  }
  __syncthreads();
  gbp_block_scan(seg, nb, wtmp);
  const uint32_t proc = min(total, (uint32_t)GBP_OWN_LIMIT);
  const uint32_t start = seg[b];
  const uint32_t p0 = start + (total - proc);  // processed: [p0, p0+proc)

  GbPair buf[2][GBP_OWN_G];  // chunk c in buf[c & 1], c + 1 in flight
#pragma unroll
  for (int j = 0; j < GBP_OWN_G; ++j) {
    const uint32_t r = j * GBP_THREADS + threadIdx.x;
    if (r < proc && (int64_t)p0 + r < n) buf[0][j] = pairs[p0 + r];
  }

  const int64_t s0 = (int64_t)b * S;
  if (S >= 2) {
    const longlong2* gk = (const longlong2*)(tkeys + s0);
    const longlong2* gv = (const longlong2*)(tab + s0);
#pragma unroll 4
    for (uint32_t i = threadIdx.x; i < S / 2; i += GBP_THREADS) {
      ((longlong2*)lk)[i] = gk[i];
      ((longlong2*)lv)[i] = gv[i];
    }
  } else if (threadIdx.x == 0) {
    lk[0] = tkeys[s0];
    lv[0] = tab[s0];
  }

  const uint32_t maxp =
      (uint32_t)min(max_probes, (int64_t)GBP_LDS_SLOTS);  // S <= slots
  bool won = false;
  // A chunk's spills go to the front of the processed region.  Their
  // count never exceeds the rows of the chunks loaded so far, so a spill
  // never lands on a pair that is still to be read, PROVIDED a chunk's
  // loads are ordered before the other threads' later stores.  Every
  // thread issues the loads of chunk c before the barrier of chunk c and
  // stores spills only after it.  The ordering comes from the workgroup
  // fence that __syncthreads() carries: it keeps the compiler from
  // sinking the loads below the barrier, and the hardware performs a
  // workgroup's loads and stores through one CU in issue order.  A bare
  // __builtin_amdgcn_s_barrier() has no fence and would not be enough.
#pragma unroll
  for (int c = 0; c < GBP_OWN_LIMIT / GBP_OWN_CHUNK; ++c) {
    if ((uint32_t)c * GBP_OWN_CHUNK < proc) {  // uniform
      __syncthreads();  // first chunk: also the slice is in LDS
      if ((uint32_t)(c + 1) * GBP_OWN_CHUNK < proc) {
#pragma unroll
        for (int j = 0; j < GBP_OWN_G; ++j) {
          const uint32_t r =
              (c + 1) * GBP_OWN_CHUNK + j * GBP_THREADS + threadIdx.x;
          if (r < proc && (int64_t)p0 + r < n)
            buf[(c + 1) & 1][j] = pairs[p0 + r];
        }
      }
#pragma unroll
      for (int j = 0; j < GBP_OWN_G; ++j) {
        const uint32_t r = c * GBP_OWN_CHUNK + j * GBP_THREADS + threadIdx.x;
        if (r < proc && (int64_t)p0 + r < n) {
          const GbPair pr = buf[c & 1][j];
          const long long k = pr.k;
          const bool placed =
              k != GB_SENTINEL &&
              gbp_own_add(k, pr.v, mm3_u64((uint64_t)k, seed) & (S - 1),
                          lk, lv, S, maxp, &won);
          if (!placed) {
            const uint32_t d = p0 + atomicAdd(&nspill, 1u);
            if (d < n) pairs[d] = pr;  // always true, as in the scatter
          }
        }
      }
    }
  }
  if (won) lwon = 1;
  __syncthreads();

  if (S >= 2) {
    longlong2* gk = (longlong2*)(tkeys + s0);
    longlong2* gv = (longlong2*)(tab + s0);
    const bool keys_too = lwon != 0;  // no new key: the keys are unchanged
    for (uint32_t i = threadIdx.x; i < S / 2; i += GBP_THREADS) {
      gv[i] = ((const longlong2*)lv)[i];
      if (keys_too) gk[i] = ((const longlong2*)lk)[i];
    }
  } else if (threadIdx.x == 0) {
    tab[s0] = lv[0];
    if (lwon) tkeys[s0] = lk[0];
  }
  if (threadIdx.x == 0) {
    const uint32_t c = (total - proc) + nspill;
    clean[b] = c;
    todo[b] = make_uint2(start, start + c);
  }
}

extern "C" __global__ __launch_bounds__(GBP_THREADS) void k_gbp_cleanup(
    const GbPair* pairs, int64_t n, int64_t* tkeys, long long* tab,
    int64_t cap, uint32_t seed, int32_t* sentinel_seen, int32_t* overflow,
    int64_t max_probes, const uint2* todo, uint32_t nb, uint32_t shift) {
  gbp_aggregate_tile<true>(pairs, n, tkeys, tab, cap, seed, sentinel_seen,
                           overflow, max_probes, todo, nb, shift);
}
