// K20: device tokenizer — split the rows of a BYTES column into tokens.
//
// A token is a maximal run of non-delimiter bytes inside one row: byte
// p starts a token iff it is kept (not in the delimiter set) and either
// p is the first byte of its row or byte p-1 is a delimiter.  Splitting
// is therefore a double stream compaction over bytes: kept bytes
// compact into out_data, token starts compact into out_offsets (the
// rank of the start among kept bytes) and, on request, tok_row.
//
// Three steps on one stream, no workgroup waits on another:
//   k_tok_count  per tile (kept bytes, token starts) -> counts[tile][2]
//   (host side)  scan of counts over tiles (torch.cumsum; plumbing)
//   k_tok_write  re-read the tile, rank inside it, add the tile bases
//
// Geometry: a tile is TOK_TILE bytes = TOK_CHUNKS slabs of TOK_BLOCK
// 16-byte chunks; in slab j thread t owns the chunk at tile offset
// (j*TOK_BLOCK + t)*16, so a wave's 16-byte loads cover 1 KiB
// contiguous.  Byte order inside a tile is (slab, wave, lane, byte) and
// that is also position order.  A lane's chunk yields two 16-bit masks
// (kept, start); ranks across lanes are bit-sliced ballot/popcount
// sums, ranks across the TOK_CHUNKS*WAVES (slab, wave) segments come
// from a small LDS scan.
//
// Row starts: one binary search per tile finds the first row starting
// at or after the tile; the workgroup then walks the rows that begin in
// the tile with a strided loop, OR-ing one bit per row start into an
// LDS bitmask — thousands of empty rows in one tile are just more loop
// trips, nothing is sized by rows per tile.

#include <hip/hip_runtime.h>

#include <cstdint>

#define TOK_BLOCK 256
#define TOK_CHUNKS 4
#define TOK_TILE (TOK_BLOCK * TOK_CHUNKS * 16)  // 16 KiB
#define TOK_WAVES (TOK_BLOCK / 64)
#define TOK_SEGS (TOK_CHUNKS * TOK_WAVES)

struct TokMask {
  unsigned long long w0, w1, w2, w3;  // bit b of the 256-bit set
};

struct TokTile {
  unsigned int keep_lut[256 / 4];        // byte b -> 1 if kept
  unsigned int rowbits[TOK_TILE / 32];   // row start at tile offset q
  int64_t row_lo, row_hi;                // tok_row search bracket
};

__device__ __forceinline__ unsigned int tok_lut(const TokTile& s,
                                                unsigned int b) {
  return ((const unsigned char*)s.keep_lut)[b];
}

// First index r in [0, n] with offsets[r] >= x (n when none).
__device__ __forceinline__ int64_t tok_lower_bound(
    const int64_t* __restrict__ offsets, int64_t n, int64_t x) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (offsets[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Fill the kept-byte table and the row-start bitmask of this tile.
// Ends with a barrier; row_lo/row_hi bracket every position of the tile
// for the per-token row search: offsets[row_lo] <= p < offsets[row_hi].
__device__ __forceinline__ void tok_prologue(
    TokTile& s, const int64_t* __restrict__ offsets, int64_t n,
    int64_t tile_base, int64_t tile_end, TokMask m, bool with_rows) {
  const int t = threadIdx.x;
  {
    const unsigned long long w =
        (t < 64) ? m.w0 : (t < 128) ? m.w1 : (t < 192) ? m.w2 : m.w3;
    ((unsigned char*)s.keep_lut)[t] =
        (unsigned char)(((w >> (t & 63)) & 1ull) ^ 1ull);
  }
  for (int i = t; i < TOK_TILE / 32; i += TOK_BLOCK) s.rowbits[i] = 0;
  if (t == 0) {
    const int64_t r0 = tok_lower_bound(offsets, n, tile_base);
    s.row_lo = r0 > 0 ? r0 - 1 : 0;
  }
  if (with_rows && t == 64)
    s.row_hi = tok_lower_bound(offsets, n, tile_end);
  __syncthreads();
  // rows 0..n-1 start at offsets[r]; offsets[n] (== total) starts none
  int64_t r = s.row_lo + t;
  while (r < n) {
    const int64_t off = offsets[r];
    if (off >= tile_end) break;
    if (off >= tile_base) {
      const unsigned int q = (unsigned int)(off - tile_base);
      atomicOr(&s.rowbits[q >> 5], 1u << (q & 31));
    }
    r += TOK_BLOCK;
  }
  __syncthreads();
}

// One 16-byte chunk at absolute position p (tile offset q): the bytes,
// the mask of kept bytes and the mask of token starts.
__device__ __forceinline__ void tok_chunk(
    const TokTile& s, const uint8_t* __restrict__ data, int64_t total,
    int64_t p, unsigned int q, uint4& v, unsigned int& keep,
    unsigned int& start) {
  const int lane = threadIdx.x & 63;
  v = make_uint4(0, 0, 0, 0);
  int valid = 0;
  if (p + 16 <= total) {
    v = *reinterpret_cast<const uint4*>(data + p);
    valid = 16;
  } else if (p < total) {
    valid = (int)(total - p);
    unsigned int w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (i < valid) w[i >> 2] |= (unsigned int)data[p + i] << ((i & 3) * 8);
    v = make_uint4(w[0], w[1], w[2], w[3]);
  }
  const unsigned int vw[4] = {v.x, v.y, v.z, v.w};
  unsigned int k = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const unsigned int b = (vw[i >> 2] >> ((i & 3) * 8)) & 0xFFu;
    k |= tok_lut(s, b) << i;
  }
  k &= (1u << valid) - 1u;
  // kept flag of byte p-1: the previous lane's last byte, except for
  // lane 0, whose neighbour lies in another wave, slab or tile
  unsigned int prev = (unsigned int)__shfl_up((int)(k >> 15), 1, 64);
  if (lane == 0) prev = (p > 0 && p < total) ? tok_lut(s, data[p - 1]) : 0u;
  const unsigned int rb = (s.rowbits[q >> 5] >> (q & 31)) & 0xFFFFu;
  keep = k;
  start = k & (~((k << 1) | prev) | rb) & 0xFFFFu;
}

// Exclusive prefix over the wave's lanes, and the wave total, of a
// per-lane count c in [0, 16]: five ballots, one per bit of c.
__device__ __forceinline__ void tok_wave_scan(unsigned int c, uint64_t lt,
                                              unsigned int& excl,
                                              unsigned int& total) {
  excl = 0;
  total = 0;
#pragma unroll
  for (int b = 0; b < 5; ++b) {
    const uint64_t m = __ballot((c >> b) & 1u);
    excl += (unsigned int)__popcll(m & lt) << b;
    total += (unsigned int)__popcll(m) << b;
  }
}

__global__ __launch_bounds__(TOK_BLOCK) void k_tok_count(
    const uint8_t* __restrict__ data, int64_t total,
    const int64_t* __restrict__ offsets, int64_t n, TokMask m,
    unsigned int* __restrict__ counts) {
  __shared__ TokTile s;
  __shared__ unsigned int part[TOK_WAVES][2];
  const int64_t tile_base = (int64_t)blockIdx.x * TOK_TILE;
  const int64_t tile_end = tile_base + TOK_TILE;
  tok_prologue(s, offsets, n, tile_base, tile_end, m, false);
  unsigned int nk = 0, ns = 0;
#pragma unroll
  for (int j = 0; j < TOK_CHUNKS; ++j) {
    const unsigned int q = (unsigned int)(j * TOK_BLOCK + threadIdx.x) * 16u;
    uint4 v;
    unsigned int keep, start;
    tok_chunk(s, data, total, tile_base + q, q, v, keep, start);
    nk += __popc(keep);
    ns += __popc(start);
  }
  for (int off = 32; off; off >>= 1) {
    nk += (unsigned int)__shfl_xor((int)nk, off, 64);
    ns += (unsigned int)__shfl_xor((int)ns, off, 64);
  }
  const int wave = threadIdx.x / 64;
  if ((threadIdx.x & 63) == 0) {
    part[wave][0] = nk;
    part[wave][1] = ns;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    unsigned int sum = 0;
#pragma unroll
    for (int w = 0; w < TOK_WAVES; ++w) sum += part[w][threadIdx.x];
    counts[(int64_t)blockIdx.x * 2 + threadIdx.x] = sum;
  }
}

// incl: inclusive scan of counts over tiles, uint32 [tiles][2].  nkept
// and ntok are its last row; they size the outputs and every store is
// checked against them.
__global__ __launch_bounds__(TOK_BLOCK) void k_tok_write(
    const uint8_t* __restrict__ data, int64_t total,
    const int64_t* __restrict__ offsets, int64_t n, TokMask m,
    const unsigned int* __restrict__ incl, int64_t nkept, int64_t ntok,
    uint8_t* __restrict__ out_data, int64_t* __restrict__ out_offsets,
    int64_t* __restrict__ tok_row) {
  __shared__ TokTile s;
  __shared__ unsigned int seg[2][TOK_SEGS + 1];
  // kept bytes of the tile in order; the pad lets the copy-out read
  // whole dwords past the last kept byte
  __shared__ unsigned int stage[TOK_TILE / 4 + 8];
  const bool with_rows = tok_row != nullptr;
  const int tile = blockIdx.x;
  const int64_t tile_base = (int64_t)tile * TOK_TILE;
  const int64_t tile_end = tile_base + TOK_TILE;
  tok_prologue(s, offsets, n, tile_base, tile_end, m, with_rows);
  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x & 63;
  const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));

  uint4 v[TOK_CHUNKS];
  unsigned int keep[TOK_CHUNKS], start[TOK_CHUNKS];
  unsigned int kex[TOK_CHUNKS], sex[TOK_CHUNKS];
#pragma unroll
  for (int j = 0; j < TOK_CHUNKS; ++j) {
    const unsigned int q = (unsigned int)(j * TOK_BLOCK + threadIdx.x) * 16u;
    tok_chunk(s, data, total, tile_base + q, q, v[j], keep[j], start[j]);
    unsigned int kt, st;
    tok_wave_scan(__popc(keep[j]), lt, kex[j], kt);
    tok_wave_scan(__popc(start[j]), lt, sex[j], st);
    if (lane == 0) {
      seg[0][j * TOK_WAVES + wave] = kt;
      seg[1][j * TOK_WAVES + wave] = st;
    }
  }
  __syncthreads();
  // exclusive scan of the segment totals, in place; entry TOK_SEGS
  // receives the tile total
  if (threadIdx.x < 2) {
    unsigned int run = 0;
    for (int i = 0; i < TOK_SEGS; ++i) {
      const unsigned int c = seg[threadIdx.x][i];
      seg[threadIdx.x][i] = run;
      run += c;
    }
    seg[threadIdx.x][TOK_SEGS] = run;
  }
  __syncthreads();
  const int64_t kbase = tile > 0 ? incl[(int64_t)(tile - 1) * 2] : 0;
  const int64_t tbase = tile > 0 ? incl[(int64_t)(tile - 1) * 2 + 1] : 0;
  const unsigned int tile_kept = seg[0][TOK_SEGS];

  unsigned char* sb = (unsigned char*)stage;
#pragma unroll
  for (int j = 0; j < TOK_CHUNKS; ++j) {
    const unsigned int q = (unsigned int)(j * TOK_BLOCK + threadIdx.x) * 16u;
    const unsigned int k = keep[j];
    const unsigned int kpos0 = seg[0][j * TOK_WAVES + wave] + kex[j];
    const unsigned int vw[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
    unsigned int kpos = kpos0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if ((k >> i) & 1u) {
        // kpos < TOK_TILE: at most one kept byte per tile byte
        sb[kpos] = (unsigned char)(vw[i >> 2] >> ((i & 3) * 8));
        ++kpos;
      }
    }
    unsigned int st = start[j];
    int64_t spos = tbase + seg[1][j * TOK_WAVES + wave] + sex[j];
    while (st) {
      const int i = __ffs(st) - 1;
      st &= st - 1;
      if (spos < ntok) {
        out_offsets[spos] =
            kbase + kpos0 + __popc(k & ((1u << i) - 1u));
        if (with_rows) {
          const int64_t p = tile_base + q + i;
          int64_t lo = s.row_lo, hi = s.row_hi;
          while (hi - lo > 1) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (offsets[mid] <= p) lo = mid; else hi = mid;
          }
          tok_row[spos] = lo;
        }
      }
      ++spos;
    }
  }
  if (tile == (int)gridDim.x - 1 && threadIdx.x == 0)
    out_offsets[ntok] = kbase + tile_kept;
  __syncthreads();

  // copy the staged bytes out as contiguous runs: single bytes up to
  // the first 16-byte boundary of the destination, 16-byte stores, then
  // the remaining bytes
  int64_t cnt = tile_kept;
  if (kbase + cnt > nkept) cnt = nkept > kbase ? nkept - kbase : 0;
  uint8_t* dst = out_data + kbase;
  int head = (int)((16u - (unsigned int)((uintptr_t)dst & 15u)) & 15u);
  if (head > cnt) head = (int)cnt;
  if ((int)threadIdx.x < head) dst[threadIdx.x] = sb[threadIdx.x];
  const int nvec = (int)((cnt - head) >> 4);
  const unsigned int sh = (unsigned int)(head & 3) * 8u;
  for (int u = threadIdx.x; u < nvec; u += TOK_BLOCK) {
    const int d0 = (head + u * 16) >> 2;  // <= TOK_TILE/4 - 4 + 3
    unsigned int d[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) d[i] = stage[d0 + i];
    uint4 o;
    o.x = (unsigned int)((((uint64_t)d[1] << 32) | d[0]) >> sh);
    o.y = (unsigned int)((((uint64_t)d[2] << 32) | d[1]) >> sh);
    o.z = (unsigned int)((((uint64_t)d[3] << 32) | d[2]) >> sh);
    o.w = (unsigned int)((((uint64_t)d[4] << 32) | d[3]) >> sh);
    *reinterpret_cast<uint4*>(dst + head + (int64_t)u * 16) = o;
  }
  const int tail0 = head + nvec * 16;
  const int ntail = (int)cnt - tail0;  // < 16
  if ((int)threadIdx.x < ntail)
    dst[tail0 + threadIdx.x] = sb[tail0 + threadIdx.x];
}
