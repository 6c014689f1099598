// K23: variable-length row gather — out row j is source row rows[j] of a
// BYTES column (data, offsets).  offsets is absolute into data and need
// not start at 0: a zero-copy slice gathers without compacting first.
//
// Three steps on one stream:
//   k_bg_lens   length of every selected row, one thread per row; a row
//               index outside [0, n) has length 0
//   (host side) 1-D inclusive scan of the lengths -> out_offsets
//   k_bg_copy   output-centric copy: every lane owns one aligned 16-byte
//               chunk of the output.  It finds the row of its first byte
//               by binary search over out_offsets inside a bracket its
//               workgroup found once, walks forward over the row
//               boundaries (zero-length rows are just more steps of the
//               walk) while it assembles its bytes, and stores them with
//               one 16-byte store.  Only the last, partial chunk leaves
//               byte by byte.
//
// Every store is checked against the output length and every load
// against the length of data, so a wrong total or corrupt offsets leave
// bytes unwritten; they do not fault.

#include <hip/hip_runtime.h>

#include <cstdint>

#define BG_BLOCK 256
#define BG_TILE (BG_BLOCK * 16)  // output bytes per workgroup

__global__ void k_bg_lens(const int64_t* __restrict__ offsets, int64_t n,
                          const int64_t* __restrict__ rows, int64_t m,
                          int64_t* __restrict__ lens) {
  int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; j < m; j += stride) {
    const int64_t r = rows[j];
    int64_t len = 0;
    if (r >= 0 && r < n) len = offsets[r + 1] - offsets[r];
    lens[j] = len > 0 ? len : 0;
  }
}

// Largest j in [lo, hi] with out_off[j] <= x; out_off[lo] <= x is given.
__device__ __forceinline__ int64_t bg_last_le(
    const int64_t* __restrict__ out_off, int64_t lo, int64_t hi, int64_t x) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo + 1) >> 1);
    if (out_off[mid] <= x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// out_off: int64[m + 1], out_off[0] == 0; total: bytes of out, m >= 1.
__global__ __launch_bounds__(BG_BLOCK) void k_bg_copy(
    const uint8_t* __restrict__ data, int64_t data_len,
    const int64_t* __restrict__ offsets, int64_t n,
    const int64_t* __restrict__ rows, int64_t m,
    const int64_t* __restrict__ out_off, int64_t total,
    uint8_t* __restrict__ out) {
  __shared__ int64_t s_lo, s_hi;
  const int64_t tile_base = (int64_t)blockIdx.x * BG_TILE;
  if (tile_base >= total) return;
  const int64_t tile_last =
      (tile_base + BG_TILE <= total ? tile_base + BG_TILE : total) - 1;
  // the rows of the tile's first and last byte bracket every lane's
  if (threadIdx.x == 0) s_lo = bg_last_le(out_off, 0, m - 1, tile_base);
  if (threadIdx.x == 64) s_hi = bg_last_le(out_off, 0, m - 1, tile_last);
  __syncthreads();
  const int64_t p = tile_base + (int64_t)threadIdx.x * 16;
  if (p >= total) return;
  int64_t j = bg_last_le(out_off, s_lo, s_hi, p);
  // row j covers out bytes [row_beg, row_end); out byte q is data byte
  // q + delta while ok (the row index is in range)
  int64_t row_beg = out_off[j];
  int64_t row_end = out_off[j + 1];
  int64_t r = rows[j];
  bool ok = r >= 0 && r < n;
  int64_t delta = ok ? offsets[r] - row_beg : 0;
  const int valid = total - p < 16 ? (int)(total - p) : 16;
  unsigned int w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int b = 0; b < 16; ++b) {
    if (b < valid) {
      const int64_t q = p + b;
      while (j < m && q >= row_end) {
        ++j;
        if (j < m) {
          row_beg = row_end;
          row_end = out_off[j + 1];
          r = rows[j];
          ok = r >= 0 && r < n;
          delta = ok ? offsets[r] - row_beg : 0;
        }
      }
      if (j < m && ok) {
        const int64_t s = q + delta;
        if (s >= 0 && s < data_len)
          w[b >> 2] |= (unsigned int)data[s] << ((b & 3) * 8);
      }
    }
  }
  if (valid == 16) {
    *reinterpret_cast<uint4*>(out + p) = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
#pragma unroll
    for (int b = 0; b < 16; ++b)
      if (b < valid) out[p + b] = (uint8_t)(w[b >> 2] >> ((b & 3) * 8));
  }
}
