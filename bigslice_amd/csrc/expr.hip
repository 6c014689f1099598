// K13: fused Map/Filter expression kernel.
//
// A Map/Filter chain written in the expression vocabulary (exprs.py)
// arrives as a flat typed bytecode.  k_expr interprets it for a whole
// batch in ONE launch: every needed input column is read once, the
// program runs out of an LDS register file, and the surviving rows are
// written once, in order.
//
// * Program delivery: the ExprProgram struct travels BY VALUE in the
//   kernel arguments (< 1 KiB), so instruction decode is wave-uniform
//   scalar work on the kernarg segment and a launch needs no H2D copy.
// * Register file: virtual registers are 64-bit LDS slots reg[r][tid].
//   A per-thread array indexed by a runtime register number would go to
//   scratch; reg[r][tid] is private to its thread (no barrier between
//   instructions) and consecutive lanes hit consecutive banks.
//   The file is dynamic LDS sized to the program: registers x J x 2 KiB,
//   at most 32 KiB.
// * J rows per thread per decode: an interpreted instruction costs a
//   kernarg fetch, a decode and an LDS round trip, ~400 cycles of
//   latency that 4-8 waves/SIMD cannot hide (measured: one row per
//   decode ran config 2 at 0.7 TB/s).  A program that needs R registers
//   runs J = 4, 2 or 1 slabs per decode (R x J <= 16): the J operand
//   reads go out back to back and the decode is paid once.
// * Slot encoding: bool 0/1, int32 sign-extended, int64 as is, float32
//   bits in the low word, float64 bits.  Integer ops therefore run once
//   in unsigned 64-bit arithmetic (wrapping, no UB) and an int32 result
//   is re-sign-extended from its low word; AND/OR/XOR/WHERE and the
//   integer compares need no dtype at all.
// * One machine op per instruction, each result stored to LDS before
//   the next decode: nothing can contract into an FMA, so float results
//   carry the bits of the same chain of eager torch ops.
// * Geometry as k_runs_sorted (runs.hip): 256-thread blocks, consecutive
//   lanes hold consecutive rows, a tile is BLOCK x IPT rows walked slab
//   by slab, and the next slab's column loads are issued as one burst
//   before the current slab is interpreted.
// * HAS_PRED: pass A runs the predicate section and ballots per-(slab,
//   wave) survivor counts; the in-block scan and the decoupled-lookback
//   tile prefix are the protocol of runs.hip (one {flag|count} word per
//   tile, agent-scope atomics, tile == blockIdx.x, a single spin loop
//   with s_sleep, last tile publishes the total); pass B runs the output
//   section for slabs that kept a row (inputs re-read L2-warm) and
//   writes survivors at tile_base + slab_base + lane rank.

#include <hip/hip_runtime.h>

#include <cstdint>

#define EXPR_BLOCK 256
#define EXPR_IPT 32
#define EXPR_MAX_REGS 16
#define EXPR_MAX_INSTRS 48
#define EXPR_MAX_IN 4
#define EXPR_MAX_OUT 4
#define EXPR_FLAG_AGG 1ull
#define EXPR_FLAG_PREFIX 2ull

enum ExprDt : int { XD_BOOL = 0, XD_I32, XD_I64, XD_F32, XD_F64, XD_N };

enum ExprOp : int {
  XO_CONST = 0, XO_LOAD, XO_CAST, XO_ADD, XO_SUB, XO_MUL, XO_NEG, XO_ABS,
  XO_DIV, XO_FLOORDIV, XO_MOD, XO_AND, XO_OR, XO_XOR, XO_NOT, XO_SHL,
  XO_SHR, XO_EQ, XO_NE, XO_LT, XO_LE, XO_GT, XO_GE, XO_WHERE, XO_MIN,
  XO_MAX, XO_N
};

// w: op | dt<<8 | dst<<16 | a<<24 | b<<32 | c<<40 | flags<<48
struct ExprInstr {
  uint64_t w;
  uint64_t imm;
};

struct ExprProgram {
  ExprInstr ins[EXPR_MAX_INSTRS];
  const void* in_ptr[EXPR_MAX_IN];
  void* out_ptr[EXPR_MAX_OUT];
  uint8_t in_dt[EXPR_MAX_IN];
  uint8_t out_dt[EXPR_MAX_OUT];
  uint8_t out_reg[EXPR_MAX_OUT];
  // Each section opens with its LOADs; the host peels them off into
  // ld_reg (destination register per input slot, section 0 = predicate,
  // 1 = outputs) and the kernel performs them with static slot numbers.
  uint8_t ld_reg[2][EXPR_MAX_IN];
  int32_t pred_begin, n_pred;  // predicate section [pred_begin, n_pred)
  int32_t out_begin, n_total;  // output section [out_begin, n_total)
  int32_t n_in;
  int32_t n_out;
  int32_t pred_reg;
  uint32_t mask_pred;  // input slots the predicate section loads
  uint32_t mask_out;   // input slots the output section loads
};

typedef uint64_t ExprRegs[EXPR_BLOCK];

__device__ __forceinline__ float xf32(uint64_t v) {
  return __uint_as_float((uint32_t)v);
}
__device__ __forceinline__ uint64_t xbits(float f) {
  return (uint64_t)__float_as_uint(f);
}
__device__ __forceinline__ double xf64(uint64_t v) {
  return __longlong_as_double((long long)v);
}
__device__ __forceinline__ uint64_t xbits(double d) {
  return (uint64_t)__double_as_longlong(d);
}
__device__ __forceinline__ uint64_t xsext32(uint64_t v) {
  return (uint64_t)(int64_t)(int32_t)(uint32_t)v;
}

// torch.minimum / torch.maximum: the first NaN operand propagates
__device__ __forceinline__ float xmin(float a, float b) {
  if (a != a) return a;
  if (b != b) return b;
  return fminf(a, b);
}
__device__ __forceinline__ double xmin(double a, double b) {
  if (a != a) return a;
  if (b != b) return b;
  return fmin(a, b);
}
__device__ __forceinline__ float xmax(float a, float b) {
  if (a != a) return a;
  if (b != b) return b;
  return fmaxf(a, b);
}
__device__ __forceinline__ double xmax(double a, double b) {
  if (a != a) return a;
  if (b != b) return b;
  return fmax(a, b);
}
__device__ __forceinline__ float xabs(float a) { return fabsf(a); }
__device__ __forceinline__ double xabs(double a) { return fabs(a); }

template <typename T>
__device__ __forceinline__ uint64_t expr_float_op(int op, T a, T b,
                                                  bool b_imm) {
  switch (op) {
    case XO_ADD: return xbits(a + b);
    case XO_SUB: return xbits(a - b);
    case XO_MUL: return xbits(a * b);
    case XO_NEG: return xbits(-a);
    case XO_ABS: return xbits(xabs(a));
    // torch divides by a scalar as a * (1 / b) on the device
    case XO_DIV: return b_imm ? xbits(a * ((T)1 / b)) : xbits(a / b);
    case XO_MIN: return xbits(xmin(a, b));
    case XO_MAX: return xbits(xmax(a, b));
    case XO_EQ: return a == b;
    case XO_NE: return a != b;
    case XO_LT: return a < b;
    case XO_LE: return a <= b;
    case XO_GT: return a > b;
    case XO_GE: return a >= b;
    default: return 0;
  }
}

// bool / int32 / int64 on the 64-bit slot image; y > 0 for FLOORDIV/MOD
// and 0 <= y < bits for the shifts (both checked at construction)
__device__ __forceinline__ uint64_t expr_int_op(int op, uint64_t x,
                                                uint64_t y) {
  const int64_t sx = (int64_t)x, sy = (int64_t)y;
  switch (op) {
    case XO_ADD: return x + y;
    case XO_SUB: return x - y;
    case XO_MUL: return x * y;
    case XO_NEG: return 0ull - x;
    case XO_ABS: return sx < 0 ? 0ull - x : x;
    case XO_FLOORDIV: {
      if (sy <= 0) return 0;
      const int64_t q = sx / sy;
      return (uint64_t)((sx % sy) < 0 ? q - 1 : q);
    }
    case XO_MOD: {
      if (sy <= 0) return 0;
      const int64_t r = sx % sy;
      return (uint64_t)(r < 0 ? r + sy : r);
    }
    case XO_SHL: return x << (y & 63);
    case XO_SHR: return (uint64_t)(sx >> (y & 63));
    case XO_MIN: return sx < sy ? x : y;
    case XO_MAX: return sx > sy ? x : y;
    case XO_EQ: return sx == sy;
    case XO_NE: return sx != sy;
    case XO_LT: return sx < sy;
    case XO_LE: return sx <= sy;
    case XO_GT: return sx > sy;
    case XO_GE: return sx >= sy;
    default: return 0;
  }
}

__device__ __forceinline__ uint64_t expr_cast(int from, int to,
                                              uint64_t x) {
  if (from <= XD_I64) {
    const int64_t v = (int64_t)x;
    switch (to) {
      case XD_BOOL: return v != 0;
      case XD_I32: return xsext32(x);
      case XD_I64: return x;
      case XD_F32: return xbits((float)v);
      default: return xbits((double)v);
    }
  }
  if (from == XD_F32) {
    const float f = xf32(x);
    switch (to) {
      case XD_BOOL: return f != 0.0f;
      case XD_I32: return (uint64_t)(int64_t)(int32_t)f;
      case XD_I64: return (uint64_t)(int64_t)f;
      case XD_F32: return x;
      default: return xbits((double)f);
    }
  }
  const double d = xf64(x);
  switch (to) {
    case XD_BOOL: return d != 0.0;
    case XD_I32: return (uint64_t)(int64_t)(int32_t)d;
    case XD_I64: return (uint64_t)(int64_t)d;
    case XD_F32: return xbits((float)d);
    default: return x;
  }
}

// Prefetched raw column bits, one named scalar per input slot (an
// array here would be indexed by the unrolled slot loops early enough
// to land in scratch).
struct ExprIn {
  uint64_t v0, v1, v2, v3;
};
static_assert(EXPR_MAX_IN == 4, "ExprIn holds four slots");

template <int K>
__device__ __forceinline__ uint64_t expr_fetch1(const ExprProgram& P,
                                                uint32_t mask, int64_t r,
                                                int64_t n) {
  uint64_t x = 0;
  if (((mask >> K) & 1u) && r < n) {
    const int dt = P.in_dt[K];
    const void* p = P.in_ptr[K];
    if (dt == XD_BOOL)
      x = ((const uint8_t*)p)[r];
    else if (dt == XD_I32 || dt == XD_F32)
      x = ((const uint32_t*)p)[r];
    else
      x = ((const uint64_t*)p)[r];
  }
  return x;
}

// Raw column bits of row r for the input slots in `mask` (zero past n).
__device__ __forceinline__ ExprIn expr_fetch(const ExprProgram& P,
                                             uint32_t mask, int64_t r,
                                             int64_t n) {
  ExprIn v;
  v.v0 = expr_fetch1<0>(P, mask, r, n);
  v.v1 = expr_fetch1<1>(P, mask, r, n);
  v.v2 = expr_fetch1<2>(P, mask, r, n);
  v.v3 = expr_fetch1<3>(P, mask, r, n);
  return v;
}

// The section's LOADs: widen each prefetched column value into its
// register slot.
template <int K, int J>
__device__ __forceinline__ void expr_load1(const ExprProgram& P, int sec,
                                           uint32_t mask, ExprRegs* R,
                                           int tid, int j, uint64_t x) {
  if ((mask >> K) & 1u) {
    const int dt = P.in_dt[K];
    R[P.ld_reg[sec][K] * J + j][tid] =
        dt == XD_BOOL ? (uint64_t)(x != 0)
                      : (dt == XD_I32 ? xsext32(x) : x);
  }
}
template <int J>
__device__ __forceinline__ void expr_load(const ExprProgram& P, int sec,
                                          uint32_t mask, ExprRegs* R,
                                          int tid, int j,
                                          const ExprIn& in) {
  expr_load1<0, J>(P, sec, mask, R, tid, j, in.v0);
  expr_load1<1, J>(P, sec, mask, R, tid, j, in.v1);
  expr_load1<2, J>(P, sec, mask, R, tid, j, in.v2);
  expr_load1<3, J>(P, sec, mask, R, tid, j, in.v3);
}

// One decoded instruction on one row's operand values.
__device__ __forceinline__ uint64_t expr_exec(int op, int dt, int c,
                                              bool b_imm, uint64_t x,
                                              uint64_t y, uint64_t z) {
  if (op == XO_CAST) return expr_cast(c, dt, x);
  if (op == XO_WHERE) return (x & 1u) ? y : z;
  if (op == XO_AND) return x & y;
  if (op == XO_OR) return x | y;
  if (op == XO_XOR) return x ^ y;
  if (op == XO_NOT) return dt == XD_BOOL ? (x ^ 1ull) : ~x;
  if (dt == XD_F32)
    return expr_float_op<float>(op, xf32(x), xf32(y), b_imm);
  if (dt == XD_F64)
    return expr_float_op<double>(op, xf64(x), xf64(y), b_imm);
  const uint64_t res = expr_int_op(op, x, y);
  return (dt == XD_I32 && op < XO_EQ) ? xsext32(res) : res;
}

// Interpret instructions [i0, i1) for this thread's J rows; register r
// of row j is R[r * J + j][tid].
template <int J>
__device__ __forceinline__ void expr_run(const ExprProgram& P, int i0,
                                         int i1, ExprRegs* R, int tid) {
#pragma unroll 1
  for (int i = i0; i < i1; ++i) {
    const uint64_t w = P.ins[i].w;
    const uint64_t imm = P.ins[i].imm;
    const int op = (int)(w & 0xff);
    const int dt = (int)((w >> 8) & 0xff);
    const int dst = (int)((w >> 16) & 0xff);
    const int a = (int)((w >> 24) & 0xff);
    const int b = (int)((w >> 32) & 0xff);
    const int c = (int)((w >> 40) & 0xff);
    const bool b_imm = (w >> 48) & 1u;
    uint64_t x[J], y[J], z[J];
    if (op == XO_CONST) {
#pragma unroll
      for (int j = 0; j < J; ++j) R[dst * J + j][tid] = imm;
      continue;
    }
#pragma unroll
    for (int j = 0; j < J; ++j) x[j] = R[a * J + j][tid];
#pragma unroll
    for (int j = 0; j < J; ++j) y[j] = b_imm ? imm : R[b * J + j][tid];
#pragma unroll
    for (int j = 0; j < J; ++j)
      z[j] = (op == XO_WHERE) ? R[c * J + j][tid] : 0;
#pragma unroll
    for (int j = 0; j < J; ++j)
      R[dst * J + j][tid] = expr_exec(op, dt, c, b_imm, x[j], y[j], z[j]);
  }
}

template <int J>
__device__ __forceinline__ void expr_store(const ExprProgram& P,
                                           ExprRegs* R, int tid, int j,
                                           int64_t pos) {
#pragma unroll
  for (int o = 0; o < EXPR_MAX_OUT; ++o) {
    if (o < P.n_out) {
      const uint64_t v = R[P.out_reg[o] * J + j][tid];
      const int dt = P.out_dt[o];
      void* p = P.out_ptr[o];
      if (dt == XD_BOOL)
        ((uint8_t*)p)[pos] = (uint8_t)(v & 1u);
      else if (dt == XD_I32 || dt == XD_F32)
        ((uint32_t*)p)[pos] = (uint32_t)v;
      else
        ((uint64_t*)p)[pos] = v;
    }
  }
}

extern __shared__ uint64_t expr_lds[];

template <bool HAS_PRED, int J>
__global__ __launch_bounds__(EXPR_BLOCK, 4) void k_expr(
    const ExprProgram P, int64_t n, int64_t* __restrict__ count_out,
    unsigned long long* __restrict__ state) {
  constexpr int WAVES = EXPR_BLOCK / 64;
  constexpr int IPT = EXPR_IPT;
  constexpr int64_t TILE = (int64_t)EXPR_BLOCK * IPT;
  static_assert(EXPR_IPT % J == 0, "a tile is whole groups of J slabs");
  ExprRegs* R = (ExprRegs*)expr_lds;  // [registers * J], host-sized
  const int tid = threadIdx.x;
  const int tile = blockIdx.x;
  const int64_t base = (int64_t)tile * TILE;

  if constexpr (!HAS_PRED) {
    ExprIn nxt[J];
#pragma unroll
    for (int j = 0; j < J; ++j)
      nxt[j] = expr_fetch(P, P.mask_out,
                          base + (int64_t)j * EXPR_BLOCK + tid, n);
#pragma unroll 1
    for (int k0 = 0; k0 < IPT; k0 += J) {
      const int64_t r0 = base + (int64_t)k0 * EXPR_BLOCK + tid;
      if (r0 - tid >= n) break;  // block-uniform
#pragma unroll
      for (int j = 0; j < J; ++j)
        expr_load<J>(P, 1, P.mask_out, R, tid, j, nxt[j]);
      if (k0 + J < IPT) {
#pragma unroll
        for (int j = 0; j < J; ++j)
          nxt[j] = expr_fetch(P, P.mask_out,
                              r0 + (int64_t)(J + j) * EXPR_BLOCK, n);
      }
      expr_run<J>(P, P.out_begin, P.n_total, R, tid);
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const int64_t r = r0 + (int64_t)j * EXPR_BLOCK;
        if (r < n) expr_store<J>(P, R, tid, j, r);
      }
    }
    return;
  } else {
    __shared__ unsigned int cnt[IPT * WAVES];  // slab-major
    __shared__ unsigned int wtot[WAVES];       // per-wave totals
    __shared__ unsigned long long lds_base[1];
    const int wave = tid / 64;
    const int lane = tid % 64;
    const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));

    // pass A: predicate -> keep bits + per-(slab, wave) counts
    unsigned int fb = 0;  // this thread's keep bit per slab (IPT <= 32)
    unsigned int my_wtot = 0;
    {
      ExprIn nxt[J];
#pragma unroll
      for (int j = 0; j < J; ++j)
        nxt[j] = expr_fetch(P, P.mask_pred,
                            base + (int64_t)j * EXPR_BLOCK + tid, n);
#pragma unroll 1
      for (int k0 = 0; k0 < IPT; k0 += J) {
        const int64_t r0 = base + (int64_t)k0 * EXPR_BLOCK + tid;
        const bool live = r0 - lane < n;  // wave-uniform
        if (live) {
#pragma unroll
          for (int j = 0; j < J; ++j)
            expr_load<J>(P, 0, P.mask_pred, R, tid, j, nxt[j]);
          if (k0 + J < IPT) {
#pragma unroll
            for (int j = 0; j < J; ++j)
              nxt[j] = expr_fetch(P, P.mask_pred,
                                  r0 + (int64_t)(J + j) * EXPR_BLOCK, n);
          }
          expr_run<J>(P, P.pred_begin, P.n_pred, R, tid);
        }
#pragma unroll
        for (int j = 0; j < J; ++j) {
          const int k = k0 + j;
          const int64_t r = r0 + (int64_t)j * EXPR_BLOCK;
          const bool flag =
              live && (r < n) && (R[P.pred_reg * J + j][tid] & 1u);
          fb |= flag ? (1u << k) : 0u;
          const uint64_t bal = __ballot(flag);
          if (lane == 0) {
            const unsigned int c = (unsigned int)__popcll(bal);
            cnt[k * WAVES + wave] = c;
            my_wtot += c;
          }
        }
      }
    }
    if (lane == 0) wtot[wave] = my_wtot;
    __syncthreads();

    // Inter-tile prefix, as k_runs_sorted: wave 0 publishes the tile
    // aggregate at once and walks 64 predecessors per round; wave 1
    // meanwhile scans the slab counters (totals come from wtot, not
    // cnt, which wave 1 is overwriting).
    constexpr int NCNT = IPT * WAVES;
    unsigned int run = 0;
    if (wave == 0) {
      unsigned int s = (lane < WAVES) ? wtot[lane] : 0;
      for (int off = 32; off; off >>= 1)
        s += (unsigned int)__shfl_xor((int)s, off, 64);
      run = s;  // wave-uniform total
      if (lane == 0) {
        const unsigned long long pub =
            ((tile == 0 ? EXPR_FLAG_PREFIX : EXPR_FLAG_AGG) << 62) |
            (unsigned long long)run;
        __hip_atomic_store(&state[tile], pub, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
      }
      unsigned long long excl = 0;
      if (tile > 0) {
        int j0 = tile - 1;
        bool done = false;
        while (!done) {
          const int idx = j0 - lane;
          unsigned long long x = 0;
          if (idx >= 0) {
            x = __hip_atomic_load(&state[idx], __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);
            while ((x >> 62) == 0) {
              __builtin_amdgcn_s_sleep(1);
              x = __hip_atomic_load(&state[idx], __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_AGENT);
            }
          }
          const uint64_t pmask =
              __ballot(idx >= 0 && (x >> 62) == EXPR_FLAG_PREFIX);
          unsigned long long c = x & ((1ull << 62) - 1);
          if (pmask) {
            const int lp = __ffsll((unsigned long long)pmask) - 1;
            if (lane > lp) c = 0;
            done = true;
          } else if (idx < 0) {
            c = 0;
          }
          for (int off = 32; off; off >>= 1)
            c += __shfl_xor((unsigned long long)c, off, 64);
          excl += c;
          j0 -= 64;
          if (j0 < 0) done = true;
        }
        if (lane == 0)
          __hip_atomic_store(
              &state[tile],
              (EXPR_FLAG_PREFIX << 62) | (excl + (unsigned long long)run),
              __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      if (lane == 0) {
        lds_base[0] = excl;
        if (tile == (int)gridDim.x - 1)
          *count_out = (int64_t)(excl + run);
      }
    } else if (wave == 1) {
      unsigned int carry = 0;
      for (int i0 = 0; i0 < NCNT; i0 += 64) {
        const unsigned int v = cnt[i0 + lane];
        unsigned int incl = v;
        for (int off = 1; off < 64; off <<= 1) {
          const unsigned int up =
              (unsigned int)__shfl_up((int)incl, off, 64);
          if (lane >= off) incl += up;
        }
        cnt[i0 + lane] = carry + incl - v;
        carry += (unsigned int)__shfl((int)incl, 63, 64);
      }
    }
    __syncthreads();
    const unsigned long long tb = lds_base[0];

    // pass B: outputs for the groups that kept a row, ordered writes
#pragma unroll 1
    for (int k0 = 0; k0 < IPT; k0 += J) {
      const unsigned int grp = (fb >> k0) & ((J == 32) ? ~0u : ((1u << J) - 1));
      if (__ballot(grp != 0) == 0) continue;  // wave-uniform
      const int64_t r0 = base + (int64_t)k0 * EXPR_BLOCK + tid;
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const ExprIn cur = expr_fetch(
            P, P.mask_out, r0 + (int64_t)j * EXPR_BLOCK, n);
        expr_load<J>(P, 1, P.mask_out, R, tid, j, cur);
      }
      expr_run<J>(P, P.out_begin, P.n_total, R, tid);
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const bool flag = (grp >> j) & 1u;
        const uint64_t bal = __ballot(flag);
        if (flag) {
          const unsigned int pos = cnt[(k0 + j) * WAVES + wave] +
                                   (unsigned int)__popcll(bal & lt);
          expr_store<J>(P, R, tid, j, (int64_t)(tb + pos));
        }
      }
    }
  }
}
