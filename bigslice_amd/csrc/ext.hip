// bigslice_amd._C — torch extension binding the CDNA4 kernels:
//   hash_columns      (K3 murmur3 row hash)
//   hash_partition /  (K4 fused hash+histogram+scatter partitioner)
//   scatter_by_partition
//   groupby           (K9 hash-aggregate)
//   radix_argsort     (K6 device radix sort)
//   runs_multi /      (K22 run boundaries and lexicographic search over
//   lex_searchsorted   multi-column keys)
//
// Single translation unit: the kernel files are included directly.

#include <torch/extension.h>

#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include <vector>

#include "hash_partition.hip"
#include "groupby.hip"
#include "groupby_part.hip"
#include "groupby_finish.hip"
#include "sort.hip"
#include "radix.hip"
#include "runs.hip"
#include "runs_multi.hip"
#include "vecagg.hip"
#include "strings.hip"
#include "expr.hip"
#include "tokenize.hip"
#include "groupby_multi.hip"
#include "iddict.hip"
#include "bytes_gather.hip"
#include "bytes_order.hip"

namespace {

#define HIP_CHECK(expr)                                              \
  do {                                                               \
    hipError_t _e = (expr);                                          \
    TORCH_CHECK(_e == hipSuccess, "HIP error: ",                     \
                hipGetErrorString(_e));                              \
  } while (0)

int32_t dtype_code(const torch::Tensor& t) {
  switch (t.scalar_type()) {
    case torch::kInt8: return DT_I8;
    case torch::kUInt8: return DT_U8;
    case torch::kInt16: return DT_I16;
    case torch::kInt32: return DT_I32;
    case torch::kInt64: return DT_I64;
    case torch::kFloat32: return DT_F32;
    case torch::kFloat64: return DT_F64;
    case torch::kBool: return DT_BOOL;
    case torch::kUInt32: return DT_U32;
    case torch::kUInt64: return DT_U64;
    default:
      TORCH_CHECK(false, "unsupported column dtype ", t.scalar_type());
  }
}

KeyCols make_key_cols(const std::vector<torch::Tensor>& cols) {
  TORCH_CHECK(!cols.empty() && (int)cols.size() <= MAX_KEY_COLS,
              "1..", MAX_KEY_COLS, " key columns supported");
  KeyCols k;
  k.n = (int)cols.size();
  for (size_t i = 0; i < cols.size(); ++i) {
    TORCH_CHECK(cols[i].is_cuda() && cols[i].is_contiguous(),
                "key columns must be contiguous device tensors");
    k.cols[i] = {cols[i].data_ptr(), dtype_code(cols[i])};
  }
  return k;
}

hipStream_t current_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

// Blocks of a grid-stride launch over n rows, `threads` rows per block.
int grid_blocks(int64_t n, int threads = THREADS) {
  return (int)std::min<int64_t>((n + threads - 1) / threads, 32768);
}

// Launch a kernel templated on the number of key columns at the
// instantiation for nk columns: 2, 3 and 4 have their own, the rest take
// the generic one, <0>.
#define LAUNCH_NK(kernel, nk, blocks, threads, ...)                       \
  do {                                                                    \
    switch (nk) {                                                         \
      case 2:                                                             \
        hipLaunchKernelGGL(kernel<2>, dim3(blocks), dim3(threads), 0,     \
                           current_stream(), __VA_ARGS__);                \
        break;                                                            \
      case 3:                                                             \
        hipLaunchKernelGGL(kernel<3>, dim3(blocks), dim3(threads), 0,     \
                           current_stream(), __VA_ARGS__);                \
        break;                                                            \
      case 4:                                                             \
        hipLaunchKernelGGL(kernel<4>, dim3(blocks), dim3(threads), 0,     \
                           current_stream(), __VA_ARGS__);                \
        break;                                                            \
      default:                                                            \
        hipLaunchKernelGGL(kernel<0>, dim3(blocks), dim3(threads), 0,     \
                           current_stream(), __VA_ARGS__);                \
    }                                                                     \
    HIP_CHECK(hipGetLastError());                                         \
  } while (0)

// lo..hi contiguous int64 device columns of one length on one device,
// `what` in the message; returns the length.
int64_t int64_cols(const std::vector<torch::Tensor>& cols, int lo, int hi,
                   const char* what) {
  TORCH_CHECK((int)cols.size() >= lo && (int)cols.size() <= hi, what, ": ",
              lo, "..", hi, " columns supported");
  const int64_t n = cols[0].size(0);
  for (const auto& c : cols)
    TORCH_CHECK(c.is_cuda() && c.is_contiguous() &&
                    c.scalar_type() == torch::kInt64 && c.dim() == 1 &&
                    c.size(0) == n && c.device() == cols[0].device(),
                what, " must be contiguous int64 device tensors of one "
                "length");
  return n;
}

constexpr int32_t MAX_LDS_PARTS = 4096;

// Rows per block for the partition kernels: target ~4096 workgroups so
// the grid comfortably fills 256 CUs across 8 XCDs, with a floor that
// keeps per-block LDS histogram work worthwhile.
int64_t rows_per_block(int64_t n) {
  int64_t rpb = (n + 4095) / 4096;
  if (rpb < 1024) rpb = 1024;
  return rpb;
}

// ---------------------------------------------------------------- hash

torch::Tensor hash_columns(std::vector<torch::Tensor> cols, int64_t seed) {
  KeyCols k = make_key_cols(cols);
  int64_t n = cols[0].size(0);
  auto out = torch::empty({n}, cols[0].options().dtype(torch::kUInt32));
  if (n == 0) return out;
  int blocks = (int)std::min<int64_t>((n + THREADS - 1) / THREADS, 65535);
  hipLaunchKernelGGL(k_hash_rows, dim3(blocks), dim3(THREADS), 0,
                     current_stream(), k, n, (uint32_t)seed,
                     out.data_ptr<uint32_t>());
  HIP_CHECK(hipGetLastError());
  return out;
}

// ----------------------------------------------------------- partition

std::tuple<std::vector<torch::Tensor>, torch::Tensor> partition_common(
    const std::vector<torch::Tensor>& cols, torch::Tensor pids,
    torch::Tensor block_hist, int64_t n, int64_t nparts, int64_t nblocks,
    int64_t rpb) {
  // Destination offsets: one small kernel computes per-block reserved
  // ranges + partition totals (stays on device).
  auto opts64 = cols[0].options().dtype(torch::kInt64);
  auto block_off = torch::empty({nblocks * nparts}, opts64);
  auto part_counts = torch::empty({nparts}, opts64);
  // 1024 threads = 16 waves; the kernel assigns one wave per partition
  hipLaunchKernelGGL(k_part_offsets, dim3(1), dim3(1024), 0,
                     current_stream(), block_hist.data_ptr<uint32_t>(),
                     nblocks, (int32_t)nparts,
                     block_off.data_ptr<int64_t>(),
                     part_counts.data_ptr<int64_t>());
  HIP_CHECK(hipGetLastError());

  ScatterCols sc;
  sc.n = (int)cols.size();
  TORCH_CHECK(sc.n <= MAX_COLS, "at most ", MAX_COLS, " columns");
  std::vector<torch::Tensor> dst;
  for (int c = 0; c < sc.n; ++c) {
    TORCH_CHECK(cols[c].is_cuda() && cols[c].is_contiguous(),
                "columns must be contiguous device tensors");
    dst.push_back(torch::empty_like(cols[c]));
    sc.src[c] = {cols[c].data_ptr(), dtype_code(cols[c])};
    sc.dst[c] = {dst[c].data_ptr(), dtype_code(cols[c])};
  }
  size_t lds = (size_t)nparts * sizeof(uint32_t);
  hipLaunchKernelGGL(k_part_scatter, dim3((uint32_t)nblocks), dim3(THREADS),
                     lds, current_stream(), sc,
                     pids.data_ptr<int32_t>(), n, (int32_t)nparts,
                     rpb, block_off.data_ptr<int64_t>());
  HIP_CHECK(hipGetLastError());
  return {dst, part_counts.cpu()};
}

std::tuple<std::vector<torch::Tensor>, torch::Tensor> hash_partition(
    std::vector<torch::Tensor> cols, std::vector<torch::Tensor> key_cols,
    int64_t nparts, int64_t seed) {
  TORCH_CHECK(nparts >= 1 && nparts <= MAX_LDS_PARTS,
              "nparts must be in [1, ", MAX_LDS_PARTS, "]");
  KeyCols k = make_key_cols(key_cols);
  int64_t n = cols.at(0).size(0);
  int64_t rpb = rows_per_block(n);
  int64_t nblocks = (n + rpb - 1) / rpb;
  auto pids = torch::empty({n}, cols[0].options().dtype(torch::kInt32));
  auto block_hist = torch::empty({nblocks * nparts},
                                 cols[0].options().dtype(torch::kUInt32));
  size_t lds = (size_t)nparts * sizeof(uint32_t);
  hipLaunchKernelGGL(k_part_hist, dim3((uint32_t)nblocks), dim3(THREADS),
                     lds, current_stream(), k, n, (int32_t)nparts,
                     (uint32_t)seed, rpb,
                     pids.data_ptr<int32_t>(),
                     block_hist.data_ptr<uint32_t>());
  HIP_CHECK(hipGetLastError());
  return partition_common(cols, pids, block_hist, n, nparts, nblocks, rpb);
}

std::tuple<std::vector<torch::Tensor>, torch::Tensor> scatter_by_partition(
    std::vector<torch::Tensor> cols, torch::Tensor pids, int64_t nparts) {
  TORCH_CHECK(nparts >= 1 && nparts <= MAX_LDS_PARTS);
  TORCH_CHECK(pids.scalar_type() == torch::kInt32 && pids.is_cuda());
  pids = pids.contiguous();
  int64_t n = cols.at(0).size(0);
  int64_t rpb = rows_per_block(n);
  int64_t nblocks = (n + rpb - 1) / rpb;
  auto block_hist = torch::empty({nblocks * nparts},
                                 cols[0].options().dtype(torch::kUInt32));
  size_t lds = (size_t)nparts * sizeof(uint32_t);
  hipLaunchKernelGGL(k_pids_hist, dim3((uint32_t)nblocks), dim3(THREADS),
                     lds, current_stream(), pids.data_ptr<int32_t>(), n,
                     (int32_t)nparts, rpb,
                     block_hist.data_ptr<uint32_t>());
  HIP_CHECK(hipGetLastError());
  return partition_common(cols, pids, block_hist, n, nparts, nblocks, rpb);
}

// ------------------------------------------------------------- groupby

torch::Tensor agg_identity(torch::Tensor like, int32_t agg, int64_t size) {
  auto opt = like.options();
  switch (agg) {
    case AGG_SUM: return torch::zeros({size}, opt);
    case AGG_PROD: return torch::ones({size}, opt);
    case AGG_MIN:
      if (like.is_floating_point())
        return torch::full({size}, std::numeric_limits<double>::infinity(),
                           opt);
      return torch::full({size},
                         like.scalar_type() == torch::kInt64
                             ? std::numeric_limits<int64_t>::max()
                             : (int64_t)std::numeric_limits<int32_t>::max(),
                         opt);
    default:  // AGG_MAX
      if (like.is_floating_point())
        return torch::full({size}, -std::numeric_limits<double>::infinity(),
                           opt);
      return torch::full({size},
                         like.scalar_type() == torch::kInt64
                             ? std::numeric_limits<int64_t>::min()
                             : (int64_t)std::numeric_limits<int32_t>::min(),
                         opt);
  }
}

ValCols make_val_cols(const std::vector<torch::Tensor>& vals,
                      const std::vector<torch::Tensor>& tabs,
                      const std::vector<int64_t>& aggs) {
  ValCols vc;
  vc.n = (int)vals.size();
  TORCH_CHECK(vals.size() == tabs.size() && vals.size() == aggs.size());
  TORCH_CHECK((int)vals.size() <= MAX_COLS);
  for (size_t c = 0; c < vals.size(); ++c) {
    TORCH_CHECK(vals[c].is_cuda() && vals[c].is_contiguous());
    TORCH_CHECK(tabs[c].scalar_type() == vals[c].scalar_type());
    vc.src[c] = {vals[c].data_ptr(), dtype_code(vals[c])};
    vc.tab[c] = {tabs[c].data_ptr(), dtype_code(tabs[c])};
    vc.agg[c] = (int32_t)aggs[c];
  }
  return vc;
}

// Hash seed of every combiner table (the reference combiner's
// hashSeed): not the partitioner's, so a previous partitioning step
// does not strip hash entropy.
constexpr uint32_t GB_HASH_SEED = 0x9acb0442u;

// A caller-owned table: tkeys holds cap+1 slots filled with the
// sentinel (cap a power of two; slot cap takes the sentinel key itself),
// every tab cap+1 slots at its agg identity, flags is int32[2] =
// {sentinel_seen, overflow}.  Returns cap.
int64_t table_cap(const torch::Tensor& tkeys,
                  at::ArrayRef<torch::Tensor> tabs,
                  const torch::Tensor& flags) {
  const int64_t cap = tkeys.size(0) - 1;
  TORCH_CHECK(cap > 0 && (cap & (cap - 1)) == 0, "capacity must be 2^k");
  TORCH_CHECK(tkeys.is_cuda() && tkeys.is_contiguous() &&
              tkeys.scalar_type() == torch::kInt64);
  for (const auto& tab : tabs)
    TORCH_CHECK(tab.is_cuda() && tab.is_contiguous() &&
                tab.size(0) == cap + 1);
  TORCH_CHECK(flags.is_cuda() && flags.is_contiguous() &&
              flags.scalar_type() == torch::kInt32 && flags.numel() >= 2);
  return cap;
}

// Bucket id of the partitioned insert = slot >> shift: the high bits of
// the table slot, for nbuckets buckets over cap slots.
uint32_t bucket_shift(int64_t cap, int64_t nbuckets) {
  TORCH_CHECK(cap > 0 && (cap & (cap - 1)) == 0 && cap <= (int64_t(1) << 31),
              "capacity must be 2^k");
  TORCH_CHECK(nbuckets >= 2 && nbuckets <= GBP_MAX_BUCKETS &&
                  (nbuckets & (nbuckets - 1)) == 0 && nbuckets <= cap,
              "nbuckets must be a power of two in [2, ", GBP_MAX_BUCKETS,
              "] and at most the capacity");
  uint32_t shift = 0;
  while ((cap >> shift) > nbuckets) ++shift;
  return shift;
}

// Streaming insert into a caller-owned table.  Multiple insert calls
// accumulate into the same table; the host checks flags[1] after
// compaction and regrows on overflow.
void groupby_insert(torch::Tensor keys, std::vector<torch::Tensor> vals,
                    std::vector<int64_t> aggs, torch::Tensor tkeys,
                    std::vector<torch::Tensor> tabs, torch::Tensor flags,
                    int64_t max_probes) {
  TORCH_CHECK(keys.is_cuda() && keys.scalar_type() == torch::kInt64);
  keys = keys.contiguous();
  int64_t n = keys.size(0);
  if (n == 0) return;
  int64_t cap = table_cap(tkeys, tabs, flags);
  ValCols vc = make_val_cols(vals, tabs, aggs);
  int blocks = grid_blocks(n);
  hipLaunchKernelGGL(k_groupby_insert, dim3(blocks), dim3(THREADS), 0,
                     current_stream(), keys.data_ptr<int64_t>(), n, vc,
                     tkeys.data_ptr<int64_t>(), cap, GB_HASH_SEED,
                     flags.data_ptr<int32_t>(),
                     flags.data_ptr<int32_t>() + 1, max_probes);
  HIP_CHECK(hipGetLastError());
}

torch::Tensor slot_pids(torch::Tensor keys, int64_t cap,
                        int64_t nparts) {
  TORCH_CHECK(keys.is_cuda() && keys.scalar_type() == torch::kInt64);
  keys = keys.contiguous();
  int64_t n = keys.size(0);
  auto pids = torch::empty({n}, keys.options().dtype(torch::kInt32));
  int blocks = grid_blocks(n);
  hipLaunchKernelGGL(k_slot_pids, dim3(blocks), dim3(THREADS), 0,
                     current_stream(), keys.data_ptr<int64_t>(), n, cap,
                     (int32_t)nparts, GB_HASH_SEED,
                     pids.data_ptr<int32_t>());
  HIP_CHECK(hipGetLastError());
  return pids;
}

// Two-level LDS insert (single int64 SUM value): see groupby.hip.
void groupby_insert_lds(torch::Tensor keys, torch::Tensor vals,
                        torch::Tensor tkeys, torch::Tensor tab,
                        torch::Tensor flags, int64_t max_probes,
                        int64_t target_blocks) {
  TORCH_CHECK(keys.is_cuda() && keys.scalar_type() == torch::kInt64);
  TORCH_CHECK(vals.scalar_type() == torch::kInt64);
  keys = keys.contiguous();
  vals = vals.contiguous();
  int64_t n = keys.size(0);
  if (n == 0) return;
  int64_t cap = table_cap(tkeys, {tab}, flags);
  // grid-stride geometry (matches the one-level kernel); target_blocks
  // caps the grid so the LDS flush volume stays bounded
  if (target_blocks <= 0) target_blocks = 32768;
  int64_t nblocks = std::min<int64_t>((n + THREADS - 1) / THREADS,
                                      target_blocks);
  hipLaunchKernelGGL(k_groupby_insert_sum_i64_lds, dim3((uint32_t)nblocks),
                     dim3(THREADS), 0, current_stream(),
                     keys.data_ptr<int64_t>(), vals.data_ptr<int64_t>(), n,
                     tkeys.data_ptr<int64_t>(),
                     (long long*)tab.data_ptr<int64_t>(), cap, GB_HASH_SEED,
                     flags.data_ptr<int32_t>(),
                     flags.data_ptr<int32_t>() + 1, max_probes);
  HIP_CHECK(hipGetLastError());
}

// Tiles per group of the partitioned insert (groupby_part.hip): the
// histogram and the scatter run one workgroup per group of G consecutive
// tiles.  G is the smallest value that leaves at most GBP_GROUP_WGS
// workgroups (two per CU of a 256-CU chip, what the scatter's LDS lets be
// resident at once), capped at GBP_MAX_GROUP: 1 up to 2M rows, 4 at 8M.
constexpr int64_t GBP_GROUP_WGS = 512;
constexpr int64_t GBP_MAX_GROUP = 8;

int64_t part_group_tiles(int64_t n) {
  const int64_t ntiles = (n + GBP_SCATTER_ROWS - 1) / GBP_SCATTER_ROWS;
  const int64_t g = (ntiles + GBP_GROUP_WGS - 1) / GBP_GROUP_WGS;
  return std::min(std::max(g, (int64_t)1), GBP_MAX_GROUP);
}

// Partitioned LDS pre-aggregation (single int64 SUM value): see
// groupby_part.hip.  Histogram, offsets and scatter; returns the
// partitioned (key, value) pairs [n, 2] and the rows per bucket.
// group_tiles: G, 0 = part_group_tiles(rows).
std::tuple<torch::Tensor, torch::Tensor> part_scatter_impl(
    const torch::Tensor& keys, const torch::Tensor& vals, int64_t cap,
    int64_t nbuckets, int64_t group_tiles) {
  int64_t n = keys.size(0);
  TORCH_CHECK(n > 0 && n < (int64_t(1) << 31), "1 <= rows < 2^31");
  TORCH_CHECK(group_tiles >= 0 && group_tiles <= 65536,
              "0 <= group_tiles <= 65536");
  const uint32_t shift = bucket_shift(cap, nbuckets);
  const uint32_t seed = GB_HASH_SEED;
  const uint32_t mask = (uint32_t)(cap - 1);
  const uint32_t nb = (uint32_t)nbuckets;
  const int64_t ntiles = (n + GBP_SCATTER_ROWS - 1) / GBP_SCATTER_ROWS;
  const int64_t G = group_tiles ? group_tiles : part_group_tiles(n);
  const int64_t ngroups = (ntiles + G - 1) / G;
  auto opts32 = keys.options().dtype(torch::kInt32);
  auto gsum = torch::empty({ngroups * nbuckets}, opts32);
  auto totals = torch::empty({nbuckets}, opts32);
  auto pairs = torch::empty({n, 2}, keys.options());
  auto stream = current_stream();
  hipLaunchKernelGGL(k_gbp_hist, dim3((uint32_t)ngroups), dim3(GBP_THREADS),
                     0, stream, keys.data_ptr<int64_t>(), n, ntiles,
                     (uint32_t)G, nb, seed, mask, shift,
                     (uint32_t*)gsum.data_ptr<int32_t>());
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_gbp_offsets, dim3((nb + 63) / 64),
                     dim3(GBP_OFF_THREADS), 0, stream,
                     (uint32_t*)gsum.data_ptr<int32_t>(), ngroups, nb,
                     (uint32_t*)totals.data_ptr<int32_t>());
  HIP_CHECK(hipGetLastError());
  const int64_t per_xcd = (ngroups + 7) / 8;
  hipLaunchKernelGGL(k_gbp_scatter, dim3((uint32_t)(8 * per_xcd)),
                     dim3(GBP_THREADS), 0, stream,
                     keys.data_ptr<int64_t>(), vals.data_ptr<int64_t>(), n,
                     ntiles, (uint32_t)G, ngroups, nb, seed, mask, shift,
                     (const uint32_t*)gsum.data_ptr<int32_t>(),
                     (const uint32_t*)totals.data_ptr<int32_t>(),
                     (GbPair*)pairs.data_ptr<int64_t>());
  HIP_CHECK(hipGetLastError());
  return {pairs, totals};
}

// Tiled aggregate with its global flush over already partitioned pairs.
void launch_gbp_aggregate(const torch::Tensor& pairs,
                          const torch::Tensor& tkeys,
                          const torch::Tensor& tab,
                          const torch::Tensor& flags, int64_t cap,
                          int64_t max_probes) {
  const int64_t n = pairs.size(0);
  const int64_t ntiles = (n + GBP_TILE_ROWS - 1) / GBP_TILE_ROWS;
  hipLaunchKernelGGL(k_gbp_aggregate, dim3((uint32_t)ntiles),
                     dim3(GBP_THREADS), 0, current_stream(),
                     (const GbPair*)pairs.data_ptr<int64_t>(), n,
                     tkeys.data_ptr<int64_t>(),
                     (long long*)tab.data_ptr<int64_t>(), cap, GB_HASH_SEED,
                     flags.data_ptr<int32_t>(),
                     flags.data_ptr<int32_t>() + 1, max_probes);
  HIP_CHECK(hipGetLastError());
}

// Owner pass + cleanup pass over already partitioned pairs (see "Owned
// slices" in groupby_part.hip).  pairs is reordered in place (spilled
// rows move to the front of the region their owner consumed).  Returns
// clean[b]: rows at the front of segment b left to the cleanup pass.
torch::Tensor part_owned_impl(const torch::Tensor& pairs,
                              const torch::Tensor& totals,
                              const torch::Tensor& tkeys,
                              const torch::Tensor& tab,
                              const torch::Tensor& flags,
                              int64_t max_probes) {
  const int64_t n = pairs.size(0);
  const int64_t cap = table_cap(tkeys, {tab}, flags);
  const int64_t nbuckets = totals.size(0);
  TORCH_CHECK(n > 0 && n < (int64_t(1) << 31), "1 <= rows < 2^31");
  const uint32_t shift = bucket_shift(cap, nbuckets);
  const int64_t S = cap / nbuckets;
  TORCH_CHECK(S <= GBP_LDS_SLOTS, "owned pass needs capacity / nbuckets <= ",
              GBP_LDS_SLOTS);
  TORCH_CHECK((uintptr_t)tkeys.data_ptr() % 16 == 0 &&
                  (uintptr_t)tab.data_ptr() % 16 == 0,
              "table must be 16-byte aligned");
  const uint32_t nb = (uint32_t)nbuckets;
  const uint32_t seed = GB_HASH_SEED;
  auto clean = torch::empty({nbuckets}, totals.options());
  auto todo = torch::empty({nbuckets, 2}, totals.options());
  auto stream = current_stream();
  // the static counters put a 4096-slot slice just over the 64 KiB a
  // kernel gets without asking
  // (the attribute is per device and cheap to set: no once-flag)
  HIP_CHECK(hipFuncSetAttribute(
      (const void*)k_gbp_owned, hipFuncAttributeMaxDynamicSharedMemorySize,
      16 * GBP_LDS_SLOTS));
  hipLaunchKernelGGL(k_gbp_owned, dim3(nb), dim3(GBP_THREADS),
                     (size_t)(16 * S), stream,
                     (GbPair*)pairs.data_ptr<int64_t>(), n,
                     (const uint32_t*)totals.data_ptr<int32_t>(), nb,
                     (uint32_t)S, tkeys.data_ptr<int64_t>(),
                     (long long*)tab.data_ptr<int64_t>(), seed, max_probes,
                     (uint32_t*)clean.data_ptr<int32_t>(),
                     (uint2*)todo.data_ptr<int32_t>());
  HIP_CHECK(hipGetLastError());
  const int64_t ntiles = (n + GBP_TILE_ROWS - 1) / GBP_TILE_ROWS;
  hipLaunchKernelGGL(k_gbp_cleanup, dim3((uint32_t)ntiles),
                     dim3(GBP_THREADS), 0, stream,
                     (const GbPair*)pairs.data_ptr<int64_t>(), n,
                     tkeys.data_ptr<int64_t>(),
                     (long long*)tab.data_ptr<int64_t>(), cap, seed,
                     flags.data_ptr<int32_t>(),
                     flags.data_ptr<int32_t>() + 1, max_probes,
                     (const uint2*)todo.data_ptr<int32_t>(), nb, shift);
  HIP_CHECK(hipGetLastError());
  return clean;
}

// owned != 0: bucket-owning aggregate (needs capacity / nbuckets <=
// GBP_LDS_SLOTS); owned == 0: the tiled aggregate with its global flush.
// group_tiles: scatter tiles per workgroup, 0 = part_group_tiles(rows).
void groupby_insert_part(torch::Tensor keys, torch::Tensor vals,
                         torch::Tensor tkeys, torch::Tensor tab,
                         torch::Tensor flags, int64_t max_probes,
                         int64_t nbuckets, int64_t owned,
                         int64_t group_tiles) {
  TORCH_CHECK(keys.is_cuda() && keys.scalar_type() == torch::kInt64);
  TORCH_CHECK(vals.scalar_type() == torch::kInt64 &&
              vals.size(0) == keys.size(0));
  TORCH_CHECK(tab.scalar_type() == torch::kInt64);
  keys = keys.contiguous();
  vals = vals.contiguous();
  if (keys.size(0) == 0) return;
  int64_t cap = table_cap(tkeys, {tab}, flags);
  auto parts = part_scatter_impl(keys, vals, cap, nbuckets, group_tiles);
  const torch::Tensor& pairs = std::get<0>(parts);
  if (owned)
    part_owned_impl(pairs, std::get<1>(parts), tkeys, tab, flags,
                    max_probes);
  else
    launch_gbp_aggregate(pairs, tkeys, tab, flags, cap, max_probes);
}

// The scatter alone (tests, kernel timing): (pairs [n, 2], rows per
// bucket [nbuckets]).
std::tuple<torch::Tensor, torch::Tensor> groupby_part_scatter(
    torch::Tensor keys, torch::Tensor vals, int64_t cap,
    int64_t nbuckets, int64_t group_tiles) {
  TORCH_CHECK(keys.is_cuda() && keys.scalar_type() == torch::kInt64);
  TORCH_CHECK(vals.scalar_type() == torch::kInt64 &&
              vals.size(0) == keys.size(0));
  return part_scatter_impl(keys.contiguous(), vals.contiguous(), cap,
                           nbuckets, group_tiles);
}

// Aggregate pass alone over already partitioned pairs (kernel timing).
void groupby_part_aggregate(torch::Tensor pairs, torch::Tensor tkeys,
                            torch::Tensor tab, torch::Tensor flags,
                            int64_t max_probes) {
  TORCH_CHECK(pairs.is_cuda() && pairs.scalar_type() == torch::kInt64 &&
              pairs.is_contiguous() && pairs.dim() == 2 &&
              pairs.size(1) == 2);
  if (pairs.size(0) == 0) return;
  TORCH_CHECK(tab.scalar_type() == torch::kInt64);
  launch_gbp_aggregate(pairs, tkeys, tab, flags,
                       table_cap(tkeys, {tab}, flags), max_probes);
}

// Owner + cleanup passes alone over already partitioned pairs and their
// rows per bucket (tests, kernel timing).  Reorders pairs in place;
// returns clean [nbuckets].
torch::Tensor groupby_part_owned(torch::Tensor pairs, torch::Tensor totals,
                                 torch::Tensor tkeys, torch::Tensor tab,
                                 torch::Tensor flags, int64_t max_probes) {
  TORCH_CHECK(pairs.is_cuda() && pairs.scalar_type() == torch::kInt64 &&
              pairs.is_contiguous() && pairs.dim() == 2 &&
              pairs.size(1) == 2);
  TORCH_CHECK(totals.is_cuda() && totals.scalar_type() == torch::kInt32 &&
              totals.is_contiguous() && totals.dim() == 1);
  TORCH_CHECK(tab.scalar_type() == torch::kInt64);
  return part_owned_impl(pairs, totals, tkeys, tab, flags, max_probes);
}

// Compact used slots into freshly-allocated output arrays; returns
// [out_keys(cap), out_vals...(cap)]; cursor (u64[1], zeroed by caller)
// receives the used-slot count — the caller narrows after reading it.
std::vector<torch::Tensor> groupby_compact(torch::Tensor tkeys,
                                           std::vector<torch::Tensor> tabs,
                                           torch::Tensor cursor) {
  int64_t cap = tkeys.size(0) - 1;
  CompactCols cc;
  cc.n = (int)tabs.size();
  std::vector<torch::Tensor> out;
  auto out_keys = torch::empty({cap}, tkeys.options());
  out.push_back(out_keys);
  for (size_t c = 0; c < tabs.size(); ++c) {
    out.push_back(torch::empty({cap}, tabs[c].options()));
    cc.tab[c] = {tabs[c].data_ptr(), dtype_code(tabs[c])};
    cc.out[c] = {out[c + 1].data_ptr(), dtype_code(tabs[c])};
  }
  // ~2048 blocks: fills the chip while keeping cursor atomics rare.
  int64_t spb = (cap + 2047) / 2048;
  if (spb < THREADS) spb = THREADS;
  int blocks = (int)((cap + spb - 1) / spb);
  hipLaunchKernelGGL(k_groupby_compact, dim3(blocks), dim3(THREADS), 0,
                     current_stream(), tkeys.data_ptr<int64_t>(), cap, spb,
                     cc, out_keys.data_ptr<int64_t>(),
                     (unsigned long long*)cursor.data_ptr());
  HIP_CHECK(hipGetLastError());
  return out;
}

// Workgroups of the fused finish (groupby_finish.hip) and the slots each
// owns.  The histogram matrix has blocks x nparts counters, written once
// and read twice, so wide fans take fewer blocks (at most 2^18 counters,
// 1 MiB); a block owns at least 2048 slots and an even number of them.
std::pair<int64_t, int64_t> gbf_blocks(int64_t cap, int64_t nparts) {
  int64_t blocks = std::min<int64_t>(
      GBF_THREADS, std::max<int64_t>(64, (int64_t(1) << 18) / nparts));
  blocks = std::min(blocks, (cap + 1 + 2047) / 2048);
  int64_t spb = (cap + 1 + blocks - 1) / blocks;
  spb += spb & 1;
  return {(cap + 1 + spb - 1) / spb, spb};
}

// Compact the used slots of a table straight into nparts hash partitions
// (hash_row over the key, seed 0, % nparts).  Returns ([out_keys,
// out_vals...], host): every output has cap + 1 rows of which the first
// sum(counts) are set, partition after partition; host is one int64 host
// tensor {counts[nparts], sentinel_seen, overflow} — the one readback.
std::tuple<std::vector<torch::Tensor>, torch::Tensor>
groupby_compact_partition(torch::Tensor tkeys,
                          std::vector<torch::Tensor> tabs,
                          torch::Tensor flags, int64_t nparts) {
  TORCH_CHECK(nparts >= 1 && nparts <= MAX_LDS_PARTS &&
                  nparts <= GBF_MAX_PARTS,
              "nparts must be in [1, ", MAX_LDS_PARTS, "]");
  const int64_t cap = table_cap(tkeys, tabs, flags);
  TORCH_CHECK(cap <= (int64_t(1) << 31), "capacity above 2^31");
  FinishCols fc;
  fc.n = (int)tabs.size();
  TORCH_CHECK(fc.n <= MAX_COLS, "at most ", MAX_COLS, " value columns");
  std::vector<torch::Tensor> out;
  out.push_back(torch::empty({cap + 1}, tkeys.options()));
  for (int c = 0; c < fc.n; ++c) {
    const auto st = tabs[c].scalar_type();
    TORCH_CHECK(st == torch::kInt64 || st == torch::kInt32 ||
                    st == torch::kFloat32 || st == torch::kFloat64,
                "unsupported value dtype ", st);
    out.push_back(torch::empty({cap + 1}, tabs[c].options()));
    fc.tab[c] = {tabs[c].data_ptr(), dtype_code(tabs[c])};
    fc.out[c] = {out[c + 1].data_ptr(), dtype_code(tabs[c])};
  }
  const auto [blocks, spb] = gbf_blocks(cap, nparts);
  auto opts32 = tkeys.options().dtype(torch::kInt32);
  auto hist = torch::empty({nparts * blocks}, opts32);
  auto totals = torch::empty({nparts}, opts32);
  auto dev = torch::empty({nparts + 2}, tkeys.options());
  auto stream = current_stream();
  const uint32_t np = (uint32_t)nparts;
  const int32_t* fl = flags.data_ptr<int32_t>();
  hipLaunchKernelGGL(k_gbf_count, dim3((uint32_t)blocks), dim3(GBF_THREADS),
                     0, stream, tkeys.data_ptr<int64_t>(), cap, spb, np, fl,
                     (uint32_t*)hist.data_ptr<int32_t>());
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_gbf_offsets, dim3(np), dim3(GBF_THREADS), 0, stream,
                     (uint32_t*)hist.data_ptr<int32_t>(), (uint32_t)blocks,
                     np, fl, (uint32_t*)totals.data_ptr<int32_t>(),
                     dev.data_ptr<int64_t>());
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_gbf_write, dim3((uint32_t)blocks), dim3(GBF_THREADS),
                     0, stream, tkeys.data_ptr<int64_t>(), cap, spb, np, fl,
                     (const uint32_t*)hist.data_ptr<int32_t>(),
                     (const uint32_t*)totals.data_ptr<int32_t>(), fc,
                     out[0].data_ptr<int64_t>());
  HIP_CHECK(hipGetLastError());
  return {out, dev.cpu()};
}

// Exact count of distinct keys in keys[:rows], minus one, as a device
// int64 scalar (groupby.hip, "Cardinality sample"): an init and a count
// launch, no host sync.
torch::Tensor groupby_sample_distinct(torch::Tensor keys, int64_t rows) {
  TORCH_CHECK(keys.is_cuda() && keys.scalar_type() == torch::kInt64 &&
              keys.dim() == 1 && keys.stride(0) == 1);
  TORCH_CHECK(rows >= 1 && rows <= keys.size(0) &&
                  rows <= (int64_t(1) << 30),
              "1 <= rows <= min(len(keys), 2^30)");
  int64_t m = 2;
  while (m < 2 * rows) m <<= 1;
  auto tags = torch::empty({m}, keys.options());
  auto state = torch::empty({2}, keys.options());
  auto result = state.select(0, 0);
  auto stream = current_stream();
  hipLaunchKernelGGL(k_gbs_init, dim3(grid_blocks(m / 2)), dim3(THREADS), 0,
                     stream, tags.data_ptr<int64_t>(), m,
                     state.data_ptr<int64_t>());
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_gbs_count, dim3(grid_blocks((rows + 1) / 2)),
                     dim3(THREADS), 0, stream, keys.data_ptr<int64_t>(),
                     rows, tags.data_ptr<int64_t>(), m,
                     state.data_ptr<int64_t>());
  HIP_CHECK(hipGetLastError());
  return result;
}

// ------------------------------------------- multi-column group-by (K21)

uint64_t gbm_fp_mask(int64_t fp_bits) {
  TORCH_CHECK(fp_bits >= 1 && fp_bits <= 64, "fp_bits must be in [1, 64]");
  return fp_bits == 64 ? ~uint64_t(0) : (uint64_t(1) << fp_bits) - 1;
}

// The batch side of MkCols: 2..MAX_KEY_COLS contiguous int64 device
// columns of one length, which is returned.
int64_t gbm_batch_keys(MkCols& kc, const std::vector<torch::Tensor>& keys) {
  const int64_t n = int64_cols(keys, 2, MAX_KEY_COLS, "key columns");
  kc.n = (int)keys.size();
  for (size_t c = 0; c < keys.size(); ++c) {
    kc.src[c] = keys[c].data_ptr<int64_t>();
    kc.tab[c] = nullptr;
  }
  return n;
}

// The table side: tags int64[cap+1], one int64[cap+1] array per key
// column, flags int32[3] = {unused, overflow, collision}.  Returns cap.
int64_t gbm_table(MkCols& kc, const torch::Tensor& tags,
                  const std::vector<torch::Tensor>& kcols,
                  at::ArrayRef<torch::Tensor> tabs,
                  const torch::Tensor& flags) {
  const int64_t cap = table_cap(tags, tabs, flags);
  // a row's slot travels between the launches as a uint32, all-ones
  // meaning "none"
  TORCH_CHECK(cap <= (int64_t(1) << 31), "capacity above 2^31");
  TORCH_CHECK(flags.numel() >= 3, "flags must be int32[3]");
  TORCH_CHECK((int)kcols.size() == kc.n, "one key array per key column");
  for (size_t c = 0; c < kcols.size(); ++c) {
    TORCH_CHECK(kcols[c].is_cuda() && kcols[c].is_contiguous() &&
                kcols[c].scalar_type() == torch::kInt64 &&
                kcols[c].dim() == 1 && kcols[c].size(0) == cap + 1);
    kc.tab[c] = kcols[c].data_ptr<int64_t>();
  }
  return cap;
}

// The device tag of every row (tests compare it with the torch mirror,
// kernels/groupby_multi.fingerprint64).
torch::Tensor groupby_mk_fingerprint(std::vector<torch::Tensor> keys,
                                     int64_t fp_bits) {
  MkCols kc{};
  const int64_t n = gbm_batch_keys(kc, keys);
  const uint64_t fp_mask = gbm_fp_mask(fp_bits);
  auto out = torch::empty({n}, keys[0].options());
  if (n == 0) return out;
  LAUNCH_NK(k_gbm_fingerprint, kc.n, grid_blocks(n), THREADS, kc, n,
            GB_HASH_SEED, fp_mask, out.data_ptr<int64_t>());
  return out;
}

// Launch 1: claim slots by tag; returns each row's slot (uint32 bits in
// an int32 tensor, -1 = none: the probe chain overflowed).
torch::Tensor groupby_mk_claim(std::vector<torch::Tensor> keys,
                               torch::Tensor tags,
                               std::vector<torch::Tensor> kcols,
                               torch::Tensor flags, int64_t max_probes,
                               int64_t fp_bits) {
  MkCols kc{};
  const int64_t n = gbm_batch_keys(kc, keys);
  const int64_t cap = gbm_table(kc, tags, kcols, {}, flags);
  const uint64_t fp_mask = gbm_fp_mask(fp_bits);
  TORCH_CHECK(max_probes >= 1);
  auto slots = torch::empty({n}, keys[0].options().dtype(torch::kInt32));
  if (n == 0) return slots;
  LAUNCH_NK(k_gbm_claim, kc.n, grid_blocks(n), THREADS, kc, n,
            tags.data_ptr<int64_t>(), cap, GB_HASH_SEED, fp_mask,
            (uint32_t*)slots.data_ptr<int32_t>(),
            flags.data_ptr<int32_t>() + 1, max_probes);
  return slots;
}

// Launch 2: compare the stored tuple and accumulate.  slots must come
// from groupby_mk_claim on the same table and batch.
void groupby_mk_accum(std::vector<torch::Tensor> keys,
                      std::vector<torch::Tensor> vals,
                      std::vector<int64_t> aggs, torch::Tensor slots,
                      torch::Tensor tags, std::vector<torch::Tensor> kcols,
                      std::vector<torch::Tensor> tabs,
                      torch::Tensor flags) {
  MkCols kc{};
  const int64_t n = gbm_batch_keys(kc, keys);
  const int64_t cap = gbm_table(kc, tags, kcols, tabs, flags);
  TORCH_CHECK(keys.size() + vals.size() <= (size_t)MAX_COLS,
              "at most ", MAX_COLS, " key and value columns");
  TORCH_CHECK(slots.is_cuda() && slots.is_contiguous() &&
              slots.scalar_type() == torch::kInt32 && slots.dim() == 1 &&
              slots.size(0) == n);
  ValCols vc = make_val_cols(vals, tabs, aggs);
  for (const auto& v : vals)
    TORCH_CHECK(v.dim() == 1 && v.size(0) == n,
                "value columns must have one entry per row");
  if (n == 0) return;
  LAUNCH_NK(k_gbm_accum, kc.n, grid_blocks(n), THREADS, kc, n, vc,
            (const uint32_t*)slots.data_ptr<int32_t>(), cap,
            flags.data_ptr<int32_t>() + 2);
}

// Streaming insert of one batch: both launches on the current stream.
// Nothing is read back; the host reads flags after compaction.
void groupby_mk_insert(std::vector<torch::Tensor> keys,
                       std::vector<torch::Tensor> vals,
                       std::vector<int64_t> aggs, torch::Tensor tags,
                       std::vector<torch::Tensor> kcols,
                       std::vector<torch::Tensor> tabs, torch::Tensor flags,
                       int64_t max_probes, int64_t fp_bits) {
  auto slots = groupby_mk_claim(keys, tags, kcols, flags, max_probes,
                                fp_bits);
  groupby_mk_accum(keys, vals, aggs, slots, tags, kcols, tabs, flags);
}

// ---------------------------------------------------------------- sort


// ---------------------------------------------------------------------
// Hand-written LSD radix sort orchestration (kernels in radix.hip):
// one fused histogram prepass (all digit positions in one read), then
// one decoupled-lookback scatter kernel per non-constant digit.
// Set BIGSLICE_SORT_ROCPRIM=1 to force the rocPRIM path (A/B harness).

// Re-read each call so one process can A/B implementations.
static bool force_rocprim_sort() {
  const char* e = getenv("BIGSLICE_SORT_ROCPRIM");
  return e && e[0] == '1';
}

// Geometry A/B harness: BIGSLICE_RADIX_VARIANT=2 selects the monolithic
// shape (see hand_radix_sort).  Re-read each call so one process can A/B
// the shapes back-to-back.
static int radix_variant() {
  const char* e = getenv("BIGSLICE_RADIX_VARIANT");
  return e ? atoi(e) : 0;
}

template <typename K, int HAS_VAL, int TILE, int BLOCK, int SPLIT>
static void hand_radix_passes(const torch::Tensor& keys,
                              const torch::Tensor& vals,
                              torch::Tensor& keys_out,
                              torch::Tensor& vals_out,
                              const std::vector<int>& passes,
                              int npass, uint64_t bias,
                              hipStream_t stream) {
  const int64_t n = keys.size(0);
  const int P = (int)passes.size();
  const int64_t ntiles = (n + TILE - 1) / TILE;
  auto state = torch::empty({ntiles * RDX_RADIX},
                            keys.options().dtype(torch::kInt64));
  // hist ping-pong + digit_base, all device-resident: after the first
  // pass's histogram, each scatter tallies the NEXT pass's histogram
  // itself, so no further prepass and no host syncs between passes.
  auto i64 = keys.options().dtype(torch::kInt64);
  auto hist_a = torch::zeros({RDX_RADIX}, i64);
  auto hist_b = torch::zeros({RDX_RADIX}, i64);
  auto dbase = torch::empty({RDX_RADIX}, i64);
  {
    const int64_t nb = std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL((k_radix_hist_one<K>), dim3((int)nb), dim3(256),
                       0, stream, (const K*)keys.data_ptr(), n,
                       passes[0] * 8,
                       (unsigned long long*)hist_a.data_ptr<int64_t>());
    HIP_CHECK(hipGetLastError());
  }
  torch::Tensor keys_tmp, vals_tmp;
  if (P > 1) {
    keys_tmp = torch::empty_like(keys);
    if (HAS_VAL) vals_tmp = torch::empty_like(vals);
  }
  const K* src_k = (const K*)keys.data_ptr();
  const int64_t* src_v =
      HAS_VAL ? (const int64_t*)vals.data_ptr() : nullptr;
  torch::Tensor hist_cur = hist_a, hist_next = hist_b;
  for (int i = 0; i < P; ++i) {
    const bool to_out = ((P - i) % 2) == 1;
    K* dst_k = (K*)(to_out ? keys_out : keys_tmp).data_ptr();
    int64_t* dst_v =
        HAS_VAL ? (int64_t*)(to_out ? vals_out : vals_tmp).data_ptr()
                : nullptr;
    const int xm = (passes[i] == npass - 1) ? 0x80 : 0;
    hipLaunchKernelGGL(
        k_radix_scan_hist, dim3(1), dim3(RDX_RADIX), 0, stream,
        (const unsigned long long*)hist_cur.data_ptr<int64_t>(),
        (unsigned long long*)dbase.data_ptr<int64_t>(), xm);
    HIP_CHECK(hipGetLastError());
    const int next_shift = (i + 1 < P) ? passes[i + 1] * 8 : -1;
    if (next_shift >= 0)
      HIP_CHECK(hipMemsetAsync(hist_next.data_ptr(), 0,
                               RDX_RADIX * 8, stream));
    HIP_CHECK(hipMemsetAsync(state.data_ptr(), 0,
                             (size_t)ntiles * RDX_RADIX * 8, stream));
    hipLaunchKernelGGL(
        (k_radix_scatter<K, HAS_VAL, TILE, BLOCK, SPLIT>),
        dim3((int)ntiles), dim3(BLOCK), 0, stream, src_k, dst_k, src_v,
        dst_v, n, passes[i] * 8, bias,
        (const unsigned long long*)dbase.data_ptr<int64_t>(),
        (unsigned long long*)state.data_ptr<int64_t>(), next_shift,
        (unsigned long long*)hist_next.data_ptr<int64_t>());
    HIP_CHECK(hipGetLastError());
    src_k = dst_k;
    src_v = dst_v;
    std::swap(hist_cur, hist_next);
  }
}

// pass-skip probe: byte position p is constant across all keys iff the
// bitwise AND and OR of the keys agree on that byte — one
// pure-bandwidth reduction replaces a full histogram prepass AND the
// old aminmax end_bit probe.
template <typename K>
static std::vector<int> probe_passes(const torch::Tensor& keys) {
  const int64_t n = keys.size(0);
  auto stream = current_stream();
  const int npass = (int)keys.element_size();
  auto i64 = keys.options().dtype(torch::kInt64);
  auto andor = torch::empty({2}, i64);
  andor[0] = -1;  // all ones
  andor[1] = 0;
  // 512 grid-strided blocks saturate HBM with the 8-deep load burst
  // while keeping the same-address atomic tail at ~1 op/block
  const int64_t nb = std::min<int64_t>((n + 2047) / 2048, 512);
  hipLaunchKernelGGL(
      (k_radix_andor<K>), dim3((int)nb), dim3(256), 0, stream,
      (const K*)keys.data_ptr(), n,
      (unsigned long long*)andor.data_ptr<int64_t>(),
      (unsigned long long*)(andor.data_ptr<int64_t>() + 1));
  HIP_CHECK(hipGetLastError());
  auto andor_h = andor.cpu();  // the one host sync
  const uint64_t band = (uint64_t)andor_h[0].item<int64_t>();
  const uint64_t bor = (uint64_t)andor_h[1].item<int64_t>();
  std::vector<int> passes;
  for (int p = 0; p < npass; ++p) {
    if (((band >> (p * 8)) & 0xFF) != ((bor >> (p * 8)) & 0xFF))
      passes.push_back(p);  // constant digit: pass skipped
  }
  return passes;
}

template <typename K, int HAS_VAL>
static void hand_radix_sort(const torch::Tensor& keys,
                            const torch::Tensor& vals,
                            torch::Tensor& keys_out,
                            torch::Tensor& vals_out,
                            const std::vector<int>& passes) {
  auto stream = current_stream();
  const int width = (int)keys.element_size() * 8;
  const int npass = width / 8;
  const uint64_t bias = 1ull << (width - 1);
  if (radix_variant() == 2)
    // monolithic: 8K tiles, both columns staged, one 1024-thread
    // workgroup per CU (the shape of profiles/sort_variants*.txt)
    hand_radix_passes<K, HAS_VAL, 8192, 1024, 0>(
        keys, vals, keys_out, vals_out, passes, npass, bias, stream);
  else
    // default: split reorder, 8K tiles, two workgroups per CU
    hand_radix_passes<K, HAS_VAL, 8192, 512, 1>(
        keys, vals, keys_out, vals_out, passes, npass, bias, stream);
}

// Production dispatch: the AND/OR probe picks the executed byte set.
// A CONTIGUOUS set runs on the in-tree rocPRIM onesweep with the bit
// range trimmed at both ends (measured fastest on uniform keys); a set
// with interior constant bytes runs on the hand-written scatter, which
// skips arbitrary bytes.  BIGSLICE_SORT_HAND=1 forces the hand path,
// BIGSLICE_SORT_ROCPRIM=1 forces full-control rocPRIM (A/B harness).
static bool force_hand_sort() {
  const char* e = getenv("BIGSLICE_SORT_HAND");
  return e && e[0] == '1';
}

static bool probed_sortable(const torch::Tensor& keys) {
  return keys.scalar_type() == torch::kInt64 ||
         keys.scalar_type() == torch::kInt32;
}

static bool use_hand_path(const std::vector<int>& passes) {
  if (force_rocprim_sort()) return false;
  if (force_hand_sort()) return true;
  const bool contiguous =
      (int)passes.size() == passes.back() - passes.front() + 1;
  return !contiguous;
}

// The probe and the engine choice, for all three sorts.  Returns true
// when the result is already in keys_out (and vals_out): every byte was
// constant and the input went through as it is, or the hand path ran.
// Otherwise narrows [begin_bit, end_bit) for rocPRIM.
template <int HAS_VAL>
static bool sort_probed(const torch::Tensor& keys, const torch::Tensor& vals,
                        torch::Tensor& keys_out, torch::Tensor& vals_out,
                        int& begin_bit, int& end_bit) {
  if (keys.size(0) == 0 || !probed_sortable(keys)) return false;
  const bool i64 = keys.scalar_type() == torch::kInt64;
  std::vector<int> passes =
      i64 ? probe_passes<int64_t>(keys) : probe_passes<int32_t>(keys);
  if (passes.empty()) {
    keys_out.copy_(keys);
    if (HAS_VAL) vals_out.copy_(vals);
    return true;
  }
  if (use_hand_path(passes)) {
    if (i64)
      hand_radix_sort<int64_t, HAS_VAL>(keys, vals, keys_out, vals_out,
                                        passes);
    else
      hand_radix_sort<int32_t, HAS_VAL>(keys, vals, keys_out, vals_out,
                                        passes);
    return true;
  }
  begin_bit = passes.front() * 8;
  end_bit = (passes.back() + 1) * 8;
  return false;
}

// rocPRIM's two-call protocol: call(nullptr, bytes) reports the
// temporary storage it needs, the second call runs in it.
template <typename F>
static void with_rocprim_temp(const torch::Tensor& like, F call) {
  size_t temp_bytes = 0;
  call((void*)nullptr, temp_bytes);
  auto temp = torch::empty({(int64_t)temp_bytes},
                           like.options().dtype(torch::kUInt8));
  call(temp.data_ptr(), temp_bytes);
}

torch::Tensor radix_sort_keys(torch::Tensor keys, bool probe) {
  TORCH_CHECK(keys.is_cuda() && keys.is_contiguous());
  int64_t n = keys.size(0);
  auto keys_out = torch::empty_like(keys);
  int begin_bit = 0, end_bit = (int)keys.element_size() * 8;
  torch::Tensor nil;
  // probe=false: full-width rocPRIM with no byte-constancy probe (the
  // probe's host readback is a stream sync — callers that must stay
  // async, like the cardinality sample, opt out)
  if (probe && sort_probed<0>(keys, nil, keys_out, nil, begin_bit, end_bit))
    return keys_out;
  auto run = [&](auto fn) {
    with_rocprim_temp(keys, [&](void* temp, size_t& temp_bytes) {
      fn(keys.data_ptr(), keys_out.data_ptr(), n, begin_bit, end_bit, temp,
         temp_bytes, current_stream());
    });
  };
  switch (keys.scalar_type()) {
    case torch::kInt64: run(radix_sort_keys_int64_t); break;
    case torch::kInt32: run(radix_sort_keys_int32_t); break;
    case torch::kFloat32: run(radix_sort_keys_float); break;
    case torch::kFloat64: run(radix_sort_keys_double); break;
    default:
      TORCH_CHECK(false, "radix_sort_keys: unsupported dtype");
  }
  return keys_out;
}

// Stable sort of (key, 8-byte value) pairs into fresh tensors; the
// value column does not participate in ordering.
static std::vector<torch::Tensor> sort_pairs(const torch::Tensor& keys,
                                             const torch::Tensor& vals,
                                             const char* unsupported) {
  int64_t n = keys.size(0);
  auto keys_out = torch::empty_like(keys);
  auto vals_out = torch::empty_like(vals);
  int begin_bit = 0, end_bit = (int)keys.element_size() * 8;
  if (sort_probed<1>(keys, vals, keys_out, vals_out, begin_bit, end_bit))
    return {keys_out, vals_out};
  auto run = [&](auto fn) {
    with_rocprim_temp(keys, [&](void* temp, size_t& temp_bytes) {
      fn(keys.data_ptr(), keys_out.data_ptr(),
         (const int64_t*)vals.data_ptr(), (int64_t*)vals_out.data_ptr(), n,
         begin_bit, end_bit, temp, temp_bytes, current_stream());
    });
  };
  switch (keys.scalar_type()) {
    case torch::kInt64: run(radix_sort_pairs_int64_t); break;
    case torch::kInt32: run(radix_sort_pairs_int32_t); break;
    case torch::kFloat32: run(radix_sort_pairs_float); break;
    case torch::kFloat64: run(radix_sort_pairs_double); break;
    default:
      TORCH_CHECK(false, unsupported);
  }
  return {keys_out, vals_out};
}

// Direct (key, value) sort for 2-column frames: no permutation, no
// gather passes.  The value column is bit-cast to int64.
std::vector<torch::Tensor> radix_sort_kv(torch::Tensor keys,
                                         torch::Tensor vals) {
  TORCH_CHECK(keys.is_cuda() && keys.is_contiguous());
  TORCH_CHECK(vals.is_cuda() && vals.is_contiguous());
  TORCH_CHECK(vals.element_size() == 8, "8-byte values only");
  return sort_pairs(keys, vals, "radix_sort_kv: unsupported key dtype");
}

// The sorting permutation: the row ids, sorted as the value column.
torch::Tensor radix_argsort(torch::Tensor keys) {
  TORCH_CHECK(keys.is_cuda() && keys.is_contiguous());
  auto perm_in = torch::arange(keys.size(0),
                               keys.options().dtype(torch::kInt64));
  return sort_pairs(keys, perm_in, "radix_argsort: unsupported dtype")[1];
}

// K16: (unique_keys, aggregates, count) over key-sorted pairs via
// rocPRIM reduce-by-key: deterministic segmented reduction (fixed tree
// order — float sums are run-to-run reproducible, unlike atomics).
// count comes back as a 1-element device tensor; the caller slices
// after one sync.  code: 0=sum 1=min 2=max.
std::vector<torch::Tensor> segment_reduce_sorted(torch::Tensor keys,
                                                 torch::Tensor vals,
                                                 int64_t code) {
  TORCH_CHECK(keys.is_cuda() && keys.is_contiguous());
  TORCH_CHECK(vals.is_cuda() && vals.is_contiguous());
  TORCH_CHECK(keys.scalar_type() == torch::kInt64,
              "segment_reduce_sorted: int64 keys only");
  int64_t n = keys.size(0);
  auto uniq = torch::empty_like(keys);
  auto aggs = torch::empty_like(vals);
  auto count = torch::zeros({1}, keys.options());
  if (n == 0) return {uniq, aggs, count};
  auto run = [&](auto fn) {
    with_rocprim_temp(keys, [&](void* temp, size_t& temp_bytes) {
      fn(keys.data_ptr<int64_t>(), vals.data_ptr(), n,
         uniq.data_ptr<int64_t>(), aggs.data_ptr(),
         count.data_ptr<int64_t>(), (int)code, temp, temp_bytes,
         current_stream());
    });
  };
  switch (vals.scalar_type()) {
    case torch::kInt64: run(reduce_by_key_int64_t); break;
    case torch::kInt32: run(reduce_by_key_int32_t); break;
    case torch::kFloat32: run(reduce_by_key_float); break;
    case torch::kFloat64: run(reduce_by_key_double); break;
    default:
      TORCH_CHECK(false, "segment_reduce_sorted: unsupported val dtype");
  }
  return {uniq, aggs, count};
}

// K16 fast path (runs.hip): int64 segmented reduction over sorted
// values with precomputed run boundaries.  The caller computes runs
// once via runs_sorted and reuses them for every value column (the
// rocPRIM reduce_by_key path redoes the key scan per column).
torch::Tensor segment_reduce_runs(torch::Tensor vals,
                                  torch::Tensor starts, int64_t n,
                                  int64_t code) {
  TORCH_CHECK(vals.is_cuda() && vals.is_contiguous() &&
              vals.scalar_type() == torch::kInt64,
              "segment_reduce_runs: contiguous int64 values required");
  TORCH_CHECK(starts.is_cuda() && starts.is_contiguous());
  TORCH_CHECK(code >= 0 && code <= 2,
              "segment_reduce_runs: sum/min/max only");
  const int64_t m = starts.size(0);
  auto out = torch::empty({m}, vals.options());
  if (m == 0) return out;
  const int64_t nb = std::min<int64_t>((m + 255) / 256, 4096);
  hipLaunchKernelGGL(k_segreduce_i64, dim3((int)nb), dim3(256), 0,
                     current_stream(), vals.data_ptr<int64_t>(),
                     starts.data_ptr<int64_t>(), m, n, (int)code,
                     out.data_ptr<int64_t>());
  HIP_CHECK(hipGetLastError());
  return out;
}

// (count, max_run_length) of a runs_sorted result in ONE device
// tensor, so the host guard pays a single readback.
torch::Tensor runs_guard(torch::Tensor starts, torch::Tensor cnt,
                         int64_t n) {
  TORCH_CHECK(starts.is_cuda() && starts.is_contiguous() &&
              cnt.is_cuda());
  auto out = torch::zeros({2}, starts.options());
  out.index_put_({0}, cnt[0]);
  hipLaunchKernelGGL(k_runs_guard, dim3(512), dim3(256), 0,
                     current_stream(),
                     starts.data_ptr<int64_t>(),
                     cnt.data_ptr<int64_t>(), n,
                     (unsigned long long*)(out.data_ptr<int64_t>() + 1));
  HIP_CHECK(hipGetLastError());
  return out;
}

// K18: (unique_keys, run_starts, count) of a SORTED key array in one
// pass (runs.hip: ballot compaction + single-channel lookback;
// measured 5.4x the rocPRIM reduce-by-key fallback kept behind
// BIGSLICE_RUNS_ROCPRIM=1).  count is a 1-element device tensor; the
// caller slices after one sync.
std::vector<torch::Tensor> runs_sorted(torch::Tensor keys) {
  TORCH_CHECK(keys.is_cuda() && keys.is_contiguous() &&
              keys.scalar_type() == torch::kInt64,
              "runs_sorted: contiguous int64 device keys required");
  const int64_t n = keys.size(0);
  auto uniq = torch::empty_like(keys);
  auto starts = torch::empty_like(keys);
  auto count = torch::zeros({1}, keys.options());
  if (n == 0) return {uniq, starts, count};
  const char* rp = getenv("BIGSLICE_RUNS_ROCPRIM");
  if (rp && rp[0] == '1') {
    with_rocprim_temp(keys, [&](void* temp, size_t& temp_bytes) {
      runs_sorted_i64(keys.data_ptr<int64_t>(), n,
                      uniq.data_ptr<int64_t>(), starts.data_ptr<int64_t>(),
                      count.data_ptr<int64_t>(), temp, temp_bytes,
                      current_stream());
    });
    return {uniq, starts, count};
  }
  auto stream = current_stream();
  // 64K-row tiles amortize per-block fixed costs on large inputs;
  // 8K-row tiles keep small inputs on >=2 blocks/CU
  const int ipt = (n >= (16 << 20)) ? 256 : 32;
  const int64_t tile = (int64_t)RUNS_BLOCK * ipt;
  const int64_t ntiles = (n + tile - 1) / tile;
  auto state = torch::empty({ntiles},
                            keys.options().dtype(torch::kInt64));
  HIP_CHECK(hipMemsetAsync(state.data_ptr(), 0, (size_t)ntiles * 8,
                           stream));
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3((int)ntiles), dim3(RUNS_BLOCK), 0,
                       stream, keys.data_ptr<int64_t>(), n,
                       uniq.data_ptr<int64_t>(),
                       starts.data_ptr<int64_t>(),
                       count.data_ptr<int64_t>(),
                       (unsigned long long*)state.data_ptr<int64_t>());
  };
  if (ipt == 256)
    launch(k_runs_sorted<256>);
  else
    launch(k_runs_sorted<32>);
  HIP_CHECK(hipGetLastError());
  return {uniq, starts, count};
}

// ------------------------------ multi-column sorted-key primitives (K22)

// (distinct tuples per column, run starts, count) of lexicographically
// SORTED key columns: count, scan and write on the current stream
// (runs_multi.hip).  The outputs hold n entries; count is a 1-element
// device tensor and the caller slices after one readback.
std::tuple<std::vector<torch::Tensor>, torch::Tensor, torch::Tensor>
runs_multi(std::vector<torch::Tensor> cols) {
  const int64_t n =
      int64_cols(cols, 1, MAX_KEY_COLS, "runs_multi: key columns");
  MrCols kc{};
  kc.n = (int)cols.size();
  std::vector<torch::Tensor> uniq;
  for (int c = 0; c < kc.n; ++c) {
    uniq.push_back(torch::empty_like(cols[c]));
    kc.src[c] = cols[c].data_ptr<int64_t>();
    kc.uniq[c] = uniq[c].data_ptr<int64_t>();
  }
  auto starts = torch::empty_like(cols[0]);
  if (n == 0) return {uniq, starts, torch::zeros({1}, cols[0].options())};
  const int64_t ntiles = (n + MRUNS_TILE - 1) / MRUNS_TILE;
  TORCH_CHECK(ntiles < (1ll << 31), "runs_multi: batch too large");
  auto counts = torch::empty({ntiles}, cols[0].options());
  LAUNCH_NK(k_mruns_count, kc.n, (uint32_t)ntiles, MRUNS_BLOCK, kc, n,
            counts.data_ptr<int64_t>());
  // 1-D on purpose: a 2-D cumsum over dim 0 takes torch's strided
  // outer-dim scan (see tokenize_bytes)
  auto incl = at::cumsum(counts, 0);
  LAUNCH_NK(k_mruns_write, kc.n, (uint32_t)ntiles, MRUNS_BLOCK, kc, n,
            (const int64_t*)incl.data_ptr<int64_t>(), n,
            starts.data_ptr<int64_t>());
  return {uniq, starts, incl.slice(0, ntiles - 1, ntiles)};
}

// Lower (right = false) or upper bound of every query tuple among
// lexicographically SORTED tuples, torch.searchsorted's meaning.
// Nothing is read back.
torch::Tensor lex_searchsorted(std::vector<torch::Tensor> sorted_cols,
                               std::vector<torch::Tensor> query_cols,
                               bool right) {
  const int64_t u = int64_cols(sorted_cols, 1, MAX_KEY_COLS,
                               "lex_searchsorted: key columns");
  const int64_t m = int64_cols(query_cols, 1, MAX_KEY_COLS,
                               "lex_searchsorted: key columns");
  TORCH_CHECK(sorted_cols.size() == query_cols.size() &&
                  sorted_cols[0].device() == query_cols[0].device(),
              "lex_searchsorted: sorted and query tuples must have the "
              "same columns on one device");
  LexCols kc{};
  kc.n = (int)sorted_cols.size();
  for (int c = 0; c < kc.n; ++c) {
    kc.sorted[c] = sorted_cols[c].data_ptr<int64_t>();
    kc.query[c] = query_cols[c].data_ptr<int64_t>();
  }
  auto out = torch::empty({m}, query_cols[0].options());
  if (m == 0) return out;
  LAUNCH_NK(k_lex_search, kc.n, grid_blocks(m, 256), 256, kc, u, m,
            (int)right, out.data_ptr<int64_t>());
  return out;
}

// K17: murmur3 over variable-length byte rows (device strings).
torch::Tensor hash_bytes(torch::Tensor bytes, torch::Tensor offsets,
                         int64_t seed) {
  TORCH_CHECK(bytes.is_cuda() && bytes.is_contiguous() &&
              bytes.scalar_type() == torch::kUInt8);
  TORCH_CHECK(offsets.is_cuda() && offsets.is_contiguous() &&
              offsets.scalar_type() == torch::kInt64);
  int64_t n = offsets.size(0) - 1;
  auto out = torch::empty({n}, bytes.options().dtype(torch::kUInt32));
  if (n == 0) return out;
  int blocks = grid_blocks(n);
  hipLaunchKernelGGL(k_hash_bytes, dim3(blocks), dim3(THREADS), 0,
                     current_stream(), bytes.data_ptr<uint8_t>(),
                     offsets.data_ptr<int64_t>(), n, (uint32_t)seed,
                     out.data_ptr<uint32_t>());
  HIP_CHECK(hipGetLastError());
  return out;
}

torch::Tensor hash_bytes64(torch::Tensor bytes, torch::Tensor offsets,
                           int64_t seed_hi, int64_t seed_lo) {
  TORCH_CHECK(bytes.is_cuda() && bytes.is_contiguous() &&
              bytes.scalar_type() == torch::kUInt8);
  TORCH_CHECK(offsets.is_cuda() && offsets.is_contiguous() &&
              offsets.scalar_type() == torch::kInt64);
  int64_t n = offsets.size(0) - 1;
  auto out = torch::empty({n}, bytes.options().dtype(torch::kInt64));
  if (n == 0) return out;
  int blocks = grid_blocks(n);
  hipLaunchKernelGGL(k_hash_bytes64, dim3(blocks), dim3(THREADS), 0,
                     current_stream(), bytes.data_ptr<uint8_t>(),
                     offsets.data_ptr<int64_t>(), n, (uint32_t)seed_hi,
                     (uint32_t)seed_lo, out.data_ptr<int64_t>());
  HIP_CHECK(hipGetLastError());
  return out;
}

// Vector-aggregate experiment (see vecagg.hip): colsum of [N,16] f32.
torch::Tensor colsum16(torch::Tensor x, bool mfma) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() &&
              x.scalar_type() == torch::kFloat32 && x.dim() == 2 &&
              x.size(1) == 16);
  int64_t n = x.size(0);
  auto out = torch::zeros({16}, x.options());
  int blocks = (int)std::min<int64_t>((n + THREADS - 1) / THREADS, 8192);
  if (mfma)
    hipLaunchKernelGGL(k_colsum_mfma, dim3(blocks), dim3(THREADS), 0,
                       current_stream(), x.data_ptr<float>(), n,
                       out.data_ptr<float>());
  else
    hipLaunchKernelGGL(k_colsum_valu, dim3(blocks), dim3(THREADS), 0,
                       current_stream(), x.data_ptr<float>(), n,
                       out.data_ptr<float>());
  HIP_CHECK(hipGetLastError());
  return out;
}

// K13: one launch of the expression interpreter (expr.hip) over a
// batch.  code is the [n_instr, 2] int64 host image of the program
// (packed fields, immediate); it is validated here, field by field,
// before it reaches the device: every register, input slot and dtype
// the kernel will index with is in range.  Returns the output columns
// (n rows each) and, with a predicate, the survivor count as a
// 1-element device tensor; the caller narrows after one readback.
std::vector<torch::Tensor> expr_apply(
    torch::Tensor code, int64_t n_pred, int64_t pred_reg,
    std::vector<torch::Tensor> in_cols, std::vector<int64_t> out_regs,
    std::vector<int64_t> out_dts) {
  static const torch::ScalarType kDt[XD_N] = {
      torch::kBool, torch::kInt32, torch::kInt64, torch::kFloat32,
      torch::kFloat64};
  TORCH_CHECK(!code.is_cuda() && code.scalar_type() == torch::kInt64 &&
                  code.is_contiguous() && code.dim() == 2 &&
                  code.size(1) == 2,
              "expr_apply: code must be a [n, 2] int64 host tensor");
  const int64_t n_total = code.size(0);
  const int n_in = (int)in_cols.size(), n_out = (int)out_regs.size();
  const bool has_pred = pred_reg >= 0;
  TORCH_CHECK(n_total <= EXPR_MAX_INSTRS && n_pred >= 0 &&
                  n_pred <= n_total && n_in >= 1 &&
                  n_in <= EXPR_MAX_IN && n_out >= 1 &&
                  n_out <= EXPR_MAX_OUT && out_dts.size() == out_regs.size() &&
                  pred_reg < EXPR_MAX_REGS && (has_pred || n_pred == 0),
              "expr_apply: program over the kernel's limits");
  ExprProgram P;
  memset(&P, 0, sizeof(P));
  int nregs = (int)pred_reg + 1;  // registers the program names
  const int64_t n = in_cols[0].size(0);
  for (int k = 0; k < n_in; ++k) {
    const auto& c = in_cols[k];
    TORCH_CHECK(c.is_cuda() && c.is_contiguous() && c.dim() == 1 &&
                    c.size(0) == n &&
                    c.device() == in_cols[0].device(),
                "expr_apply: inputs must be contiguous 1-D device "
                "columns of one length");
    int dt = -1;
    for (int d = 0; d < XD_N; ++d)
      if (c.scalar_type() == kDt[d]) dt = d;
    TORCH_CHECK(dt >= 0, "expr_apply: unsupported input dtype ",
                c.scalar_type());
    P.in_ptr[k] = c.data_ptr();
    P.in_dt[k] = (uint8_t)dt;
  }
  const int64_t* w = code.data_ptr<int64_t>();
  P.pred_begin = 0;
  P.out_begin = (int32_t)n_pred;
  for (int64_t i = 0; i < n_total; ++i) {
    const uint64_t x = (uint64_t)w[2 * i];
    const int op = x & 0xff, dt = (x >> 8) & 0xff, dst = (x >> 16) & 0xff,
              a = (x >> 24) & 0xff, b = (x >> 32) & 0xff,
              c = (x >> 40) & 0xff;
    TORCH_CHECK(op < XO_N && dt < XD_N && dst < EXPR_MAX_REGS &&
                    b < EXPR_MAX_REGS && c < EXPR_MAX_REGS &&
                    (x >> 49) == 0,
                "expr_apply: malformed instruction ", i);
    if (op == XO_LOAD) {
      // a section's LOADs lead it; the kernel runs them from ld_reg
      const int sec = i < n_pred ? 0 : 1;
      int32_t& begin = sec ? P.out_begin : P.pred_begin;
      TORCH_CHECK(a < n_in && P.in_dt[a] == dt && begin == i,
                  "expr_apply: LOAD of a missing or mistyped input, or "
                  "not at the head of its section");
      begin = (int32_t)i + 1;
      (sec ? P.mask_out : P.mask_pred) |= 1u << a;
      P.ld_reg[sec][a] = (uint8_t)dst;
    } else {
      TORCH_CHECK(a < EXPR_MAX_REGS && (op != XO_CAST || c < XD_N),
                  "expr_apply: malformed instruction ", i);
    }
    nregs = std::max(nregs, dst + 1);
    P.ins[i].w = x;
    P.ins[i].imm = (uint64_t)w[2 * i + 1];
  }
  P.n_pred = (int32_t)n_pred;
  P.n_total = (int32_t)n_total;
  P.n_in = n_in;
  P.n_out = n_out;
  P.pred_reg = (int32_t)pred_reg;
  std::vector<torch::Tensor> outs;
  for (int o = 0; o < n_out; ++o) {
    TORCH_CHECK(out_regs[o] >= 0 && out_regs[o] < EXPR_MAX_REGS &&
                    out_dts[o] >= 0 && out_dts[o] < XD_N,
                "expr_apply: malformed output ", o);
    outs.push_back(torch::empty(
        {n}, in_cols[0].options().dtype(kDt[out_dts[o]])));
    P.out_ptr[o] = outs.back().data_ptr();
    P.out_dt[o] = (uint8_t)out_dts[o];
    P.out_reg[o] = (uint8_t)out_regs[o];
    nregs = std::max(nregs, (int)out_regs[o] + 1);
  }
  auto count = torch::zeros({1}, in_cols[0].options().dtype(torch::kInt64));
  if (has_pred) outs.push_back(count);
  if (n == 0) return outs;
  constexpr int64_t tile = (int64_t)EXPR_BLOCK * EXPR_IPT;
  const int64_t ntiles = (n + tile - 1) / tile;
  TORCH_CHECK(ntiles < (1ll << 31), "expr_apply: batch too large");
  auto stream = current_stream();
  // J slabs per decode, the most the 16-slot register file allows; a
  // register never written is never read for a result that matters,
  // but it is still indexed: count every register field
  for (int64_t i = 0; i < n_total; ++i) {
    const uint64_t x = P.ins[i].w;
    const int op = x & 0xff;
    if (op == XO_LOAD || op == XO_CONST) continue;
    nregs = std::max(nregs, (int)((x >> 24) & 0xff) + 1);
    nregs = std::max(nregs, (int)((x >> 32) & 0xff) + 1);
    if (op == XO_WHERE)
      nregs = std::max(nregs, (int)((x >> 40) & 0xff) + 1);
  }
  TORCH_CHECK(nregs >= 1 && nregs <= EXPR_MAX_REGS);
  const int J = nregs <= 4 ? 4 : (nregs <= 8 ? 2 : 1);
  const size_t lds = (size_t)nregs * J * sizeof(ExprRegs);
  int64_t* count_ptr = nullptr;
  unsigned long long* state_ptr = nullptr;
  torch::Tensor state;
  if (has_pred) {
    // per-tile lookback words, zeroed on the launch stream every time
    state = torch::empty({ntiles},
                         in_cols[0].options().dtype(torch::kInt64));
    HIP_CHECK(hipMemsetAsync(state.data_ptr(), 0, (size_t)ntiles * 8,
                             stream));
    count_ptr = count.data_ptr<int64_t>();
    state_ptr = (unsigned long long*)state.data_ptr<int64_t>();
  }
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3((int)ntiles), dim3(EXPR_BLOCK), lds,
                       stream, P, n, count_ptr, state_ptr);
  };
  if (has_pred) {
    if (J == 4) launch(k_expr<true, 4>);
    else if (J == 2) launch(k_expr<true, 2>);
    else launch(k_expr<true, 1>);
  } else {
    if (J == 4) launch(k_expr<false, 4>);
    else if (J == 2) launch(k_expr<false, 2>);
    else launch(k_expr<false, 1>);
  }
  HIP_CHECK(hipGetLastError());
  return outs;
}

// K20: split the rows of a compacted BYTES column into tokens
// (tokenize.hip).  data must be zero-based and contiguous under offsets
// (offsets[0] == 0, offsets[n] == data.size(0)); mask4 is the 256-bit
// delimiter set.  Returns (out_data, out_offsets[, tok_row]), sized
// exactly after ONE readback of the two totals.
std::vector<torch::Tensor> tokenize_bytes(torch::Tensor data,
                                          torch::Tensor offsets,
                                          std::vector<uint64_t> mask4,
                                          bool with_rows) {
  TORCH_CHECK(data.is_cuda() && data.is_contiguous() && data.dim() == 1 &&
              data.scalar_type() == torch::kUInt8,
              "tokenize_bytes: contiguous uint8 device data required");
  TORCH_CHECK(offsets.is_cuda() && offsets.is_contiguous() &&
              offsets.dim() == 1 && offsets.size(0) >= 1 &&
              offsets.scalar_type() == torch::kInt64,
              "tokenize_bytes: contiguous int64 device offsets required");
  TORCH_CHECK(mask4.size() == 4, "tokenize_bytes: mask4 has 4 words");
  const int64_t total = data.size(0);
  const int64_t n = offsets.size(0) - 1;
  TORCH_CHECK(total < (1ll << 31),
              "tokenize_bytes: total bytes must be below 2^31");
  TORCH_CHECK(n > 0 || total == 0, "tokenize_bytes: bytes without rows");
  auto i64 = offsets.options();
  if (total == 0) {
    std::vector<torch::Tensor> out = {torch::empty({0}, data.options()),
                                      torch::zeros({1}, i64)};
    if (with_rows) out.push_back(torch::empty({0}, i64));
    return out;
  }
  // the kernels read the text with 16-byte loads
  if (((uintptr_t)data.data_ptr<uint8_t>() & 15) != 0) data = data.clone();
  const TokMask m{mask4[0], mask4[1], mask4[2], mask4[3]};
  auto stream = current_stream();
  const int64_t ntiles = (total + TOK_TILE - 1) / TOK_TILE;
  auto counts = torch::empty({ntiles, 2}, i64.dtype(torch::kInt32));
  hipLaunchKernelGGL(k_tok_count, dim3((int)ntiles), dim3(TOK_BLOCK), 0,
                     stream, data.data_ptr<uint8_t>(), total,
                     offsets.data_ptr<int64_t>(), n, m,
                     (unsigned int*)counts.data_ptr<int32_t>());
  HIP_CHECK(hipGetLastError());
  // Scan both counters at once: a tile's uint32 pair is one int64
  // (kept in the low word), and neither sum reaches 2^31, so the low
  // word never carries into the high one.  (A [tiles, 2] cumsum over
  // dim 0 takes torch's strided outer-dim scan: measured 569 us for
  // 4096 tiles, against 83 us for the two kernels.)
  auto incl = at::cumsum(counts.view(torch::kInt64).flatten(), 0);
  // the one host readback
  const uint64_t totals = (uint64_t)incl[ntiles - 1].item<int64_t>();
  const int64_t nkept = (int64_t)(totals & 0xFFFFFFFFull);
  const int64_t ntok = (int64_t)(totals >> 32);
  auto out_data = torch::empty({nkept}, data.options());
  auto out_offsets = torch::empty({ntok + 1}, i64);
  torch::Tensor tok_row;
  if (with_rows) tok_row = torch::empty({ntok}, i64);
  hipLaunchKernelGGL(k_tok_write, dim3((int)ntiles), dim3(TOK_BLOCK), 0,
                     stream, data.data_ptr<uint8_t>(), total,
                     offsets.data_ptr<int64_t>(), n, m,
                     (const unsigned int*)incl.data_ptr<int64_t>(), nkept,
                     ntok,
                     out_data.data_ptr<uint8_t>(),
                     out_offsets.data_ptr<int64_t>(),
                     with_rows ? tok_row.data_ptr<int64_t>() : nullptr);
  HIP_CHECK(hipGetLastError());
  std::vector<torch::Tensor> out = {out_data, out_offsets};
  if (with_rows) out.push_back(tok_row);
  return out;
}

// ------------------------------------------------- id dictionary (K23)

// A caller-owned dictionary table: tags int64[cap+1] filled with the
// sentinel, ref int64[cap+1], cap a power of two below 2^31.  Returns cap.
int64_t idd_table(const torch::Tensor& tags, const torch::Tensor& ref) {
  const int64_t cap = tags.size(0) - 1;
  TORCH_CHECK(cap > 0 && (cap & (cap - 1)) == 0 && cap < (int64_t(1) << 31),
              "capacity must be 2^k below 2^31");
  for (const auto* t : {&tags, &ref})
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() && t->dim() == 1 &&
                    t->scalar_type() == torch::kInt64 &&
                    t->size(0) == cap + 1,
                "tags and ref must be contiguous int64[cap+1] device tensors");
  return cap;
}

// Claim a slot for every id not yet in the table.  lens[i] is the byte
// length of row i; counters is int64[3] = {new rows, new bytes, overflow},
// zeroed by the caller.  Returns newrows int64[n]: its first counters[0]
// entries are the rows whose strings the caller appends, in the order of
// their positions base, base + 1, ...
torch::Tensor iddict_claim(torch::Tensor ids, torch::Tensor lens,
                           torch::Tensor tags, torch::Tensor ref,
                           int64_t base, torch::Tensor counters,
                           int64_t max_probes) {
  const int64_t n = int64_cols({ids}, 1, 1, "ids");
  const int64_t cap = idd_table(tags, ref);
  TORCH_CHECK(lens.is_cuda() && lens.is_contiguous() && lens.dim() == 1 &&
                  lens.scalar_type() == torch::kInt64 && lens.size(0) == n,
              "lens must be a contiguous int64 device tensor, one per id");
  TORCH_CHECK(counters.is_cuda() && counters.is_contiguous() &&
                  counters.scalar_type() == torch::kInt64 &&
                  counters.numel() >= 3,
              "counters must be int64[3]");
  TORCH_CHECK(max_probes >= 1 && base >= 0);
  auto newrows = torch::empty({n}, ids.options());
  if (n == 0) return newrows;
  hipLaunchKernelGGL(k_idd_claim, dim3(grid_blocks(n)), dim3(THREADS), 0,
                     current_stream(), ids.data_ptr<int64_t>(), n,
                     lens.data_ptr<int64_t>(), tags.data_ptr<int64_t>(),
                     ref.data_ptr<int64_t>(), cap, base,
                     newrows.data_ptr<int64_t>(),
                     (unsigned long long*)counters.data_ptr<int64_t>(),
                     max_probes);
  HIP_CHECK(hipGetLastError());
  return newrows;
}

// The position of every id, -1 when absent.
torch::Tensor iddict_lookup(torch::Tensor ids, torch::Tensor tags,
                            torch::Tensor ref, int64_t max_probes) {
  const int64_t n = int64_cols({ids}, 1, 1, "ids");
  const int64_t cap = idd_table(tags, ref);
  TORCH_CHECK(max_probes >= 1);
  auto out = torch::empty({n}, ids.options());
  if (n == 0) return out;
  hipLaunchKernelGGL(k_idd_lookup, dim3(grid_blocks(n)), dim3(THREADS), 0,
                     current_stream(), ids.data_ptr<int64_t>(), n,
                     tags.data_ptr<int64_t>(), ref.data_ptr<int64_t>(), cap,
                     out.data_ptr<int64_t>(), max_probes);
  HIP_CHECK(hipGetLastError());
  return out;
}

// Move every entry of the old table into the new, empty one; overflow
// (int32[1], zeroed by the caller) is raised when a probe chain of the
// new table reaches max_probes.
void iddict_rehash(torch::Tensor old_tags, torch::Tensor old_ref,
                   torch::Tensor new_tags, torch::Tensor new_ref,
                   torch::Tensor overflow, int64_t max_probes) {
  const int64_t old_cap = idd_table(old_tags, old_ref);
  const int64_t new_cap = idd_table(new_tags, new_ref);
  TORCH_CHECK(overflow.is_cuda() && overflow.is_contiguous() &&
                  overflow.scalar_type() == torch::kInt32 &&
                  overflow.numel() >= 1,
              "overflow must be int32[1]");
  TORCH_CHECK(max_probes >= 1);
  hipLaunchKernelGGL(k_idd_rehash, dim3(grid_blocks(old_cap)), dim3(THREADS),
                     0, current_stream(), old_tags.data_ptr<int64_t>(),
                     old_ref.data_ptr<int64_t>(), old_cap,
                     new_tags.data_ptr<int64_t>(),
                     new_ref.data_ptr<int64_t>(), new_cap,
                     overflow.data_ptr<int32_t>(), max_probes);
  HIP_CHECK(hipGetLastError());
}

// ------------------------------------------------ varlen row gather (K23)

// Rows `rows` of the BYTES column (data, offsets) as a new zero-based
// column (out_data, out_offsets).  offsets is absolute into data and may
// be a slice (offsets[0] != 0).  total is the byte count of the result
// when the caller knows it; -1 reads it back (the one host readback).
std::vector<torch::Tensor> bytes_gather(torch::Tensor data,
                                        torch::Tensor offsets,
                                        torch::Tensor rows, int64_t total) {
  TORCH_CHECK(data.is_cuda() && data.is_contiguous() && data.dim() == 1 &&
                  data.scalar_type() == torch::kUInt8,
              "bytes_gather: contiguous uint8 device data required");
  TORCH_CHECK(offsets.is_cuda() && offsets.is_contiguous() &&
                  offsets.dim() == 1 && offsets.size(0) >= 1 &&
                  offsets.scalar_type() == torch::kInt64,
              "bytes_gather: contiguous int64 device offsets required");
  TORCH_CHECK(rows.is_cuda() && rows.dim() == 1 &&
                  rows.scalar_type() == torch::kInt64,
              "bytes_gather: int64 device row indices required");
  rows = rows.contiguous();
  const int64_t n = offsets.size(0) - 1;
  const int64_t m = rows.size(0);
  auto out_offsets = torch::zeros({m + 1}, offsets.options());
  if (m == 0 || total == 0)
    return {torch::empty({0}, data.options()), out_offsets};
  auto stream = current_stream();
  auto lens = torch::empty({m}, offsets.options());
  hipLaunchKernelGGL(k_bg_lens, dim3(grid_blocks(m)), dim3(THREADS), 0,
                     stream, offsets.data_ptr<int64_t>(), n,
                     rows.data_ptr<int64_t>(), m, lens.data_ptr<int64_t>());
  HIP_CHECK(hipGetLastError());
  // 1-D: an outer-dim scan is several times slower (see tokenize_bytes)
  auto incl = out_offsets.narrow(0, 1, m);
  at::cumsum_out(incl, lens, 0);
  if (total < 0) total = out_offsets[m].item<int64_t>();
  if (total == 0) return {torch::empty({0}, data.options()), out_offsets};
  auto out_data = torch::empty({total}, data.options());
  TORCH_CHECK(((uintptr_t)out_data.data_ptr<uint8_t>() & 15) == 0,
              "bytes_gather: output must be 16-byte aligned");
  const int64_t ntiles = (total + BG_TILE - 1) / BG_TILE;
  TORCH_CHECK(ntiles < (int64_t(1) << 31), "bytes_gather: result too large");
  hipLaunchKernelGGL(k_bg_copy, dim3((uint32_t)ntiles), dim3(BG_BLOCK), 0,
                     stream, data.data_ptr<uint8_t>(), data.size(0),
                     offsets.data_ptr<int64_t>(), n,
                     rows.data_ptr<int64_t>(), m,
                     out_offsets.data_ptr<int64_t>(), total,
                     out_data.data_ptr<uint8_t>());
  HIP_CHECK(hipGetLastError());
  return {out_data, out_offsets};
}

// ------------------------------------------- byte-order refinement (K24)

// Round-w keys of rows `rows` of the BYTES column (data, offsets): the
// bytes [7w, 7w+7) big-endian over the count of real ones, top bit
// flipped (bytes_order.hip).  offsets may be a slice; a row index
// outside the column has length 0.  max_blocks > 0 caps the grid (the
// tests take the grid-stride loop with it at small sizes).
torch::Tensor bytes_order_keys(torch::Tensor data, torch::Tensor offsets,
                               torch::Tensor rows, int64_t w,
                               int64_t max_blocks) {
  TORCH_CHECK(data.is_cuda() && data.is_contiguous() && data.dim() == 1 &&
                  data.scalar_type() == torch::kUInt8,
              "bytes_order_keys: contiguous uint8 device data required");
  TORCH_CHECK(offsets.is_cuda() && offsets.is_contiguous() &&
                  offsets.dim() == 1 && offsets.size(0) >= 1 &&
                  offsets.scalar_type() == torch::kInt64,
              "bytes_order_keys: contiguous int64 device offsets required");
  TORCH_CHECK(rows.is_cuda() && rows.dim() == 1 &&
                  rows.scalar_type() == torch::kInt64,
              "bytes_order_keys: int64 device row indices required");
  TORCH_CHECK(w >= 0 && w < (int64_t(1) << 59), "bytes_order_keys: bad round");
  rows = rows.contiguous();
  const int64_t m = rows.size(0);
  auto keys = torch::empty({m}, rows.options());
  if (m == 0) return keys;
  int blocks = grid_blocks(m, BO_BLOCK);
  if (max_blocks > 0 && max_blocks < blocks) blocks = (int)max_blocks;
  hipLaunchKernelGGL(k_bo_keys, dim3(blocks),
                     dim3(BO_BLOCK), 0, current_stream(),
                     data.data_ptr<uint8_t>(), data.size(0),
                     offsets.data_ptr<int64_t>(), offsets.size(0) - 1,
                     rows.data_ptr<int64_t>(), m, w,
                     keys.data_ptr<int64_t>());
  HIP_CHECK(hipGetLastError());
  return keys;
}

// One refinement pass over slots sorted by (grp, key): {head int64[m],
// stay bool[m]}.  head[j] is j where slot j starts a (grp, key) group,
// else 0; stay[j] is set where slot j is tied with a neighbour and its
// key says 7 real bytes.
std::vector<torch::Tensor> bytes_order_refine(torch::Tensor grp,
                                              torch::Tensor key) {
  const int64_t m = int64_cols({grp, key}, 2, 2, "grp and key");
  auto head = torch::empty({m}, grp.options());
  auto stay = torch::empty({m}, grp.options().dtype(torch::kBool));
  if (m == 0) return {head, stay};
  // a thread moves its slots with 16-byte loads and stores
  if (((uintptr_t)grp.data_ptr<int64_t>() & 15) != 0) grp = grp.clone();
  if (((uintptr_t)key.data_ptr<int64_t>() & 15) != 0) key = key.clone();
  TORCH_CHECK((((uintptr_t)grp.data_ptr<int64_t>() |
                (uintptr_t)key.data_ptr<int64_t>() |
                (uintptr_t)head.data_ptr<int64_t>()) & 15) == 0 &&
                  ((uintptr_t)stay.data_ptr<bool>() & 3) == 0,
              "bytes_order_refine: 16-byte aligned tensors required");
  const int64_t ntiles = (m + BO_TILE - 1) / BO_TILE;
  TORCH_CHECK(ntiles < (int64_t(1) << 31), "bytes_order_refine: too large");
  hipLaunchKernelGGL(k_bo_refine, dim3((uint32_t)ntiles), dim3(BO_BLOCK), 0,
                     current_stream(), grp.data_ptr<int64_t>(),
                     key.data_ptr<int64_t>(), m, head.data_ptr<int64_t>(),
                     reinterpret_cast<uint8_t*>(stay.data_ptr<bool>()));
  HIP_CHECK(hipGetLastError());
  return {head, stay};
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("hash_columns", &hash_columns, "murmur3 row hash (K3)");
  m.def("hash_partition", &hash_partition,
        "fused hash+histogram+scatter partitioner (K4)");
  m.def("scatter_by_partition", &scatter_by_partition,
        "scatter rows by precomputed partition ids");
  m.def("groupby_insert", &groupby_insert,
        "hash-aggregate insert pass (K9)");
  m.def("groupby_insert_lds", &groupby_insert_lds,
        "two-level LDS+global insert (int64 sum)");
  m.def("groupby_insert_part", &groupby_insert_part,
        "partitioned LDS pre-aggregating insert (single i64 sum)",
        py::arg("keys"), py::arg("vals"), py::arg("tkeys"), py::arg("tab"),
        py::arg("flags"), py::arg("max_probes"), py::arg("nbuckets"),
        py::arg("owned") = 0, py::arg("group_tiles") = 0);
  m.def("groupby_part_owned", &groupby_part_owned,
        "owner + cleanup passes of the partitioned insert; returns clean");
  m.attr("GBP_OWN_LIMIT") = (int64_t)GBP_OWN_LIMIT;
  m.def("groupby_part_scatter", &groupby_part_scatter,
        "bucket scatter of the partitioned insert", py::arg("keys"),
        py::arg("vals"), py::arg("cap"), py::arg("nbuckets"),
        py::arg("group_tiles") = 0);
  m.def("groupby_part_group_tiles", &part_group_tiles,
        "tiles per group the partitioned insert picks for n rows");
  m.attr("GBP_SCATTER_ROWS") = (int64_t)GBP_SCATTER_ROWS;
  m.def("groupby_part_aggregate", &groupby_part_aggregate,
        "aggregate pass of the partitioned insert");
  m.attr("GBP_TILE_ROWS") = (int64_t)GBP_TILE_ROWS;
  m.attr("GBP_LDS_SLOTS") = (int64_t)GBP_LDS_SLOTS;
  m.attr("GBP_MAX_BUCKETS") = (int64_t)GBP_MAX_BUCKETS;
  m.def("groupby_compact", &groupby_compact,
        "hash-aggregate table compaction (K9)");
  m.def("groupby_compact_partition", &groupby_compact_partition,
        "compact a group-by table straight into hash partitions");
  m.attr("MAX_LDS_PARTS") = (int64_t)MAX_LDS_PARTS;
  m.def("groupby_sample_distinct", &groupby_sample_distinct,
        "distinct keys of a prefix, minus one, as a device scalar");
  m.def("groupby_mk_insert", &groupby_mk_insert,
        "multi-column-key hash-aggregate insert: claim + accumulate (K21)",
        py::arg("keys"), py::arg("vals"), py::arg("aggs"), py::arg("tags"),
        py::arg("kcols"), py::arg("tabs"), py::arg("flags"),
        py::arg("max_probes"), py::arg("fp_bits") = 64);
  m.def("groupby_mk_claim", &groupby_mk_claim,
        "launch 1 of groupby_mk_insert; returns the rows' slots");
  m.def("groupby_mk_accum", &groupby_mk_accum,
        "launch 2 of groupby_mk_insert");
  m.def("groupby_mk_fingerprint", &groupby_mk_fingerprint,
        "the tuple fingerprint groupby_mk_insert claims slots by",
        py::arg("keys"), py::arg("fp_bits") = 64);
  m.attr("MAX_KEY_COLS") = (int64_t)MAX_KEY_COLS;
  m.attr("MAX_COLS") = (int64_t)MAX_COLS;
  m.def("agg_identity", &agg_identity, "aggregation identity fill");
  m.def("radix_argsort", &radix_argsort, "device radix argsort (K6)");
  m.def("radix_sort_keys", &radix_sort_keys, "device radix key sort",
        py::arg("keys"), py::arg("probe") = true);
  m.def("runs_sorted", &runs_sorted,
        "run boundaries of sorted keys (K18)");
  m.def("runs_multi", &runs_multi,
        "run boundaries of lexicographically sorted key columns (K22)");
  m.attr("MRUNS_TILE_ROWS") = (int64_t)MRUNS_TILE;
  m.def("lex_searchsorted", &lex_searchsorted,
        "searchsorted over lexicographically sorted tuples (K22)",
        py::arg("sorted_cols"), py::arg("query_cols"),
        py::arg("right") = false);
  m.def("segment_reduce_runs", &segment_reduce_runs,
        "int64 segmented reduce with precomputed runs (K16 fast path)");
  m.def("runs_guard", &runs_guard,
        "(count, max run length) of a runs_sorted result");
  m.def("segment_reduce_sorted", &segment_reduce_sorted,
        "typed reduce-by-key over sorted pairs (K16; deterministic)");
  m.def("hash_bytes", &hash_bytes,
        "murmur3-32 over varlen byte rows (K17, device strings)");
  m.def("hash_bytes64", &hash_bytes64,
        "64-bit two-seed murmur3 dictionary ids (K17)");
  m.def("colsum16", &colsum16,
        "vector-aggregate experiment: [N,16] f32 colsum, VALU vs MFMA");
  m.def("radix_sort_kv", &radix_sort_kv,
        "direct (key, 8-byte value) radix sort");
  m.def("slot_pids", &slot_pids, "table-slot-range partition ids");
  m.def("expr_apply", &expr_apply,
        "fused Map/Filter expression interpreter (K13)");
  m.def("tokenize_bytes", &tokenize_bytes,
        "split BYTES rows into tokens on a delimiter set (K20)");
  m.attr("TOKENIZE_TILE_BYTES") = (int64_t)TOK_TILE;
  m.def("iddict_claim", &iddict_claim,
        "id dictionary: claim slots for new ids; returns the new rows (K23)");
  m.def("iddict_lookup", &iddict_lookup,
        "id dictionary: position of every id, -1 when absent (K23)");
  m.def("iddict_rehash", &iddict_rehash,
        "id dictionary: move a table into a larger one (K23)");
  m.def("bytes_gather", &bytes_gather,
        "variable-length row gather of a BYTES column (K23)",
        py::arg("data"), py::arg("offsets"), py::arg("rows"),
        py::arg("total") = -1);
  m.attr("BYTES_GATHER_TILE_BYTES") = (int64_t)BG_TILE;
  m.def("bytes_order_keys", &bytes_order_keys,
        "round keys of the byte-order refinement of a BYTES column (K24)",
        py::arg("data"), py::arg("offsets"), py::arg("rows"), py::arg("w"),
        py::arg("max_blocks") = 0);
  m.def("bytes_order_refine", &bytes_order_refine,
        "head markers and stays-active flags of sorted refinement slots");
  m.attr("BYTES_ORDER_BLOCK") = (int64_t)BO_BLOCK;
  m.attr("BYTES_ORDER_TILE_SLOTS") = (int64_t)BO_TILE;
}
