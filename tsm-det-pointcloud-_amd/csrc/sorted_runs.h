// sorted_runs.h — the shared front half of every float-atomic-free scatter-add backward of libspx: turn (entry -> target)
// pairs into per-target runs of a sorted entry list.  Included only by pointnet2.hip, pointnet2_stack.hip,
// group_project.hip and voxel_pool.hip (it pulls in rocprim).
//
// The contract, stated once:
//   - the caller's key kernel writes, for every entry e in [0, total), keys_in[e] = its target row in [0, targets), or
//     the SENTINEL = targets when the entry is dropped (index out of range, empty ball, dead row), and vals_in[e] = e;
//   - the pairs are sorted by key with rocprim::radix_sort_pairs over the low key_bits(sentinel) bits — enough to tell
//     the sentinel from every target.  A radix sort is STABLE, so the entries of one target keep their ascending order;
//   - start[k] / end[k] then bound target k's run in keys_out / vals_out: the caller's sum kernel adds vals_out[start[k]
//     .. end[k]) front to back, which is ascending entry order whatever the launch geometry — the determinism of the
//     backward rests on this and on nothing else.  start[k] == end[k] (both 0) means that no entry reaches target k: its
//     gradient is exactly 0.  Runs of the sentinel are not marked;
//   - limits: total < INT32_MAX (positions are int32) and targets < UINT32_MAX (the sentinel must fit a uint32 key).  The
//     callers check both before they come here.
// The per-op key kernels and sum kernels stay with their ops: their thread-to-(target, channel) maps and their
// summation orders differ on purpose.
#pragma once
#include "spx_common.h"

#include <rocprim/device/device_radix_sort.hpp>

struct SortedRunsWs {
  uint32_t *keys_in, *vals_in, *keys_out, *vals_out;
  int32_t *start, *end;
  void* sort_tmp;
  size_t sort_bytes;
};

static inline unsigned spx_key_bits(uint64_t sentinel) {
  unsigned bits = 1;
  while (bits < 32 && (sentinel >> bits) != 0) ++bits;
  return bits;
}

static inline size_t spx_sort_tmp_bytes(int64_t total, int64_t targets) {
  size_t bytes = 0;
  (void)rocprim::radix_sort_pairs((void*)nullptr, bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                  (uint32_t*)nullptr, (size_t)total, 0, spx_key_bits((uint64_t)targets));
  return bytes;
}

// keys_in | vals_in | keys_out | vals_out | start | end | sort_tmp, each 256-byte aligned.  Returns the bytes used; the
// caller places its own extras at base + that.  ws == NULL: size only.  tmp_when_empty: whether total == 0 (nothing is
// sorted) still reserves rocprim's temporary storage.
static inline size_t spx_sorted_runs_layout(int64_t total, int64_t targets, char* base, SortedRunsWs* ws,
                                            bool tmp_when_empty = true) {
  const size_t a = spx_align((size_t)total * 4), t = spx_align((size_t)targets * 4);
  const size_t sb = spx_align(total > 0 || tmp_when_empty ? spx_sort_tmp_bytes(total, targets) : 0);
  if (ws) {
    ws->keys_in = (uint32_t*)base;
    ws->vals_in = (uint32_t*)(base + a);
    ws->keys_out = (uint32_t*)(base + 2 * a);
    ws->vals_out = (uint32_t*)(base + 3 * a);
    ws->start = (int32_t*)(base + 4 * a);
    ws->end = (int32_t*)(base + 4 * a + t);
    ws->sort_tmp = base + 4 * a + 2 * t;
    ws->sort_bytes = sb;
  }
  return 4 * a + 2 * t + sb;
}

static __global__ __launch_bounds__(256) void spx_k_run_bounds(const uint32_t* __restrict__ keys, int64_t total,
                                                               uint32_t sentinel, int32_t* __restrict__ start,
                                                               int32_t* __restrict__ end) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= total) return;
  const uint32_t k = keys[p];
  if (k == sentinel) return;
  if (p == 0 || keys[p - 1] != k) start[k] = (int32_t)p;
  if (p == total - 1 || keys[p + 1] != k) end[k] = (int32_t)(p + 1);
}

// After the caller's key kernel: sort (total > 0), zero start and end, mark the runs (total > 0).
static inline int spx_sorted_runs(const SortedRunsWs& L, int64_t total, int64_t targets, hipStream_t s) {
  const uint32_t sentinel = (uint32_t)targets;
  if (total > 0) {
    size_t sb = L.sort_bytes;
    if (rocprim::radix_sort_pairs(L.sort_tmp, sb, L.keys_in, L.keys_out, L.vals_in, L.vals_out, (size_t)total, 0,
                                  spx_key_bits(sentinel), s) != hipSuccess)
      return SPX_ERR_LAUNCH;
  }
  // start and end are adjacent in ws (with the alignment gap): one fill zeroes both
  spx_fill_async(L.start, 0, (size_t)((char*)(L.end + targets) - (char*)L.start), s);
  if (total > 0)
    hipLaunchKernelGGL(spx_k_run_bounds, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, L.keys_out, total,
                       sentinel, L.start, L.end);
  return SPX_OK;
}
