// Task order of a RAGGED pool of the dataflow factorisation (chol_df.hip: chol_pool_kernel) -- up to DF_MAX_BATCH independent
// bordered matrices, each with its own tile grid, factored by one launch.  Plain integer functions that also compile for the
// host, as df_tasks.h does: tests/df_pool_host.cpp enumerates whole pools on the CPU and replays the kernel's task loop.
//
// The pool serves the loops that evaluate one model on data sets of different sizes -- folds, learning curves, one GP per
// series (the reference's examples/getting_started/script.jl:154-213 runs such a loop member by member).
//
// The order is a MERGE of the members' own column-major orders (df_tasks.h): member b sees its tasks in the order of its own
// launch, so every input of a task belongs to a smaller id of the same member and the holder of the smallest unfinished id
// can always finish -- the progress argument of the single launch, unchanged, whatever the merge.  The merge itself is
// proportional dealing: task ql of member b sits at the key (ql + 1/2) / ntasks_b, ties broken by the member index, so every
// member's chain advances over the whole launch (a short member is not finished first and a long one not left for last).
// For equal shapes the key of task ql is the same in every member: the order is df_batch_task's round robin id for id.
//
// The kernel reads the order from a table the host builds and uploads with the launch: one 32-bit entry per task.
#pragma once
#include "df_tasks.h"
#include <vector>

namespace sgp {

constexpr int DF_POOL_MAX = 16;        // members of one pool (= DF_MAX_BATCH, common.h)
constexpr int DF_POOL_MAX_T = 4095;    // tile rows / columns an entry can name

// entry: member << 24 | tile row << 12 | tile column
__host__ __device__ __forceinline__ uint32_t df_pool_pack(int b, int i, int j) {
  return ((uint32_t)b << 24) | ((uint32_t)i << 12) | (uint32_t)j;
}
__host__ __device__ __forceinline__ void df_pool_unpack(uint32_t e, int& b, int& i, int& j) {
  b = (int)(e >> 24);
  i = (int)((e >> 12) & 0xfffu);
  j = (int)(e & 0xfffu);
}

// tasks of the whole pool
inline long df_pool_ntasks(const int* T_r, const int* T_c, int nb) {
  long n = 0;
  for (int b = 0; b < nb; ++b) n += df_ntasks(T_r[b], T_c[b]);
  return n;
}

// The table: order[q] = entry of global task id q.  Returns false when a shape does not fit an entry.
// (keys compared exactly: (2 ql + 1) / (2 nt_b) < (2 ql' + 1) / (2 nt_b')  <=>  (2 ql + 1) nt_b' < (2 ql' + 1) nt_b)
inline bool df_pool_order(const int* T_r, const int* T_c, int nb, std::vector<uint32_t>& order) {
  order.clear();
  if (nb < 1 || nb > DF_POOL_MAX) return false;
  long nt[DF_POOL_MAX], next[DF_POOL_MAX];
  for (int b = 0; b < nb; ++b) {
    if (T_c[b] < 1 || T_r[b] < T_c[b] || T_r[b] > DF_POOL_MAX_T) return false;
    nt[b] = df_ntasks(T_r[b], T_c[b]);
    next[b] = 0;
  }
  const long total = df_pool_ntasks(T_r, T_c, nb);
  order.reserve((size_t)total);
  for (long q = 0; q < total; ++q) {
    int best = -1;
    for (int b = 0; b < nb; ++b) {
      if (next[b] >= nt[b]) continue;
      if (best < 0 || (2 * next[b] + 1) * nt[best] < (2 * next[best] + 1) * nt[b]) best = b;   // strict: ties keep the smaller b
    }
    int i, j;
    df_task_tile(next[best], T_r[best], T_c[best], i, j);
    order.push_back(df_pool_pack(best, i, j));
    ++next[best];
  }
  return true;
}

}  // namespace sgp
