// Host check of the ragged pool's task order (stheno.jl_amd/csrc/df_pool.h), see tests/test_df_pool_host.py.
#include "../stheno.jl_amd/csrc/df_pool.h"
#include "../stheno.jl_amd/csrc/sz_pattern.h"
#include <algorithm>
#include <cstdio>
#include <vector>

using namespace sgp;

struct Pool {
  std::vector<int> T_r, T_c;
  std::vector<SzPattern> pat;   // per member; words == 0: dense
  int nb() const { return (int)T_r.size(); }
};

static bool nonzero(const Pool& P, int b, int i, int j) {
  const SzPattern& p = P.pat[(size_t)b];
  return p.words == 0 || ((p.nz[(size_t)i * p.words + (j >> 6)] >> (j & 63)) & 1) != 0;
}

// ids map one to one onto (member, i, j); each member's ids ascend in its own column-major order
static bool bijective_and_ordered(const Pool& P, const std::vector<uint32_t>& order) {
  if ((long)order.size() != df_pool_ntasks(P.T_r.data(), P.T_c.data(), P.nb())) return false;
  std::vector<long> next((size_t)P.nb(), 0);
  for (uint32_t e : order) {
    int b, i, j;
    df_pool_unpack(e, b, i, j);
    if (b < 0 || b >= P.nb()) return false;
    int wi, wj;
    if (next[(size_t)b] >= df_ntasks(P.T_r[(size_t)b], P.T_c[(size_t)b])) return false;
    df_task_tile(next[(size_t)b], P.T_r[(size_t)b], P.T_c[(size_t)b], wi, wj);
    if (wi != i || wj != j) return false;   // the member's next task in ITS column-major order: also one to one
    ++next[(size_t)b];
  }
  for (int b = 0; b < P.nb(); ++b)
    if (next[(size_t)b] != df_ntasks(P.T_r[(size_t)b], P.T_c[(size_t)b])) return false;
  return true;
}

// Replay of chol_pool_body's task loop with W workgroups (tests/df_tasks_host.cpp's replay, per member geometry and pattern):
// a held task finishes once its inputs are final.  A computed tile (i, j) needs the k blocks k < j for which both (i, k) and
// (j, k) are structurally non-zero -- prog[i] > k and prog[j] > k, i.e. (counters move in column order) both beyond the LAST
// such k -- the diagonal tile for i > j, and, before it publishes, every earlier tile of its row (prog[i] == j).  A
// structurally zero tile only waits for prog[i] == j.  Odd rounds retire one held task only.
static bool replay(const Pool& P, const std::vector<uint32_t>& order, int W) {
  const long nt = (long)order.size();
  std::vector<std::vector<int>> prog((size_t)P.nb());
  for (int b = 0; b < P.nb(); ++b) prog[(size_t)b].assign((size_t)P.T_r[(size_t)b], 0);
  std::vector<long> held;
  long head = 0, done = 0, round = 0;
  while (done < nt) {
    while ((int)held.size() < W && head < nt) held.push_back(head++);
    bool any = false;
    const size_t n0 = held.size();
    for (size_t k = 0; k < n0 && k < held.size();) {
      const size_t h = (k + (size_t)round) % held.size();
      int b, i, j;
      df_pool_unpack(order[(size_t)held[h]], b, i, j);
      std::vector<int>& p = prog[(size_t)b];
      bool ready = p[(size_t)i] == j;
      if (nonzero(P, b, i, j)) {
        int need = 0;   // one past the last k block the contraction reads
        for (int kk = 0; kk < j; ++kk)
          if (nonzero(P, b, i, kk) && nonzero(P, b, j, kk)) need = kk + 1;
        ready = ready && p[(size_t)i] >= need && p[(size_t)j] >= need && (i == j || p[(size_t)j] >= j + 1);
      }
      if (ready) {
        p[(size_t)i] = j + 1;
        held[h] = held.back();
        held.pop_back();
        ++done;
        any = true;
        if (round & 1) break;
      } else {
        ++k;
      }
    }
    if (!any) return false;   // nobody can move: a deadlock
    ++round;
  }
  for (int b = 0; b < P.nb(); ++b)
    for (int i = 0; i < P.T_r[(size_t)b]; ++i)
      if (prog[(size_t)b][(size_t)i] != std::min(i + 1, P.T_c[(size_t)b])) return false;
  return true;
}

static Pool dense_pool(const std::vector<std::pair<int, int>>& shapes) {
  Pool P;
  for (auto s : shapes) {
    P.T_r.push_back(s.first);
    P.T_c.push_back(s.second);
    P.pat.emplace_back();
  }
  return P;
}

int main() {
  long pools = 0, replays = 0, bad = 0;
  std::vector<Pool> all;
  all.push_back(dense_pool({{2, 1}, {2, 1}, {3, 2}, {9, 8}}));
  {
    std::vector<std::pair<int, int>> ramp;
    for (int c = 1; c <= 16; ++c) ramp.push_back({c + 1, c});
    all.push_back(dense_pool(ramp));
  }
  {
    // the gradient's [K ; (y - m)' ; I] of 2, 3, 6 tile columns: T_r = 2 T_c + 1, each with the border pattern of a dense K
    Pool P = dense_pool({{5, 2}, {7, 3}, {13, 6}});
    for (int b = 0; b < P.nb(); ++b) {
      const long n_pad = 128L * P.T_c[(size_t)b];
      sz_symbolic(std::vector<char>(1, 1), 1, std::vector<long>(1, 0), std::vector<long>(1, n_pad), n_pad, 128, P.T_c[(size_t)b],
                  P.T_r[(size_t)b], P.pat[(size_t)b], true);
      if (P.pat[(size_t)b].words == 0) {
        ++bad;
        printf("BAD no border pattern for member %d\n", b);
      }
    }
    all.push_back(P);
    // the same shapes with NO tile skipped
    all.push_back(dense_pool({{5, 2}, {7, 3}, {13, 6}}));
  }
  all.push_back(dense_pool(std::vector<std::pair<int, int>>(16, {33, 32})));
  for (const Pool& P : all) {
    ++pools;
    std::vector<uint32_t> order;
    if (!df_pool_order(P.T_r.data(), P.T_c.data(), P.nb(), order) || !bijective_and_ordered(P, order)) {
      ++bad;
      printf("BAD order of pool %ld\n", pools);
      continue;
    }
    for (int W : {1, 2, 7, 256, 512}) {
      ++replays;
      if (!replay(P, order, W)) {
        ++bad;
        printf("BAD replay pool %ld W=%d\n", pools, W);
      }
    }
  }
  // equal shapes reproduce df_batch_task id for id
  long equal = 0;
  for (int nb : {2, 3, 8, 16})
    for (int T_c : {1, 2, 5, 32})
      for (int border : {1, 2}) {
        ++equal;
        std::vector<int> T_r((size_t)nb, T_c + border), T_cs((size_t)nb, T_c);
        std::vector<uint32_t> order;
        bool ok = df_pool_order(T_r.data(), T_cs.data(), nb, order) && (long)order.size() == nb * df_ntasks(T_c + border, T_c);
        for (long q = 0; ok && q < (long)order.size(); ++q) {
          int b, i, j, wb, wi, wj;
          long ql;
          df_pool_unpack(order[(size_t)q], b, i, j);
          df_batch_task(q, nb, wb, ql);
          df_task_tile(ql, T_c + border, T_c, wi, wj);
          ok = b == wb && i == wi && j == wj;
        }
        if (!ok) {
          ++bad;
          printf("BAD equal shapes nb=%d T_c=%d border=%d\n", nb, T_c, border);
        }
      }
  // shapes an entry cannot name are refused
  {
    int T_r[1] = {DF_POOL_MAX_T + 1}, T_c[1] = {1};
    std::vector<uint32_t> order;
    if (df_pool_order(T_r, T_c, 1, order)) ++bad;
    int T_r2[1] = {1}, T_c2[1] = {2};
    if (df_pool_order(T_r2, T_c2, 1, order)) ++bad;
  }
  printf("pools %ld replays %ld equal %ld bad %ld\n", pools, replays, equal, bad);
  return bad ? 1 : 0;
}
