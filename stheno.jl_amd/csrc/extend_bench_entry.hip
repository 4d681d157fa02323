// libsthenomi_extend_bench.so -- the measurement hook of include/sthenomi_extend_bench.h.  Links against libsthenomi.so
// (extend.hip: drv_extend_row_solve_ms); not part of the product boundary.
#include "ctx.h"
#include "driver.h"
#include "../../include/sthenomi_extend_bench.h"

extern "C" int sgp_bench_extend_row_solve(sgp_post* post, int64_t tile_rows, int schedule, int reps, double* ms_out) {
  return sgp::drv_extend_row_solve_ms(post, tile_rows, schedule, reps, ms_out);
}
