/* sthenomi_extend_bench.h -- measurement hook of the posterior extension, exported by libsthenomi_extend_bench.so.
 *
 * Not part of the drop-in boundary (include/sthenomi.h, sthenomi_extend.h): like include/sthenomi_bench.h, whose table of
 * hooks is fixed (tests/capi_smoke.c checks it one by one), this is for tools/ and tests only.  The library links against
 * libsthenomi.so and works on posteriors created there. */
#ifndef STHENOMI_EXTEND_BENCH_H
#define STHENOMI_EXTEND_BENCH_H

#include "sthenomi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the row solve R <- R L^-T of sgp_posterior_extend on a scratch block of tile_rows x 128 rows against the kept columns
 * [0, 128 floor(N / 128)) of post, by one of its two schedules -- 0: deep products as single launches (the schedule of
 * sgp_posterior_predict), 1: deep products split over K.  ms_out receives the time of each of `reps` repetitions in
 * milliseconds (tools/extend_bench.py).  The posterior is not changed. */
int sgp_bench_extend_row_solve(sgp_post* post, int64_t tile_rows, int schedule, int reps, double* ms_out);

#ifdef __cplusplus
}
#endif

#endif /* STHENOMI_EXTEND_BENCH_H */
