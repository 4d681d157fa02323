// libsthenomi_stencil.so -- the entry point of include/sthenomi_stencil.h.  Links against libsthenomi.so, which keeps the
// stencils on its contexts and assembles the stencil terms (capi.hip: drv_stencil_register, stencil.hip); this file only
// gives the registration its C name.
#include "ctx.h"
#include "driver.h"
#include "../../include/sthenomi_stencil.h"

extern "C" int sgp_stencil_register(sgp_ctx* ctx, const sgp_stencil* st, int32_t* id_out) {
  if (!st) {
    sgp::set_error("sgp_stencil_register: NULL stencil");
    return -1;
  }
  return sgp::drv_stencil_register(ctx, st->dim, st->npoints, st->offsets, st->weights, id_out);
}
