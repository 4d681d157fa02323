// libsthenomi_conv.so -- the entry point of include/sthenomi_conv.h.  Links against libsthenomi.so, which keeps the
// geometries on its contexts and assembles the patch terms (capi.hip: drv_conv_geom, conv.hip); this file only gives the
// registration its C name.
#include "ctx.h"
#include "driver.h"
#include "../../include/sthenomi_conv.h"

extern "C" int sgp_conv_geom(sgp_ctx* ctx, const sgp_patch_geom* geom, int32_t* id_out) {
  if (!geom) {
    sgp::set_error("sgp_conv_geom: NULL geometry");
    return -1;
  }
  return sgp::drv_conv_geom(ctx, geom->height, geom->width, geom->patch_h, geom->patch_w, id_out);
}
