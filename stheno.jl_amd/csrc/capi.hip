// libsthenomi.so host driver + C ABI (include/sthenomi.h).  gfx950 only; no CPU fallback:
// every numerical result is produced by the HIP kernels in this directory.
#include "ctx.h"
#include "driver.h"
#include "kept.h"
#include "asm_frame.h"
#include "tilemap.h"
#include "sz_pattern.h"
#include "df_tasks.h"
#include "df_pool.h"
#include "../../include/sthenomi_kprod.h"
#include "kprod_kinds_table.h"
#include "spec_segments.h"
#include <limits>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <mutex>
#include <set>
#include <vector>

namespace sgp {

static thread_local std::string g_err;
void set_error(const std::string& s) { g_err = s; }

static inline long rup(long x, long m) { return (x + m - 1) / m * m; }
static inline long spec_rows_host(const sgp_cov_spec* sp) {
  long n = 0;
  for (int i = 0; i < sp->n_row_blocks; ++i) n += sp->row_len[i];
  return n;
}
constexpr long NOMASK = -(1L << 40);
constexpr long INVD_STRIDE = 8 * 256;  // eight 16x16 inverse diagonal blocks per 128-block
constexpr long WOUT_SMALL = 512;   // outer panel width of the two-level blocked Cholesky
constexpr long WOUT_LARGE = 1024;  // ... for n_pad >= 32768 (halves the C-tile traffic per flop)

}  // namespace sgp

using namespace sgp;

// product chains (include/sthenomi_kprod.h) have no sharded instantiation: refused before a multi-GPU context's ranks see them
#define REFUSE_KPROD_MULTI(ctx, sp)                                                                          \
  do {                                                                                                       \
    CHECK_ARG(!((ctx)->multi && spec_has_deriv(sp)), sgp::DERIV_REFUSAL_MULTI); /* (deriv.hip: likewise) */  \
    CHECK_ARG(!((ctx)->multi && spec_has_kprod(sp)),                                                         \
              "spec: product chains and the RQ / LINEAR kinds are not supported on a multi-GPU context");    \
  } while (0)

extern "C" int sgp_abi_version(void) { return SGP_ABI_VERSION; }
extern "C" const char* sgp_last_error(void) { return g_err.c_str(); }

extern "C" int sgp_geometry(int64_t N, int64_t S, int64_t* n_pad, int64_t* m_tot) {
  long np = rup(N, TILE);
  if (np == 0) np = TILE;
  long mt = np + (S > 0 ? rup(S, TILE) : 0);
  if (n_pad) *n_pad = np;
  if (m_tot) *m_tot = mt;
  return 0;
}

// ---------------------------------------------------------------------------------------
// device-memory cache of a context
// ---------------------------------------------------------------------------------------
namespace sgp {
thread_local sgp_ctx* tl_ctx = nullptr;

void* pool_alloc(sgp_ctx* ctx, size_t bytes) {
  bytes = (bytes + 255) / 256 * 256;
  if (ctx->pool_enabled) {
    // best fit among the unused blocks that are not wastefully large for the request
    const size_t cap = bytes < (1u << 20) ? (4u << 20) : bytes + bytes / 4;
    long best = -1;
    for (size_t i = 0; i < ctx->pool.size(); ++i) {
      const sgp_pool_block& b = ctx->pool[i];
      if (b.used || b.bytes < bytes || b.bytes > cap) continue;
      if (best < 0 || b.bytes < ctx->pool[best].bytes) best = (long)i;
    }
    if (best >= 0) {
      ctx->pool[best].used = true;
      return ctx->pool[best].p;
    }
  }
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess && ctx->pool_enabled) {  // give cached blocks back to the driver and retry once
    (void)hipGetLastError();
    pool_trim(ctx);
    e = hipMalloc(&p, bytes);
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    set_error("hipMalloc failed (" + std::to_string(bytes) + " bytes)");
    return nullptr;
  }
  if (ctx->pool_enabled) {
    sgp_pool_block b;
    b.p = p;
    b.bytes = bytes;
    b.used = true;
    ctx->pool.push_back(b);
    ctx->pool_bytes += bytes;
  }
  return p;
}

void pool_free(sgp_ctx* ctx, void* p) {
  if (!p) return;
  for (auto& b : ctx->pool)
    if (b.p == p) {
      b.used = false;
      return;
    }
  hipFree(p);  // not a cached block (cache disabled)
}

void pool_trim(sgp_ctx* ctx) {
  hipStreamSynchronize(ctx->stream);
  hipStreamSynchronize(ctx->stream2);
  std::vector<sgp_pool_block> keep;
  for (auto& b : ctx->pool) {
    if (b.used) {
      keep.push_back(b);
    } else {
      hipFree(b.p);
      ctx->pool_bytes -= b.bytes;
    }
  }
  ctx->pool.swap(keep);
}
}  // namespace sgp

extern "C" int sgp_ctx_trim(sgp_ctx* ctx) {
  CHECK_ARG(ctx != nullptr, "sgp_ctx_trim: NULL argument");
  CtxScope scope(ctx);
  pool_trim(ctx);
  return 0;
}

extern "C" int sgp_ctx_stage_timing(sgp_ctx* ctx, int enable) {
  CHECK_ARG(ctx != nullptr, "sgp_ctx_stage_timing: NULL argument");
  CtxScope scope(ctx);
  ctx->stage_timing = enable ? 1 : 0;
  for (double& v : ctx->stage_ms) v = 0.0;
  return 0;
}

extern "C" int sgp_ctx_stage_ms(sgp_ctx* ctx, double* out16) {
  CHECK_ARG(ctx && out16, "sgp_ctx_stage_ms: NULL argument");
  CtxScope scope(ctx);
  for (int i = 0; i < 16; ++i) out16[i] = ctx->stage_ms[i];
  return 0;
}

// Live contexts.  A posterior handle (sgp_post / sgp_sparse_post) may outlive the context it was created on -- it is freed
// without it -- but predicting against it needs the context's streams, scratch and (multi-GPU) ranks: the predict entry
// points look the context up here and fail cleanly when it is gone (advisor, round 3: that was a use-after-free).
// (a destroyed context's address may be handed out again by the allocator: handles remember the context's SERIAL, too)
static std::mutex g_live_mu;
static std::set<const sgp_ctx*> g_live_ctx;
static long g_ctx_serial = 0;
static bool ctx_is_live(const sgp_ctx* c, long serial) {
  std::lock_guard<std::mutex> lk(g_live_mu);
  return g_live_ctx.count(c) != 0 && c->serial == serial;
}

// ---------------------------------------------------------------------------------------
// Run-time switches of a context: ONE table, read once when the context is created (docs/03_kernels.md section 3.5 lists
// every entry with the test that exercises it).  Round 6 pruned the switches whose A/B was closed -- the XCD task queues of
// the dataflow kernel, the explicit-inverse panel solves (SGP_REFINE), the stamp-kernel experiments, the fp32 driver's
// panel widths, the VFE two-chunk overlap, SGP_POOL, SGP_FUSE_MAX_N, SGP_LA_MAX_N, SGP_SPLITK_SUB, SGP_HYBRID_GROW.
// What is left selects between schedules that all give the same bits (the bit-identity tests flip them) or bounds a wait.
// ---------------------------------------------------------------------------------------
namespace {
struct CtxKnob {
  const char* name;
  void (*set)(sgp_ctx*, const char*);
};
const CtxKnob kCtxKnobs[] = {
    // ---- schedule of the blocked Cholesky (capi.hip: chol_bordered; every choice gives the same factor)
    {"SGP_LOOKAHEAD", [](sgp_ctx* c, const char* v) { c->lookahead = atoi(v); }},          // 0: no second stream, 2: at every size
    {"SGP_WOUT", [](sgp_ctx* c, const char* v) { c->wout = atol(v) / TILE * TILE; }},       // outer panel width of the launches
    {"SGP_WMID", [](sgp_ctx* c, const char* v) { c->wmid = atol(v) / TILE * TILE; }},       // middle blocking level
    {"SGP_FUSE_POTRF", [](sgp_ctx* c, const char* v) { c->fuse_potrf = atoi(v); }},        // fused update + diagonal block
    {"SGP_DATAFLOW", [](sgp_ctx* c, const char* v) { c->dataflow = atoi(v); }},            // 0 never / 1 always / unset by size
    {"SGP_DF_MIN_N", [](sgp_ctx* c, const char* v) { c->df_min_n = atol(v); }},
    {"SGP_DF_MAX_N", [](sgp_ctx* c, const char* v) { c->df_max_n = atol(v); }},
    {"SGP_DF_FAT_MAX_N", [](sgp_ctx* c, const char* v) { c->df_fat_max_n = atol(v); }},    // one workgroup per CU below this
    {"SGP_DF_WGS", [](sgp_ctx* c, const char* v) { if (atoi(v) > 0) c->df_wgs = atoi(v); }},
    {"SGP_DF_TIMEOUT_S", [](sgp_ctx* c, const char* v) { c->df_timeout_s = atof(v); }},    // bound of one wait inside the kernel
    {"SGP_DF_FALLBACK", [](sgp_ctx* c, const char* v) { c->df_fallback = atoi(v); }},      // 0: report the time-out (tests)
    {"SGP_HYBRID", [](sgp_ctx* c, const char* v) { c->hybrid = atoi(v); }},                // 0 never / 1 from 4096 columns on
    {"SGP_HYBRID_W", [](sgp_ctx* c, const char* v) { c->hybrid_w = std::max<long>(TILE, atol(v) / TILE * TILE); }},
    {"SGP_HYBRID_WGS", [](sgp_ctx* c, const char* v) { c->hybrid_wgs = std::max(8, atoi(v)); }},
    {"SGP_HYBRID_FAT", [](sgp_ctx* c, const char* v) { c->hybrid_fat = atoi(v); }},
    // (the gradient path's crossover -- 16384 by default -- follows a limit the user sets: advisor, round 5: it used to stay at
    // min(limit, 16384), so raising the limit could not move it; SGP_HYBRID_GROW_MIN_N, read after it, names it separately)
    {"SGP_HYBRID_MIN_N", [](sgp_ctx* c, const char* v) { c->hybrid_min_n = c->hybrid_grow_min_n = atol(v); }},
    {"SGP_HYBRID_GROW_MIN_N", [](sgp_ctx* c, const char* v) { c->hybrid_grow_min_n = atol(v); }},
    {"SGP_HYBRID_SERIAL", [](sgp_ctx* c, const char* v) { c->hybrid_serial = atoi(v); }},  // one stream (bench.py: uncontended leg)
    {"SGP_BATCH_MAX_N", [](sgp_ctx* c, const char* v) { c->batch_max_n = atol(v); }},      // sgp_logpdf_batch: pooled up to this size
    // ---- structural zeros
    {"SGP_STRUCT_ZEROS", [](sgp_ctx* c, const char* v) { c->struct_zeros = atoi(v); }},    // 0: the dense schedule (A/B, same bits)
};
void apply_env_knobs(sgp_ctx* c) {
  for (const CtxKnob& k : kCtxKnobs)
    if (const char* v = getenv(k.name)) k.set(c, v);
}
}  // namespace

extern "C" int sgp_ctx_create(int device, sgp_ctx** out) {
  CHECK_ARG(out != nullptr, "sgp_ctx_create: out is NULL");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) {
    set_error("sgp_ctx_create: no HIP device visible (libsthenomi has no CPU path)");
    return -3;
  }
  CHECK_ARG(device >= 0 && device < ndev, "sgp_ctx_create: bad device ordinal");
  SGP_HIP(hipSetDevice(device));
  hipDeviceProp_t prop;
  SGP_HIP(hipGetDeviceProperties(&prop, device));
  if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos) {
    set_error(std::string("sgp_ctx_create: device is ") + prop.gcnArchName +
              ", libsthenomi is built for gfx950 only");
    return -3;
  }
  sgp_ctx* c = new sgp_ctx();
  c->device = device;
  auto init = [&]() -> int {
    int lo = 0, hi = 0;
    SGP_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
    // the panel (critical-path) stream at high priority, the trailing-update stream below it
    SGP_HIP(hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, hi));
    SGP_HIP(hipStreamCreateWithPriority(&c->stream2, hipStreamNonBlocking, lo));
    SGP_HIP(hipEventCreateWithFlags(&c->ev_panel, hipEventDisableTiming));
    SGP_HIP(hipEventCreateWithFlags(&c->ev_rest, hipEventDisableTiming));
    {
      hipDeviceProp_t prop;
      SGP_HIP(hipGetDeviceProperties(&prop, device));
      c->df_wgs = 2 * prop.multiProcessorCount;
    }
    apply_env_knobs(c);
    SGP_HIP(hipMalloc(&c->d_invd, sizeof(double) * 8 * 256));
    c->n_slots = 1 << 15;
    SGP_HIP(hipMalloc(&c->d_slots, sizeof(double) * c->n_slots));
    c->n_scal = 16 + (1 << 16);
    SGP_HIP(hipMalloc(&c->d_scal, sizeof(double) * c->n_scal));
    SGP_HIP(hipMalloc(&c->d_info, sizeof(int)));
    return 0;
  };
  int rc = init();
  if (rc) {
    sgp_ctx_destroy(c);
    return rc;
  }
  {
    std::lock_guard<std::mutex> lk(g_live_mu);
    c->serial = ++g_ctx_serial;
    g_live_ctx.insert(c);
  }
  *out = c;
  return 0;
}

extern "C" int sgp_ctx_destroy(sgp_ctx* c) {
  if (!c) return 0;
  {
    std::lock_guard<std::mutex> lk(g_live_mu);
    g_live_ctx.erase(c);
  }
  if (c->multi) sgp_multi_destroy(c->multi);
  c->multi = nullptr;
  hipSetDevice(c->device);
  if (c->stream) hipStreamSynchronize(c->stream);
  if (c->stream2) hipStreamSynchronize(c->stream2);
  for (auto e : c->ev) hipEventDestroy(e);
  for (auto& b : c->pool) hipFree(b.p);
  if (c->h_stage) hipHostFree(c->h_stage);
  if (c->d_invd) hipFree(c->d_invd);
  if (c->d_slots) hipFree(c->d_slots);
  if (c->d_scal) hipFree(c->d_scal);
  if (c->d_info) hipFree(c->d_info);
  for (auto& st : c->stencils) hipFree(st.dev);
  if (c->d_df_state) hipFree(c->d_df_state);
  if (c->d_sz) hipFree(c->d_sz);
  if (c->d_szmap) hipFree(c->d_szmap);
  if (c->h_sz_pin) hipHostFree(c->h_sz_pin);
  if (c->ev_sz) hipEventDestroy(c->ev_sz);
  if (c->d_df_inv) hipFree(c->d_df_inv);
  if (c->d_df_stats) hipFree(c->d_df_stats);
  if (c->ev_panel) hipEventDestroy(c->ev_panel);
  if (c->ev_rest) hipEventDestroy(c->ev_rest);
  if (c->stream2) hipStreamDestroy(c->stream2);
  if (c->stream) hipStreamDestroy(c->stream);
  delete c;
  return 0;
}

// ---------------------------------------------------------------------------------------
// device-resident specs
// ---------------------------------------------------------------------------------------
// Uploads a spec with ONE host -> device copy: inputs (packed to ld == dim), row / column scale
// vectors and the term table are laid out in a pinned staging buffer of the context and moved in
// one piece into one cached device block.  Caller holds the context (CtxScope / ctx->mu).
static void dspec_free(sgp_dspec* ds);
static int dspec_create(sgp_ctx* ctx, const sgp_cov_spec* sp, sgp_dspec** out) {
  CHECK_ARG(ctx && sp && out, "sgp_dspec_create: NULL argument");
  CHECK_ARG(sp->n_row_blocks >= 1 && sp->n_col_blocks >= 1, "spec: need >= 1 block");
  sgp_dspec* ds = new sgp_dspec();
  ds->ctx = ctx;
  ds->nrb = sp->n_row_blocks;
  ds->ncb = sp->n_col_blocks;
  ds->symmetric = sp->symmetric;
  long off = 0;
  for (int i = 0; i < ds->nrb; ++i) {
    ds->row_len.push_back(sp->row_len[i]);
    ds->row_off.push_back(off);
    off += sp->row_len[i];
  }
  ds->N = off;
  off = 0;
  for (int j = 0; j < ds->ncb; ++j) {
    ds->col_len.push_back(sp->col_len[j]);
    ds->col_off.push_back(off);
    off += sp->col_len[j];
  }
  ds->M = off;
  auto fail = [&](const char* msg) {
    set_error(msg);
    dspec_free(ds);
    return -1;
  };
  if (ds->symmetric && (ds->nrb != ds->ncb || ds->row_len != ds->col_len))
    return fail("spec: symmetric spec needs identical row / col blocks");
  // ---- pass 1: validate, lay everything out (byte offsets into one block, 256-byte aligned)
  size_t total = 0;
  auto place = [&](size_t bytes) {
    size_t at = total;
    total += (std::max<size_t>(bytes, 8) + 255) / 256 * 256;
    return at;
  };
  std::vector<size_t> in_off(sp->n_inputs);
  for (int k = 0; k < sp->n_inputs; ++k) {
    const sgp_input& in = sp->inputs[k];
    if (in.dim < 1 || in.dim > (1 << 20)) return fail("spec: input dimension must be >= 1");
    if (in.n < 0 || in.ld < in.dim) return fail("spec: bad input n / ld");
    in_off[k] = place(sizeof(double) * (size_t)(in.dim * in.n));
    ds->in_dim.push_back((int)in.dim);
    ds->in_n.push_back((long)in.n);
  }
  int npairs = ds->nrb * ds->ncb;
  ds->term_ptr.assign(sp->term_ptr, sp->term_ptr + npairs + 1);
  ds->pair_dmax.assign(npairs, 1);
  const int nterms = sp->term_ptr[npairs];
  std::vector<size_t> rs_off(nterms, (size_t)-1), cs_off(nterms, (size_t)-1);
  std::vector<long> rs_len(nterms, 0), cs_len(nterms, 0);
  // product chains and terms of the kinds above SGP_CONST (include/sthenomi_kprod.h): a class of their own
  // (kprod.hip)
  std::vector<char> is_kp(std::max(1, nterms), 0);
  // terms of the derivative kinds (include/sthenomi.h: SGP_DERIV_*): a class of their own (deriv.hip), validated against a table
  // of its own (deriv_kinds.h) -- the product path's table does not know them
  std::vector<char> is_dv(std::max(1, nterms), 0);
  std::vector<size_t> nuc_off(std::max(1, nterms), (size_t)-1);   // SGP_MATERN_NU: the term's constants of nu (kprod.hip)
  for (int I = 0; I < ds->nrb; ++I)
    for (int J = 0; J < ds->ncb; ++J) {
      int p = I * ds->ncb + J;
      int chain_len = 0, chain_dmax = 1;
      for (int t = sp->term_ptr[p]; t < sp->term_ptr[p + 1]; ++t) {
        const sgp_term& T = sp->terms[t];
        if (T.kind < 0 || (T.kind & ~(0xff | SGP_KIND_TIMES_PREV)) ||
            !(kp_kind_known(T.kind & 0xff) || deriv_kind_known(T.kind & 0xff)))
          return fail("spec: unknown kernel kind");
        const bool cont = (T.kind & SGP_KIND_TIMES_PREV) != 0;
        const bool next_cont = t + 1 < sp->term_ptr[p + 1] && sp->terms[t + 1].kind >= 0 &&
                               (sp->terms[t + 1].kind & SGP_KIND_TIMES_PREV);
        is_dv[t] = deriv_kind_known(T.kind & 0xff);
        if (is_dv[t]) {
          if (cont || next_cont) return fail(DERIV_REFUSAL_CHAIN);
          if (T.reserved) return fail(DERIV_REFUSAL_RESERVED);
          if (T.row_input >= 0 && T.row_input < sp->n_inputs)
            if (const char* refusal = deriv_param_refusal(T.param, (long)sp->inputs[T.row_input].dim)) return fail(refusal);
          ++ds->n_deriv;
        }
        is_kp[t] = !is_dv[t] && (cont || next_cont || (T.kind & 0xff) > SGP_CONST);
        if (is_kp[t]) {
          if (cont && t == sp->term_ptr[p])
            return fail("spec: product chain: a continuation (SGP_KIND_TIMES_PREV) cannot be the first term of a block pair");
          if (T.reserved)
            return fail("spec: product chain: reserved must be 0 (no products with patch or stencil sides, none for the RQ / "
                        "LINEAR kinds)");
          if (cont && (T.coef != 1.0 || T.row_scale || T.col_scale))
            return fail("spec: product chain: a continuation must have coef == 1.0 and NULL scales (the head carries them)");
          if (const char* refusal = kp_param_refusal(T.kind & 0xff, T.param)) return fail(refusal);   // kprod_kinds_table.h
          if (T.row_input >= 0 && T.row_input < sp->n_inputs) {
            const int64_t dim = sp->inputs[T.row_input].dim;
            if (dim > SGP_KPROD_MAX_DIM)
              return fail("spec: product chain: the input dimension of a factor (or of an RQ / LINEAR term) must be <= 16");
            if (!cont) chain_len = 0, chain_dmax = 1;
            ++chain_len;
            chain_dmax = std::max(chain_dmax, pow2ceil((int)std::max<int64_t>(dim, 1)));
            if (chain_len > SGP_KPROD_MAX_FACTORS || chain_len * chain_dmax > 64)
              return fail("spec: product chain beyond the limits: at most 8 factors, and factors x (largest factor dimension "
                          "rounded up to a power of two) <= 64");
          }
          if ((T.kind & 0xff) == SGP_MATERN_NU) nuc_off[t] = place(sizeof(double) * MN_COUNT);
          ++ds->n_kprod;
        }
        if (T.row_input < 0 || T.row_input >= sp->n_inputs || T.col_input < 0 ||
            T.col_input >= sp->n_inputs)
          return fail("spec: term input index out of range");
        const sgp_input& ri = sp->inputs[T.row_input];
        const sgp_input& ci = sp->inputs[T.col_input];
        if (T.reserved) {
          // a patch or stencil term (include/sthenomi_conv.h, include/sthenomi_stencil.h): reserved = row id | column id
          // << 16 into the context's table, 0 = plain side
          const int gid[2] = {(int)((uint32_t)T.reserved & 0xffffu), (int)((uint32_t)T.reserved >> 16)};
          const PatchGeom* g[2] = {nullptr, nullptr};
          const StencilDesc* st[2] = {nullptr, nullptr};
          for (int k = 0; k < 2; ++k) {
            if (gid[k] > (int)ctx->conv_geoms.size())
              return fail("spec: unknown patch geometry or stencil id (register it on this context with sgp_conv_geom / "
                          "sgp_stencil_register; a multi-GPU context takes none)");
            if (!gid[k]) continue;
            const PatchGeom& e = ctx->conv_geoms[gid[k] - 1];
            if (e.st > 0) st[k] = &ctx->stencils[e.st - 1];
            else g[k] = &e;
          }
          if ((g[0] || g[1]) && (st[0] || st[1])) return fail("spec: a term cannot pair a patch side with a stencil side");
          if (st[0] || st[1]) {
            if (ri.dim != ci.dim) return fail("spec: stencil term: row / col input dimension mismatch");
            if ((st[0] && st[0]->dim != ri.dim) || (st[1] && st[1]->dim != ci.dim))
              return fail("spec: a stencil's dim must equal the input dimension of its side");
            ++ds->n_stencil;
          } else {
            if (g[0] && ri.dim != (int64_t)g[0]->h * g[0]->w) return fail("spec: a patched row input must have dim = height * width");
            if (g[1] && ci.dim != (int64_t)g[1]->h * g[1]->w) return fail("spec: a patched column input must have dim = height * width");
            if (g[0] && g[1] && (g[0]->ph != g[1]->ph || g[0]->pw != g[1]->pw))
              return fail("spec: both sides patched with different patch sizes");
            const PatchGeom* gp = g[0] ? g[0] : g[1];
            if (!g[0] && ri.dim != (int64_t)gp->ph * gp->pw) return fail("spec: a plain row side must have dim = patch_h * patch_w");
            if (!g[1] && ci.dim != (int64_t)gp->ph * gp->pw) return fail("spec: a plain column side must have dim = patch_h * patch_w");
            ++ds->n_patch;
          }
        } else if (ri.dim != ci.dim) {
          return fail("spec: row / col input dimension mismatch");
        }
        if (ri.n != ds->row_len[I] || ci.n != ds->col_len[J])
          return fail("spec: input length does not match block length");
        if (T.row_scale && ds->row_len[I] > 0) {
          rs_len[t] = ds->row_len[I];
          rs_off[t] = place(sizeof(double) * (size_t)rs_len[t]);
        }
        if (T.col_scale && ds->col_len[J] > 0) {
          cs_len[t] = ds->col_len[J];
          cs_off[t] = place(sizeof(double) * (size_t)cs_len[t]);
        }
        if (!T.reserved && !is_kp[t] && !is_dv[t]) ds->pair_dmax[p] = std::max(ds->pair_dmax[p], pow2ceil((int)ri.dim));
      }
    }
  if (ds->n_kprod && (ctx->multi || ctx->multi_rank))
    return fail("spec: product chains and the RQ / LINEAR kinds are not supported on a multi-GPU context");
  if (ds->n_deriv && (ctx->multi || ctx->multi_rank)) return fail(DERIV_REFUSAL_MULTI);
  const size_t terms_off = place(sizeof(DevTerm) * (size_t)std::max(1, nterms));
  // ---- one cached device block, one pinned staging buffer
  char* d_base = (char*)pool_alloc(ctx, total);
  if (!d_base) {
    dspec_free(ds);
    return -2;
  }
  ds->d_bufs.push_back((double*)d_base);
  if (total > ctx->stage_cap) {
    if (ctx->h_stage) hipHostFree(ctx->h_stage);
    ctx->h_stage = nullptr;
    ctx->stage_cap = 0;
    size_t cap = std::max<size_t>(total + total / 2, 1u << 20);
    if (hipHostMalloc((void**)&ctx->h_stage, cap, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      return fail("spec: hipHostMalloc failed (staging buffer)");
    }
    ctx->stage_cap = cap;
  }
  char* h_base = ctx->h_stage;
  // ---- pass 2: fill the staging buffer
  for (int k = 0; k < sp->n_inputs; ++k) {
    const sgp_input& in = sp->inputs[k];
    double* dst = (double*)(h_base + in_off[k]);
    if (in.ld == in.dim) {
      if (in.n > 0) memcpy(dst, in.x, sizeof(double) * (size_t)(in.dim * in.n));
    } else {
      for (long j = 0; j < in.n; ++j) memcpy(dst + j * in.dim, in.x + j * in.ld, sizeof(double) * (size_t)in.dim);
    }
  }
  DevTerm* h_terms = (DevTerm*)(h_base + terms_off);
  for (int I = 0; I < ds->nrb; ++I)
    for (int J = 0; J < ds->ncb; ++J) {
      int p = I * ds->ncb + J;
      // plain | patch | stencil | derivative | product chains within every pair (the caller's order when the spec has none of
      // the last four; chains and the groups of derivative terms stay contiguous and in the caller's order: the passes below
      // are stable)
      auto cls = [&](int t) {
        if (is_kp[t]) return 4;
        if (is_dv[t]) return 3;
        const uint32_t code = (uint32_t)sp->terms[t].reserved;
        if (!code) return 0;
        const uint32_t id = (code & 0xffffu) ? (code & 0xffffu) : (code >> 16);
        return ctx->conv_geoms[id - 1].st > 0 ? 2 : 1;
      };
      std::vector<int> order;
      int ncls[5] = {0, 0, 0, 0, 0};
      for (int pass = 0; pass < 5; ++pass)
        for (int t = sp->term_ptr[p]; t < sp->term_ptr[p + 1]; ++t)
          if (cls(t) == pass) order.push_back(t), ++ncls[pass];
      ds->pair_nplain.push_back(ncls[0]);
      ds->pair_npatch.push_back(ncls[1]);
      ds->pair_nderiv.push_back(ncls[3]);
      ds->pair_nkprod.push_back(ncls[4]);
      for (size_t k = 0; k < order.size(); ++k) {
        const int t = order[k], pos = sp->term_ptr[p] + (int)k;
        const sgp_term& T = sp->terms[t];
        const sgp_input& ri = sp->inputs[T.row_input];
        const sgp_input& ci = sp->inputs[T.col_input];
        DevTerm D;
        D.kind = T.kind;
        D.dim = (int)ri.dim;
        D.ph = D.pw = D.hr = D.wr = D.hc = D.wc = 0;
        D.qr = D.qc = 0;
        D.str = D.stc = nullptr;
        if (cls(t) == 2) {
          const int gr = (int)((uint32_t)T.reserved & 0xffffu), gc = (int)((uint32_t)T.reserved >> 16);
          if (gr) {
            const StencilDesc& sd = ctx->stencils[ctx->conv_geoms[gr - 1].st - 1];
            D.qr = sd.npoints, D.str = sd.dev;
          }
          if (gc) {
            const StencilDesc& sd = ctx->stencils[ctx->conv_geoms[gc - 1].st - 1];
            D.qc = sd.npoints, D.stc = sd.dev;
          }
        } else if (T.reserved) {
          const int gr = (int)((uint32_t)T.reserved & 0xffffu), gc = (int)((uint32_t)T.reserved >> 16);
          const PatchGeom& g = ctx->conv_geoms[(gr ? gr : gc) - 1];
          D.ph = g.ph;
          D.pw = g.pw;
          D.dim = g.ph * g.pw;
          if (gr) D.hr = ctx->conv_geoms[gr - 1].h, D.wr = ctx->conv_geoms[gr - 1].w;
          if (gc) D.hc = ctx->conv_geoms[gc - 1].h, D.wc = ctx->conv_geoms[gc - 1].w;
        }
        D.coef = T.coef;
        D.param = T.param;
        D.xr = (const double*)(d_base + in_off[T.row_input]);
        D.ldr = ri.dim;
        D.xc = (const double*)(d_base + in_off[T.col_input]);
        D.ldc = ci.dim;
        D.rs = nullptr;
        D.cs = nullptr;
        if (rs_len[t]) {
          memcpy(h_base + rs_off[t], T.row_scale, sizeof(double) * (size_t)rs_len[t]);
          D.rs = (const double*)(d_base + rs_off[t]);
        }
        if (cs_len[t]) {
          memcpy(h_base + cs_off[t], T.col_scale, sizeof(double) * (size_t)cs_len[t]);
          D.cs = (const double*)(d_base + cs_off[t]);
        }
        if (nuc_off[t] != (size_t)-1) {
          matern_nu_constants(T.param, (double*)(h_base + nuc_off[t]));
          D.nuc = (const double*)(d_base + nuc_off[t]);
        }
        h_terms[pos] = D;
        ds->h_terms.push_back(D);
        ds->term_src.push_back(t);
        ds->term_row_input.push_back(T.row_input);
        ds->term_col_input.push_back(T.col_input);
      }
    }
  ds->d_terms = (DevTerm*)(d_base + terms_off);
  if (hipMemcpy(d_base, h_base, total, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    return fail("spec: upload failed");
  }
  *out = ds;
  return 0;
}

extern "C" int sgp_dspec_create(sgp_ctx* ctx, const sgp_cov_spec* sp, sgp_dspec** out) {
  CHECK_ARG(ctx && sp && out, "sgp_dspec_create: NULL argument");
  CtxScope scope(ctx);
  return dspec_create(ctx, sp, out);
}

// Internal: caller already holds ds->ctx (or is tearing it down from a failed create).
static void dspec_free(sgp_dspec* ds) {
  if (!ds) return;
  for (double* p : ds->d_bufs) pool_free(ds->ctx, p);
  delete ds;
}

// for the other translation units (f32.hip): the caller holds the context
int sgp_dspec_create_nolock(sgp_ctx* ctx, const sgp_cov_spec* sp, sgp_dspec** out) { return dspec_create(ctx, sp, out); }
void sgp_dspec_free_nolock(sgp_dspec* ds) { dspec_free(ds); }

extern "C" int sgp_dspec_destroy(sgp_dspec* ds) {
  if (!ds) return 0;
  if (tl_ctx == ds->ctx) {  // called from inside an entry point of the same context
    dspec_free(ds);
    return 0;
  }
  CtxScope scope(ds->ctx);
  dspec_free(ds);
  return 0;
}

// which terms of pair p are what (spec_segments.h), from the counts dspec_create fills for every spec
static inline PairSegs pair_segments(const sgp_dspec* ds, int p) {
  return pair_segments(ds->term_ptr.data(), ds->pair_nplain.data(), ds->pair_npatch.data(), ds->pair_nderiv.data(),
                       ds->pair_nkprod.data(), p);
}
// the chain whose head sits at device position t: one past its last factor, and its DMAX
static inline int chain_end(const sgp_dspec* ds, int t, int t1) { return chain_end(ds->h_terms.data(), t, t1); }
static inline int chain_dmax(const sgp_dspec* ds, int t, int e) { return chain_dmax(ds->h_terms.data(), t, e); }

// Assemble the block pairs of `ds` into the matrix whose element (r, c) (global indices,
// optionally shifted by row_shift) lives at Kv[r + row_shift + c*ld], restricted to the
// global tile window [tile_r_lo, tile_r_hi) x [tile_c_lo, tile_c_hi).
static int assemble(const sgp_dspec* ds, double* Kv, long ld, long tile_r_lo, long tile_r_hi,
                    long tile_c_lo, long tile_c_hi, int lower_only, int noise_kind, double sigma2,
                    const double* d_noise_diag, hipStream_t s) {
  AsmLaunch L{Kv, ld, lower_only, noise_kind, sigma2, d_noise_diag};   // the target: once per call
  for (int I = 0; I < ds->nrb; ++I) {
    if (ds->row_len[I] == 0) continue;
    for (int J = 0; J < ds->ncb; ++J) {
      if (ds->col_len[J] == 0) continue;
      if (lower_only && I < J) continue;
      long r0 = ds->row_off[I], nr = ds->row_len[I], c0 = ds->col_off[J], nc = ds->col_len[J];
      long trf = std::max(r0 / TILE, tile_r_lo), trl = std::min((r0 + nr - 1) / TILE + 1, tile_r_hi);
      long tcf = std::max(c0 / TILE, tile_c_lo), tcl = std::min((c0 + nc - 1) / TILE + 1, tile_c_hi);
      if (trf >= trl || tcf >= tcl) continue;
      // the pair's rectangle and tile window: once per pair.  Sigma_y lands in the diagonal blocks of a symmetric matrix
      L.r0 = r0, L.nr = nr, L.c0 = c0, L.nc = nc, L.diag = ds->symmetric && I == J;
      L.r_first = trf, L.c_first = tcf, L.r_cnt = trl - trf, L.c_cnt = tcl - tcf;
      int p = I * ds->ncb + J;
      // plain | patch (conv.hip) | stencil (stencil.hip) | derivative (deriv.hip) | chains (kprod.hip)
      const auto [t0, tp, ts, tk, t1, td] = pair_segments(ds, p);
      int dmax = ds->pair_dmax[p];
      int per = assemble_terms_per_launch(dmax);  // terms per launch: <= 64 KiB of LDS
      L.first = true;
      if (t0 == t1) {   // a pair without terms: zeros (+ Sigma_y)
        CHECK_RC(launch_assemble_block(L, ds->d_terms, 0, 1, s));
        continue;
      }
      for (int t = t0; t < tp; t += per) {
        int cnt = std::min(per, tp - t);
        L.first = t == t0;
        CHECK_RC(launch_assemble_block(L, ds->d_terms + t, cnt, dmax, s));
      }
      for (int t = tp; t < ts; ++t) {
        L.first = t == t0;
        CHECK_RC(launch_assemble_conv(L, ds->h_terms[t], ds->d_terms + t, s));
      }
      for (int t = ts; t < td; ++t) {
        L.first = t == t0;
        CHECK_RC(launch_assemble_stencil(L, ds->h_terms[t], ds->d_terms + t, s));
      }
      for (int t = td; t < tk;) {   // one group per launch: one exponential per point pair for all its terms (deriv.hip)
        const int cnt = deriv_group(ds->h_terms.data(), t, tk);
        L.first = t == t0;
        CHECK_RC(launch_assemble_deriv(L, ds->h_terms.data() + t, ds->d_terms + t, cnt, s));
        t += cnt;
      }
      for (int t = tk; t < t1;) {   // whole chains per launch, as many as fit its LDS (kprod.hip: kprod_group)
        int kdmax = 1;
        const int cnt = kprod_group(ds->h_terms.data(), t, t1, &kdmax);
        L.first = t == t0;
        CHECK_RC(launch_assemble_kprod(L, ds->h_terms.data() + t, ds->d_terms + t, cnt, kdmax, s));
        t += cnt;
      }
    }
  }
  return 0;
}

// ---------------------------------------------------------------------------------------
// blocked Cholesky on the bordered matrix
// ---------------------------------------------------------------------------------------
// X <- X inv(Lkk)' for `rows` (multiple of 128) rows at X: the panel TRSM.
// A product with the explicit inverse W = inv(Lkk) alone is not backward stable -- on the ill-conditioned covariances smooth
// kernels produce it loses 2+ digits against LAPACK dtrsm and can push the Schur complement indefinite -- so the solve is
// panel_solve_kernel: blocked substitution over 16-column blocks, each diagonal solve = inverse product + one refinement
// step; one launch, no inv(Lkk) needed.  (Rounds 2 - 5 kept the explicit-inverse product and a 128-level refinement as
// SGP_REFINE = 0 / 2 A/B modes; removed in round 6.)
// `inv` points at the eight 16x16 inverse diagonal blocks (block c at inv + c * inv_cstride, element [m][k] at
// + k * inv_kstride + m): what potrf_diag just wrote (ctx scratch or a kept copy).
static int solve_rows(sgp_ctx* ctx, double* X, long ldx, long rows, const double* Lkk, long ldl, const double* inv,
                      long inv_cstride, long inv_kstride, hipStream_t s) {
  (void)ctx;
  if (rows <= 0) return 0;
  // (structured models: the 128-row tiles of this block column that are structurally zero are left alone -- the record
  // chol_bordered / the sharded driver set for the matrix or packed panel being factored, gemm_nt.hip: strip_skip_for)
  const StripSkip sk = strip_skip_for(X, ldx);
  return launch_panel_solve(X, ldx, rows, Lkk, ldl, inv, inv_cstride, inv_kstride, s, sk.nz ? &sk : nullptr);
}

// Factor one column panel in place (inner right-looking loop, nb = 128).
// P: m x w, top w x w block is the diagonal block.  d_invstore: optional array that keeps the
// eight 16x16 inverse diagonal blocks of every 128-block (INVD_STRIDE doubles per block, the
// layout potrf_diag writes) for later solves against the factor; else ctx scratch.
// Which fused update + potrf_diag launches a factorisation of `n` columns (or a panel of `n` rows) uses: the
// context's SGP_FUSE_POTRF below SGP_FUSE_MAX_N, nothing from there on unless bit 2 asks for every size.
// `serial`: the factorisation runs without the two-stream look-ahead (every kernel has the chip to itself) -- there
// the fused launches pay at every size: the diagonal block's pivot chain runs under the other tiles of its own
// launch (N = 65536: 1541 -> 1525 ms).
static int fuse_mode(const sgp_ctx* ctx, long n, bool serial = false) {
  if (n < ctx->fuse_max_n || serial) return ctx->fuse_potrf;
  return (ctx->fuse_potrf & 4) ? (ctx->fuse_potrf | 3) : 0;
}
struct FuseScope {   // panel_factor reads ctx->fuse_now; restored on every exit path
  sgp_ctx* c;
  int saved;
  FuseScope(sgp_ctx* c_, int v) : c(c_), saved(c_->fuse_now) { c->fuse_now = v; }
  ~FuseScope() { c->fuse_now = saved; }
};

// first_done: the panel's first diagonal block is already factored -- the trailing update that produced it had
// potrf_diag fused into the workgroup of that tile (ctx->fuse_potrf, gemm_nt.hip: gemm_nt_dma_potrf_kernel).
static int panel_factor(sgp_ctx* ctx, double* P, long ld, long m, long w, long g0, double* d_slots,
                        int* d_info, double* d_invstore, hipStream_t s, bool first_done = false) {
  // Fused inner updates (SGP_FUSE_POTRF bit 0): the K = 128 update with block column j also factors the diagonal
  // block of block column j + 1 in the workgroup that updates it, so the 128-pivot chain runs under the rest of
  // the update instead of after it and one launch per block column disappears.
  const bool fuse = (ctx->fuse_now & 1) != 0;
  bool diag_done = first_done;
  for (long j = 0; j < w; j += TILE) {
    double* D = P + j + j * ld;
    double* invd = d_invstore ? d_invstore + (j / TILE) * INVD_STRIDE : ctx->d_invd;
    if (!diag_done) CHECK_RC(launch_potrf_diag(D, ld, invd, d_slots + j / TILE, d_info, g0 + j, s));
    diag_done = false;
    long mrest = m - j - TILE;
    if (mrest > 0) {
      double* A21 = P + (j + TILE) + j * ld;
      CHECK_RC(solve_rows(ctx, A21, ld, mrest, D, ld, invd, 256, 16, s));  // L21 = A21 * L11^-T
      long wrest = w - j - TILE;
      if (wrest > 0) {
        if (fuse) {
          // the scratch inverse blocks (no d_invstore) are free again: the row solve that read block column j's
          // ran before this launch on the same stream
          double* invn = d_invstore ? d_invstore + (j / TILE + 1) * INVD_STRIDE : ctx->d_invd;
          CHECK_RC(launch_gemm_nt_potrf(A21, ld, P + (j + TILE) + (j + TILE) * ld, ld, mrest, wrest, TILE, 0,
                                        (ctx->fuse_now & 8) ? 1 : 0, invn, d_slots + j / TILE + 1, d_info,
                                        g0 + j + TILE, s));
          diag_done = true;
        } else {
          CHECK_RC(launch_gemm_nt(A21, ld, A21, ld, P + (j + TILE) + (j + TILE) * ld, ld, mrest, wrest, TILE, -1.0, 1.0,
                                  0, 0, 0, s));
        }
      }
    }
  }
  return 0;
}

static double update_flops(long m, long nc, long k) {
  // algorithmic flops of C[lower, m x nc] -= P P': triangle of the square part + rows below
  double sq = (double)k * (double)nc * (double)(nc + 1);
  double below = 2.0 * (double)k * (double)(m - nc) * (double)nc;
  return sq + below;
}

// timed (optional) trailing-update launch
struct FusedDiag {   // the diagonal block a fused trailing update factors: tile (0, 0) of its C
  double* invd;
  double* slot;
  int* info;
  long gcol0;
  int handoff;   // accumulators -> potrf_diag's LDS layout directly (SGP_FUSE_POTRF bit 3)
};
static int launch_update_kernel(const double* P, long ld, double* C, long M, long Nc, long K, hipStream_t s,
                                const FusedDiag* fz) {
  if (fz)
    return launch_gemm_nt_potrf(P, ld, C, ld, M, Nc, K, 1, fz->handoff, fz->invd, fz->slot, fz->info, fz->gcol0, s);
  return launch_gemm_nt_update(P, ld, C, ld, M, Nc, K, s);
}
static int launch_update(sgp_ctx* ctx, const double* P, long ld, double* C, long M, long Nc, long K,
                         hipStream_t s, const FusedDiag* fz = nullptr) {
  if (M <= 0 || Nc <= 0) return 0;
  if (ctx->time_updates) {
    // the context owns both events from the moment they exist (destroyed with the next timed call or the
    // context), whatever happens below
    hipEvent_t e0 = nullptr, e1 = nullptr;
    SGP_HIP(hipEventCreate(&e0));
    ctx->ev.push_back(e0);
    if (hipEventCreate(&e1) != hipSuccess) {
      ctx->ev.pop_back();
      hipEventDestroy(e0);
      set_error("hipEventCreate failed");
      return -2;
    }
    ctx->ev.push_back(e1);
    ctx->ev_flops.push_back(update_flops(M, Nc, K) * ctx->sz_live_fraction(P, ld, C, M, Nc, K));
    SGP_HIP(hipEventRecord(e0, s));
    CHECK_RC(launch_update_kernel(P, ld, C, M, Nc, K, s, fz));
    SGP_HIP(hipEventRecord(e1, s));
    return 0;
  }
  return launch_update_kernel(P, ld, C, M, Nc, K, s, fz);
}

// Middle blocking level: an outer panel of w columns wider than `wmid` is factored as sub-panels of wmid columns, each
// followed by ONE K = wmid update of the panel's remaining columns (lower trapezoid; the next sub-panel's first diagonal
// block fused into it).  The outer trailing updates then run with K = w -- half the C-tile passes per flop of K = w / 2,
// i.e. half the per-tile prologue / epilogue share -- while the shallow K = 128 work stays that of a wmid-wide panel.
static int panel_factor_mid(sgp_ctx* ctx, double* P, long ld, long m, long w, long g0, double* d_slots, int* d_info,
                            double* d_invstore, hipStream_t s, bool first_done, long wmid) {
  if (wmid < TILE || wmid >= w) return panel_factor(ctx, P, ld, m, w, g0, d_slots, d_info, d_invstore, s, first_done);
  // recursive halving down to wmid: the left half, ONE update of the right half with it (K = w / 2), the right half
  const bool fuse_mid = (ctx->fuse_now & 2) != 0;
  const long wl = std::max(wmid, (w / 2 + wmid - 1) / wmid * wmid), c = wl, rest = w - wl;
  CHECK_RC(panel_factor_mid(ctx, P, ld, m, wl, g0, d_slots, d_info, d_invstore, s, first_done, wmid));
  if (rest <= 0) return 0;
  const FusedDiag fz = {d_invstore ? d_invstore + (c / TILE) * INVD_STRIDE : ctx->d_invd, d_slots + c / TILE, d_info,
                        g0 + c, (ctx->fuse_now & 8) ? 1 : 0};
  CHECK_RC(launch_update(ctx, P + c, ld, P + c + c * ld, m - c, rest, wl, s, fuse_mid ? &fz : nullptr));
  return panel_factor_mid(ctx, P + c + c * ld, ld, m - c, rest, g0 + c, d_slots + c / TILE, d_info,
                          d_invstore ? d_invstore + (c / TILE) * INVD_STRIDE : nullptr, s, fuse_mid, wmid);
}

// Which schedule factors n_pad columns (measured on MI355X, profiles/archive/r03_dataflow.md; Matern-5/2, D = 8, whole logpdf):
//   n_pad <  3072            launches (one outer panel; the dataflow chain of 68 us per 128 columns loses to the fused
//                            launches' 62: N = 2048 1.18 vs 1.25 ms)
//   3072 <= n_pad < 24576    dataflow, one workgroup per CU (256 VGPRs: no spills in the chain tasks, and a chain task never
//                            shares its CU with a contraction): N = 4096 2.51 -> 2.41 ms, 8192 7.7 -> 5.1, 16384 32.7 -> 27.8
//   24576 <= n_pad < 65536   dataflow, two workgroups per CU (the contractions are the work): 32768 218.7 -> 204.8 ms
//   n_pad >= 65536           launches, serial schedule with deep outer blocking: the lock-step trailing updates share
//                            every operand k slice through L2, the desynchronised contractions of the dataflow kernel
//                            stream theirs from HBM and the clock pays for it (-11 %, profiles/archive/r03_experiments/)
// SGP_DATAFLOW = 0 / 1 forces never / always; SGP_DF_MIN_N, SGP_DF_MAX_N, SGP_DF_FAT_MAX_N move the limits.
// (Round 4 also measured XCD-affine task queues for the dataflow kernel -- profiles/r04_experiments/dataflow_xcd_queues.md: handing
// a queue's patches to the free workgroups of its XCD does not make them share operand panels, they start their tiles whenever
// they become free; +3.6 % at 32768 columns.  The code was removed in round 6.)
// Hybrid schedule (round 5; the round-4 verdict's item 4): the look-ahead schedule of the launches with every outer PANEL (2048
// columns) factored by ONE launch of the dataflow kernel on the panel -- its diagonal chain and the row solves below it as
// tile tasks with tile-level dependencies (the rows below the panel's diagonal block are that kernel's "bordered rows") --
// while the trailing updates stay lock-step launches of K = 2048 (operand sharing through L2, 0.85 in situ).  The panel
// kernel runs beside the previous panel's trailing update: the chain that the serial-deep schedule pays in full (57 ms at
// N = 65536) and that the launch-based look-ahead ran 2.5 - 3 x slower beside an update (many small dependent launches) is
// hidden.  Same arithmetic order per tile (k ascending): bit-identical.  Measured (profiles/r05_experiments/hybrid.md):
// N = 65536 1454 -> 1395 ms, 32768 197 -> 182 ms, 16384 26.7 -> 28.6 (stays on the dataflow kernel).
// The gradient path's factorisations (`grow`: an identity border rides along, 3 x the flops per column, no whole-matrix
// dataflow form) take it from 16384 columns on: N = 16384 82.2 -> 81.1 ms, 24576 260.8 -> 253.5, 32768 605.8 -> 582.0
// (profiles/r05_experiments/hybrid_grad.txt).
static bool use_hybrid(const sgp_ctx* ctx, long n_pad, bool grow = false) {
  if (ctx->hybrid == 0 || n_pad < 4096) return false;
  if (ctx->hybrid == 1) return true;
  // by size -- unless the caller pinned another schedule (SGP_DATAFLOW = 0 / 1, SGP_LOOKAHEAD = 0)
  return ctx->dataflow < 0 && ctx->lookahead != 0 && n_pad >= (grow ? ctx->hybrid_grow_min_n : ctx->hybrid_min_n);
}
static bool use_dataflow(const sgp_ctx* ctx, long n_pad) {
  if (ctx->dataflow == 0) return false;
  return ctx->dataflow == 1 || (n_pad >= ctx->df_min_n && n_pad < ctx->df_max_n);
}
extern "C" int sgp_ctx_factor_work(sgp_ctx* ctx, double* executed, double* dense) {
  CHECK_ARG(ctx && executed && dense, "sgp_ctx_factor_work: NULL argument");
  if (ctx->multi) return sgp_multi_factor_work(ctx->multi, executed, dense);
  *executed = ctx->sz_executed;
  *dense = ctx->sz_dense;
  return 0;
}
// A block order that keeps the factor sparse (sthenomi.h): greedy minimum fill on the block graph, host only.
extern "C" int sgp_cov_spec_suggest_order(const sgp_cov_spec* sp, int32_t* perm_out, int32_t* changes) {
  CHECK_ARG(sp && perm_out, "sgp_cov_spec_suggest_order: NULL argument");
  CHECK_ARG(sp->symmetric && sp->n_row_blocks == sp->n_col_blocks && sp->n_row_blocks >= 1,
            "sgp_cov_spec_suggest_order: the spec must be symmetric (cov(f, x))");
  const int nb = sp->n_row_blocks;
  std::vector<std::vector<char>> adj((size_t)nb, std::vector<char>((size_t)nb, 0));
  for (int I = 0; I < nb; ++I)
    for (int J = 0; J < nb; ++J) {
      const int p = I * nb + J, q = J * nb + I;
      if (I != J && (sp->term_ptr[p + 1] > sp->term_ptr[p] || sp->term_ptr[q + 1] > sp->term_ptr[q])) adj[(size_t)I][(size_t)J] = 1;
    }
  // weighted fill of eliminating the blocks in a given order (what the order costs: lengths of the block pairs that fill in)
  auto total_fill = [&](const std::vector<int>& order) {
    std::vector<std::vector<char>> a = adj;
    std::vector<char> gone((size_t)nb, 0);
    double fill = 0;
    for (int v : order) {
      for (int x = 0; x < nb; ++x)
        for (int y = x + 1; y < nb; ++y)
          if (!gone[(size_t)x] && !gone[(size_t)y] && x != v && y != v && a[(size_t)v][(size_t)x] && a[(size_t)v][(size_t)y] &&
              !a[(size_t)x][(size_t)y]) {
            a[(size_t)x][(size_t)y] = a[(size_t)y][(size_t)x] = 1;
            fill += (double)sp->row_len[x] * (double)sp->row_len[y];
          }
      gone[(size_t)v] = 1;
    }
    return fill;
  };
  std::vector<std::vector<char>> a = adj;
  std::vector<char> left((size_t)nb, 1);
  std::vector<int> order;
  for (int step = 0; step < nb; ++step) {
    int best = -1;
    double best_fill = 0;
    for (int v = 0; v < nb; ++v) {
      if (!left[(size_t)v]) continue;
      double fill = 0;
      for (int x = 0; x < nb; ++x)
        for (int y = x + 1; y < nb; ++y)
          if (left[(size_t)x] && left[(size_t)y] && x != v && y != v && a[(size_t)v][(size_t)x] && a[(size_t)v][(size_t)y] &&
              !a[(size_t)x][(size_t)y])
            fill += (double)sp->row_len[x] * (double)sp->row_len[y];
      const bool better = best < 0 || fill < best_fill || (fill == best_fill && sp->row_len[v] < sp->row_len[best]);
      if (better) {
        best = v;
        best_fill = fill;
      }
    }
    for (int x = 0; x < nb; ++x)
      for (int y = x + 1; y < nb; ++y)
        if (left[(size_t)x] && left[(size_t)y] && x != best && y != best && a[(size_t)best][(size_t)x] && a[(size_t)best][(size_t)y])
          a[(size_t)x][(size_t)y] = a[(size_t)y][(size_t)x] = 1;
    left[(size_t)best] = 0;
    order.push_back(best);
  }
  for (int k = 0; k < nb; ++k) perm_out[k] = order[(size_t)k];
  if (changes) {
    std::vector<int> ident((size_t)nb);
    for (int k = 0; k < nb; ++k) ident[(size_t)k] = k;
    *changes = total_fill(order) < total_fill(ident) ? 1 : 0;
  }
  return 0;
}
extern "C" const char* sgp_ctx_factor_schedule(sgp_ctx* ctx, int64_t N) {
  if (!ctx || N < 1) return "";
  const long n_pad = rup(N, TILE);
  if (use_hybrid(ctx, n_pad)) return "hybrid";
  if (use_dataflow(ctx, n_pad)) return n_pad < ctx->df_fat_max_n ? "dataflow-fat" : "dataflow";
  const bool la = ctx->lookahead && (n_pad < ctx->la_max_n || ctx->lookahead == 2);
  if (la) return n_pad <= 4096 && ctx->wout <= 0 ? "launches-one-panel" : "launches-lookahead";
  return n_pad >= 65536 ? "launches-serial-deep" : "launches-serial";
}

// Two-level right-looking Cholesky of the bordered matrix with one-panel look-ahead:
// the outer panel J+1 is updated and factored on the (high-priority) panel stream while the
// rest of the trailing matrix is still being updated with panel J on the update stream.
// grow > 0: bordered rows >= n_pad hold a matrix that is upper triangular by tile from row `grow` on
// (the identity rows of the gradient path: row grow + i stays zero left of column i), so panel
// J0..J0+wj only touches rows < grow + J0 + wj.
// The tile-level pattern of the factor of the matrix a caller is about to factor (structural zeros, common.h).
struct SzMask {
  const sz_word* d_nz = nullptr;   // device rows (ctx->d_sz), nullptr: dense
  int words = 0;
};
struct SzScope {   // the launch-based updates read the pattern through gemm_nt.hip's per-thread record
  sgp_ctx* c;
  bool on;
  SzScope(sgp_ctx* ctx, const double* A, long ld, long ncols, const SzMask* sz) : c(ctx), on(sz && sz->d_nz) {
    if (on) {
      gemm_set_structure(A, ld, sz->d_nz, sz->words, ncols);
      c->sz_base = A;
      c->sz_ld = ld;
      c->sz_words = sz->words;
    }
  }
  ~SzScope() {
    if (on) {
      gemm_set_structure(nullptr, 0, nullptr, 0);
      c->sz_base = nullptr;
    }
  }
};

// scratch of a dataflow launch on this context (grow-only): progress words for nb matrices of m_tot rows and -- when the caller
// keeps no inverse diagonal blocks itself -- room for those of inv_cols columns (0: not needed)
// (the state words alone: a ragged pool counts them itself -- df_pool_state_words)
static int df_scratch_state(sgp_ctx* ctx, long need_state, hipStream_t s) {
  if (need_state > ctx->n_df_state) {
    SGP_HIP(hipStreamSynchronize(s));
    if (ctx->d_df_state) hipFree(ctx->d_df_state);
    ctx->d_df_state = nullptr;
    ctx->n_df_state = 0;
    SGP_HIP(hipMalloc(&ctx->d_df_state, sizeof(int) * need_state));
    ctx->n_df_state = need_state;
  }
  return 0;
}
static int df_scratch(sgp_ctx* ctx, long m_tot, int nb, long inv_cols, hipStream_t s) {
  const long need_inv = (inv_cols / TILE) * INVD_STRIDE;
  CHECK_RC(df_scratch_state(ctx, df_state_words(m_tot, nb), s));
  if (need_inv > ctx->n_df_inv) {
    SGP_HIP(hipStreamSynchronize(s));
    if (ctx->d_df_inv) hipFree(ctx->d_df_inv);
    ctx->d_df_inv = nullptr;
    ctx->n_df_inv = 0;
    SGP_HIP(hipMalloc(&ctx->d_df_inv, sizeof(double) * need_inv));
    ctx->n_df_inv = need_inv;
  }
  return 0;
}

// ---- one function per schedule of the blocked Cholesky (round 6: rounds 3 - 5 had grown ONE loop that threaded six booleans --
// hybrid, la, deep, fuse_outer, grow, sz -- through itself); chol_bordered below only chooses.  Every schedule performs the
// same arithmetic per tile (k ascending): the factor is bit-identical whichever runs (tests/test_gpu_dataflow.py).

// (1) the whole bordered factorisation as ONE launch of the dataflow kernel (chol_df.hip): persistent workgroups, tile-level
// dependencies instead of launches, streams and events.  3072 <= n_pad < 24576 by default.
static int chol_dataflow_whole(sgp_ctx* ctx, double* A, long ld, long n_pad, long m_tot, double* d_wall, hipStream_t s,
                               const SzMask* sz) {
  CHECK_RC(df_scratch(ctx, m_tot, 1, d_wall ? 0 : n_pad, s));
  {
    const int fat = n_pad < ctx->df_fat_max_n ? 1 : 0;
    if (getenv("SGP_DF_STATS") && !ctx->d_df_stats)   // + 8 stamps for each of up to 4096 tile columns
      SGP_HIP(hipMalloc(&ctx->d_df_stats, sizeof(long long) * 8 * ((size_t)ctx->df_wgs + 4096)));
    long long* d_cols = ctx->d_df_stats && n_pad / TILE <= 4096 ? ctx->d_df_stats + 8 * (size_t)ctx->df_wgs : nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (ctx->d_df_stats) {
      SGP_HIP(hipEventCreate(&e0));
      SGP_HIP(hipEventCreate(&e1));
      SGP_HIP(hipEventRecord(e0, s));
    }
    CHECK_RC(launch_chol_dataflow(A, ld, n_pad, m_tot, ctx->d_df_state, d_wall ? d_wall : ctx->d_df_inv, ctx->d_slots,
                                  ctx->d_info, ctx->df_wgs, ctx->df_timeout_s, s, ctx->d_df_stats, d_cols, fat,
                                  sz ? sz->d_nz : nullptr, sz ? sz->words : 0));
    if (ctx->d_df_stats) {   // diagnosis only: drains the stream
      hipEventRecord(e1, s);
      hipStreamSynchronize(s);
      float ms = 0;
      hipEventElapsedTime(&ms, e0, e1);
      hipEventDestroy(e0);
      hipEventDestroy(e1);
      std::vector<long long> h((size_t)8 * ctx->df_wgs);
      SGP_HIP(hipMemcpy(h.data(), ctx->d_df_stats, sizeof(long long) * h.size(), hipMemcpyDeviceToHost));
      double sum[8] = {0};
      long nw = 0;
      long off_xcd = 0;
      for (int w = 0; w < ctx->df_wgs; ++w) {
        if (h[(size_t)8 * w + 1] == 0) continue;
        ++nw;
        if ((int)((h[(size_t)8 * w] >> 40) & 15) != (w & 7)) ++off_xcd;   // not on XCD (id % 8)
        h[(size_t)8 * w] &= (1LL << 40) - 1;
        for (int q = 0; q < 8; ++q) sum[q] += (double)h[(size_t)8 * w + q];
      }
      fprintf(stderr, "dataflow: %ld of %ld workgroups NOT on XCD (id %% 8)\n", off_xcd, nw);
      const double us = 0.01 / (double)std::max<long>(nw, 1);   // ticks (100 MHz) -> us, averaged over the workgroups
      fprintf(stderr,
              "dataflow n_pad=%ld m_tot=%ld: %.3f ms, %ld workgroups, %.0f tasks; per workgroup (us): in kernel %.1f | "
              "contraction %.1f (of which waiting %.1f) | wait diag %.1f | potrf %.1f | solve %.1f | publish+dequeue %.1f\n",
              n_pad, m_tot, ms, nw, sum[0], sum[1] * us, sum[2] * us, sum[7] * us, sum[3] * us, sum[4] * us, sum[5] * us,
              sum[6] * us);
      {   // spread over the workgroups: time in the kernel and tasks taken (min / quartiles / max)
        std::vector<double> tk, nt;
        for (int w = 0; w < ctx->df_wgs; ++w)
          if (h[(size_t)8 * w + 1]) {
            tk.push_back((double)h[(size_t)8 * w + 1] * 0.01);
            nt.push_back((double)h[(size_t)8 * w]);
          }
        std::sort(tk.begin(), tk.end());
        std::sort(nt.begin(), nt.end());
        auto q = [](const std::vector<double>& v, double f) { return v.empty() ? 0.0 : v[(size_t)(f * (double)(v.size() - 1))]; };
        fprintf(stderr, "  per workgroup: in kernel (us) min %.0f q1 %.0f median %.0f q3 %.0f max %.0f | tasks min %.0f median %.0f max %.0f\n",
                q(tk, 0), q(tk, 0.25), q(tk, 0.5), q(tk, 0.75), q(tk, 1), q(nt, 0), q(nt, 0.5), q(nt, 1));
      }
      if (d_cols && n_pad / TILE >= 3) {
        const long T = n_pad / TILE;
        std::vector<long long> c((size_t)8 * T);
        SGP_HIP(hipMemcpy(c.data(), d_cols, sizeof(long long) * c.size(), hipMemcpyDeviceToHost));
        // the chain, column j -> j + 1 (averages over the columns, us): diagonal tile published [4] -> the task below
        // sees it [5] -> solved [6] -> published [7] -> next diagonal task sees it [1'] -> last k block done [2'] ->
        // factored [3'] -> published [4']
        double seg[7] = {0};
        long cnt = 0;
        for (long j = 1; j + 2 < T; ++j) {
          const long long* a0 = &c[(size_t)8 * j];
          const long long* a1 = &c[(size_t)8 * (j + 1)];
          if (!a0[4] || !a0[5] || !a0[6] || !a0[7] || !a1[1] || !a1[2] || !a1[3] || !a1[4]) continue;
          seg[0] += (double)(a0[5] - a0[4]);
          seg[1] += (double)(a0[6] - a0[5]);
          seg[2] += (double)(a0[7] - a0[6]);
          seg[3] += (double)(a1[1] - a0[7]);
          seg[4] += (double)(a1[2] - a1[1]);
          seg[5] += (double)(a1[3] - a1[2]);
          seg[6] += (double)(a1[4] - a1[3]);
          ++cnt;
        }
        if (cnt) {
          const double u = 0.01 / (double)cnt;
          fprintf(stderr,
                  "  chain per column (us, %ld columns): diag published -> seen below %.1f | solve %.1f | publish %.1f | -> "
                  "seen by next diag %.1f | last k block %.1f | potrf %.1f | publish %.1f | sum %.1f\n",
                  cnt, seg[0] * u, seg[1] * u, seg[2] * u, seg[3] * u, seg[4] * u, seg[5] * u, seg[6] * u,
                  (seg[0] + seg[1] + seg[2] + seg[3] + seg[4] + seg[5] + seg[6]) * u);
        }
      }
    }
  }
  return 0;
}

// what the two launch-based schedules share: the trailing updates of outer panel [J0, J0 + wj) -- with look-ahead (`la`) the
// next panel's columns on the panel stream s (optionally factoring that panel's first diagonal block in the same launch, fz)
// and the rest on the update stream sB; without it one launch on s
struct OuterSweep {
  sgp_ctx* ctx;
  double* A;
  long ld, n_pad, m_tot, grow;
  hipStream_t s, sB;
  bool la;
  bool rest_pending = false;
  long rows(long J0, long wj) const { return grow > 0 ? std::min(m_tot, grow + J0 + wj) : m_tot; }   // rows panel J0 touches
  int begin() {
    if (!la) return 0;
    // the update stream must see everything enqueued on s so far (assembly)
    SGP_HIP(hipEventRecord(ctx->ev_panel, s));
    SGP_HIP(hipStreamWaitEvent(sB, ctx->ev_panel, 0));
    return 0;
  }
  int updates(long J0, long wj, long WOUT, const FusedDiag* fz) {
    const long c0 = J0 + wj, m_eff = rows(J0, wj);
    const long w1 = std::min(WOUT, n_pad - c0), c1 = c0 + w1;   // the next panel
    if (la) {
      SGP_HIP(hipEventRecord(ctx->ev_panel, s));
      // look-ahead: next panel's columns on the panel stream (after the previous rest update)
      if (rest_pending) SGP_HIP(hipStreamWaitEvent(s, ctx->ev_rest, 0));
      CHECK_RC(launch_update(ctx, A + c0 + J0 * ld, ld, A + c0 + c0 * ld, m_eff - c0, w1, wj, s, fz));
      if (c1 < n_pad) {
        SGP_HIP(hipStreamWaitEvent(sB, ctx->ev_panel, 0));
        CHECK_RC(launch_update(ctx, A + c1 + J0 * ld, ld, A + c1 + c1 * ld, m_eff - c1, n_pad - c1, wj, sB));
        SGP_HIP(hipEventRecord(ctx->ev_rest, sB));
        rest_pending = true;
      }
    } else {
      if (rest_pending) {
        SGP_HIP(hipStreamWaitEvent(s, ctx->ev_rest, 0));
        rest_pending = false;
      }
      CHECK_RC(launch_update(ctx, A + c0 + J0 * ld, ld, A + c0 + c0 * ld, m_eff - c0, n_pad - c0, wj, s, fz));
    }
    return 0;
  }
  int end() {
    if (la && rest_pending) SGP_HIP(hipStreamWaitEvent(s, ctx->ev_rest, 0));
    return 0;
  }
};

// (2) hybrid (round 5; use_hybrid above): the look-ahead schedule of the launches with every outer PANEL (2048 columns) factored
// by ONE launch of the dataflow kernel on the panel -- also for the gradient path's border (`grow`: a panel launch takes the
// rows its panel touches, the identity rows among them as bordered rows; only the few tiles above the identity's diagonal
// inside one panel are multiplied out, or skipped when the caller's pattern covers them).  From 24576 columns on.
static int chol_hybrid(sgp_ctx* ctx, double* A, long ld, long n_pad, long m_tot, double* d_wall, hipStream_t s, long grow,
                       const SzMask* sz) {
  CHECK_RC(df_scratch(ctx, m_tot, 1, d_wall ? 0 : n_pad, s));
  const long WOUT = std::min(ctx->hybrid_w, n_pad);
  // (Round 6 measured panel GROUPS here -- far updates once per G panels with K = G x 2048, near classes every step, the sharded
  // sweep's scheme and the round-5 verdict's item 3: c5 1373 -> 1466 / 1476 / 1472 ms at G = 2 / 3 / 4, bit-identical; the near
  // launches cost more than the deeper far launches save.  profiles/r06_experiments/hybrid_groups.md; removed.)
  // (SGP_HYBRID_SERIAL=1, measurement only: the far updates on the panel stream too -- every kernel has the chip alone)
  OuterSweep sw{ctx, A, ld, n_pad, m_tot, grow, s, ctx->hybrid_serial ? s : ctx->stream2, true};
  CHECK_RC(sw.begin());
  for (long J0 = 0; J0 < n_pad; J0 += WOUT) {
    const long wj = std::min(WOUT, n_pad - J0);
    // the panel as ONE launch of persistent workgroups: its diagonal chain and the row solves below it with tile-level
    // dependencies (the rows below the panel's diagonal block are the kernel's "bordered rows")
    CHECK_RC(launch_chol_dataflow(A + J0 + J0 * ld, ld, wj, sw.rows(J0, wj) - J0, ctx->d_df_state,
                                  (d_wall ? d_wall : ctx->d_df_inv) + (J0 / TILE) * INVD_STRIDE, ctx->d_slots + J0 / TILE,
                                  ctx->d_info, ctx->hybrid_wgs, ctx->df_timeout_s, s, nullptr, nullptr, ctx->hybrid_fat,
                                  sz ? sz->d_nz : nullptr, sz ? sz->words : 0, J0));
    if (J0 + wj >= n_pad) break;
    CHECK_RC(sw.updates(J0, wj, WOUT, nullptr));   // (the dataflow panel factors its own first block: nothing fused)
  }
  return sw.end();
}

// (3) launches: the two-level right-looking schedule of rounds 1 - 3 -- n_pad < 3072, and whenever the other two are switched
// off (SGP_DATAFLOW=0 SGP_HYBRID=0: the dataflow time-out fallback, the A/B tests).
//   outer panel width, measured (profiles/archive/r02_summary.md): one panel for n_pad <= 4096 (the outer level only adds
//   launches there: 1.52 -> 1.30 ms at N = 2048), 1024 up to 8192, 512 in the mid range where the panel stream is the
//   critical path (N = 16384: 34.8 vs 35.4 ms), 1024 from 32768 on (halves the C-tile traffic per flop of the big updates);
//   look-ahead below 65536 columns only (la_max_n): at N = 65536 the overlap hides ~70 ms of panel chain but the sharing costs
//   the trailing updates as much; SGP_LOOKAHEAD=2: look-ahead at every size;
//   serial-deep at n_pad >= 65536 (round 3): outer panels of 4096 columns factored by recursive halving down to 1024
//   (panel_factor_mid) -- the big trailing updates run with K = 4096, the mid updates with K = 2048 / 1024;
//   SGP_FUSE_POTRF bit 1: the trailing update that finishes the next panel's first diagonal block factors that block in the
//   same launch, below 32768 columns where the panel chain is the critical path (fuse_max_n; bit 2: at every size).
static int chol_launches(sgp_ctx* ctx, double* A, long ld, long n_pad, long m_tot, double* d_wall, hipStream_t s, long grow) {
  const bool la = ctx->lookahead && s == ctx->stream && (n_pad < ctx->la_max_n || ctx->lookahead == 2);
  const bool deep = !la && n_pad >= 65536;
  const long WOUT = ctx->wout > 0 ? ctx->wout
                    : n_pad <= 4096 ? n_pad
                    : n_pad <= 8192 ? WOUT_LARGE
                    : deep ? 4 * WOUT_LARGE
                    : n_pad >= 32768 ? WOUT_LARGE
                                     : WOUT_SMALL;
  const long WMID = ctx->wmid > 0 ? ctx->wmid : (deep && ctx->wout <= 0 ? WOUT_LARGE : 0);
  FuseScope fuse_scope(ctx, fuse_mode(ctx, n_pad, !la));
  const bool fuse_outer = (ctx->fuse_now & 2) != 0;
  OuterSweep sw{ctx, A, ld, n_pad, m_tot, grow, s, la ? ctx->stream2 : s, la};
  CHECK_RC(sw.begin());
  bool first_done = false;
  for (long J0 = 0; J0 < n_pad; J0 += WOUT) {
    const long wj = std::min(WOUT, n_pad - J0);
    CHECK_RC(panel_factor_mid(ctx, A + J0 + J0 * ld, ld, sw.rows(J0, wj) - J0, wj, J0, ctx->d_slots + J0 / TILE, ctx->d_info,
                              d_wall ? d_wall + (J0 / TILE) * INVD_STRIDE : nullptr, s, first_done, WMID));
    const long c0 = J0 + wj;
    if (c0 >= n_pad) break;
    const FusedDiag fz_next = {d_wall ? d_wall + (c0 / TILE) * INVD_STRIDE : ctx->d_invd, ctx->d_slots + c0 / TILE,
                               ctx->d_info, c0, (ctx->fuse_now & 8) ? 1 : 0};
    first_done = fuse_outer;
    CHECK_RC(sw.updates(J0, wj, WOUT, fuse_outer ? &fz_next : nullptr));
  }
  return sw.end();
}

// The dispatcher.  grow > 0 (the gradient path): bordered rows >= n_pad hold a matrix that is upper triangular by tile from row
// `grow` on (the identity rows: row grow + i stays zero left of column i), so panel J0 .. J0 + wj only touches rows
// < grow + J0 + wj; its pattern (sz) covers the identity rows (sz_pattern's grad_border form).
static int chol_bordered(sgp_ctx* ctx, double* A, long ld, long n_pad, long m_tot, double* d_wall,
                         hipStream_t s, long grow = 0, const SzMask* sz = nullptr) {
  CHECK_ARG(n_pad / TILE <= ctx->n_slots, "matrix too large for the logdet slot buffer");
  SzScope sz_scope(ctx, A, ld, n_pad, sz);
  const bool hybrid = s == ctx->stream && use_hybrid(ctx, n_pad, grow != 0);
  if (!hybrid && grow == 0 && use_dataflow(ctx, n_pad)) return chol_dataflow_whole(ctx, A, ld, n_pad, m_tot, d_wall, s, sz);
  // the launch-based updates read the pattern through gemm_nt.hip's per-thread record; the compacted id maps of consecutive
  // structured launches of ONE stream may share a scratch buffer, the update stream of a look-ahead gets a map of its own
  if (sz_scope.on && s == ctx->stream) {
    const bool two = hybrid || (ctx->lookahead && (n_pad < ctx->la_max_n || ctx->lookahead == 2));
    gemm_set_structure(A, ld, sz->d_nz, sz->words, n_pad, ctx->d_szmap, ctx->n_szmap / 2, 0, two ? ctx->stream2 : nullptr,
                       two ? ctx->d_szmap + ctx->n_szmap / 2 : nullptr);
  }
  if (hybrid) return chol_hybrid(ctx, A, ld, n_pad, m_tot, d_wall, s, grow, sz);
  return chol_launches(ctx, A, ld, n_pad, m_tot, d_wall, s, grow);
}

// K + Sigma_y (lower tiles), identity padding, bordered rows
// Structural zeros: the tile pattern of the factor of K + Sigma_y for a symmetric spec.
//   block level : block pair (I, J) has terms, or not (flatten.py emits none for independent processes: exact zeros)
//   tile level  : tile (ti, tj) of the matrix is non-zero when some block pair it overlaps has terms; diagonal tiles always
//                 (noise, identity padding); the bordered rows (y - m, extra right-hand sides) are dense
//   factor      : symbolic factorisation, column by column -- tile (i, j) fills in when rows i and j share a non-zero
//                 tile in an earlier column
// Nothing is returned (dense) for one block, dense noise, or a pattern without zeros.  Also counts the k-block products of
// the contractions with and without the skipping (ctx->sz_executed / sz_dense: what the bench lines report).
// sz_pattern: the host part (ctx->h_sz, ctx->sz_executed / sz_dense); returns the words per row through *words, 0 = dense.
// grad_border (round 5): the matrix is the gradient path's [K ; (y - m)' ; I] (m_tot = 2 n_pad + 128: logpdf_grad_core) -- the
// identity rows get their own pattern (sz_symbolic: border_identity), and T_c more rows follow the T_r factor rows: row
// T_r + t = the tiles (t, .) of K itself that overlap a block pair with terms (+ the diagonal), i.e. the tiles of
// G = (alpha alpha' - C^-1) / 2 the contractions with the kernel derivatives read (TileSkip::need0).
static int sz_pattern(sgp_ctx* ctx, const sgp_dspec* ds, int noise_kind, long n_pad, long m_tot, int* words,
                      bool grad_border = false) {
  *words = 0;
  const long T_c = n_pad / TILE, T_r = m_tot / TILE;
  double dense = 0;
  for (long j = 0; j < T_c; ++j) dense += (double)j * (double)(T_r - j);
  if (grad_border) {
    // the dense count of the gradient's border: an identity row q only ever holds tiles at columns >= q, so column j sees
    // j - q of its k tiles (q < j) -- j (T_c - j) for the rows of K, j for the observation row, j (j + 1) / 2 for the identity rows
    if (T_r != 2 * T_c + 1) return 0;
    dense = 0;
    for (long j = 0; j < T_c; ++j) dense += (double)j * (double)(T_c - j) + (double)j + 0.5 * (double)j * (double)(j + 1);
  }
  ctx->sz_dense = ctx->sz_executed = dense;
  if (!ctx->struct_zeros || !ds->symmetric || noise_kind == SGP_NOISE_DENSE || ds->nrb < 2 || ds->nrb != ds->ncb) return 0;
  const int nb = ds->nrb;
  std::vector<char> bnz((size_t)nb * nb, 0);
  bool any_zero = false;
  for (int I = 0; I < nb; ++I)
    for (int J = 0; J < nb; ++J) {
      const int p = I * nb + J, q = J * nb + I;
      const bool has = ds->term_ptr[p + 1] > ds->term_ptr[p] || ds->term_ptr[q + 1] > ds->term_ptr[q];
      bnz[(size_t)I * nb + J] = has ? 1 : 0;
      if (!has && ds->row_len[I] > 0 && ds->row_len[J] > 0) any_zero = true;
    }
  if (!any_zero) return 0;
  SzPattern pat;   // sz_pattern.h: host-only, checked on the CPU by tests/sz_pattern_host.cpp
  sz_symbolic(bnz, nb, ds->row_off, ds->row_len, ds->N, TILE, T_c, T_r, pat, grad_border);
  if (grad_border) ctx->sz_dense = dense = pat.dense;
  ctx->sz_executed = pat.zeros_left ? pat.executed : dense;
  if (!pat.zeros_left) return 0;
  if (grad_border) {   // the needed result tiles: K's own (unfilled) tile pattern
    const int W = pat.words;
    std::vector<sz_pattern_word> need((size_t)T_c * W, 0);
    for (long i = 0; i < T_c; ++i) {
      const long p0 = i * TILE, p1 = std::min<long>(p0 + TILE, ds->N);
      for (long k = 0; k <= i; ++k) {
        const long q0 = k * TILE, q1 = std::min<long>(q0 + TILE, ds->N);
        bool on = i == k;
        for (int I = 0; I < nb && !on; ++I) {
          if (ds->row_len[I] <= 0 || !(ds->row_off[I] < p1 && ds->row_off[I] + ds->row_len[I] > p0)) continue;
          for (int J = 0; J < nb && !on; ++J)
            on = ds->row_len[J] > 0 && ds->row_off[J] < q1 && ds->row_off[J] + ds->row_len[J] > q0 && bnz[(size_t)I * nb + J] != 0;
        }
        if (on) need[(size_t)i * W + (k >> 6)] |= (sz_pattern_word)1 << (k & 63);
      }
    }
    pat.nz.insert(pat.nz.end(), need.begin(), need.end());
  }
  ctx->h_sz.swap(pat.nz);
  *words = pat.words;
  return 0;
}

// Per tile column of the factor of K + Sigma_y: the executed tile products of its contractions (SzPattern::col_work), from
// the HOST spec -- what multi.hip prices the column panels with before it deals them out to the ranks (own_table.h).  Empty:
// the model is structurally dense (one block, dense noise, no zero block pair, skipping switched off).
int sgp::drv_sz_col_work(const sgp_ctx* ctx, const sgp_cov_spec* sp, int noise_kind, long n_pad, long m_tot,
                         std::vector<double>& col_work) {
  col_work.clear();
  if (!ctx->struct_zeros || !sp || !sp->symmetric || noise_kind == SGP_NOISE_DENSE || sp->n_row_blocks < 2 ||
      sp->n_row_blocks != sp->n_col_blocks)
    return 0;
  const int nb = sp->n_row_blocks;
  std::vector<long> len((size_t)nb), off((size_t)nb);
  long N = 0;
  for (int I = 0; I < nb; ++I) {
    len[(size_t)I] = (long)sp->row_len[I];
    off[(size_t)I] = N;
    N += len[(size_t)I];
  }
  std::vector<char> bnz((size_t)nb * nb, 0);
  bool any_zero = false;
  for (int I = 0; I < nb; ++I)
    for (int J = 0; J < nb; ++J) {
      const int p = I * nb + J, q = J * nb + I;
      const bool has = sp->term_ptr[p + 1] > sp->term_ptr[p] || sp->term_ptr[q + 1] > sp->term_ptr[q];
      bnz[(size_t)I * nb + J] = has ? 1 : 0;
      if (!has && len[(size_t)I] > 0 && len[(size_t)J] > 0) any_zero = true;
    }
  if (!any_zero) return 0;
  SzPattern pat;
  sz_symbolic(bnz, nb, off, len, N, TILE, n_pad / TILE, m_tot / TILE, pat);
  if (pat.zeros_left) col_work.swap(pat.col_work);
  return 0;
}

// the device copy of a pattern (`h`: rows x words, possibly another context's -- the ranks of a multi-GPU context share one)
// (the words alone, into ctx->d_sz: a pooled launch stages the border patterns of its members in one copy)
static int sz_stage(sgp_ctx* ctx, const std::vector<sz_word>& h, hipStream_t s) {
  if (h.size() > ctx->n_sz) {
    SGP_HIP(hipStreamSynchronize(s));
    if (ctx->d_sz) hipFree(ctx->d_sz);
    ctx->d_sz = nullptr;
    ctx->n_sz = 0;
    SGP_HIP(hipMalloc(&ctx->d_sz, sizeof(sz_word) * h.size()));
    ctx->n_sz = h.size();
  }
  // `h` is pageable and the next call swaps / frees it (in a multi-GPU context every rank copies out of rank 0's): it is staged
  // through a pinned buffer of the context, so the copy is asynchronous AND safe (advisor, round 4: the pageable source; round
  // 5: the stream synchronisation that fixed it stalled the host enqueue of every structured logpdf / gradient call).  The
  // staging buffer is reused only after the previous copy out of it has completed (ev_sz: long done by then).
  const size_t bytes = sizeof(sz_word) * h.size();
  if (!ctx->ev_sz) SGP_HIP(hipEventCreateWithFlags(&ctx->ev_sz, hipEventDisableTiming));
  else SGP_HIP(hipEventSynchronize(ctx->ev_sz));
  if (bytes > ctx->n_sz_pin) {
    if (ctx->h_sz_pin) hipHostFree(ctx->h_sz_pin);
    ctx->h_sz_pin = nullptr;
    ctx->n_sz_pin = 0;
    SGP_HIP(hipHostMalloc((void**)&ctx->h_sz_pin, bytes + bytes / 2, hipHostMallocDefault));
    ctx->n_sz_pin = bytes + bytes / 2;
  }
  std::memcpy(ctx->h_sz_pin, h.data(), bytes);
  SGP_HIP(hipMemcpyAsync(ctx->d_sz, ctx->h_sz_pin, bytes, hipMemcpyHostToDevice, s));
  SGP_HIP(hipEventRecord(ctx->ev_sz, s));
  return 0;
}
static int sz_upload(sgp_ctx* ctx, const std::vector<sz_word>& h, int words, hipStream_t s, SzMask* out) {
  *out = SzMask();
  if (words <= 0 || h.empty()) return 0;
  CHECK_RC(sz_stage(ctx, h, s));
  {   // room for the id map of the largest lower update this matrix can see
    const long rows = (long)(h.size() / (size_t)words);
    const long half = 16 + 8 * tri_ids_per_xcd(tri_shape(rows, std::min<long>(rows, (long)words * 64), -1));
    const long need = 2 * half;   // two maps: the look-ahead schedules launch structured updates on two streams
    if (need > ctx->n_szmap) {
      SGP_HIP(hipStreamSynchronize(s));
      if (ctx->d_szmap) hipFree(ctx->d_szmap);
      ctx->d_szmap = nullptr;
      ctx->n_szmap = 0;
      SGP_HIP(hipMalloc(&ctx->d_szmap, sizeof(int) * need));
      ctx->n_szmap = need;
    }
  }
  out->d_nz = ctx->d_sz;
  out->words = words;
  return 0;
}
static int sz_build(sgp_ctx* ctx, const sgp_dspec* ds, int noise_kind, long n_pad, long m_tot, hipStream_t s, SzMask* out) {
  *out = SzMask();
  int words = 0;
  CHECK_RC(sz_pattern(ctx, ds, noise_kind, n_pad, m_tot, &words));
  return sz_upload(ctx, ctx->h_sz, words, s, out);
}
static int build_bordered(sgp_ctx* ctx, const sgp_dspec* ds, double* dA, long n_pad, long m_tot,
                          const double* d_mean, int noise_kind, double sigma2,
                          const double* d_noise, const double* d_dense, long ld_dense,
                          const double* d_Y, long ldy, long ncols, hipStream_t s, SzMask* sz = nullptr) {
  long N = ds->N;
  if (sz) CHECK_RC(sz_build(ctx, ds, noise_kind, n_pad, m_tot, s, sz));
  int nk = noise_kind == SGP_NOISE_DENSE ? -1 : noise_kind;
  CHECK_RC(assemble(ds, dA, m_tot, 0, n_pad / TILE, 0, n_pad / TILE, 1, nk, sigma2, d_noise, s));
  if (noise_kind == SGP_NOISE_DENSE) CHECK_RC(launch_add_dense(dA, m_tot, d_dense, ld_dense, N, 1, s));
  CHECK_RC(launch_fill_pad(dA, m_tot, N, n_pad, 0, n_pad, m_tot, 0, s));
  CHECK_RC(launch_border_rows(dA, m_tot, n_pad, N, 0, n_pad, d_Y, ldy, ncols, d_mean, s));
  return 0;
}

static int fetch_info(sgp_ctx* ctx, hipStream_t s) {
  int info = 0;
  SGP_HIP(hipMemcpyAsync(&info, ctx->d_info, sizeof(int), hipMemcpyDeviceToHost, s));
  SGP_HIP(hipStreamSynchronize(s));
  if (info == SGP_DF_TIMEOUT) {
    ctx->df_timed_out = true;   // the entry point reruns the operator on the launch-based schedule (with_df_fallback)
    set_error("dataflow factorisation: a dependency wait inside the kernel ran into its bound (SGP_DF_TIMEOUT_S)");
  }
  return info;
}

static int dev_logpdf_impl(sgp_ctx* ctx, const sgp_dspec* ds, double* dA, const double* d_mean,
                           int noise_kind, double sigma2, const double* d_noise,
                           const double* d_dense, long ld_dense, const double* d_Y, long ldy,
                           long ncols, double* out_host, double* timings) {
  CHECK_ARG(ds->symmetric, "logpdf: spec must be symmetric");
  CHECK_ARG(ncols >= 1 && ncols + 16 <= ctx->n_scal, "logpdf: bad number of columns");
  hipStream_t s = ctx->stream;
  long N = ds->N;
  int64_t n_pad, m_tot;
  sgp_geometry(N, ncols, &n_pad, &m_tot);
  struct StageEvents {   // destroyed on every exit path
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    ~StageEvents() {
      for (auto x : e)
        if (x) hipEventDestroy(x);
    }
  } stage_events;
  hipEvent_t* ev = stage_events.e;
  if (timings)
    for (int q = 0; q < 4; ++q) SGP_HIP(hipEventCreate(&ev[q]));
  SGP_HIP(hipMemsetAsync(ctx->d_info, 0, sizeof(int), s));
  if (timings) SGP_HIP(hipEventRecord(ev[0], s));
  SzMask sz;
  CHECK_RC(build_bordered(ctx, ds, dA, n_pad, m_tot, d_mean, noise_kind, sigma2, d_noise, d_dense,
                          ld_dense, d_Y, ldy, ncols, s, &sz));
  if (timings) SGP_HIP(hipEventRecord(ev[1], s));
  ctx->time_updates = timings != nullptr;
  for (auto e : ctx->ev) hipEventDestroy(e);
  ctx->ev.clear();
  ctx->ev_flops.clear();
  int rc = chol_bordered(ctx, dA, m_tot, n_pad, m_tot, nullptr, s, 0, &sz);
  ctx->time_updates = false;
  if (rc) return rc;
  if (timings) SGP_HIP(hipEventRecord(ev[2], s));
  double* d_logdet = ctx->d_scal;
  double* d_sq = ctx->d_scal + 16;
  double* d_out = ctx->d_scal + 16 + ncols;
  CHECK_ARG(16 + 2 * ncols <= ctx->n_scal, "logpdf: too many columns");
  CHECK_RC(launch_rowsumsq(dA + n_pad, m_tot, N, ncols, d_sq, 0, s));
  CHECK_RC(launch_sum_array(ctx->d_slots, n_pad / TILE, d_logdet, s));
  CHECK_RC(launch_logpdf_final(d_logdet, d_sq, N, ncols, d_out, s));
  if (timings) SGP_HIP(hipEventRecord(ev[3], s));
  SGP_HIP(hipMemcpyAsync(out_host, d_out, sizeof(double) * ncols, hipMemcpyDeviceToHost, s));
  int info = fetch_info(ctx, s);
  if (timings) {
    float a = 0, b = 0, c = 0;
    SGP_HIP(hipEventElapsedTime(&a, ev[0], ev[1]));
    SGP_HIP(hipEventElapsedTime(&b, ev[1], ev[2]));
    SGP_HIP(hipEventElapsedTime(&c, ev[2], ev[3]));
    timings[0] = a;
    timings[1] = b;
    timings[2] = c;
    double ms_sum = 0, fl = 0;
    for (size_t i = 0; i + 1 < ctx->ev.size(); i += 2) {
      float ms = 0;
      SGP_HIP(hipEventElapsedTime(&ms, ctx->ev[i], ctx->ev[i + 1]));
      ms_sum += ms;
      fl += ctx->ev_flops[i / 2];
    }
    timings[3] = ms_sum;
    timings[4] = (double)(ctx->ev.size() / 2);
    timings[5] = fl;
    // the look-ahead runs update launches of two streams concurrently, so their durations overlap:
    // [6] = length of the union of the launch intervals (ms), the time the kernel was on the chip
    {
      std::vector<std::pair<float, float>> iv;
      for (size_t i = 0; i + 1 < ctx->ev.size(); i += 2) {
        float t0 = 0, t1 = 0;
        SGP_HIP(hipEventElapsedTime(&t0, ev[0], ctx->ev[i]));
        SGP_HIP(hipEventElapsedTime(&t1, ev[0], ctx->ev[i + 1]));
        iv.emplace_back(t0, t1);
      }
      std::sort(iv.begin(), iv.end());
      double uni = 0;
      if (!iv.empty()) {
        float cs = iv[0].first, ce = iv[0].second;
        for (size_t i = 1; i < iv.size(); ++i) {
          if (iv[i].first > ce) {
            uni += ce - cs;
            cs = iv[i].first;
            ce = iv[i].second;
          } else {
            ce = std::max(ce, iv[i].second);
          }
        }
        uni += ce - cs;
      }
      timings[6] = uni;
      timings[7] = 0.0;
    }
  }
  if (info < 0) return -3;
  if (info > 0) {
    set_error("matrix is not positive definite; Cholesky factorization failed at leading minor " +
              std::to_string(info));
    return info;
  }
  return 0;
}

// The dataflow kernel bounds every inter-workgroup wait by WALL-CLOCK time (SGP_DF_TIMEOUT_S): if the queue is preempted or
// time-sliced (another process on the GPU, a profiler serialising kernels) producers can be descheduled while the clock
// runs, and the kernel aborts although nothing is wrong (advisor, round 3).  An operator that comes back with that
// timeout is therefore run again, once, on the launch-based schedule -- every operator rebuilds its matrix from the spec,
// and every schedule gives the same bits, so the caller sees the result it would have seen, only later.
template <class F>
static int with_df_fallback(sgp_ctx* ctx, F&& run) {
  // the flag reset, the operator and its rerun are ONE critical section of the context (advisor, round 4: two host threads
  // on one context could erase each other's timeout flag, and the temporary dataflow = 0 leaked into the other's schedule)
  std::unique_lock<std::recursive_mutex> hold;
  if (ctx) hold = std::unique_lock<std::recursive_mutex>(ctx->mu);
  if (ctx) ctx->df_timed_out = false;
  int rc = run();
  if (ctx && rc == -3 && ctx->df_timed_out && ctx->df_fallback) {
    const int keep = ctx->dataflow, keep_h = ctx->hybrid;
    ctx->dataflow = 0;
    ctx->hybrid = 0;
    ctx->df_timed_out = false;
    ctx->df_fallbacks += 1;
    rc = run();
    ctx->dataflow = keep;
    ctx->hybrid = keep_h;
  }
  return rc;
}

static int sgp_dev_logpdf_impl(sgp_ctx* ctx, const sgp_dspec* ds, double* d_A, const double* d_mean,
                              int noise_kind, const double* noise_host, const double* d_noise,
                              const double* d_Y, int64_t ldy, int64_t ncols, double* out_host,
                              double* timings) {
  CHECK_ARG(ctx && ds && d_A && d_Y && out_host, "sgp_dev_logpdf: NULL argument");
  CHECK_ARG(noise_kind == SGP_NOISE_SCALAR || noise_kind == SGP_NOISE_DIAG,
            "sgp_dev_logpdf: noise kind must be SCALAR or DIAG");
  CtxScope scope(ctx);
  double s2 = noise_host ? noise_host[0] : 0.0;
  return dev_logpdf_impl(ctx, ds, d_A, d_mean, noise_kind, s2, d_noise, nullptr, 0, d_Y, ldy, ncols,
                         out_host, timings);
}
extern "C" int sgp_dev_logpdf(sgp_ctx* ctx, const sgp_dspec* ds, double* d_A, const double* d_mean,
                              int noise_kind, const double* noise_host, const double* d_noise,
                              const double* d_Y, int64_t ldy, int64_t ncols, double* out_host,
                              double* timings) {
  return with_df_fallback(ctx, [&]() { return sgp_dev_logpdf_impl(ctx, ds, d_A, d_mean, noise_kind, noise_host, d_noise, d_Y, ldy, ncols, out_host, timings); });
}

// ---------------------------------------------------------------------------------------
// host-buffer helpers
// ---------------------------------------------------------------------------------------
static int upload_matrix(DevBuf& b, const double* h, long ldh, long nr, long nc) {
  CHECK_RC(b.alloc((size_t)nr * nc));
  if (nr && nc &&
      hipMemcpy2D(b.p, sizeof(double) * nr, h, sizeof(double) * ldh, sizeof(double) * nr, (size_t)nc,
                  hipMemcpyHostToDevice) != hipSuccess) {
    set_error("hipMemcpy2D H2D failed");
    return -2;
  }
  return 0;
}

struct NoiseDev {
  int kind = SGP_NOISE_SCALAR;
  double sigma2 = 0.0;
  DevBuf diag, dense;
  long ld_dense = 0;
};
static int upload_noise(NoiseDev& nd, int kind, const double* noise, long N) {
  CHECK_ARG(noise != nullptr, "noise is NULL");
  CHECK_ARG(kind >= SGP_NOISE_SCALAR && kind <= SGP_NOISE_DENSE, "bad noise kind");
  nd.kind = kind;
  if (kind == SGP_NOISE_SCALAR) nd.sigma2 = noise[0];
  if (kind == SGP_NOISE_DIAG) CHECK_RC(nd.diag.upload(noise, N));
  if (kind == SGP_NOISE_DENSE) {
    CHECK_RC(nd.dense.upload(noise, (size_t)N * N));
    nd.ld_dense = N;
  }
  return 0;
}

extern "C" int sgp_kernelmatrix(sgp_ctx* ctx, const sgp_cov_spec* spec, double* K, int64_t ldk) {
  CHECK_ARG(ctx && spec && K, "sgp_kernelmatrix: NULL argument");
  CtxScope scope(ctx);
  REFUSE_KPROD_MULTI(ctx, spec);
  if (ctx->multi) return sgp_multi_kernelmatrix(ctx, spec, K, ldk);
  SpecGuard g;
  CHECK_RC(dspec_create(ctx, spec, &g.ds));
  long N = g.ds->N, M = g.ds->M;
  CHECK_ARG(ldk >= N, "sgp_kernelmatrix: ldk < N");
  if (N == 0 || M == 0) return 0;
  DevBuf dK;
  CHECK_RC(dK.alloc((size_t)N * M));
  hipStream_t s = ctx->stream;
  CHECK_RC(assemble(g.ds, dK.p, N, 0, rup(N, TILE) / TILE, 0, rup(M, TILE) / TILE, g.ds->symmetric, -1, 0.0,
                    nullptr, s));
  if (g.ds->symmetric) CHECK_RC(launch_mirror_lower(dK.p, N, N, s));
  SGP_HIP(hipStreamSynchronize(s));
  SGP_HIP(hipMemcpy2D(K, sizeof(double) * ldk, dK.p, sizeof(double) * N, sizeof(double) * N, (size_t)M,
                      hipMemcpyDeviceToHost));
  return 0;
}

static int diag_of_spec(sgp_ctx* ctx, const sgp_dspec* ds, double* d_out, hipStream_t s) {
  CHECK_ARG(ds->nrb == ds->ncb, "kernelmatrix_diag: row / col block counts differ");
  for (int I = 0; I < ds->nrb; ++I) {
    CHECK_ARG(ds->row_len[I] == ds->col_len[I], "kernelmatrix_diag: block lengths differ");
    int p = I * ds->ncb + I;
    const auto [t0, tp, ts, tk, t1, td] = pair_segments(ds, p);
    if (tp < ts) {   // patch terms (conv.hip), in one launch with the plain terms in front of them
      int max_d = 1, d_all = -1, max_px = 1;
      for (int t = tp; t < ts; ++t) {
        const DevTerm& T = ds->h_terms[t];
        max_d = std::max(max_d, T.dim);
        d_all = (d_all < 0 || d_all == T.dim) ? T.dim : 0;
        max_px = std::max(max_px, T.hr * T.wr + T.hc * T.wc);
      }
      CHECK_RC(launch_diag_conv(d_out + ds->row_off[I], ds->row_len[I], ds->d_terms + t0, tp - t0, ts - t0, max_d, d_all, max_px,
                                s));
    } else {
      CHECK_RC(launch_diag_terms(d_out + ds->row_off[I], ds->row_len[I], ds->d_terms + t0, ts - t0, s));
    }
    if (ts < td) {        // stencil terms (stencil.hip), added onto the plain and patch diagonal
      int max_dim = 1;
      for (int t = ts; t < td; ++t) max_dim = std::max(max_dim, ds->h_terms[t].dim);
      CHECK_RC(launch_diag_stencil(d_out + ds->row_off[I], ds->row_len[I], ds->d_terms + ts, td - ts, max_dim, s));
    }
    for (int t = td; t < tk;) {   // derivative terms, in the groups of the matrix assembly: the same sums
      const int cnt = deriv_group(ds->h_terms.data(), t, tk);
      CHECK_RC(launch_diag_deriv(d_out + ds->row_off[I], ds->row_len[I], ds->h_terms.data() + t, ds->d_terms + t, cnt, 1, s));
      t += cnt;
    }
    for (int t = tk; t < t1;) {   // product chains, in the launch groups of the matrix assembly: the same sums
      int kdmax = 1;
      const int cnt = kprod_group(ds->h_terms.data(), t, t1, &kdmax);
      CHECK_RC(launch_diag_kprod(d_out + ds->row_off[I], ds->row_len[I], ds->h_terms.data() + t, ds->d_terms + t, cnt, 1, s));
      t += cnt;
    }
  }
  return 0;
}

extern "C" int sgp_kernelmatrix_diag(sgp_ctx* ctx, const sgp_cov_spec* spec, double* out) {
  CHECK_ARG(ctx && spec && out, "sgp_kernelmatrix_diag: NULL argument");
  CtxScope scope(ctx);
  REFUSE_KPROD_MULTI(ctx, spec);
  if (ctx->multi) return sgp_multi_kernelmatrix_diag(ctx, spec, out);
  SpecGuard g;
  CHECK_RC(dspec_create(ctx, spec, &g.ds));
  long N = g.ds->N;
  if (N == 0) return 0;
  DevBuf d;
  CHECK_RC(d.alloc(N));
  CHECK_RC(diag_of_spec(ctx, g.ds, d.p, ctx->stream));
  SGP_HIP(hipStreamSynchronize(ctx->stream));
  SGP_HIP(hipMemcpy(out, d.p, sizeof(double) * N, hipMemcpyDeviceToHost));
  return 0;
}

static int sgp_logpdf_impl(sgp_ctx* ctx, const sgp_cov_spec* spec, const double* mean, int noise_kind,
                          const double* noise, const double* Y, int64_t ldy, int64_t ncols,
                          double* out) {
  CHECK_ARG(ctx && spec && Y && out, "sgp_logpdf: NULL argument");
  CHECK_ARG(spec->symmetric, "sgp_logpdf: spec must be symmetric");
  CtxScope scope(ctx);
  // a multi-GPU context (sgp_ctx_create_multi) shards the covariance over its devices
  // (dense Sigma_y is an N x N host matrix: that case stays on devices[0])
  REFUSE_KPROD_MULTI(ctx, spec);
  if (ctx->multi && ncols >= 1 && noise)
    return sgp_multi_logpdf(ctx, spec, mean, noise_kind, noise, Y, ldy, ncols, out);
  SpecGuard g;
  CHECK_RC(dspec_create(ctx, spec, &g.ds));
  long N = g.ds->N;
  CHECK_ARG(N >= 1 && ncols >= 1 && ldy >= N, "sgp_logpdf: bad sizes");
  int64_t n_pad, m_tot;
  sgp_geometry(N, ncols, &n_pad, &m_tot);
  DevBuf dA, dmean, dY;
  NoiseDev nd;
  CHECK_RC(dA.alloc((size_t)m_tot * n_pad));
  if (mean) CHECK_RC(dmean.upload(mean, N));
  CHECK_RC(upload_noise(nd, noise_kind, noise, N));
  CHECK_RC(upload_matrix(dY, Y, ldy, N, ncols));
  return dev_logpdf_impl(ctx, g.ds, dA.p, mean ? dmean.p : nullptr, nd.kind, nd.sigma2, nd.diag.p,
                         nd.dense.p, nd.ld_dense, dY.p, N, ncols, out, nullptr);
}
extern "C" int sgp_logpdf(sgp_ctx* ctx, const sgp_cov_spec* spec, const double* mean, int noise_kind,
                          const double* noise, const double* Y, int64_t ldy, int64_t ncols,
                          double* out) {
  return with_df_fallback(ctx, [&]() { return sgp_logpdf_impl(ctx, spec, mean, noise_kind, noise, Y, ldy, ncols, out); });
}

// dst[i + c * ld] = mean[i] (i < N) else 0, for an nrows x ncols block
__global__ void fill_mean_cols_kernel(double* dst, long ld, long nrows, long ncols, long N, const double* mean) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= nrows * ncols) return;
  long i = idx % nrows, c = idx / nrows;
  dst[i + c * ld] = (mean && i < N) ? mean[i] : 0.0;
}

static int sgp_rand_impl(sgp_ctx* ctx, const sgp_cov_spec* spec, const double* mean, int noise_kind,
                        const double* noise, const double* Z, int64_t ldz, int64_t S, double* out,
                        int64_t ldo) {
  CHECK_ARG(ctx && spec && Z && out, "sgp_rand: NULL argument");
  CHECK_ARG(spec->symmetric, "sgp_rand: spec must be symmetric");
  CtxScope scope(ctx);
  REFUSE_KPROD_MULTI(ctx, spec);
  if (ctx->multi && noise)
    return sgp_multi_rand(ctx, spec, mean, noise_kind, noise, Z, ldz, S, out, ldo);
  SpecGuard g;
  CHECK_RC(dspec_create(ctx, spec, &g.ds));
  long N = g.ds->N;
  CHECK_ARG(N >= 1 && S >= 1 && ldz >= N && ldo >= N, "sgp_rand: bad sizes");
  int64_t n_pad, m_tot;
  sgp_geometry(N, 0, &n_pad, &m_tot);
  long s_pad = rup(S, TILE);
  hipStream_t s = ctx->stream;
  DevBuf dA, dmean, dZ, dZt, dOut;
  NoiseDev nd;
  CHECK_RC(dA.alloc((size_t)m_tot * n_pad));
  if (mean) CHECK_RC(dmean.upload(mean, N));
  CHECK_RC(upload_noise(nd, noise_kind, noise, N));
  CHECK_RC(upload_matrix(dZ, Z, ldz, N, S));
  CHECK_RC(dZt.alloc((size_t)s_pad * n_pad));
  CHECK_RC(dOut.alloc((size_t)n_pad * s_pad));
  SGP_HIP(hipMemsetAsync(ctx->d_info, 0, sizeof(int), s));
  SzMask sz;
  CHECK_RC(build_bordered(ctx, g.ds, dA.p, n_pad, m_tot, nullptr, nd.kind, nd.sigma2, nd.diag.p,
                          nd.dense.p, nd.ld_dense, nullptr, 0, 0, s, &sz));
  CHECK_RC(chol_bordered(ctx, dA.p, m_tot, n_pad, m_tot, nullptr, s, 0, &sz));
  SGP_HIP(hipMemsetAsync(dZt.p, 0, sizeof(double) * s_pad * n_pad, s));
  // Zt[s, k] = Z[k, s]
  CHECK_RC(launch_transpose_add(dZ.p, N, N, S, dZt.p, s_pad, nullptr, s));
  // out[i, s] = mean[i] + sum_{k <= i} L[i, k] Zt[s, k]   (n_pad x s_pad, column-major like the result)
  hipLaunchKernelGGL(fill_mean_cols_kernel, dim3((unsigned)((n_pad * s_pad + 255) / 256)), dim3(256), 0, s, dOut.p,
                     (long)n_pad, (long)n_pad, s_pad, N, mean ? dmean.p : nullptr);
  SGP_HIP(hipGetLastError());
  CHECK_RC(launch_gemm_nt_lz(dA.p, m_tot, dZt.p, s_pad, dOut.p, n_pad, n_pad, s_pad, 1.0, s));
  int info = fetch_info(ctx, s);
  if (info < 0) return -3;
  if (info > 0) {
    set_error("matrix is not positive definite; Cholesky factorization failed at leading minor " +
              std::to_string(info));
    return info;
  }
  SGP_HIP(hipMemcpy2D(out, sizeof(double) * ldo, dOut.p, sizeof(double) * n_pad, sizeof(double) * N,
                      (size_t)S, hipMemcpyDeviceToHost));
  return 0;
}
extern "C" int sgp_rand(sgp_ctx* ctx, const sgp_cov_spec* spec, const double* mean, int noise_kind,
                        const double* noise, const double* Z, int64_t ldz, int64_t S, double* out,
                        int64_t ldo) {
  return with_df_fallback(ctx, [&]() { return sgp_rand_impl(ctx, spec, mean, noise_kind, noise, Z, ldz, S, out, ldo); });
}

// whether no entry of `want` (NULL: none) asks for the gradient of an input that a patched side reads: those hold images
static bool images_unasked(const sgp_dspec* ds, double* const* want) {
  for (size_t t = 0; want && t < ds->h_terms.size(); ++t) {
    const DevTerm& T = ds->h_terms[t];
    if ((T.hr && want[ds->term_row_input[t]]) || (T.hc && want[ds->term_col_input[t]])) return false;
  }
  return true;
}

// per-term results back to the host (dst == NULL: not asked for), in the caller's order
static int fetch_terms(const sgp_dspec* ds, double* dst, const double* d_src) {
  const size_t nt = ds->h_terms.size();
  if (!dst || !nt) return 0;
  if (!ds->n_kprod && !ds->n_patch && !ds->n_stencil) {   // every term plain: the device order is the caller's (term_src[t] == t)
    SGP_HIP(hipMemcpy(dst, d_src, sizeof(double) * nt, hipMemcpyDeviceToHost));
    return 0;
  }
  std::vector<double> tmp(nt);
  SGP_HIP(hipMemcpy(tmp.data(), d_src, sizeof(double) * nt, hipMemcpyDeviceToHost));
  for (size_t k = 0; k < nt; ++k) dst[ds->term_src[k]] = tmp[k];
  return 0;
}

// Gradients with respect to the stencils' own weights and offsets (include/sthenomi_stencil_wo.h): the caller's two tables
// (2 pointers per element of spec->terms, [2 t] the row side, [2 t + 1] the column side; NULL: not asked for), checked
// against the spec, contracted by stencil.hip at the stencil terms of the cores below and copied out after the stream has run.
struct StencilWo {
  struct Job { double *hw, *ho; size_t off; int q, dim; };
  double* const* gw = nullptr;
  double* const* go = nullptr;
  DevBuf out, part;
  std::vector<Job> jobs;
  bool asked() const { return gw || go; }
  double* want_w(const sgp_dspec* ds, int t, int side) const { return gw ? gw[2 * ds->term_src[t] + side] : nullptr; }
  double* want_o(const sgp_dspec* ds, int t, int side) const { return go ? go[2 * ds->term_src[t] + side] : nullptr; }

  // refuse what has no stencil of its own, and size the output and the scratch.  diag: the diagonal pairs alone are contracted
  int prepare(const sgp_dspec* ds, const char* who, bool diag, hipStream_t s) {
    if (!asked()) return 0;
    size_t total = 0;
    long need = 1;
    for (int I = 0; I < ds->nrb; ++I)
      for (int J = 0; J < ds->ncb; ++J) {
        const PairSegs g = pair_segments(ds, I * ds->ncb + J);
        for (int t = g.t0; t < g.t1; ++t) {
          const DevTerm& T = ds->h_terms[t];
          for (int side = 0; side < 2; ++side) {
            double *hw = want_w(ds, t, side), *ho = want_o(ds, t, side);
            if (!hw && !ho) continue;
            if (t >= g.tk) {
              set_error(std::string(who) + ": a grad_weights / grad_offsets entry of a product chain term must be NULL");
              return -1;
            }
            if (T.ph) {
              set_error(std::string(who) + ": a grad_weights / grad_offsets entry of a patch (convolutional) term must be NULL");
              return -1;
            }
            const int q = side ? T.qc : T.qr;
            if (q < 1) {
              set_error(std::string(who) + ": plain side: a grad_weights / grad_offsets entry of a side without a stencil "
                                           "must be NULL");
              return -1;
            }
            jobs.push_back({hw, ho, total, q, T.dim});
            total += (size_t)q * (1 + T.dim);
            const long nr = ds->row_len[I], nc = ds->col_len[J];
            need = std::max(need, diag ? diag_grad_stencil_wo_partials(nr, T, side)
                                       : grad_stencil_wo_partials(side ? nc : nr, side ? nr : nc, T, side));
          }
        }
      }
    CHECK_RC(out.alloc(std::max<size_t>(1, total)));
    CHECK_RC(part.alloc((size_t)need));
    SGP_HIP(hipMemsetAsync(out.p, 0, sizeof(double) * std::max<size_t>(1, total), s));   // (an empty or off-diagonal pair: zeros)
    return 0;
  }
  // the device slots of (t, side), in prepare's order of visit; NULL where not asked for
  void slots(const sgp_dspec* ds, int t, int side, size_t& cursor, double** dw, double** dof) {
    *dw = *dof = nullptr;
    double *hw = want_w(ds, t, side), *ho = want_o(ds, t, side);
    if (!hw && !ho) return;
    const Job& j = jobs[cursor++];
    if (hw) *dw = out.p + j.off;
    if (ho) *dof = out.p + j.off + j.q;
  }
  // every stencil term of every pair: G(i, j) at Gm[i + j * ldg] (alpha as in contract_spec).  symmetric: G equals its
  // transpose, and the column side reads it at the mirrored address, along the lanes
  int contract(const sgp_dspec* ds, const double* Gm, long ldg, const double* alpha, bool symmetric, hipStream_t s) {
    if (!asked()) return 0;
    size_t cursor = 0;
    for (int I = 0; I < ds->nrb; ++I)
      for (int J = 0; J < ds->ncb; ++J) {
        const int p = I * ds->ncb + J;
        for (int t = ds->term_ptr[p]; t < ds->term_ptr[p + 1]; ++t) {
          const DevTerm& T = ds->h_terms[t];
          double *dw, *dof;
          slots(ds, t, 0, cursor, &dw, &dof);
          CHECK_RC(launch_grad_stencil_wo(Gm, 1, ldg, alpha, ds->row_off[I], ds->row_len[I], ds->col_off[J], ds->col_len[J], T, 0,
                                          part.p, dw, dof, s));
          slots(ds, t, 1, cursor, &dw, &dof);
          CHECK_RC(launch_grad_stencil_wo(Gm, symmetric ? 1 : ldg, symmetric ? ldg : 1, alpha, ds->col_off[J], ds->col_len[J],
                                          ds->row_off[I], ds->row_len[I], T, 1, part.p, dw, dof, s));
        }
      }
    return 0;
  }
  // the diagonal pairs: entries (i, i) with the weights dw_all (the whole diagonal, N doubles)
  int contract_diag(const sgp_dspec* ds, const double* dw_all, hipStream_t s) {
    if (!asked()) return 0;
    size_t cursor = 0;
    for (int I = 0; I < ds->nrb; ++I)
      for (int J = 0; J < ds->ncb; ++J) {
        const int p = I * ds->ncb + J;
        for (int t = ds->term_ptr[p]; t < ds->term_ptr[p + 1]; ++t)
          for (int side = 0; side < 2; ++side) {
            double *dw, *dof;
            slots(ds, t, side, cursor, &dw, &dof);
            if (I != J || ds->row_len[I] != ds->col_len[J]) continue;
            CHECK_RC(launch_diag_grad_stencil_wo(dw_all + ds->row_off[I], ds->row_len[I], ds->h_terms[t], side, part.p, dw, dof,
                                                 s));
          }
      }
    return 0;
  }
  // after the stream has run: the tables' entries, overwritten
  int fetch() {
    if (jobs.empty()) return 0;
    const Job& last = jobs.back();
    std::vector<double> h(last.off + (size_t)last.q * (1 + last.dim));
    SGP_HIP(hipMemcpy(h.data(), out.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
    for (const Job& j : jobs) {
      if (j.hw) std::copy(h.begin() + j.off, h.begin() + j.off + j.q, j.hw);
      if (j.ho) std::copy(h.begin() + j.off + j.q, h.begin() + j.off + (size_t)j.q * (1 + j.dim), j.ho);
    }
    return 0;
  }
};

// sum_ij G_ij dC_ij / d theta per flattened term of every block pair of `ds` (grad.hip):
// G = (alpha alpha' - Kinv) / 2 when alpha != nullptr, else G = the matrix at `Gm` itself.
// The terms of a pair are contracted class by class, in the order of its PairSegs (spec_segments.h): the plain terms [t0, tp)
// several per launch; the patch terms [tp, ts) one per launch (conv.hip), only where the caller carries them (leave.patch: the
// entry points of include/sthenomi_conv_grad.h); the stencil terms [ts, tk) likewise (stencil.hip; leave.stencil: the entry
// points of include/sthenomi_stencil_grad.h); the product chains [tk, t1) one chain per launch (kprod.hip), only where the
// caller says it carries them (leave.kprod: the cores set it where their entry points take chains).
// dgp (NULL: not asked for): d / d param per term, which for the plain terms is non-zero for SGP_CONST alone -- those run
// through the chain kernel once more, as chains of length one, for that entry, between the stencil terms and the chains.
static GradLeave pool_leave() {   // what sgp_logpdf_grad_batch / _pool carry beyond the plain terms: derivative terms
  GradLeave l;
  l.deriv = true;
  return l;
}
static int contract_spec(const sgp_dspec* ds, const double* Gm, long ldg, const double* alpha, long n_tr, long n_tc,
                         DevBuf& dpart, double* dgc, double* dgs, hipStream_t s, const GradLeave& leave, double* dgp) {
  CHECK_ARG(leave.stencil || !ds->n_stencil, "gradient contraction: stencil terms are not supported");
  CHECK_ARG(leave.patch || !ds->n_patch, "gradient contraction: patch (convolutional) terms are not supported");
  CHECK_ARG(leave.kprod || !ds->n_kprod,
            "gradient contraction: product chains and the RQ / LINEAR kinds are not supported here");
  CHECK_ARG(leave.deriv || !ds->n_deriv, "gradient contraction: derivative terms are not supported here");
  long need = std::max<long>(1, n_tr * n_tc) * ((ds->n_kprod || dgp) ? 24 : 16);
  if (ds->n_deriv) need = std::max(need, grad_deriv_partials(n_tr, n_tc));
  for (int p = 0; p < ds->nrb * ds->ncb; ++p) {   // the partial sums of the largest patch or stencil term
    const int I = p / ds->ncb, J = p % ds->ncb;
    const PairSegs g = pair_segments(ds, p);
    for (int t = g.tp; t < g.ts; ++t) need = std::max(need, grad_conv_partials(ds->row_len[I], ds->col_len[J], ds->h_terms[t]));
    for (int t = g.ts; t < g.td; ++t)
      need = std::max(need, grad_stencil_partials(ds->row_off[I], ds->row_len[I], ds->col_off[J], ds->col_len[J], ds->h_terms[t]));
  }
  CHECK_RC(dpart.alloc((size_t)need));
  for (int I = 0; I < ds->nrb; ++I) {
    if (ds->row_len[I] == 0) continue;
    for (int J = 0; J < ds->ncb; ++J) {
      if (ds->col_len[J] == 0) continue;
      long r0 = ds->row_off[I], nr = ds->row_len[I], c0 = ds->col_off[J], nc = ds->col_len[J];
      long trf = r0 / TILE, trl = (r0 + nr - 1) / TILE + 1, tcf = c0 / TILE, tcl = (c0 + nc - 1) / TILE + 1;
      int p = I * ds->ncb + J;
      const auto [t0, tp, ts, tk, t1, td] = pair_segments(ds, p);
      int dmax = ds->pair_dmax[p];
      int per = std::min(8, std::max(1, 64 / dmax));
      for (int t = t0; t < tp; t += per) {
        int cnt = std::min(per, tp - t);
        CHECK_RC(launch_grad_block(Gm, ldg, alpha, r0, nr, c0, nc, ds->d_terms + t, cnt, dmax, trf, tcf,
                                   trl - trf, tcl - tcf, dpart.p, dgc + t, dgs + t, s));
      }
      for (int t = tp; t < ts; ++t)
        CHECK_RC(launch_grad_conv(Gm, ldg, alpha, r0, nr, c0, nc, ds->h_terms[t], ds->d_terms + t, dpart.p, dgc + t, dgs + t, s));
      for (int t = ts; t < td; ++t)
        CHECK_RC(launch_grad_stencil(Gm, ldg, alpha, r0, nr, c0, nc, ds->h_terms[t], ds->d_terms + t, dpart.p, dgc + t, dgs + t,
                                     s));
      for (int t = td; t < tk;) {   // derivative terms, one group per launch (deriv.hip)
        const int cnt = deriv_group(ds->h_terms.data(), t, tk);
        CHECK_RC(launch_grad_deriv(Gm, ldg, alpha, r0, nr, c0, nc, ds->h_terms.data() + t, ds->d_terms + t, cnt, trf, tcf, trl - trf,
                                   tcl - tcf, dpart.p, dgc + t, dgs + t, s));
        t += cnt;
      }
      for (int t = t0; dgp && t < tp; ++t)
        if (ds->h_terms[t].kind == SGP_CONST)
          CHECK_RC(launch_grad_kprod(Gm, ldg, alpha, r0, nr, c0, nc, ds->h_terms.data() + t, ds->d_terms + t, 1, 1, trf, tcf,
                                     trl - trf, tcl - tcf, dpart.p, nullptr, nullptr, dgp + t, s));
      for (int t = tk; t < t1;) {
        const int e = chain_end(ds, t, t1), cdmax = chain_dmax(ds, t, e);
        CHECK_RC(launch_grad_kprod(Gm, ldg, alpha, r0, nr, c0, nc, ds->h_terms.data() + t, ds->d_terms + t, e - t, cdmax, trf,
                                   tcf, trl - trf, tcl - tcf, dpart.p, dgc + t, dgs + t, dgp ? dgp + t : nullptr, s));
        t = e;
      }
    }
  }
  return 0;
}

// The refusals the three gradient families share: a leave on a multi-GPU context, and stencil / patch terms without the leave.
// stem: the family's name ("sgp_logpdf_grad", ...), which the texts are built on; b: the ELBO's second spec
static int check_grad_leave(const sgp_ctx* ctx, const std::string& stem, const GradLeave& leave, const sgp_cov_spec* a,
                            const sgp_cov_spec* b = nullptr) {
  CHECK_ARG(!(leave.stencil && ctx->multi), stem + "_stencil: not supported on a multi-GPU context");
  CHECK_ARG(!(leave.patch && ctx->multi), stem + "_conv: not supported on a multi-GPU context");
  CHECK_ARG(leave.stencil || (!spec_has_stencil(ctx, a) && !spec_has_stencil(ctx, b)),
            stem + (leave.patch ? "_conv" : "") + ": gradients through stencil terms are not supported");
  CHECK_ARG(leave.patch || (!spec_has_patch(a) && !spec_has_patch(b)),
            stem + ": gradients through patch (convolutional) terms are not supported");
  return 0;
}

// The buffers of the input-point / function-scale gradients of one spec: a point-sum buffer per input (want_x) and a row /
// column scale-sum buffer per term (want[0] / want[1], one entry per element of spec->terms); a NULL table: not asked for.
// Allocated and zeroed on the stream, copied back into the caller's tables after the stream has run.
struct TermGradBufs {
  struct Scale { DevBuf buf; long len = 0; };
  const sgp_dspec* ds = nullptr;
  double* const* want_x = nullptr;
  double* const* want[2] = {nullptr, nullptr};   // [0] row scales, [1] column scales
  hipStream_t s = nullptr;
  std::vector<DevBuf> gx;
  std::vector<Scale> gs[2];

  int init(const sgp_dspec* ds_, double* const* x, double* const* r, double* const* c, hipStream_t s_) {
    ds = ds_, want_x = x, want[0] = r, want[1] = c, s = s_;
    gx = std::vector<DevBuf>(x ? ds->in_dim.size() : 0);
    for (int side = 0; side < 2; ++side) gs[side] = std::vector<Scale>(want[side] ? ds->h_terms.size() : 0);
    for (size_t k = 0; k < gx.size(); ++k) {
      const size_t cnt = (size_t)std::max<long>(1, (long)ds->in_dim[k] * ds->in_n[k]);
      CHECK_RC(gx[k].alloc(cnt));
      SGP_HIP(hipMemsetAsync(gx[k].p, 0, sizeof(double) * cnt, s));
    }
    return 0;
  }
  bool asked() const { return want_x || want[0] || want[1]; }
  double* input(int k) const { return want_x ? gx[k].p : nullptr; }
  // *out: the zeroed sums of the row (side 0) or column (side 1) scale vector `vec` (len entries) of the term at device
  // position t.  NULL unless the caller's table has an entry for the term, the term has that vector and len > 0
  int scale(int t, int side, const double* vec, long len, double** out) {
    *out = nullptr;
    if (!want[side] || !want[side][ds->term_src[t]] || !vec || len <= 0) return 0;
    Scale& b = gs[side][t];
    CHECK_RC(b.buf.alloc((size_t)len));
    SGP_HIP(hipMemsetAsync(b.buf.p, 0, sizeof(double) * len, s));
    b.len = len;
    *out = b.buf.p;
    return 0;
  }
  // after the stream has run: the inputs with points and a non-NULL entry, and every scale buffer handed out
  int fetch() {
    for (size_t k = 0; k < gx.size(); ++k)
      if (want_x[k] && ds->in_n[k] > 0)
        SGP_HIP(hipMemcpy(want_x[k], gx[k].p, sizeof(double) * ds->in_dim[k] * ds->in_n[k], hipMemcpyDeviceToHost));
    for (int side = 0; side < 2; ++side)
      for (size_t t = 0; t < gs[side].size(); ++t)
        if (gs[side][t].buf.p)
          SGP_HIP(hipMemcpy(want[side][ds->term_src[t]], gs[side][t].buf.p, sizeof(double) * gs[side][t].len,
                            hipMemcpyDeviceToHost));
    return 0;
  }
};

// the same plain term seen from its column points
static DevTerm transposed(const DevTerm& T) {
  DevTerm Tt = T;
  Tt.xr = T.xc, Tt.ldr = T.ldc, Tt.rs = T.cs;
  Tt.xc = T.xr, Tt.ldc = T.ldr, Tt.cs = T.rs;
  return Tt;
}

// The input-point / function-scale pass: what it reads and where its sums go (device pointers).
struct InputPass {
  const double* Gm;      // cotangent as in contract_spec: G(i, j) at Gm[i + j * ldg], or (alpha alpha' - Gm) / 2 with alpha
  long ldg;
  const double* alpha;
  bool symmetric;        // true: G and the spec are symmetric -- block (J, I) mirrors (I, J), so the column side of a pair is the
                         // row side of its mirror pair: the row side alone, weight 2 (patch terms 1: the mirror pair supplies
                         // the other role).  false: the row side, then the transposed pass for the column side, weight 1 each
  TermGradBufs* bufs;
};
// Every term of every pair, pair-major and in device order (PairSegs): a launch adds into its input's buffer without
// atomics, so this order is what fixes the bits.  A function-scaled term (K_ij = coef rs_i k_ij cs_j) has the sums of its
// scale vectors ride along, with k in place of its derivative; a side is launched when points or that side's scale are asked
// for.  Stencil terms form no scale sums, patch terms neither, and only the plain side of a one-sided patch term has points.
static int input_pass(const sgp_dspec* ds, const InputPass& q, hipStream_t s) {
  TermGradBufs& b = *q.bufs;
  if (!b.asked()) return 0;
  CHECK_ARG(!ds->n_deriv, "input-point and scale gradients through derivative terms are not supported");
  const bool points = b.want_x != nullptr;
  const double w = q.symmetric ? 2.0 : 1.0;
  for (int I = 0; I < ds->nrb; ++I)
    for (int J = 0; J < ds->ncb; ++J) {
      const long r0 = ds->row_off[I], nr = ds->row_len[I], c0 = ds->col_off[J], nc = ds->col_len[J];
      if (nr == 0 || nc == 0) continue;
      const int p = I * ds->ncb + J;
      const PairSegs g = pair_segments(ds, p);
      for (int t = g.t0; t < g.tp; ++t) {
        const DevTerm& T = ds->h_terms[t];
        double *gsr, *gsc;
        CHECK_RC(b.scale(t, 0, T.rs, nr, &gsr));
        CHECK_RC(b.scale(t, 1, T.cs, nc, &gsc));
        if (points || gsr)
          CHECK_RC(launch_grad_inputs(q.Gm, 1, q.ldg, q.alpha, r0, nr, c0, nc, T, ds->pair_dmax[p], w,
                                      b.input(ds->term_row_input[t]), s, gsr));
        if (!q.symmetric && (points || gsc))
          CHECK_RC(launch_grad_inputs(q.Gm, q.ldg, 1, q.alpha, c0, nc, r0, nr, transposed(T), ds->pair_dmax[p], 1.0,
                                      b.input(ds->term_col_input[t]), s, gsc));
      }
      for (int t = g.tp; points && t < g.ts; ++t) {   // (conv.hip)
        const DevTerm& T = ds->h_terms[t];
        if (T.hr && T.hc) continue;
        CHECK_RC(launch_grad_conv_points(q.Gm, q.ldg, q.alpha, r0, nr, c0, nc, T, ds->d_terms + t, 1.0,
                                         b.input(T.hr ? ds->term_col_input[t] : ds->term_row_input[t]), s));
      }
      for (int t = g.ts; points && t < g.td; ++t) {   // (stencil.hip; transposed: sides and stencils swapped)
        const DevTerm& T = ds->h_terms[t];
        CHECK_RC(launch_grad_stencil_points(q.Gm, 1, q.ldg, q.alpha, r0, nr, c0, nc, T, 0, w, b.input(ds->term_row_input[t]), s));
        if (!q.symmetric)
          CHECK_RC(launch_grad_stencil_points(q.Gm, q.ldg, 1, q.alpha, c0, nc, r0, nr, T, 1, 1.0,
                                              b.input(ds->term_col_input[t]), s));
      }
      for (int t = g.tk; t < g.t1;) {   // a chain: every factor's input and the head's scale in one launch per side (kprod.hip)
        const int e = chain_end(ds, t, g.t1), cdmax = chain_dmax(ds, t, e);
        double *gsr, *gsc, *gxr[SGP_KPROD_MAX_FACTORS], *gxc[SGP_KPROD_MAX_FACTORS];
        CHECK_RC(b.scale(t, 0, ds->h_terms[t].rs, nr, &gsr));
        CHECK_RC(b.scale(t, 1, ds->h_terms[t].cs, nc, &gsc));
        for (int f = t; f < e; ++f) gxr[f - t] = b.input(ds->term_row_input[f]), gxc[f - t] = b.input(ds->term_col_input[f]);
        if (points || gsr)
          CHECK_RC(launch_grad_kprod_inputs(q.Gm, 1, q.ldg, q.alpha, r0, nr, c0, nc, &ds->h_terms[t], e - t, cdmax, 0, w, gxr, gsr,
                                            s));
        if (!q.symmetric && (points || gsc))
          CHECK_RC(launch_grad_kprod_inputs(q.Gm, q.ldg, 1, q.alpha, c0, nc, r0, nr, &ds->h_terms[t], e - t, cdmax, 1, 1.0, gxc,
                                            gsc, s));
        t = e;
      }
    }
  return 0;
}

// ---------------------------------------------------------------------------------------
// logpdf + reverse-mode gradient
// ---------------------------------------------------------------------------------------
// (every consumer of C^-1 -- the term contractions, the input-point and row-scale sums, the noise gradient -- walks the block
// pairs WITH terms or the diagonal: none needs a tile outside K's own tile pattern)
static int logpdf_grad_core(sgp_ctx* ctx, const LogpdfGradArgs& a) {
  // (a.leave.kprod: sgp_logpdf_grad_param / _param_xs -- here it only lets grad_inputs / grad_rowscale through product chains,
  // the term contraction carries chains for every caller; a.leave.patch: sgp_logpdf_grad_conv, include/sthenomi_conv_grad.h --
  // patch terms are contracted, conv.hip; a.leave.stencil: sgp_logpdf_grad_stencil, include/sthenomi_stencil_grad.h -- stencil
  // terms too, stencil.hip; it sets a.leave.patch)
  CHECK_ARG(ctx && a.spec && a.noise && a.y && a.logpdf_out, "sgp_logpdf_grad: NULL argument");
  CHECK_ARG(a.spec->symmetric, "sgp_logpdf_grad: spec must be symmetric");
  CHECK_ARG(a.noise_kind >= SGP_NOISE_SCALAR && a.noise_kind <= SGP_NOISE_DENSE, "sgp_logpdf_grad: bad noise kind");
  // derivative terms (deriv.hip) are contracted for sgp_logpdf_grad itself -- grad_coef and grad_inscale -- and for no other
  // member of the family
  CHECK_ARG(a.leave.deriv || !spec_has_deriv(a.spec),
            "sgp_logpdf_grad_x / _xs / _param / _conv / _stencil / _stencil_wo: input-point, scale, parameter, patch and stencil "
            "gradients through derivative terms are not supported: sgp_logpdf_grad returns grad_coef and grad_inscale");
  CHECK_ARG(!(ctx->multi && spec_has_deriv(a.spec)), DERIV_REFUSAL_MULTI);
  CHECK_RC(check_grad_leave(ctx, "sgp_logpdf_grad", a.leave, a.spec));
  CHECK_ARG(!(a.grad_inputs || a.grad_rowscale) || a.leave.kprod || a.leave.stencil || !spec_has_kprod(a.spec),
            "sgp_logpdf_grad_x / _xs: input-point and scale gradients through product chains and the RQ / LINEAR kinds are "
            "not supported: call sgp_logpdf_grad_param_xs (include/sthenomi_kprod_grad.h)");
  CHECK_ARG(!(a.leave.kprod && ctx->multi), "sgp_logpdf_grad_param: not supported on a multi-GPU context");
  CtxScope scope(ctx);
  // a multi-GPU context shards the gradient -- kernel terms, noise, y, the mean and (round 6) the input points and function
  // scales, a dense Sigma_y (multi.hip)
  REFUSE_KPROD_MULTI(ctx, a.spec);
  if (ctx->multi)
    return sgp_multi_logpdf_grad(ctx, a.spec, a.mean, a.noise_kind, a.noise, a.y, a.logpdf_out, a.grad_y, a.grad_mean,
                                 a.grad_noise, a.grad_coef, a.grad_inscale, a.grad_inputs, a.grad_rowscale);
  SpecGuard g;
  CHECK_RC(dspec_create(ctx, a.spec, &g.ds));
  const sgp_dspec* ds = g.ds;
  long N = ds->N;
  CHECK_ARG(N >= 1, "sgp_logpdf_grad: empty data");
  CHECK_ARG(images_unasked(ds, a.grad_inputs),
            "sgp_logpdf_grad_stencil: an input read by a patch (convolutional) side holds images, and gradients with respect to "
            "images are not supported: its grad_inputs entry must be NULL");
  const bool dense_noise = a.noise_kind == SGP_NOISE_DENSE;   // grad_noise is then N x N (ld = N): the cotangent G itself
  long n_pad = rup(N, TILE);
  long nrows = TILE + n_pad;            // the (y - m)' row (+ zero padding), then the identity rows
  long m_tot = n_pad + nrows;
  hipStream_t s = ctx->stream;
  StencilWo wo;   // (include/sthenomi_stencil_wo.h; a no-op throughout when neither table is asked for)
  wo.gw = a.grad_weights, wo.go = a.grad_offsets;
  CHECK_RC(wo.prepare(ds, "sgp_logpdf_grad_stencil_wo", false, s));
  DevBuf dA, dKinv, dmean, dy, dalpha, dpart, dgc, dgs, dgn, dgp;
  NoiseDev nd;
  CHECK_RC(dA.alloc((size_t)m_tot * n_pad));
  CHECK_RC(dKinv.alloc((size_t)n_pad * n_pad));
  if (a.mean) CHECK_RC(dmean.upload(a.mean, N));
  CHECK_RC(dy.upload(a.y, N));
  CHECK_RC(upload_noise(nd, a.noise_kind, a.noise, N));
  CHECK_RC(dalpha.alloc(n_pad));
  size_t nterms_total = ds->h_terms.size();
  CHECK_RC(dgc.alloc(std::max<size_t>(1, nterms_total)));
  CHECK_RC(dgs.alloc(std::max<size_t>(1, nterms_total)));
  CHECK_RC(dgn.alloc(dense_noise && a.grad_noise ? (size_t)N * N : (size_t)n_pad));
  SGP_HIP(hipMemsetAsync(ctx->d_info, 0, sizeof(int), s));
  SGP_HIP(hipMemsetAsync(dalpha.p, 0, sizeof(double) * n_pad, s));
  SGP_HIP(hipMemsetAsync(dgc.p, 0, sizeof(double) * std::max<size_t>(1, nterms_total), s));
  SGP_HIP(hipMemsetAsync(dgs.p, 0, sizeof(double) * std::max<size_t>(1, nterms_total), s));
  if (a.grad_param) {
    CHECK_RC(dgp.alloc(std::max<size_t>(1, nterms_total)));
    SGP_HIP(hipMemsetAsync(dgp.p, 0, sizeof(double) * std::max<size_t>(1, nterms_total), s));
  }
  // K + Sigma_y, identity padding, bordered rows [(y - m)' ; I].  The identity rows come last so
  // that the rows a panel touches (K rows below it, the y row, identity rows above its last
  // column) are contiguous: the factorisation + inv(L) cost 2/3 N^3 instead of 4/3 N^3.
  CHECK_RC(assemble(ds, dA.p, m_tot, 0, n_pad / TILE, 0, n_pad / TILE, 1, dense_noise ? -1 : nd.kind, nd.sigma2,
                    nd.diag.p, s));
  if (dense_noise) CHECK_RC(launch_add_dense(dA.p, m_tot, nd.dense.p, nd.ld_dense, N, 1, s));
  CHECK_RC(launch_fill_pad(dA.p, m_tot, N, n_pad, 0, n_pad, m_tot, 0, s));
  CHECK_RC(launch_grad_border(dA.p, m_tot, n_pad, N, dy.p, a.mean ? dmean.p : nullptr, nrows, s));
  // Structural zeros (round 5): the factorisation of [K ; (y - m)' ; I] skips the tile products a programme with independent
  // components makes exact zeros -- in the factor AND in inv(L)', whose tile pattern is the closure of the factor's (the
  // identity rows run through the same symbolic elimination) -- C^-1 = inv(L)' inv(L) contracts only the k tiles both
  // operand tiles have, and only the tiles of C^-1 that a block pair WITH terms (or the diagonal: the noise gradient) reads
  // are computed at all.  Same bits as the dense schedule: every product left out is an exact zero or is never read.
  SzMask sz;
  {
    int words = 0;
    CHECK_RC(sz_pattern(ctx, ds, a.noise_kind, n_pad, m_tot, &words, true));
    CHECK_RC(sz_upload(ctx, ctx->h_sz, words, s, &sz));
  }
  CHECK_RC(chol_bordered(ctx, dA.p, m_tot, n_pad, m_tot, nullptr, s, n_pad + TILE, sz.d_nz ? &sz : nullptr));
  // row n_pad holds z' = (inv(L) (y - m))' ; rows n_pad + 128 .. now hold inv(L)' (upper triangular)
  const double* zrow = dA.p + n_pad;
  const double* Rinv = dA.p + n_pad + TILE;
  double* d_logdet = ctx->d_scal;
  double* d_sq = ctx->d_scal + 16;
  double* d_out = ctx->d_scal + 17;
  CHECK_RC(launch_rowsumsq(zrow, m_tot, N, 1, d_sq, 0, s));
  CHECK_RC(launch_sum_array(ctx->d_slots, n_pad / TILE, d_logdet, s));
  CHECK_RC(launch_logpdf_final(d_logdet, d_sq, N, 1, d_out, s));
  // alpha = inv(L)' z
  CHECK_RC(launch_gemv_rows(Rinv, m_tot, N, n_pad, zrow, m_tot, nullptr, dalpha.p, s, 1));
  // C^-1 = inv(L)' inv(L): lower tiles on the MFMA GEMM, then mirrored
  {
    TileSkip usk;
    if (sz.d_nz) {
      // the tiles outside K's own pattern are not computed: they must not be pool garbage for whoever reads all of C^-1
      // (today nobody does -- a dense Sigma_y has no pattern -- but the mirror below copies them; advisor, round 5)
      SGP_HIP(hipMemsetAsync(dKinv.p, 0, sizeof(double) * (size_t)n_pad * n_pad, s));
      usk.nz = sz.d_nz;
      usk.words = sz.words;
      usk.tr0 = usk.tc0 = (int)(n_pad / TILE + 1);   // the identity rows' pattern rows
      usk.need0 = (int)(m_tot / TILE);               // K's own tile pattern, behind the factor rows
    }
    CHECK_RC(launch_gemm_nt_uut(Rinv, m_tot, dKinv.p, n_pad, n_pad, s, usk.nz ? &usk : nullptr));
  }
  CHECK_RC(launch_mirror_lower(dKinv.p, n_pad, n_pad, s));
  if (a.grad_noise && dense_noise) CHECK_RC(launch_grad_noise_dense(dKinv.p, n_pad, dalpha.p, N, dgn.p, s));
  else if (a.grad_noise) CHECK_RC(launch_grad_noise(dKinv.p, n_pad, dalpha.p, N, nd.kind == SGP_NOISE_DIAG, dgn.p, s));
  GradLeave carried = a.leave;
  carried.kprod = true;   // chains are contracted for every caller of this core
  if (a.grad_coef || a.grad_inscale || a.grad_param)
    CHECK_RC(contract_spec(ds, dKinv.p, n_pad, dalpha.p, n_pad / TILE, n_pad / TILE, dpart, dgc.p, dgs.p, s, carried,
                           a.grad_param ? dgp.p : nullptr));
  // gradient w.r.t. the input points and the row-scale vectors of function-scaled processes: the spec and G are symmetric,
  // so the row side, twice, covers the column role too -- the column scale of a term is the row scale of its mirror term
  TermGradBufs bufs;
  CHECK_RC(bufs.init(ds, a.grad_inputs, a.grad_rowscale, nullptr, s));
  CHECK_RC(input_pass(ds, {dKinv.p, n_pad, dalpha.p, true, &bufs}, s));
  // the stencils' own weights and offsets: both sides of every stencil term against the same cotangent (stencil.hip)
  CHECK_RC(wo.contract(ds, dKinv.p, n_pad, dalpha.p, true, s));
  int info = fetch_info(ctx, s);
  if (info < 0) return -3;
  if (info > 0) {
    set_error("matrix is not positive definite; Cholesky factorization failed at leading minor " +
              std::to_string(info));
    return info;
  }
  CHECK_RC(wo.fetch());
  SGP_HIP(hipMemcpy(a.logpdf_out, d_out, sizeof(double), hipMemcpyDeviceToHost));
  std::vector<double> ha(N);
  SGP_HIP(hipMemcpy(ha.data(), dalpha.p, sizeof(double) * N, hipMemcpyDeviceToHost));
  if (a.grad_y)
    for (long i = 0; i < N; ++i) a.grad_y[i] = -ha[i];
  if (a.grad_mean)
    for (long i = 0; i < N; ++i) a.grad_mean[i] = ha[i];
  if (a.grad_noise)
    SGP_HIP(hipMemcpy(a.grad_noise, dgn.p,
                      sizeof(double) * (dense_noise ? (size_t)N * N : (nd.kind == SGP_NOISE_DIAG ? (size_t)N : (size_t)1)),
                      hipMemcpyDeviceToHost));
  // one entry per element of spec->terms, in the CALLER's order: a spec with product chains keeps its plain terms in front of
  // them on the device (dspec_create), so its entries go back through term_src
  CHECK_RC(fetch_terms(ds, a.grad_coef, dgc.p));
  CHECK_RC(fetch_terms(ds, a.grad_inscale, dgs.p));
  if (a.grad_param) CHECK_RC(fetch_terms(ds, a.grad_param, dgp.p));
  CHECK_RC(bufs.fetch());
  return 0;
}

// the front door of the family (driver.h): the C entry points here and in the libraries beside this one fill a record, call it
int sgp::drv_logpdf_grad(sgp_ctx* ctx, const LogpdfGradArgs& a) {
  return with_df_fallback(ctx, [&]() { return logpdf_grad_core(ctx, a); });
}

extern "C" int sgp_logpdf_grad_xs(sgp_ctx* ctx, const sgp_cov_spec* spec, const double* mean, int noise_kind,
                                  const double* noise, const double* y, double* logpdf_out, double* grad_y,
                                  double* grad_mean, double* grad_noise, double* grad_coef, double* grad_inscale,
                                  double* const* grad_inputs, double* const* grad_rowscale) {
  LogpdfGradArgs a = logpdf_grad_args(spec, mean, noise_kind, noise, y, logpdf_out, grad_y, grad_mean, grad_noise, grad_coef,
                                      grad_inscale);
  a.grad_inputs = grad_inputs, a.grad_rowscale = grad_rowscale;
  return drv_logpdf_grad(ctx, a);
}

extern "C" int sgp_logpdf_grad(sgp_ctx* ctx, const sgp_cov_spec* spec, const double* mean, int noise_kind,
                               const double* noise, const double* y, double* logpdf_out, double* grad_y,
                               double* grad_mean, double* grad_noise, double* grad_coef,
                               double* grad_inscale) {
  LogpdfGradArgs a = logpdf_grad_args(spec, mean, noise_kind, noise, y, logpdf_out, grad_y, grad_mean, grad_noise, grad_coef,
                                      grad_inscale);
  a.leave.deriv = true;   // (this entry point alone carries derivative terms)
  return drv_logpdf_grad(ctx, a);
}

extern "C" int sgp_logpdf_grad_x(sgp_ctx* ctx, const sgp_cov_spec* spec, const double* mean, int noise_kind,
                                 const double* noise, const double* y, double* logpdf_out, double* grad_y,
                                 double* grad_mean, double* grad_noise, double* grad_coef,
                                 double* grad_inscale, double* const* grad_inputs) {
  CHECK_ARG(grad_inputs != nullptr, "sgp_logpdf_grad_x: grad_inputs is NULL");
  LogpdfGradArgs a = logpdf_grad_args(spec, mean, noise_kind, noise, y, logpdf_out, grad_y, grad_mean, grad_noise, grad_coef,
                                      grad_inscale);
  a.grad_inputs = grad_inputs;
  return drv_logpdf_grad(ctx, a);
}

// ---------------------------------------------------------------------------------------
// pooled launches: independent models in one call (include/sthenomi.h: sgp_logpdf_batch, sthenomi_batch.h, sthenomi_pool.h)
// ---------------------------------------------------------------------------------------
// At the sizes where one factorisation is bound by its diagonal chain (N = 4096: 0.13 of the fp64 MFMA peak, ~220 CUs idle;
// value + gradient: 0.2) independent models are factored by ONE launch of the dataflow kernel as a single task pool
// (chol_df.hip: progress counters per matrix): the chains sit on different workgroups and hide each other.  Every member is
// assembled exactly as its own call assembles it (its own N, n_pad, m_tot, leading dimension) and the reductions behind the
// launch are each member's own, in its own call's order: every output is bit-equal to the member's own sgp_logpdf /
// sgp_logpdf_grad call.  A structured member's own call skips K's zero tiles; a pooled launch computes them as the exact
// zeros they are: same bits.
// Four entry points PLAN such launches -- which members pool, how they are cut into launches, what happens to the rest -- and
// one routine, pooled_chunk, runs a launch:
//   sgp_logpdf_batch, sgp_logpdf_grad_batch   members of ONE padded size (the folds of a cross-validation, which differ by a
//                                             point or two, pool) and one noise kind, in input order; anything else: every
//                                             member through its own call
//   sgp_logpdf_pool, sgp_logpdf_grad_pool     members of any sizes and noise kinds (folds that straddle a tile boundary,
//                                             learning curves, one GP per series -- the reference's
//                                             examples/getting_started/script.jl:154-213 runs them member by member), largest
//                                             first; the members that do not pool through their own calls
namespace {
// what one of the four entry points was called with, and the outcome of its members so far
struct PoolCall {
  const char* label;   // "batch" / "pool": names a member in a message
  bool grad;           // value + gradient (the members carry the gradient border [ (y - m)' ; I ]) or the value alone
  const sgp_cov_spec* const* specs;
  const double* const* means;
  const int* kinds;    // noise kind per member; nullptr: `kind` for every member
  int kind;
  const double* const* noises;
  const double* const* ys;
  double* out;         // logpdf per member
  double* const* grad_y;
  double* const* grad_mean;
  double* const* grad_noise;
  double* const* grad_coef;
  double* const* grad_inscale;
  int* infos;
  int first_bad = 0;

  int kind_of(int b) const { return kinds ? kinds[b] : kind; }
  static double* at(double* const* v, int b) { return v ? v[b] : nullptr; }
  // member b through its own call: < 0 an error, > 0 its info
  int own_call(sgp_ctx* ctx, int b) const {
    const double* mean = means ? means[b] : nullptr;
    if (!grad) return sgp_logpdf(ctx, specs[b], mean, kind_of(b), noises[b], ys[b], spec_rows_host(specs[b]), 1, out + b);
    return sgp_logpdf_grad(ctx, specs[b], mean, kind_of(b), noises[b], ys[b], out + b, at(grad_y, b), at(grad_mean, b),
                           at(grad_noise, b), at(grad_coef, b), at(grad_inscale, b));
  }
  // member b is not positive definite: NaN and its info; true for the first one of the call
  bool mark_bad(int b, int info) {
    out[b] = std::numeric_limits<double>::quiet_NaN();
    if (infos) infos[b] = info;
    if (first_bad) return false;
    first_bad = info;
    return true;
  }
  void note_bad(int b, int info) {   // ... and the call's error text names the first one
    if (mark_bad(b, info))
      set_error("matrix is not positive definite; Cholesky factorization failed at leading minor " + std::to_string(info) +
                " (" + label + " member " + std::to_string(b) + ")");
  }
  int rc() const { return infos ? 0 : first_bad; }
};

// the geometry of a member of N >= 1 rows, as its own call lays it out (value: sgp_geometry(N, 1); gradient: logpdf_grad_core's,
// the identity rows below the border)
void pool_geometry(long N, bool grad, long* n_pad, long* m_tot) {
  int64_t np = 0, mt = 0;
  sgp_geometry(N, 1, &np, &mt);
  *n_pad = np;
  *m_tot = grad ? 2 * np + TILE : mt;
}
// can member b run in a pooled launch (and its geometry)?  Otherwise -- dense noise, sizes beyond SGP_BATCH_MAX_N or, for the
// gradient, sizes its own call factors with the hybrid schedule, a multi-GPU context -- it goes through its own call.
bool poolable(const sgp_ctx* ctx, const PoolCall& call, int b, long* n_pad, long* m_tot) {
  const long N = spec_rows_host(call.specs[b]);
  const int kind = call.kind_of(b);
  if (ctx->multi || ctx->dataflow == 0 || ctx->batch_max_n <= 0 || N < 1 || (kind != SGP_NOISE_SCALAR && kind != SGP_NOISE_DIAG))
    return false;
  pool_geometry(N, call.grad, n_pad, m_tot);
  return *n_pad <= ctx->batch_max_n && (!call.grad || *n_pad < ctx->hybrid_grow_min_n);
}

// the launch of one chunk.  Members of one shape: the ragged task order IS the equal-size round robin (df_pool.h), and that
// kernel needs no table: this shape class takes it (8 members at N = 4096 through the ragged kernel: 5.19 ms against 5.15 --
// profiles/r09_pool.json).  Otherwise the ragged kernel: task table (host-built, uploaded on s), progress words, launch.
// `order` and `d_order` stay alive until the caller has drained s.
int pool_launch(sgp_ctx* ctx, const DfPoolMember* pm, int nb, std::vector<uint32_t>& order, DevBuf& d_order, hipStream_t s) {
  int T_r[DF_MAX_BATCH], T_c[DF_MAX_BATCH];
  bool equal = true;
  for (int b = 0; b < nb; ++b) {
    T_r[b] = pm[b].T_r;
    T_c[b] = pm[b].T_c;
    equal = equal && T_r[b] == T_r[0] && T_c[b] == T_c[0] && pm[b].ld == pm[0].ld && pm[b].nz == pm[0].nz && pm[b].nzw == pm[0].nzw;
  }
  if (equal) {
    DfProb probs[DF_MAX_BATCH];
    for (int b = 0; b < nb; ++b) probs[b] = pm[b].p;
    const long m_tot = (long)T_r[0] * TILE;
    CHECK_RC(df_scratch_state(ctx, df_state_words(m_tot, nb), s));
    return launch_chol_dataflow_batch(probs, nb, pm[0].ld, (long)T_c[0] * TILE, m_tot, ctx->d_df_state,
                                      ctx->batch_fat ? ctx->hybrid_wgs : ctx->df_wgs, ctx->df_timeout_s, ctx->batch_fat, s,
                                      pm[0].nz, pm[0].nzw);
  }
  CHECK_ARG(df_pool_order(T_r, T_c, nb, order), "pool: a member's tile grid does not fit the task table");
  CHECK_RC(d_order.alloc((order.size() + 1) / 2));   // (32-bit entries inside doubles' storage)
  SGP_HIP(hipMemcpyAsync(d_order.p, order.data(), sizeof(uint32_t) * order.size(), hipMemcpyHostToDevice, s));
  CHECK_RC(df_scratch_state(ctx, df_pool_state_words(pm, nb), s));
  return launch_chol_pool(pm, nb, ctx->d_df_state, reinterpret_cast<const uint32_t*>(d_order.p), (long)order.size(),
                          ctx->batch_fat ? ctx->hybrid_wgs : ctx->df_wgs, ctx->df_timeout_s, ctx->batch_fat, s);
}

struct PoolMember {
  SpecGuard g;
  DevBuf A, Kinv, mean, y, part;   // (Kinv, part: gradient only)
  NoiseDev nd;
  long N = 0, n_pad = 0, m_tot = 0, T_c = 0, nt = 0;
  long off = 0, inv_off = 0;   // the member's results / inverse diagonal blocks in the chunk's buffers
  size_t pat = 0;              // gradient: its border pattern among the chunk's
};
struct BorderPattern {   // the gradient border of a dense K (sz_pattern.h) at one padded size
  long n_pad, off;       // off: its first word in the chunk's one upload
  int words;
};
constexpr int CHUNK_NO_MEMORY = 1;

// ONE pooled launch: the members ids[0 .. nb) of `call` (nb <= DF_MAX_BATCH), each in its own geometry -- assembly as the
// member's own call does it, one launch that factors them all, then per member the own call's launches in its order (every
// reduction sums in the same order), one download of all small results.  Returns 0 with the members' outcomes stored in
// `call` (their padded sizes appended to `sizes`), CHUNK_NO_MEMORY when the device memory did not suffice -- nothing is
// stored, the stream is drained and the caller runs its own fallback -- or an error (-3: the launch timed out).
int pooled_chunk(sgp_ctx* ctx, PoolCall& call, const int* ids, int nb, std::vector<long>* sizes) {
  hipStream_t s = ctx->stream;
  const bool grad = call.grad;
  std::vector<PoolMember> mem((size_t)nb);
  DevBuf inv, res, infobuf, d_order;
  std::vector<uint32_t> order;
  // per member in `res`: [T_c] logdet slots | logdet | |L^-1 (y - m)|^2 | logpdf | (pad to T_c + 8), and for the gradient
  // | alpha [n_pad] | noise gradient [n_pad] | d coef [nt] | d inscale [nt]
  long res_len = 0, inv_len = 0;
  // gradient: one border pattern per distinct padded size of the chunk, all in one upload
  std::vector<sz_word> h_pat;
  std::vector<BorderPattern> pats;
  for (int b = 0; b < nb; ++b) {
    PoolMember& M = mem[(size_t)b];
    const sgp_cov_spec* sp = call.specs[ids[b]];
    M.N = spec_rows_host(sp);
    pool_geometry(M.N, grad, &M.n_pad, &M.m_tot);
    M.T_c = M.n_pad / TILE;
    M.nt = std::max<long>(1, sp->term_ptr ? sp->term_ptr[(long)sp->n_row_blocks * sp->n_col_blocks] : 0);
    M.off = res_len;
    M.inv_off = inv_len;
    res_len += M.T_c + 8 + (grad ? 2 * M.n_pad + 2 * M.nt : 0);
    inv_len += M.T_c * INVD_STRIDE;
    if (!grad) continue;
    while (M.pat < pats.size() && pats[M.pat].n_pad != M.n_pad) ++M.pat;
    if (M.pat == pats.size()) {
      SzPattern pat;
      sz_symbolic(std::vector<char>(1, 1), 1, std::vector<long>(1, 0), std::vector<long>(1, M.n_pad), M.n_pad, TILE, M.T_c,
                  M.m_tot / TILE, pat, true);
      pats.push_back(BorderPattern{M.n_pad, (long)h_pat.size(), pat.words});
      h_pat.insert(h_pat.end(), pat.nz.begin(), pat.nz.end());
    }
  }
  // device memory: an allocation that fails before anything of this chunk is needed hands the chunk back to the caller
  int arc = inv.alloc((size_t)inv_len);
  arc = arc ? arc : res.alloc((size_t)res_len);
  arc = arc ? arc : infobuf.alloc((size_t)nb);   // (ints inside doubles' storage)
  int* d_infos = reinterpret_cast<int*>(infobuf.p);
  if (!arc) SGP_HIP(hipMemsetAsync(d_infos, 0, sizeof(int) * nb, s));
  if (!arc && grad) {
    SGP_HIP(hipMemsetAsync(res.p, 0, sizeof(double) * res_len, s));
    arc = sz_stage(ctx, h_pat, s);   // (ctx->d_sz; pinned staging: the copy is asynchronous)
  }
  // 1. assembly, member by member: the next member's uploads (its spec among them) run under the assembly of the one before
  // (no structural zeros of the members' own models inside a pooled launch: they need not share a pattern, and these sizes are
  // chain-bound anyway)
  DfPoolMember pm[DF_MAX_BATCH];
  for (int b = 0; b < nb && !arc; ++b) {
    PoolMember& M = mem[(size_t)b];
    const int gb = ids[b];
    arc = dspec_create(ctx, call.specs[gb], &M.g.ds);
    // (the result layout counted the terms from the host spec, before dspec_create had validated it)
    if (!arc) CHECK_ARG((long)M.g.ds->h_terms.size() <= M.nt && M.g.ds->N == M.N, "pooled member: the device spec disagrees with the host spec's rows / terms");
    arc = arc ? arc : M.A.alloc((size_t)M.m_tot * M.n_pad);
    if (!arc && grad) arc = M.Kinv.alloc((size_t)M.n_pad * M.n_pad);
    arc = arc ? arc : M.y.upload(call.ys[gb], M.N);
    if (!arc && call.means && call.means[gb]) arc = M.mean.upload(call.means[gb], M.N);
    arc = arc ? arc : upload_noise(M.nd, call.kind_of(gb), call.noises[gb], M.N);
    if (arc) break;
    if (grad) {
      CHECK_RC(assemble(M.g.ds, M.A.p, M.m_tot, 0, M.T_c, 0, M.T_c, 1, M.nd.kind, M.nd.sigma2, M.nd.diag.p, s));
      CHECK_RC(launch_fill_pad(M.A.p, M.m_tot, M.N, M.n_pad, 0, M.n_pad, M.m_tot, 0, s));
      CHECK_RC(launch_grad_border(M.A.p, M.m_tot, M.n_pad, M.N, M.y.p, M.mean.p, TILE + M.n_pad, s));
    } else {
      CHECK_RC(build_bordered(ctx, M.g.ds, M.A.p, M.n_pad, M.m_tot, M.mean.p, M.nd.kind, M.nd.sigma2, M.nd.diag.p, nullptr, 0,
                              M.y.p, M.N, 1, s, nullptr));
    }
    pm[b] = DfPoolMember{DfProb{M.A.p, inv.p + M.inv_off, res.p + M.off, d_infos + b}, M.m_tot, (int)(M.m_tot / TILE), (int)M.T_c,
                         grad ? ctx->d_sz + pats[M.pat].off : nullptr, grad ? pats[M.pat].words : 0};
  }
  if (arc == -2) {
    SGP_HIP(hipStreamSynchronize(s));   // (assemblies of the members that did fit may still be running on their buffers)
    return CHUNK_NO_MEMORY;
  }
  CHECK_RC(arc);
  // 2. one launch: the factors (and, for the gradient, inv(L)') of every member
  CHECK_RC(pool_launch(ctx, pm, nb, order, d_order, s));
  // 3. gradient: C^-1 = inv(L)' inv(L), lower tiles -- one launch per distinct padded size (the single call's dense tile program)
  for (size_t k = 0; k < pats.size(); ++k) {
    const double* rinv[DF_MAX_BATCH];
    double* kinv[DF_MAX_BATCH];
    int ng = 0;
    for (const PoolMember& M : mem) {
      if (M.pat != k) continue;
      rinv[ng] = M.A.p + M.n_pad + TILE;
      kinv[ng] = M.Kinv.p;
      ++ng;
    }
    const long n_pad = pats[k].n_pad;
    CHECK_RC(launch_gemm_nt_uut_batch(rinv, 2 * n_pad + TILE, kinv, n_pad, n_pad, ng, s));
  }
  // 4. per member, in the single call's order
  for (int b = 0; b < nb; ++b) {
    PoolMember& M = mem[(size_t)b];
    const int gb = ids[b];
    double* sm = res.p + M.off;
    const double* zrow = M.A.p + M.n_pad;
    CHECK_RC(launch_rowsumsq(zrow, M.m_tot, M.N, 1, sm + M.T_c + 1, 0, s));
    CHECK_RC(launch_sum_array(sm, M.T_c, sm + M.T_c, s));
    CHECK_RC(launch_logpdf_final(sm + M.T_c, sm + M.T_c + 1, M.N, 1, sm + M.T_c + 2, s));
    if (!grad) continue;
    double* alpha = sm + M.T_c + 8;
    double* gn = alpha + M.n_pad;
    double* gc = gn + M.n_pad;
    double* gs = gc + M.nt;
    CHECK_RC(launch_gemv_rows(M.A.p + M.n_pad + TILE, M.m_tot, M.N, M.n_pad, zrow, M.m_tot, nullptr, alpha, s, 1));
    CHECK_RC(launch_mirror_lower(M.Kinv.p, M.n_pad, M.n_pad, s));
    if (PoolCall::at(call.grad_noise, gb))
      CHECK_RC(launch_grad_noise(M.Kinv.p, M.n_pad, alpha, M.N, M.nd.kind == SGP_NOISE_DIAG, gn, s));
    if (PoolCall::at(call.grad_coef, gb) || PoolCall::at(call.grad_inscale, gb))
      CHECK_RC(contract_spec(M.g.ds, M.Kinv.p, M.n_pad, alpha, M.T_c, M.T_c, M.part, gc, gs, s, pool_leave(), nullptr));
  }
  std::vector<double> h_res((size_t)res_len);
  std::vector<int> h_info((size_t)nb);
  int h_abort = 0;
  SGP_HIP(hipMemcpyAsync(h_res.data(), res.p, sizeof(double) * h_res.size(), hipMemcpyDeviceToHost, s));
  SGP_HIP(hipMemcpyAsync(h_info.data(), d_infos, sizeof(int) * nb, hipMemcpyDeviceToHost, s));
  SGP_HIP(hipMemcpyAsync(&h_abort, ctx->d_df_state + 1, sizeof(int), hipMemcpyDeviceToHost, s));
  SGP_HIP(hipStreamSynchronize(s));
  // the abort word is shared by every member of the launch: once raised, no member's result is complete, whatever its own
  // info says (a member that is already not positive definite loses the CAS that records the time-out in its info)
  bool timed_out = h_abort != 0;
  for (int b = 0; b < nb; ++b) timed_out = timed_out || h_info[(size_t)b] == SGP_DF_TIMEOUT;
  if (timed_out) {
    ctx->df_timed_out = true;   // (with_df_fallback reruns the call on the launch-based schedule: every member on its own)
    set_error("dataflow factorisation: a dependency wait inside the kernel ran into its bound (SGP_DF_TIMEOUT_S)");
    return -3;
  }
  for (int b = 0; b < nb; ++b) {
    const PoolMember& M = mem[(size_t)b];
    const int gb = ids[b];
    if (sizes) sizes->push_back(M.n_pad);
    if (h_info[(size_t)b] > 0) {
      call.note_bad(gb, h_info[(size_t)b]);
      continue;
    }
    const double* sm = h_res.data() + M.off;
    call.out[gb] = sm[M.T_c + 2];
    if (!grad) continue;
    const double* ha = sm + M.T_c + 8;
    const double* hn = ha + M.n_pad;
    const double* hc = hn + M.n_pad;
    const double* hs = hc + M.nt;
    const long nterms = (long)M.g.ds->h_terms.size();
    if (double* o = PoolCall::at(call.grad_y, gb))
      for (long i = 0; i < M.N; ++i) o[i] = -ha[i];
    if (double* o = PoolCall::at(call.grad_mean, gb))
      for (long i = 0; i < M.N; ++i) o[i] = ha[i];
    if (double* o = PoolCall::at(call.grad_noise, gb)) std::copy(hn, hn + (M.nd.kind == SGP_NOISE_DIAG ? M.N : 1), o);
    if (double* o = PoolCall::at(call.grad_coef, gb)) std::copy(hc, hc + nterms, o);
    if (double* o = PoolCall::at(call.grad_inscale, gb)) std::copy(hs, hs + nterms, o);
  }
  return 0;
}

// ---- the batch calls: members of ONE padded size, cut into launches in input order
// do all members pool, in one padded geometry?
bool batch_pools(const sgp_ctx* ctx, const PoolCall& call, int nspec, long* n_pad = nullptr, long* m_tot = nullptr) {
  bool pooled = nspec >= 2;
  long np0 = 0, np = 0, mt = 0;
  for (int b = 0; b < nspec && pooled; ++b) {
    pooled = poolable(ctx, call, b, &np, &mt) && (b == 0 || np == np0);
    np0 = np;
  }
  if (n_pad) *n_pad = np;
  if (m_tot) *m_tot = mt;
  return pooled;
}
// launches of at most `chunk` members; a launch the device memory does not suffice for hands its members and all later ones,
// [b0, nspec), to singles(b0)
template <class Singles>
int batch_chunks(sgp_ctx* ctx, PoolCall& call, int nspec, int chunk, Singles&& singles) {
  std::vector<int> ids((size_t)std::min(chunk, nspec));
  for (int b0 = 0; b0 < nspec; b0 += chunk) {
    const int nb = std::min(chunk, nspec - b0);
    for (int b = 0; b < nb; ++b) ids[(size_t)b] = b0 + b;
    const int rc = pooled_chunk(ctx, call, ids.data(), nb, nullptr);
    if (rc == CHUNK_NO_MEMORY) return singles(b0);
    CHECK_RC(rc);
  }
  return call.rc();
}

// ---- the pool calls: any sizes and noise kinds
struct PoolPlan {
  std::vector<int> single;                  // members that run through their own call, input order
  std::vector<std::vector<int>> chunks;     // poolable members, by task count (descending), at most DF_MAX_BATCH per launch
};
// geo(b, &n_pad, &m_tot) -> is member b poolable (and its geometry)
template <class Geo>
PoolPlan pool_plan(int nspec, Geo&& geo) {
  PoolPlan plan;
  std::vector<std::pair<long, int>> pooled;   // (tasks, member)
  for (int b = 0; b < nspec; ++b) {
    long n_pad = 0, m_tot = 0;
    if (geo(b, &n_pad, &m_tot)) pooled.emplace_back(df_ntasks((int)(m_tot / TILE), (int)(n_pad / TILE)), b);
    else plan.single.push_back(b);
  }
  std::stable_sort(pooled.begin(), pooled.end(), [](const std::pair<long, int>& x, const std::pair<long, int>& y) { return x.first > y.first; });
  for (size_t k = 0; k < pooled.size(); k += DF_MAX_BATCH) {
    const size_t e = std::min(pooled.size(), k + (size_t)DF_MAX_BATCH);
    if (e - k < 2) {   // a launch of one member is that member's own call
      plan.single.push_back(pooled[k].second);
      continue;
    }
    plan.chunks.emplace_back();
    for (size_t q = k; q < e; ++q) plan.chunks.back().push_back(pooled[q].second);
  }
  std::sort(plan.single.begin(), plan.single.end());
  return plan;
}
int pool_distinct(const std::vector<long>& sizes) {
  std::vector<long> u(sizes);
  std::sort(u.begin(), u.end());
  return (int)(std::unique(u.begin(), u.end()) - u.begin());
}
// the plan of both pool calls (the arguments are checked): the members that do not pool through their own calls, then one
// launch per chunk; a launch the device memory does not suffice for hands its chunk and the later ones to their own calls
int pool_run(sgp_ctx* ctx, PoolCall& call, int nspec, sgp_pool_report* report) {
  sgp_pool_report rep = {0, 0, 0, 0};
  if (report) *report = rep;
  const PoolPlan plan = pool_plan(nspec, [&](int b, long* n_pad, long* m_tot) { return poolable(ctx, call, b, n_pad, m_tot); });
  auto run_single = [&](int b) -> int {
    const int rc = call.own_call(ctx, b);
    if (rc < 0) return rc;
    if (rc > 0) call.note_bad(b, rc);
    rep.single_members += 1;
    return 0;
  };
  for (int b : plan.single) CHECK_RC(run_single(b));
  std::vector<long> sizes;
  CtxScope scope(ctx);
  for (size_t c = 0; c < plan.chunks.size(); ++c) {
    const std::vector<int>& ids = plan.chunks[c];
    const int rc = pooled_chunk(ctx, call, ids.data(), (int)ids.size(), &sizes);
    if (rc == CHUNK_NO_MEMORY) {
      std::vector<int> rest;
      for (size_t c2 = c; c2 < plan.chunks.size(); ++c2) rest.insert(rest.end(), plan.chunks[c2].begin(), plan.chunks[c2].end());
      std::sort(rest.begin(), rest.end());
      for (int b : rest) CHECK_RC(run_single(b));
      break;
    }
    CHECK_RC(rc);
    rep.pool_launches += 1;
    rep.pooled_members += (int)ids.size();
  }
  rep.distinct_sizes = pool_distinct(sizes);
  if (report) *report = rep;
  return call.rc();
}
}  // namespace

// sgp_logpdf_batch (include/sthenomi.h).  Members of different padded sizes, dense noise, sizes outside the batched range, a
// multi-GPU context: one after the other through sgp_logpdf's own path.
static int logpdf_batch_impl(sgp_ctx* ctx, int nspec, const sgp_cov_spec* const* specs, const double* const* means,
                             int noise_kind, const double* const* noises, const double* const* ys, double* out, int* infos) {
  CHECK_ARG(ctx && specs && noises && ys && out && nspec >= 1, "sgp_logpdf_batch: NULL argument");
  for (int b = 0; b < nspec; ++b) {
    CHECK_ARG(specs[b] && noises[b] && ys[b], "sgp_logpdf_batch: NULL member");
    CHECK_ARG(specs[b]->symmetric, "sgp_logpdf_batch: specs must be symmetric");
    if (infos) infos[b] = 0;
  }
  PoolCall call{"batch", false, specs, means, nullptr, noise_kind, noises, ys, out, nullptr, nullptr, nullptr, nullptr, nullptr, infos};
  // members [b0, nspec) one by one through their own call (whose error text stands)
  auto singles = [&](int b0) -> int {
    for (int b = b0; b < nspec; ++b) {
      const int rc = call.own_call(ctx, b);
      if (rc < 0) return rc;
      if (rc > 0) call.mark_bad(b, rc);
    }
    return call.rc();
  };
  if (!batch_pools(ctx, call, nspec)) return singles(0);
  CtxScope scope(ctx);
  return batch_chunks(ctx, call, nspec, DF_MAX_BATCH, singles);
}
extern "C" int sgp_logpdf_batch(sgp_ctx* ctx, int nspec, const sgp_cov_spec* const* specs, const double* const* means,
                                int noise_kind, const double* const* noises, const double* const* ys, double* out, int* infos) {
  return with_df_fallback(ctx, [&]() { return logpdf_batch_impl(ctx, nspec, specs, means, noise_kind, noises, ys, out, infos); });
}

// sgp_logpdf_grad_batch (include/sthenomi_batch.h) -- the optimiser loops of hyper-parameter learning run value AND gradient.
// Everything that does not pool (different padded sizes, dense noise, sizes the single call factors with the hybrid schedule
// or beyond SGP_BATCH_MAX_N, a multi-GPU context) goes member by member through sgp_logpdf_grad.
static int logpdf_grad_batch_impl(sgp_ctx* ctx, int nspec, const sgp_cov_spec* const* specs, const double* const* means,
                                  int noise_kind, const double* const* noises, const double* const* ys, double* logpdf_out,
                                  double* const* grad_y, double* const* grad_mean, double* const* grad_noise,
                                  double* const* grad_coef, double* const* grad_inscale, int* infos) {
  CHECK_ARG(ctx && specs && noises && ys && logpdf_out && nspec >= 1, "sgp_logpdf_grad_batch: NULL argument");
  CHECK_ARG(noise_kind >= SGP_NOISE_SCALAR && noise_kind <= SGP_NOISE_DENSE, "sgp_logpdf_grad_batch: bad noise kind");
  for (int b = 0; b < nspec; ++b) {
    CHECK_ARG(specs[b] && noises[b] && ys[b], "sgp_logpdf_grad_batch: NULL member");
    CHECK_ARG(specs[b]->symmetric, "sgp_logpdf_grad_batch: specs must be symmetric");
    CHECK_ARG(!spec_has_stencil(ctx, specs[b]), "sgp_logpdf_grad_batch: gradients through stencil terms are not supported");
    CHECK_ARG(!spec_has_patch(specs[b]), "sgp_logpdf_grad_batch: gradients through patch (convolutional) terms are not supported");
    CHECK_ARG(!spec_has_kprod(specs[b]), "sgp_logpdf_grad_batch: gradients through product chains and the RQ / LINEAR kinds are not supported: call sgp_logpdf_grad per member");
    if (infos) infos[b] = 0;
  }
  PoolCall call{"batch", true, specs, means, nullptr, noise_kind, noises, ys, logpdf_out, grad_y, grad_mean, grad_noise, grad_coef,
                grad_inscale, infos};
  // members [b0, nspec) one by one through their own call
  auto singles = [&](int b0) -> int {
    for (int b = b0; b < nspec; ++b) {
      const int rc = call.own_call(ctx, b);
      if (rc < 0) return rc;
      if (rc > 0) call.note_bad(b, rc);
    }
    return call.rc();
  };
  long n_pad = 0, m_tot = 0;
  if (!batch_pools(ctx, call, nspec, &n_pad, &m_tot)) return singles(0);
  CtxScope scope(ctx);
  // chunk size from the device memory left (the unused blocks of the context's cache count as free)
  const long T_c = n_pad / TILE;
  const double member_bytes =
      8.0 * ((double)m_tot * n_pad + (double)n_pad * n_pad + (double)T_c * INVD_STRIDE + 16.0 * T_c * T_c + 8.0 * n_pad);
  int chunk = DF_MAX_BATCH;
  {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
      double avail = (double)free_b;
      for (const auto& pb : ctx->pool)
        if (!pb.used) avail += (double)pb.bytes;
      chunk = (int)std::max(1.0, std::min((double)DF_MAX_BATCH, 0.9 * avail / member_bytes));
    } else {
      (void)hipGetLastError();
    }
  }
  return batch_chunks(ctx, call, nspec, chunk, singles);
}
// (the C entry point, sgp_logpdf_grad_batch, is in batch_entry.hip: libsthenomi_batch.so, include/sthenomi_batch.h)
int sgp::drv_logpdf_grad_batch(sgp_ctx* ctx, int nspec, const sgp_cov_spec* const* specs, const double* const* means,
                               int noise_kind, const double* const* noises, const double* const* ys, double* logpdf_out,
                               double* const* grad_y, double* const* grad_mean, double* const* grad_noise,
                               double* const* grad_coef, double* const* grad_inscale, int* infos) {
  return with_df_fallback(ctx, [&]() {
    return logpdf_grad_batch_impl(ctx, nspec, specs, means, noise_kind, noises, ys, logpdf_out, grad_y, grad_mean, grad_noise,
                                  grad_coef, grad_inscale, infos);
  });
}

// sgp_logpdf_pool (include/sthenomi_pool.h)
static int logpdf_pool_impl(sgp_ctx* ctx, int nspec, const sgp_cov_spec* const* specs, const double* const* means,
                            const int* kinds, const double* const* noises, const double* const* ys, double* out, int* infos,
                            sgp_pool_report* report) {
  CHECK_ARG(ctx && specs && kinds && noises && ys && out && nspec >= 1, "sgp_logpdf_pool: NULL argument");
  for (int b = 0; b < nspec; ++b) {
    CHECK_ARG(specs[b] && noises[b] && ys[b], "sgp_logpdf_pool: NULL member");
    CHECK_ARG(specs[b]->symmetric, "sgp_logpdf_pool: specs must be symmetric");
    CHECK_ARG(kinds[b] >= SGP_NOISE_SCALAR && kinds[b] <= SGP_NOISE_DENSE, "sgp_logpdf_pool: bad noise kind");
    if (infos) infos[b] = 0;
  }
  PoolCall call{"pool", false, specs, means, kinds, 0, noises, ys, out, nullptr, nullptr, nullptr, nullptr, nullptr, infos};
  return pool_run(ctx, call, nspec, report);
}
int sgp::drv_logpdf_pool(sgp_ctx* ctx, int nspec, const sgp_cov_spec* const* specs, const double* const* means,
                         const int* noise_kinds, const double* const* noises, const double* const* ys, double* out, int* infos,
                         sgp_pool_report* report) {
  return with_df_fallback(ctx, [&]() { return logpdf_pool_impl(ctx, nspec, specs, means, noise_kinds, noises, ys, out, infos, report); });
}

// sgp_logpdf_grad_pool (include/sthenomi_pool.h)
static int logpdf_grad_pool_impl(sgp_ctx* ctx, int nspec, const sgp_cov_spec* const* specs, const double* const* means,
                                 const int* kinds, const double* const* noises, const double* const* ys, double* logpdf_out,
                                 double* const* grad_y, double* const* grad_mean, double* const* grad_noise,
                                 double* const* grad_coef, double* const* grad_inscale, int* infos, sgp_pool_report* report) {
  CHECK_ARG(ctx && specs && kinds && noises && ys && logpdf_out && nspec >= 1, "sgp_logpdf_grad_pool: NULL argument");
  for (int b = 0; b < nspec; ++b) {
    CHECK_ARG(specs[b] && noises[b] && ys[b], "sgp_logpdf_grad_pool: NULL member");
    CHECK_ARG(specs[b]->symmetric, "sgp_logpdf_grad_pool: specs must be symmetric");
    CHECK_ARG(kinds[b] >= SGP_NOISE_SCALAR && kinds[b] <= SGP_NOISE_DENSE, "sgp_logpdf_grad_pool: bad noise kind");
    CHECK_ARG(!spec_has_stencil(ctx, specs[b]), "sgp_logpdf_grad_pool: gradients through stencil terms are not supported");
    CHECK_ARG(!spec_has_patch(specs[b]), "sgp_logpdf_grad_pool: gradients through patch (convolutional) terms are not supported");
    CHECK_ARG(!spec_has_kprod(specs[b]), "sgp_logpdf_grad_pool: gradients through product chains and the RQ / LINEAR kinds are not supported: call sgp_logpdf_grad per member");
    if (infos) infos[b] = 0;
  }
  PoolCall call{"pool", true, specs, means, kinds, 0, noises, ys, logpdf_out, grad_y, grad_mean, grad_noise, grad_coef, grad_inscale,
                infos};
  return pool_run(ctx, call, nspec, report);
}
int sgp::drv_logpdf_grad_pool(sgp_ctx* ctx, int nspec, const sgp_cov_spec* const* specs, const double* const* means,
                              const int* noise_kinds, const double* const* noises, const double* const* ys, double* logpdf_out,
                              double* const* grad_y, double* const* grad_mean, double* const* grad_noise,
                              double* const* grad_coef, double* const* grad_inscale, int* infos, sgp_pool_report* report) {
  return with_df_fallback(ctx, [&]() {
    return logpdf_grad_pool_impl(ctx, nspec, specs, means, noise_kinds, noises, ys, logpdf_out, grad_y, grad_mean, grad_noise,
                                 grad_coef, grad_inscale, infos, report);
  });
}

// ---------------------------------------------------------------------------------------
// posterior
// ---------------------------------------------------------------------------------------
// (struct sgp_post: ctx.h -- extend.hip grows the kept factor)

// rows <- rows * L^-T for `nrows` (multiple of 128) rows stored at R (ld = ldr), against the factor L
// (ld = ldl) with its stored inverse 16x16 diagonal blocks.  Blocked left-looking: a 512-column
// block first receives everything left of it in ONE deep GEMM (K = its column offset: the efficient
// shape of the MFMA kernel), then is solved in place in 128-column steps with K = 128 updates inside
// the block only.  Same flops as the right-looking sweep, a fraction of its C-tile traffic.
// the columns [c, c + w) of a block, everything left of the block already applied: by halving -- the left half, ONE update
// of the right half with it (K = the left half's width), the right half.  The same ascending-k accumulation per entry as
// 128-column steps with K = 128 updates of everything to their right (each launch seeds its accumulators with the stored
// value), at 2 / 3 of their C-tile traffic in a 512-column block.
static int row_trsm_block(double* R, long ldr, long nrows, const double* L, long ldl, const double* d_invall, long c, long w,
                          long solve_div, hipStream_t s) {
  if (w <= TILE)
    return launch_panel_solve(R + c * ldr, ldr, nrows, L + c + c * ldl, ldl, d_invall + (c / TILE) * INVD_STRIDE, 256, 16, s,
                              nullptr, solve_div);
  const long wl = (w / TILE + 1) / 2 * TILE;
  CHECK_RC(row_trsm_block(R, ldr, nrows, L, ldl, d_invall, c, wl, solve_div, s));
  CHECK_RC(launch_gemm_nt(R + c * ldr, ldr, L + (c + wl) + c * ldl, ldl, R + (c + wl) * ldr, ldr, nrows, w - wl, wl, -1.0, 1.0,
                          NOMASK, 0, 0, s));
  return row_trsm_block(R, ldr, nrows, L, ldl, d_invall, c + wl, w - wl, solve_div, s);
}
static int row_trsm(sgp_ctx* ctx, double* R, long ldr, long nrows, const double* L, long ldl,
                    const double* d_invall, long n_pad, hipStream_t s) {
  // (block width measured round 3 on the N = 262144, M = 4096 ELBO: 128 / 256 / 512 / 1024 columns -> row solve
  // 80.3 / 78.7 / 78.6 / 80.6 ms: flat -- the in-block part is not what bounds it; round 6, with the halving inside the block
  // and two solve workgroups per CU: 256 / 512 / 1024 / 2048 columns -> step 152.2 / 150.7 / 150.7 / 150.4 ms, against 154.2
  // for the 128-column steps with K = 128 updates -- profiles/r06_experiments/elbo_c4.md)
  const long WB = 4 * TILE;
  for (long c0 = 0; c0 < n_pad; c0 += WB) {
    long wb = std::min(WB, n_pad - c0);
    // (with a leading dimension beyond ~64k rows every operand column sits in its own page and a deep
    // contraction thrashes the TLB: fall back to 512-column slices there)
    const long KC = (ldr > 65536 || ldl > 65536) ? WB : c0;
    for (long k0 = 0; k0 < c0; k0 += KC)
      CHECK_RC(launch_gemm_nt(R + k0 * ldr, ldr, L + c0 + k0 * ldl, ldl, R + c0 * ldr, ldr, nrows, wb,
                              std::min(KC, c0 - k0), -1.0, 1.0, NOMASK, 0, 0, s));
    CHECK_RC(row_trsm_block(R, ldr, nrows, L, ldl, d_invall, c0, wb, 512, s));
  }
  return 0;
}

// back substitution kernels for alpha = L^-T z (reduce.hip would do; kept here: tiny)
__global__ void backsolve_gemvt_kernel(const double* L, long ld, long k0, long n_pad,
                                       const double* alpha, double* z) {
  // z[k0 + j] -= sum_{r >= k0+128} L[r, k0+j] * alpha[r], one workgroup per j
  __shared__ double sh[4];
  const int j = blockIdx.x;
  const double* col = L + (long)(k0 + j) * ld;
  double acc = 0.0;
  for (long r = k0 + TILE + threadIdx.x; r < n_pad; r += blockDim.x) acc = fma(col[r], alpha[r], acc);
  for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) z[k0 + j] -= (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
// alpha_k = L_kk^-T z_k for one 128-block: blocked back substitution over its eight 16x16
// sub-blocks, each diagonal solve an inverse product + one refinement step (as panel_solve_kernel).
// Thread (m, q): element m of the current sub-block, q = contraction lane (16 aligned lanes).
__global__ __launch_bounds__(256) void backsolve_diag_kernel(const double* invd, const double* Lkk, long ld,
                                                            const double* z, double* alpha, long k0) {
  __shared__ double zs[TILE], as[TILE], ts[16], a1s[16], rs[16];
  const int t = threadIdx.x, m = t >> 4, q = t & 15;
  if (t < TILE) zs[t] = z[k0 + t];
  __syncthreads();
  for (int c = 7; c >= 0; --c) {
    double acc = 0.0;  // sum_{p > c} L[16p + q][16c + m] a[16p + q]
    for (int p = c + 1; p < 8; ++p) acc = fma(Lkk[(16 * p + q) + (long)(16 * c + m) * ld], as[16 * p + q], acc);
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (q == 0) ts[m] = zs[16 * c + m] - acc;
    __syncthreads();
    const double iv = invd[c * 256 + m * 16 + q];  // inv(L_cc)[q][m]
    double v = iv * ts[q];
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    if (q == 0) a1s[m] = v;
    __syncthreads();
    double w = (q >= m) ? Lkk[(16 * c + q) + (long)(16 * c + m) * ld] * a1s[q] : 0.0;
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) w += __shfl_xor(w, off, 64);
    if (q == 0) rs[m] = ts[m] - w;  // t - L_cc' a1
    __syncthreads();
    double d = iv * rs[q];
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) d += __shfl_xor(d, off, 64);
    if (q == 0) as[16 * c + m] = a1s[m] + d;
    __syncthreads();
  }
  if (t < TILE) alpha[k0 + t] = as[t];
}

static int back_substitute_range(const double* Lv, long ld, const double* wall_v, long k_first, long k_last,
                                 long n_end, double* d_z, double* d_alpha, hipStream_t s) {
  for (long k0 = k_first; k0 >= k_last; k0 -= TILE) {
    if (k0 + TILE < n_end) {
      hipLaunchKernelGGL(backsolve_gemvt_kernel, dim3(TILE), dim3(256), 0, s, Lv, ld, k0, n_end, d_alpha, d_z);
      SGP_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(backsolve_diag_kernel, dim3(1), dim3(256), 0, s, wall_v + (k0 / TILE) * INVD_STRIDE,
                       Lv + k0 + k0 * ld, ld, d_z, d_alpha, k0);
    SGP_HIP(hipGetLastError());
  }
  return 0;
}
static int back_substitute(const sgp_post* post, double* d_z /*n_pad, overwritten*/,
                           double* d_alpha, hipStream_t s) {
  return back_substitute_range(post->dA, post->ld, post->d_wall, post->n_pad - TILE, 0, post->n_pad, d_z, d_alpha,
                               s);
}

__global__ void copy_strided_kernel(const double* src, long lds, long n, double* dst) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[i * lds];
}

extern "C" int sgp_posterior_destroy(sgp_post* p) {
  if (!p) return 0;
  if (p->mp) sgp_multi_posterior_destroy(p->mp);
  if (p->dA) hipFree(p->dA);
  if (p->d_wall) hipFree(p->d_wall);
  delete p;
  return 0;
}

static int sgp_posterior_create_impl(sgp_ctx* ctx, const sgp_cov_spec* spec, const double* mean,
                                    int noise_kind, const double* noise, const double* y,
                                    double* alpha_out, sgp_post** out) {
  CHECK_ARG(ctx && spec && y && out, "sgp_posterior_create: NULL argument");
  CHECK_ARG(spec->symmetric, "sgp_posterior_create: spec must be symmetric");
  CtxScope scope(ctx);
  REFUSE_KPROD_MULTI(ctx, spec);
  if (ctx->multi && noise) {
    sgp_mpost* mp = nullptr;
    CHECK_RC(sgp_multi_posterior_create(ctx, spec, mean, noise_kind, noise, y, alpha_out, &mp));
    sgp_post* post = new sgp_post();
    post->ctx = ctx;
    post->ctx_serial = ctx->serial;
    post->mp = mp;
    *out = post;
    return 0;
  }
  SpecGuard g;
  CHECK_RC(dspec_create(ctx, spec, &g.ds));
  long N = g.ds->N;
  CHECK_ARG(N >= 1, "sgp_posterior_create: empty data");
  int64_t n_pad, m_tot;
  sgp_geometry(N, 1, &n_pad, &m_tot);
  hipStream_t s = ctx->stream;
  DevBuf dmean, dY;
  NoiseDev nd;
  if (mean) CHECK_RC(dmean.upload(mean, N));
  CHECK_RC(upload_noise(nd, noise_kind, noise, N));
  CHECK_RC(dY.upload(y, N));
  sgp_post* post = new sgp_post();
  post->ctx = ctx;
  post->ctx_serial = ctx->serial;
  post->N = N;
  post->n_pad = n_pad;
  post->m_tot = m_tot;
  post->ld = m_tot;
  post->n_cap = n_pad;
  post->noise_kind = noise_kind;
  post->sigma2 = (noise_kind == SGP_NOISE_SCALAR && noise) ? noise[0] : 0.0;
  struct PostGuard {  // every error exit (incl. the SGP_HIP early returns) frees the 8 N^2-byte factor
    sgp_post* p;
    ~PostGuard() {
      if (p) sgp_posterior_destroy(p);
    }
  } guard{post};
  auto fail = [&](int rc) { return rc; };
  if (hipMalloc(&post->dA, sizeof(double) * m_tot * n_pad) != hipSuccess ||
      hipMalloc(&post->d_wall, sizeof(double) * (n_pad / TILE) * INVD_STRIDE) != hipSuccess) {
    set_error("sgp_posterior_create: hipMalloc failed");
    return fail(-2);
  }
  SGP_HIP(hipMemsetAsync(ctx->d_info, 0, sizeof(int), s));
  SzMask sz;
  int rc = build_bordered(ctx, g.ds, post->dA, n_pad, m_tot, mean ? dmean.p : nullptr, nd.kind,
                          nd.sigma2, nd.diag.p, nd.dense.p, nd.ld_dense, dY.p, N, 1, s, &sz);
  if (rc) return fail(rc);
  rc = chol_bordered(ctx, post->dA, m_tot, n_pad, m_tot, post->d_wall, s, 0, &sz);
  if (rc) return fail(rc);
  if (alpha_out) {
    DevBuf dz, dal;
    if (dz.alloc(n_pad) || dal.alloc(n_pad)) return fail(-2);
    hipLaunchKernelGGL(copy_strided_kernel, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, s,
                       post->dA + n_pad, post->ld, n_pad, dz.p);
    rc = back_substitute(post, dz.p, dal.p, s);
    if (rc) return fail(rc);
    SGP_HIP(hipStreamSynchronize(s));
    SGP_HIP(hipMemcpy(alpha_out, dal.p, sizeof(double) * N, hipMemcpyDeviceToHost));
  }
  int info = fetch_info(ctx, s);
  if (info < 0) return -3;
  if (info > 0) {
    set_error("matrix is not positive definite; Cholesky factorization failed at leading minor " +
              std::to_string(info));
    return fail(info);
  }
  guard.p = nullptr;
  *out = post;
  return 0;
}
extern "C" int sgp_posterior_create(sgp_ctx* ctx, const sgp_cov_spec* spec, const double* mean,
                                    int noise_kind, const double* noise, const double* y,
                                    double* alpha_out, sgp_post** out) {
  return with_df_fallback(ctx, [&]() { return sgp_posterior_create_impl(ctx, spec, mean, noise_kind, noise, y, alpha_out, out); });
}

// What the three predict entry points do past the solved cross rows (kept.h): mean and variance off them, the covariance
// K** - V V' (+ V2 V2') from the prior spec or the caller's prior_cov (leading dimension ldp), one drain, the copies back
struct PredictOut {
  double *mean, *var, *cov;
  int64_t ldcov;
};
static int predict_read(sgp_ctx* ctx, const Kept& k, CrossRows& R, const sgp_dspec* prior, const double* prior_var,
                        const double* prior_cov, long ldp, const PredictOut& o, hipStream_t s) {
  const long Ns = R.Ns, ns_pad = R.ns_pad;
  DevBuf dcov;
  if (o.mean) CHECK_RC(R.mean(k, s));
  if (o.var) {
    CHECK_ARG(prior || prior_var, "predict: prior_ss spec required for var");
    CHECK_RC(R.variance(ctx, k, prior, prior_var, s));
  }
  if (o.cov) {
    CHECK_ARG(prior || prior_cov, "predict: prior_ss spec required for cov");
    CHECK_RC(dcov.alloc((size_t)ns_pad * ns_pad));
    SGP_HIP(hipMemsetAsync(dcov.p, 0, sizeof(double) * ns_pad * ns_pad, s));
    if (prior)
      CHECK_RC(assemble(prior, dcov.p, ns_pad, 0, ns_pad / TILE, 0, ns_pad / TILE, 0, -1, 0.0, nullptr, s));
    else
      SGP_HIP(hipMemcpy2DAsync(dcov.p, sizeof(double) * ns_pad, prior_cov, sizeof(double) * ldp, sizeof(double) * Ns, (size_t)Ns,
                               hipMemcpyHostToDevice, s));
    CHECK_RC(launch_gemm_nt(R.V.p, ns_pad, R.V.p, ns_pad, dcov.p, ns_pad, ns_pad, ns_pad, k.n_pad, -1.0, 1.0, NOMASK, 0, 0, s));
    if (k.L2)
      CHECK_RC(launch_gemm_nt(R.V2.p, ns_pad, R.V2.p, ns_pad, dcov.p, ns_pad, ns_pad, ns_pad, k.n_pad, +1.0, 1.0, NOMASK, 0, 0, s));
  }
  SGP_HIP(hipStreamSynchronize(s));
  if (o.mean) SGP_HIP(hipMemcpy(o.mean, R.mu.p, sizeof(double) * Ns, hipMemcpyDeviceToHost));
  if (o.var) SGP_HIP(hipMemcpy(o.var, R.var.p, sizeof(double) * Ns, hipMemcpyDeviceToHost));
  if (o.cov)
    SGP_HIP(hipMemcpy2D(o.cov, sizeof(double) * o.ldcov, dcov.p, sizeof(double) * ns_pad, sizeof(double) * Ns, (size_t)Ns,
                        hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int sgp_posterior_predict(sgp_post* post, const sgp_cov_spec* cross,
                                     const sgp_cov_spec* prior_ss, const double* mean_s,
                                     double* mean_out, double* var_out, double* cov_out,
                                     int64_t ldcov) {
  CHECK_RC(kept_door(post, cross, "sgp_posterior_predict"));
  sgp_ctx* ctx = post->ctx;
  CtxScope scope(ctx);
  if (post->mp) return sgp_multi_posterior_predict(post->mp, cross, prior_ss, mean_s, mean_out, var_out, cov_out, ldcov);
  SpecGuard gc, gp;
  CHECK_RC(dspec_create(ctx, cross, &gc.ds));
  if (prior_ss) CHECK_RC(dspec_create(ctx, prior_ss, &gp.ds));
  long Ns = gc.ds->N;
  CHECK_ARG(gc.ds->M == post->N, "sgp_posterior_predict: cross spec columns != training size");
  CHECK_ARG(!gp.ds || gp.ds->N == Ns, "sgp_posterior_predict: prior_ss size != number of x*");
  CHECK_ARG(!cov_out || ldcov >= Ns, "sgp_posterior_predict: ldcov < Ns");
  if (Ns == 0) return 0;
  const Kept k = PostRef(post).kept();
  CrossRows R;
  CHECK_RC(R.solve(ctx, k, CrossSource{gc.ds, nullptr, 0, Ns, mean_s}, rup(Ns, TILE), ctx->stream));
  return predict_read(ctx, k, R, gp.ds, nullptr, nullptr, 0, PredictOut{mean_out, var_out, cov_out, ldcov}, ctx->stream);
}

// Predictions against a kept factor with the cross-covariance GIVEN as a matrix (round 5): what conditioning on top of a process
// that is not a prior Stheno process needs -- the approximate (VFE) posterior is an ordinary AbstractGP in the reference
// (src/gp/sparse_finite_gp.jl:60-62: posterior(VFE(f(z)), fx, y) can be observed and conditioned again), but its covariance
// is not a sum of kernel terms, so the flattened spec cannot say it.  The host evaluates cov(f, x*, x), var / cov(f, x*) and
// mean(f, x*) with the operators it has (on the device) and hands them over; the factor was built by sgp_posterior_create on
// the zero-term spec with dense noise = cov(f, x) + Sigma_y.
extern "C" int sgp_posterior_predict_explicit(sgp_post* post, const double* cross, int64_t ldc, int64_t ns,
                                              const double* prior_var, const double* prior_cov, int64_t ldp,
                                              const double* mean_s, double* mean_out, double* var_out, double* cov_out,
                                              int64_t ldcov) {
  CHECK_RC(kept_door(post, cross, "sgp_posterior_predict_explicit", "not available on a multi-GPU context's sharded factor", false));
  sgp_ctx* ctx = post->ctx;
  const long Ns = ns;
  CHECK_ARG(Ns >= 0 && ldc >= std::max<long>(Ns, 1), "sgp_posterior_predict_explicit: bad sizes");
  CHECK_ARG(!var_out || prior_var, "sgp_posterior_predict_explicit: prior_var required for var");
  CHECK_ARG(!cov_out || (prior_cov && ldp >= Ns && ldcov >= Ns), "sgp_posterior_predict_explicit: prior_cov required for cov");
  if (Ns == 0) return 0;
  CtxScope scope(ctx);
  const Kept k = PostRef(post).kept();
  CrossRows R;
  CHECK_RC(R.solve(ctx, k, CrossSource{nullptr, cross, (long)ldc, Ns, mean_s}, rup(Ns, TILE), ctx->stream));
  return predict_read(ctx, k, R, nullptr, prior_var, prior_cov, ldp, PredictOut{mean_out, var_out, cov_out, ldcov}, ctx->stream);
}

// ---------------------------------------------------------------------------------------
// VFE: elbo and sparse posterior (App. A.6)
// ---------------------------------------------------------------------------------------
// o[0] = sum log s2_n, o[1] = sum delta_n^2, o[2] = sum var_n / s2_n, delta_n = (y_n - m_n)/sqrt(s2_n)
// Two stages (round 5: one 256-thread block over N = 262144 elements took 1.2 ms of the c4 step, latency-bound on its four
// waves): up to 128 blocks stride over the elements and leave one partial sum each, one block adds the partials in a fixed
// order -- the result depends on N only, not on the launch.
constexpr int ELBO_SC_BLOCKS = 128;
__global__ void elbo_scalars_kernel(const double* y, const double* mean, const double* var_x,
                                    int noise_kind, double sigma2, const double* noise, long N,
                                    double* delta, double* rsig, double* part) {
  __shared__ double sh[3][4];
  double a0 = 0, a1 = 0, a2 = 0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long)gridDim.x * blockDim.x) {
    double s2 = noise_kind == 0 ? sigma2 : noise[i];
    double rs = 1.0 / sqrt(s2);
    double d = (y[i] - (mean ? mean[i] : 0.0)) * rs;
    delta[i] = d;
    rsig[i] = rs;
    a0 += log(s2);
    a1 = fma(d, d, a1);
    if (var_x) a2 += var_x[i] / s2;
  }
  for (int off = 32; off >= 1; off >>= 1) {
    a0 += __shfl_xor(a0, off, 64);
    a1 += __shfl_xor(a1, off, 64);
    a2 += __shfl_xor(a2, off, 64);
  }
  int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sh[0][w] = a0;
    sh[1][w] = a1;
    sh[2][w] = a2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 0; q < 3; ++q) part[q * ELBO_SC_BLOCKS + blockIdx.x] = (sh[q][0] + sh[q][1]) + (sh[q][2] + sh[q][3]);
  }
}
__global__ void elbo_scalars_sum_kernel(const double* part, int blocks, double* o) {   // <<<1, ELBO_SC_BLOCKS>>>
  __shared__ double sh[3][2];
  const int t = threadIdx.x;
  double a[3];
  for (int q = 0; q < 3; ++q) a[q] = t < blocks ? part[q * ELBO_SC_BLOCKS + t] : 0.0;
  for (int off = 32; off >= 1; off >>= 1)
    for (int q = 0; q < 3; ++q) a[q] += __shfl_xor(a[q], off, 64);
  if ((t & 63) == 0)
    for (int q = 0; q < 3; ++q) sh[q][t >> 6] = a[q];
  __syncthreads();
  if (t == 0)
    for (int q = 0; q < 3; ++q) o[q] = sh[q][0] + sh[q][1];
}
static int launch_elbo_scalars(sgp_ctx* ctx, const double* y, const double* mean, const double* var_x, int noise_kind,
                               double sigma2, const double* noise, long N, double* delta, double* rsig, double* o,
                               hipStream_t s) {
  // the partial sums live at the tail of the context's scalar buffer (the per-column sums of a many-column logpdf use its
  // head; a context runs one operator at a time)
  double* part = ctx->d_scal + ctx->n_scal - 3 * ELBO_SC_BLOCKS;
  const int blocks = (int)std::max<long>(1, std::min<long>(ELBO_SC_BLOCKS, (N + 255) / 256));
  hipLaunchKernelGGL(elbo_scalars_kernel, dim3((unsigned)blocks), dim3(256), 0, s, y, mean, var_x, noise_kind, sigma2, noise, N,
                     delta, rsig, part);
  SGP_HIP(hipGetLastError());
  hipLaunchKernelGGL(elbo_scalars_sum_kernel, dim3(1), dim3(ELBO_SC_BLOCKS), 0, s, (const double*)part, blocks, o);
  SGP_HIP(hipGetLastError());
  return 0;
}
// per column j of the bordered rows R (nrows x ncols): dots[j] = sum_n R[n, j] delta[n],
// sq[j] = sum_n R[n, j]^2
__global__ void coldot_kernel(const double* R, long ld, long nrows, const double* delta, double* dots, double* sq) {
  __shared__ double sh[2][4];
  const long j = blockIdx.x;
  const double* col = R + j * ld;
  double a = 0, b = 0;
  for (long n = threadIdx.x; n < nrows; n += blockDim.x) {
    double v = col[n];
    a = fma(v, delta[n], a);
    b = fma(v, v, b);
  }
  for (int off = 32; off >= 1; off >>= 1) {
    a += __shfl_xor(a, off, 64);
    b += __shfl_xor(b, off, 64);
  }
  int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sh[0][w] = a;
    sh[1][w] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    dots[j] = (sh[0][0] + sh[0][1]) + (sh[0][2] + sh[0][3]);
    sq[j] = (sh[1][0] + sh[1][1]) + (sh[1][2] + sh[1][3]);
  }
}
__global__ void add_identity_kernel(double* G, long ld, long n) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) G[i + i * ld] += 1.0;
}
__global__ void accum_kernel(double* dst, const double* src) { dst[0] += src[0]; }
__global__ void set_row_kernel(double* G, long ld, long row, const double* v, long n) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) G[row + i * ld] = v[i];
}

// (struct sgp_sparse_post: ctx.h -- postfx.hip reads the kept factors)

extern "C" int sgp_sparse_posterior_destroy(sgp_sparse_post* p) {
  if (!p) return 0;
  if (p->dLz) hipFree(p->dLz);
  if (p->d_wz) hipFree(p->d_wz);
  if (p->dG) hipFree(p->dG);
  if (p->d_wg) hipFree(p->d_wg);
  if (p->d_sums) hipFree(p->d_sums);
  delete p;
  return 0;
}

// The same pipeline for very many data points: K(z,z) is factored on its own and
// the rows K(x,z) Lambda go through in chunks of rows, each chunk a buffer of its own
// (leading dimension = chunk rows, so operand columns share pages and the TLB survives deep
// contractions): assemble -> scale -> blocked left-looking row solve (deep-K GEMMs against Lz) ->
// A delta / |A|^2 partials -> transpose -> split-K Gram partial, accumulated into G in chunk order
// (deterministic).  Nothing of size N x M is ever resident.
// Chunks of 65 536 rows (512 KB between operand columns, like the N = 65 536 factorisation) are as fast
// as the monolithic buffers on a good day (N = 262 144, M = 4096: 174 vs 177 ms) and three times
// faster on boxes where the monolithic 270 000-row leading dimension (2.1 MB between columns, every
// column in its own page) runs into the TLB: 628 ms there, same code, same inputs.  So anything
// beyond one chunk is chunked.  SGP_VFE_CHUNK=<rows> overrides both numbers (tests).
constexpr long VFE_CHUNK_ROWS = 65536;
constexpr long VFE_CHUNK_ABOVE = 65536;
static void vfe_chunking(long* chunk_rows, long* above) {
  const char* e = getenv("SGP_VFE_CHUNK");
  long v = e ? atol(e) / TILE * TILE : 0;
  *chunk_rows = v >= TILE ? v : VFE_CHUNK_ROWS;
  *above = v >= TILE ? v : VFE_CHUNK_ABOVE;
}

// The row-chunked pipeline is split in two so that the data points can be sharded (one
// exchange of M^2 + M + 2 doubles): `vfe_rows_partial` turns a slice of the data into its partial
// sums, `vfe_finish` consumes the (reduced) sums.  Layout of a "part" (device, contiguous):
//   G    (m_pad + 128) x m_pad, ld = m_pad + 128: lower tiles of sum_n a_n a_n' (no identity yet);
//        row m_pad is reserved for (A delta)'
//   dots m_pad: A delta
//   scal 8: [0] sum log s2_n, [1] delta' delta, [2] sum var_n / s2_n, [3] |A|_F^2
static long vfe_part_len(long m_pad) { return (m_pad + TILE) * m_pad + m_pad + 8; }

// dst[i] += src[i], i < n (n <= 8): the scalars of an appended batch join the kept ones
__global__ void accum_n_kernel(double* dst, const double* src, int n) {
  if ((int)threadIdx.x < n) dst[threadIdx.x] += src[threadIdx.x];
}

// The row half of vfe_rows_partial: the rows of `dx` (with their y, mean, var, noise) are turned into sums against a GIVEN
// factor Lz.  begin() uploads the rows' vectors and leaves their scalars, chunks() runs the row-chunk loop.
// append == 0: d_part is cleared and written (the first chunk overwrites, the later ones accumulate).
// append != 0: d_part holds the sums of earlier data (sgp_sparse_post::d_sums) and every chunk accumulates onto them from
// the first one on; the batch's four scalars are formed on their own and added to the kept ones.
struct VfeRows {
  sgp_ctx* ctx;
  const sgp_dspec* dx;
  long M, N, m_pad, n_rows, ldg;
  double *dG, *d_dots, *d_sc;
  int append;
  DevBuf dR, dAt, dPart, dy, dmean, dvar, ddelta, drsig, sq, dCs, sc_new;
  NoiseDev ndx;
  VfeRows(sgp_ctx* c, const sgp_dspec* x, long M_, double* d_part, int append_)
      : ctx(c), dx(x), M(M_), N(x->N), m_pad(rup(M_, TILE)), n_rows(rup(x->N, TILE)), ldg(rup(M_, TILE) + TILE),
        dG(d_part), d_dots(d_part + (rup(M_, TILE) + TILE) * rup(M_, TILE)), d_sc(d_dots + rup(M_, TILE)), append(append_) {}
  int upload(const double* var_x, const double* mean_x, int noise_kind, const double* noise_x, const double* y) {
    CHECK_RC(dy.upload(y, N));
    if (mean_x) CHECK_RC(dmean.upload(mean_x, N));
    if (var_x) CHECK_RC(dvar.upload(var_x, N));
    CHECK_RC(upload_noise(ndx, noise_kind, noise_x, N));
    return 0;
  }
  int alloc_rows() {
    CHECK_RC(ddelta.alloc(n_rows));
    CHECK_RC(drsig.alloc(n_rows));
    CHECK_RC(sq.alloc(m_pad));
    if (append) CHECK_RC(sc_new.alloc(8));
    return 0;
  }
  int scalars(bool has_mean, bool has_var) {
    hipStream_t s = ctx->stream;
    if (!append) SGP_HIP(hipMemsetAsync(dG, 0, sizeof(double) * vfe_part_len(m_pad), s));
    SGP_HIP(hipMemsetAsync(sq.p, 0, sizeof(double) * m_pad, s));
    SGP_HIP(hipMemsetAsync(ddelta.p, 0, sizeof(double) * n_rows, s));
    SGP_HIP(hipMemsetAsync(drsig.p, 0, sizeof(double) * n_rows, s));
    CHECK_RC(launch_elbo_scalars(ctx, dy.p, has_mean ? dmean.p : nullptr, has_var ? dvar.p : nullptr, ndx.kind, ndx.sigma2,
                                 ndx.diag.p, N, ddelta.p, drsig.p, append ? sc_new.p : d_sc, s));
    return 0;
  }
  int chunks(const double* dLz, const double* d_wz, StageTimer& tm) {
    hipStream_t s = ctx->stream;
    long CH, ch_above;
    vfe_chunking(&CH, &ch_above);
    CH = std::min(CH, n_rows);
    const int nsplit = 8;  // one K slice per XCD (gemm_nt.hip, klo == 3)
    const long stride = ldg * m_pad;
    CHECK_RC(dR.alloc((size_t)CH * m_pad));
    // (Round 4 also built "two chunks in flight" -- the Gram product of chunk c on the second stream while chunk c + 1 is assembled
    // and solved on the first; measured on the N = 262144, M = 4096 bound, profiles/r04_experiments/elbo_c4.txt: 159.7 -> 161.5 ms,
    // two MFMA-bound streams lose more to each other than the solve's substitutions leave idle.  Removed in round 6.)
    CHECK_RC(dAt.alloc((size_t)m_pad * CH));
    CHECK_RC(dCs.alloc((size_t)transpose_colsum_scratch(CH, m_pad)));
    {   // slabs of the chunk lengths actually used: the `sub` split depends on K % (8 sub 16), so a shorter LAST chunk can
        // need more slabs than a full one (advisor, round 4: SGP_VFE_CHUNK = 768, M = 4096, 1280 rows -> 8 vs 32)
      const long last = n_rows % CH == 0 ? std::min(CH, n_rows) : n_rows % CH;
      const long slabs = std::max(splitk_slabs(m_pad, std::min(CH, n_rows), nsplit), splitk_slabs(m_pad, last, nsplit));
      CHECK_RC(dPart.alloc((size_t)slabs * stride));
    }
    // ---- row chunks
    long chunk = 0;
    for (long r0 = 0; r0 < n_rows; r0 += CH, ++chunk) {
      const long ch = std::min(CH, n_rows - r0);            // rows of this chunk (multiple of 128)
      const long nv = std::max<long>(0, std::min(N - r0, ch));  // of which real data points
      const int acc = (append || r0 > 0) ? 1 : 0;
      double* At = dAt.p;
      tm.mark(1);
      // (a full chunk of an unpadded M is written entry for entry by the assembly: nothing to clear)
      if (nv < ch || M < m_pad) SGP_HIP(hipMemsetAsync(dR.p, 0, sizeof(double) * ch * m_pad, s));
      // global row r of K(x,z) lands at dR[(r - r0) + c * ch]
      CHECK_RC(assemble(dx, dR.p - r0, ch, r0 / TILE, (r0 + ch) / TILE, 0, m_pad / TILE, 0, -1, 0.0, nullptr, s));
      tm.mark(2);
      // The rows' Lambda_y^-1/2 factors commute with the solve (it acts on the inducing dimension): instead of a pass of
      // their own over the chunk before it (2 x 2.1 GB at N = 262 144, M = 4096: 0.9 ms per chunk) they are applied where
      // the solved rows are read anyway -- the column sums and the transposition (padded rows carry the factor 0)
      CHECK_RC(row_trsm(ctx, dR.p, ch, ch, dLz, m_pad, d_wz, m_pad, s));
      tm.mark(3);
      // (round 6: ONE pass over the solved rows -- the column sums ride with the transposition, 6.0 -> 3.6 ms per step at
      // N = 262 144, M = 4096)
      // (append: sq was cleared and counts this call's rows only -- accumulating onto its zeros from the first chunk on gives
      // the bits that writing gives, a sum of squares is never -0)
      CHECK_RC(launch_transpose_colsum(dR.p, ch, ch, m_pad, At, m_pad, drsig.p + r0, ddelta.p + r0, d_dots, sq.p, acc, dCs.p, s));
      tm.mark(4);
      // (the split-K slices need ch to be a multiple of 16 * nsplit = 128: it is)
      CHECK_RC(launch_gemm_nt_splitk(At, m_pad, At, m_pad, dPart.p, ldg, m_pad, m_pad, ch, nsplit, stride, 1, s));
      CHECK_RC(launch_splitk_reduce(dPart.p, stride, nsplit, dG, ldg, m_pad, m_pad, 1.0, acc ? 1.0 : 0.0, 1, s, ch));
    }
    tm.mark(5);
    if (append) {
      CHECK_RC(launch_sum_array(sq.p, m_pad, sc_new.p + 3, s));
      hipLaunchKernelGGL(accum_n_kernel, dim3(1), dim3(64), 0, s, d_sc, (const double*)sc_new.p, 4);
      SGP_HIP(hipGetLastError());
    } else {
      CHECK_RC(launch_sum_array(sq.p, m_pad, d_sc + 3, s));
    }
    SGP_HIP(hipStreamSynchronize(s));  // chunk buffers go back to the cache at scope exit
    return 0;
  }
};

static int vfe_rows_partial(sgp_ctx* ctx, const sgp_dspec* dz, const sgp_dspec* dx, const double* var_x,
                            const double* mean_x, int noise_kind, const double* noise_x, int z_noise_kind,
                            const double* z_noise, const double* y, double* dLz, double* d_wz, double* d_part,
                            StageTimer& tm) {
  const long M = dz->N, N = dx->N;
  const long m_pad = rup(M, TILE);
  hipStream_t s = ctx->stream;
  VfeRows rows(ctx, dx, M, d_part, 0);
  NoiseDev ndz;
  CHECK_RC(rows.upload(var_x, mean_x, noise_kind, noise_x, y));
  CHECK_RC(upload_noise(ndz, z_noise_kind, z_noise, M));
  CHECK_RC(rows.alloc_rows());
  tm.mark(0);
  SGP_HIP(hipMemsetAsync(ctx->d_info, 0, sizeof(int), s));
  CHECK_RC(rows.scalars(mean_x != nullptr, var_x != nullptr));
  // ---- Lz (replicated on every rank of a sharded run: M^3 / 3 flops, no communication)
  int nkz = ndz.kind == SGP_NOISE_DENSE ? -1 : ndz.kind;
  CHECK_RC(assemble(dz, dLz, m_pad, 0, m_pad / TILE, 0, m_pad / TILE, 1, nkz, ndz.sigma2, ndz.diag.p, s));
  if (ndz.kind == SGP_NOISE_DENSE) CHECK_RC(launch_add_dense(dLz, m_pad, ndz.dense.p, M, M, 1, s));
  CHECK_RC(launch_fill_pad(dLz, m_pad, M, m_pad, 0, m_pad, m_pad, 0, s));
  {
    // structural zeros (round 5): inducing points spread over independent processes give K(z,z) exact zero blocks, as they
    // give K(x,x) -- the same pattern machinery (no bordered rows here: T_r = T_c)
    SzMask szz;
    CHECK_RC(sz_build(ctx, dz, ndz.kind, m_pad, m_pad, s, &szz));
    CHECK_RC(chol_bordered(ctx, dLz, m_pad, m_pad, m_pad, d_wz, s, 0, szz.d_nz ? &szz : nullptr));
  }
  int info = fetch_info(ctx, s);
  if (info < 0) return -3;
  if (info > 0) {
    set_error("vfe: Kzz + Sigma_z is not positive definite (leading minor " + std::to_string(info) + ")");
    return info;
  }
  if (N == 0) return 0;
  return rows.chunks(dLz, d_wz, tm);
}

// h[0..5] as documented at vfe_pipeline; d_wg (optional) keeps the inverse diagonal blocks of Le
static int vfe_finish(sgp_ctx* ctx, double* d_part, long m_pad, double* d_wg, double* h, StageTimer& tm) {
  hipStream_t s = ctx->stream;
  const long ldg = m_pad + TILE;
  double* dG = d_part;
  double* d_dots = d_part + ldg * m_pad;
  double* d_sc = d_dots + m_pad;
  tm.mark(5);
  hipLaunchKernelGGL(add_identity_kernel, dim3((unsigned)((m_pad + 255) / 256)), dim3(256), 0, s, dG, ldg, m_pad);
  hipLaunchKernelGGL(set_row_kernel, dim3((unsigned)((m_pad + 255) / 256)), dim3(256), 0, s, dG, ldg, m_pad, d_dots,
                     m_pad);
  SGP_HIP(hipGetLastError());
  SGP_HIP(hipMemsetAsync(ctx->d_info, 0, sizeof(int), s));
  CHECK_RC(chol_bordered(ctx, dG, ldg, m_pad, ldg, d_wg, s));
  CHECK_RC(launch_sum_array(ctx->d_slots, m_pad / TILE, d_sc + 4, s));
  CHECK_RC(launch_rowsumsq(dG + m_pad, ldg, m_pad, 1, d_sc + 5, 0, s));
  SGP_HIP(hipMemcpyAsync(h, d_sc, sizeof(double) * 6, hipMemcpyDeviceToHost, s));
  tm.finish();
  int info = fetch_info(ctx, s);
  if (info < 0) return -3;
  if (info > 0) {
    set_error("vfe: A A' + I is not positive definite (leading minor " + std::to_string(info) + ")");
    return info;
  }
  return 0;
}

static int vfe_pipeline_chunked(sgp_ctx* ctx, const sgp_dspec* dz, const sgp_dspec* dx, const double* var_x,
                                const double* mean_x, int noise_kind, const double* noise_x, int z_noise_kind,
                                const double* z_noise, const double* y, double* h, sgp_sparse_post* keep) {
  const long M = dz->N;
  const long m_pad = rup(M, TILE);
  DevBuf dLz_local, dinv_local, dG_local;
  double *dLz = nullptr, *d_wz = nullptr, *d_part = nullptr;
  if (keep) {
    SGP_HIP(hipMalloc(&keep->dLz, sizeof(double) * m_pad * m_pad));
    SGP_HIP(hipMalloc(&keep->d_wz, sizeof(double) * (m_pad / TILE) * INVD_STRIDE));
    SGP_HIP(hipMalloc(&keep->dG, sizeof(double) * vfe_part_len(m_pad)));
    SGP_HIP(hipMalloc(&keep->d_wg, sizeof(double) * (m_pad / TILE) * INVD_STRIDE));
    dLz = keep->dLz;
    d_wz = keep->d_wz;
    d_part = keep->dG;
  } else {
    CHECK_RC(dLz_local.alloc((size_t)m_pad * m_pad));
    CHECK_RC(dinv_local.alloc((size_t)(m_pad / TILE) * INVD_STRIDE));
    CHECK_RC(dG_local.alloc((size_t)vfe_part_len(m_pad)));
    dLz = dLz_local.p;
    d_wz = dinv_local.p;
    d_part = dG_local.p;
  }
  StageTimer tm(ctx, ctx->stream);
  CHECK_RC(vfe_rows_partial(ctx, dz, dx, var_x, mean_x, noise_kind, noise_x, z_noise_kind, z_noise, y, dLz, d_wz,
                            d_part, tm));
  if (keep) {   // the sums, before the identity is added and the buffer factored (sgp_sparse_post::d_sums)
    SGP_HIP(hipMalloc(&keep->d_sums, sizeof(double) * vfe_part_len(m_pad)));
    SGP_HIP(hipMemcpyAsync(keep->d_sums, d_part, sizeof(double) * vfe_part_len(m_pad), hipMemcpyDeviceToDevice, ctx->stream));
    keep->n_total = dx->N;
  }
  CHECK_RC(vfe_finish(ctx, d_part, m_pad, keep ? keep->d_wg : nullptr, h, tm));
  if (keep) {
    keep->ctx = ctx;
    keep->ctx_serial = ctx->serial;
    keep->M = M;
    keep->m_pad = m_pad;
    keep->ldg = m_pad + TILE;
  }
  return 0;
}

// ---- N-sharded ELBO building blocks (device pointers, see sthenomi.h) ---------------
extern "C" int sgp_elbo_part_len(int64_t M, int64_t* len) {
  CHECK_ARG(M >= 1 && len, "sgp_elbo_part_len: bad argument");
  *len = vfe_part_len(rup(M, TILE));
  return 0;
}

// one rank's share: its slice of the data -> partial sums in d_part; the factor of K(z,z) + Sigma_z and its inverse
// diagonal blocks go to dLz (m_pad x m_pad) / d_wz when given (a sparse posterior keeps them), else to scratch
static int elbo_partial_core(sgp_ctx* ctx, const sgp_cov_spec* zz, const sgp_cov_spec* xz, const double* var_x,
                             const double* mean_x, int noise_kind, const double* noise_x, int z_noise_kind,
                             const double* z_noise, const double* y, double* dLz_keep, double* d_wz_keep,
                             double* d_part, int64_t part_len) {
  CHECK_ARG(ctx && zz && xz && noise_x && z_noise && d_part, "sgp_dev_elbo_partial: NULL argument");
  CHECK_ARG(zz->symmetric, "vfe: zz spec must be symmetric");
  CHECK_ARG(noise_kind == SGP_NOISE_SCALAR || noise_kind == SGP_NOISE_DIAG,
            "vfe: Sigma_y must be isotropic or diagonal (as in AbstractGPs.elbo)");
  CtxScope scope(ctx);
  SpecGuard gz, gx;
  CHECK_RC(dspec_create(ctx, zz, &gz.ds));
  CHECK_RC(dspec_create(ctx, xz, &gx.ds));
  const long M = gz.ds->N, N = gx.ds->N;
  CHECK_ARG(gx.ds->M == M && M >= 1, "vfe: xz spec columns != number of inducing points");
  CHECK_ARG(N == 0 || y, "sgp_dev_elbo_partial: NULL data");
  const long m_pad = rup(M, TILE);
  CHECK_ARG(part_len >= vfe_part_len(m_pad), "sgp_dev_elbo_partial: part buffer too small (sgp_elbo_part_len)");
  DevBuf dLz, dwz;
  if (!dLz_keep) CHECK_RC(dLz.alloc((size_t)m_pad * m_pad));
  if (!d_wz_keep) CHECK_RC(dwz.alloc((size_t)(m_pad / TILE) * INVD_STRIDE));
  StageTimer tm(ctx, ctx->stream);
  CHECK_RC(vfe_rows_partial(ctx, gz.ds, gx.ds, var_x, mean_x, noise_kind, noise_x, z_noise_kind, z_noise, y,
                            dLz_keep ? dLz_keep : dLz.p, d_wz_keep ? d_wz_keep : dwz.p, d_part, tm));
  tm.finish();
  return 0;
}

extern "C" int sgp_dev_elbo_partial(sgp_ctx* ctx, const sgp_cov_spec* zz, const sgp_cov_spec* xz,
                                    const double* var_x, const double* mean_x, int noise_kind,
                                    const double* noise_x, int z_noise_kind, const double* z_noise,
                                    const double* y, double* d_part, int64_t part_len) {
  CHECK_ARG(xz == nullptr || spec_rows_host(xz) == 0 || var_x, "sgp_dev_elbo_partial: NULL data");
  return elbo_partial_core(ctx, zz, xz, var_x, mean_x, noise_kind, noise_x, z_noise_kind, z_noise, y, nullptr, nullptr,
                           d_part, part_len);
}

static int elbo_finish_core(sgp_ctx* ctx, int64_t M, double* d_part, double* d_wg, double* h) {
  CtxScope scope(ctx);
  StageTimer tm(ctx, ctx->stream);
  return vfe_finish(ctx, d_part, rup(M, TILE), d_wg, h, tm);
}

extern "C" int sgp_dev_elbo_finish(sgp_ctx* ctx, int64_t M, int64_t N_total, double* d_part, double* out) {
  CHECK_ARG(ctx && d_part && out && M >= 1 && N_total >= 1, "sgp_dev_elbo_finish: bad argument");
  double h[6];
  CHECK_RC(elbo_finish_core(ctx, M, d_part, nullptr, h));
  double tmp = h[0] + h[4] + h[1] - h[5];
  double dtc = -0.5 * ((double)N_total * 1.8378770664093453 + tmp);
  out[0] = dtc - 0.5 * (h[2] - h[3]);
  return 0;
}

// shared VFE pipeline.  Returns elbo terms in h[0..5]:
//  h[0]=sum log s2, h[1]=delta'delta, h[2]=sum var/s2, h[3]=|A|_F^2, h[4]=logdet Le, h[5]=|Le^-1 A delta|^2
static int vfe_pipeline(sgp_ctx* ctx, const sgp_cov_spec* zz, const sgp_cov_spec* xz,
                        const double* var_x, const double* mean_x, int noise_kind,
                        const double* noise_x, int z_noise_kind, const double* z_noise,
                        const double* y, double* h, sgp_sparse_post* keep) {
  CHECK_ARG(zz->symmetric, "vfe: zz spec must be symmetric");
  CHECK_ARG(noise_kind == SGP_NOISE_SCALAR || noise_kind == SGP_NOISE_DIAG,
            "vfe: Sigma_y must be isotropic or diagonal (as in AbstractGPs.elbo)");
  SpecGuard gz, gx;
  CHECK_RC(dspec_create(ctx, zz, &gz.ds));
  CHECK_RC(dspec_create(ctx, xz, &gx.ds));
  long M = gz.ds->N, N = gx.ds->N;
  CHECK_ARG(gx.ds->M == M, "vfe: xz spec columns != number of inducing points");
  CHECK_ARG(M >= 1 && N >= 1, "vfe: empty inputs");
  long m_pad = rup(M, TILE), n_rows = rup(N, TILE);
  long ch_rows, ch_above;
  vfe_chunking(&ch_rows, &ch_above);
  if (n_rows > ch_above)
    return vfe_pipeline_chunked(ctx, gz.ds, gx.ds, var_x, mean_x, noise_kind, noise_x, z_noise_kind, z_noise, y, h,
                                keep);
  long ld = m_pad + n_rows;
  hipStream_t s = ctx->stream;
  DevBuf dA, dy, dmean, dvar, ddelta, drsig, dots, sq, dG_local;
  NoiseDev ndx, ndz;
  CHECK_RC(dA.alloc((size_t)ld * m_pad));
  CHECK_RC(dy.upload(y, N));
  if (mean_x) CHECK_RC(dmean.upload(mean_x, N));
  if (var_x) CHECK_RC(dvar.upload(var_x, N));
  CHECK_RC(upload_noise(ndx, noise_kind, noise_x, N));
  CHECK_RC(upload_noise(ndz, z_noise_kind, z_noise, M));
  CHECK_RC(ddelta.alloc(n_rows));
  CHECK_RC(drsig.alloc(n_rows));
  CHECK_RC(dots.alloc(m_pad));
  CHECK_RC(sq.alloc(m_pad));
  double* d_o = ctx->d_scal + 1;  // 3 scalars
  SGP_HIP(hipMemsetAsync(ctx->d_info, 0, sizeof(int), s));
  SGP_HIP(hipMemsetAsync(ddelta.p, 0, sizeof(double) * n_rows, s));
  SGP_HIP(hipMemsetAsync(drsig.p, 0, sizeof(double) * n_rows, s));
  CHECK_RC(launch_elbo_scalars(ctx, dy.p, mean_x ? dmean.p : nullptr,
                     var_x ? dvar.p : nullptr, ndx.kind, ndx.sigma2, ndx.diag.p, N, ddelta.p, drsig.p,
                     d_o, s));
  // top: Kzz + Sigma_z (lower), identity padding; bottom rows: K(x, z) Lambda_y^-1
  int nkz = ndz.kind == SGP_NOISE_DENSE ? -1 : ndz.kind;
  CHECK_RC(assemble(gz.ds, dA.p, ld, 0, m_pad / TILE, 0, m_pad / TILE, 1, nkz, ndz.sigma2, ndz.diag.p, s));
  if (ndz.kind == SGP_NOISE_DENSE) CHECK_RC(launch_add_dense(dA.p, ld, ndz.dense.p, M, M, 1, s));
  CHECK_RC(launch_fill_pad(dA.p, ld, M, m_pad, 0, m_pad, ld, 0, s));
  // zero the row padding of the bordered block, then assemble the cross block into it
  if (n_rows > N) {
    // rows [m_pad + N, ld) of every column
    SGP_HIP(hipMemset2DAsync(dA.p + m_pad + N, sizeof(double) * ld, 0, sizeof(double) * (n_rows - N),
                             (size_t)m_pad, s));
  }
  CHECK_RC(assemble(gx.ds, dA.p + m_pad, ld, 0, n_rows / TILE, 0, m_pad / TILE, 0, -1, 0.0, nullptr, s));
  CHECK_RC(launch_scale_rows(dA.p + m_pad, ld, N, m_pad, drsig.p, s));
  double* d_wz = nullptr;
  if (keep) {
    SGP_HIP(hipMalloc(&keep->d_wz, sizeof(double) * (m_pad / TILE) * INVD_STRIDE));
    d_wz = keep->d_wz;
  }
  // The N rows K(x,z) Lambda ride along as bordered rows of the factorisation (K = 512 updates).
  // Factoring Kzz alone and solving the rows with the deep-K row_trsm was tried: with a leading
  // dimension of 270 000 doubles every operand column lies in its own 2 MiB page and a K = 3584 GEMM
  // thrashes the TLB (N = 262 144, M = 4096: 225 -> 700 ms).
  {
    SzMask szz;   // structural zeros of K(z,z) (round 5); the N rows K(x,z) Lambda are dense bordered rows of the pattern
    CHECK_RC(sz_build(ctx, gz.ds, ndz.kind, m_pad, ld, s, &szz));
    CHECK_RC(chol_bordered(ctx, dA.p, ld, m_pad, ld, d_wz, s, 0, szz.d_nz ? &szz : nullptr));
  }
  int info = fetch_info(ctx, s);
  if (info < 0) return -3;
  if (info > 0) {
    set_error("vfe: Kzz + Sigma_z is not positive definite (leading minor " + std::to_string(info) + ")");
    return info;
  }
  // rows now hold A' (N x M).  A delta, |A|_F^2
  const double* R = dA.p + m_pad;
  hipLaunchKernelGGL(coldot_kernel, dim3((unsigned)m_pad), dim3(256), 0, s, R, ld, n_rows, ddelta.p,
                     dots.p, sq.p);
  SGP_HIP(hipGetLastError());
  CHECK_RC(launch_sum_array(sq.p, m_pad, ctx->d_scal + 4, s));
  // G = A A' + I, bordered with (A delta)'
  long ldg = m_pad + TILE;
  double* dG = nullptr;
  if (keep) {
    SGP_HIP(hipMalloc(&keep->dG, sizeof(double) * ldg * m_pad));
    SGP_HIP(hipMalloc(&keep->d_wg, sizeof(double) * (m_pad / TILE) * INVD_STRIDE));
    dG = keep->dG;
  } else {
    CHECK_RC(dG_local.alloc((size_t)ldg * m_pad));
    dG = dG_local.p;
  }
  SGP_HIP(hipMemsetAsync(dG, 0, sizeof(double) * ldg * m_pad, s));
  // G = A A' with the contraction over the N data points.  The rows hold A' (N x M, row index
  // contiguous = data point), so A (M x N) is formed by one coalesced transpose and the Gram
  // matrix runs on the NT MFMA kernel, split over K to fill the chip (few output tiles, huge K),
  // then reduced in fixed order.
  {
    DevBuf dAt, dPart;
    CHECK_RC(dAt.alloc((size_t)m_pad * n_rows));
    CHECK_RC(launch_transpose_add(R, ld, n_rows, m_pad, dAt.p, m_pad, nullptr, s));
    long tiles = (m_pad / TILE) * (m_pad / TILE + 1) / 2;
    int nsplit = 1;
    while (tiles * nsplit < 4096 && nsplit < 64 && (n_rows % (16L * nsplit * 2)) == 0 &&
           n_rows / (nsplit * 2) >= 2048)
      nsplit *= 2;
    long stride = ldg * m_pad;
    CHECK_RC(dPart.alloc((size_t)splitk_slabs(m_pad, n_rows, nsplit) * stride));
    CHECK_RC(launch_gemm_nt_splitk(dAt.p, m_pad, dAt.p, m_pad, dPart.p, ldg, m_pad, m_pad, n_rows, nsplit,
                                   stride, 1, s));
    CHECK_RC(launch_splitk_reduce(dPart.p, stride, nsplit, dG, ldg, m_pad, m_pad, 1.0, 0.0, 1, s, n_rows));
    SGP_HIP(hipStreamSynchronize(s));  // dAt / dPart are freed at scope exit
  }
  if (keep) {   // the sums in the part layout (vfe_part_len), before the identity is added and the buffer factored
    SGP_HIP(hipMalloc(&keep->d_sums, sizeof(double) * vfe_part_len(m_pad)));
    double* d_sd = keep->d_sums + ldg * m_pad;
    SGP_HIP(hipMemcpyAsync(keep->d_sums, dG, sizeof(double) * ldg * m_pad, hipMemcpyDeviceToDevice, s));
    SGP_HIP(hipMemcpyAsync(d_sd, dots.p, sizeof(double) * m_pad, hipMemcpyDeviceToDevice, s));
    SGP_HIP(hipMemsetAsync(d_sd + m_pad, 0, sizeof(double) * 8, s));
    SGP_HIP(hipMemcpyAsync(d_sd + m_pad, ctx->d_scal + 1, sizeof(double) * 4, hipMemcpyDeviceToDevice, s));
    keep->n_total = N;
  }
  hipLaunchKernelGGL(add_identity_kernel, dim3((unsigned)((m_pad + 255) / 256)), dim3(256), 0, s, dG,
                     ldg, m_pad);
  hipLaunchKernelGGL(set_row_kernel, dim3((unsigned)((m_pad + 255) / 256)), dim3(256), 0, s, dG, ldg,
                     m_pad, dots.p, m_pad);
  SGP_HIP(hipGetLastError());
  SGP_HIP(hipMemsetAsync(ctx->d_info, 0, sizeof(int), s));
  CHECK_RC(chol_bordered(ctx, dG, ldg, m_pad, ldg, keep ? keep->d_wg : nullptr, s));
  CHECK_RC(launch_sum_array(ctx->d_slots, m_pad / TILE, ctx->d_scal + 5, s));
  CHECK_RC(launch_rowsumsq(dG + m_pad, ldg, m_pad, 1, ctx->d_scal + 6, 0, s));
  SGP_HIP(hipMemcpyAsync(h, ctx->d_scal + 1, sizeof(double) * 6, hipMemcpyDeviceToHost, s));
  info = fetch_info(ctx, s);
  if (info < 0) return -3;
  if (info > 0) {
    set_error("vfe: A A' + I is not positive definite (leading minor " + std::to_string(info) + ")");
    return info;
  }
  if (keep) {
    keep->ctx = ctx;
    keep->ctx_serial = ctx->serial;
    keep->M = M;
    keep->m_pad = m_pad;
    keep->ldg = ldg;
    // keep Lz: copy the top m_pad x m_pad block
    SGP_HIP(hipMalloc(&keep->dLz, sizeof(double) * m_pad * m_pad));
    SGP_HIP(hipMemcpy2DAsync(keep->dLz, sizeof(double) * m_pad, dA.p, sizeof(double) * ld,
                             sizeof(double) * m_pad, (size_t)m_pad, hipMemcpyDeviceToDevice, s));
    SGP_HIP(hipStreamSynchronize(s));
  }
  return 0;
}

static int sgp_elbo_impl(sgp_ctx* ctx, const sgp_cov_spec* zz, const sgp_cov_spec* xz,
                        const double* var_x, const double* mean_x, int noise_kind,
                        const double* noise_x, int z_noise_kind, const double* z_noise,
                        const double* y, double* out) {
  CHECK_ARG(ctx && zz && xz && var_x && noise_x && z_noise && y && out, "sgp_elbo: NULL argument");
  REFUSE_KPROD_MULTI(ctx, zz);
  REFUSE_KPROD_MULTI(ctx, xz);
  CtxScope scope(ctx);
  if (ctx->multi && ctx->multi_nranks > 1)   // data points sharded over the ranks, one reduction of M^2 + M + 2 doubles
  {
    double hm[6];
    CHECK_RC(sgp_multi_vfe(ctx, zz, xz, var_x, mean_x, noise_kind, noise_x, z_noise_kind, z_noise, y, hm, nullptr, nullptr,
                           nullptr, nullptr));
    const long Nm = spec_rows_host(xz);
    out[0] = -0.5 * ((double)Nm * 1.8378770664093453 + hm[0] + hm[4] + hm[1] - hm[5]) - 0.5 * (hm[2] - hm[3]);
    return 0;
  }
  double h[6];
  CHECK_RC(vfe_pipeline(ctx, zz, xz, var_x, mean_x, noise_kind, noise_x, z_noise_kind, z_noise, y, h,
                        nullptr));
  long N = 0;
  for (int i = 0; i < xz->n_row_blocks; ++i) N += xz->row_len[i];
  // elbo = -(N log 2pi + logdet Sy + logdet Le + d'd - |Le^-1 A d|^2)/2 - (sum var/s2 - |A|_F^2)/2
  double tmp = h[0] + h[4] + h[1] - h[5];
  double dtc = -0.5 * ((double)N * 1.8378770664093453 + tmp);
  out[0] = dtc - 0.5 * (h[2] - h[3]);
  return 0;
}
extern "C" int sgp_elbo(sgp_ctx* ctx, const sgp_cov_spec* zz, const sgp_cov_spec* xz,
                        const double* var_x, const double* mean_x, int noise_kind,
                        const double* noise_x, int z_noise_kind, const double* z_noise,
                        const double* y, double* out) {
  return with_df_fallback(ctx, [&]() { return sgp_elbo_impl(ctx, zz, xz, var_x, mean_x, noise_kind, noise_x, z_noise_kind, z_noise, y, out); });
}

// ---------------------------------------------------------------------------------------
// elbo + reverse-mode gradient (second half).  Formulas: oracle/abstractgps.py
// elbo_gradient_wrt_cov (checked against finite differences there).  Both factorisations carry
// identity rows (row-limited, `grow`) so that J = Lz^-T and Le^-T come out of the panel solves:
//   dA' = R Z + delta u'          (R = A', Z = I - B^-1 - u u')
//   G_xz = Lambda (R Z J' + delta (J u)')                      -> contraction over the xz spec
//   G_zz = -1/2 J (B + B^-1 - 2 I + u u') J'                   -> contraction over the zz spec
// ---------------------------------------------------------------------------------------
static int elbo_grad_core(sgp_ctx* ctx, const ElboGradArgs& a, const ElboGradShard* shard) {
  // shard (round 6, multi.hip: sgp_multi_elbo_grad): this call sees ONE rank's slice of the data points (xz, var_x, mean_x, a
  // diagonal noise_x, y and the per-point results are the slice's).  The sums over data points -- A A', A delta, the four
  // scalar sums -- are added up over the ranks by shard->reduce (every rank gets the total), the M x M stage runs replicated
  // on identical numbers, the data-point stage on the slice; the zz-side results are the primary rank's business only.
  CHECK_ARG(ctx && a.zz && a.xz && a.var_x && a.noise_x && a.z_noise && a.y && a.elbo_out, "sgp_elbo_grad: NULL argument");
  CHECK_ARG(a.zz->symmetric, "sgp_elbo_grad: zz spec must be symmetric");
  CHECK_ARG(a.noise_kind == SGP_NOISE_SCALAR || a.noise_kind == SGP_NOISE_DIAG,
            "sgp_elbo_grad: Sigma_y must be isotropic or diagonal (as in AbstractGPs.elbo)");
  CHECK_ARG(a.z_noise_kind >= SGP_NOISE_SCALAR && a.z_noise_kind <= SGP_NOISE_DENSE, "sgp_elbo_grad: bad Sigma_z kind");
  CHECK_ARG(!spec_has_deriv(a.zz) && !spec_has_deriv(a.xz),
            "sgp_elbo_grad: gradients of the ELBO through derivative terms are not supported");
  CtxScope scope(ctx);
  SpecGuard gz, gx;
  CHECK_RC(dspec_create(ctx, a.zz, &gz.ds));
  CHECK_RC(dspec_create(ctx, a.xz, &gx.ds));
  const long M = gz.ds->N, N = gx.ds->N;
  // a patched side reads images, and gradients with respect to those are not formed (include/sthenomi_conv_grad.h)
  CHECK_ARG(images_unasked(gz.ds, a.grad_inputs_zz) && images_unasked(gx.ds, a.grad_inputs_xz),
            "sgp_elbo_grad_conv: an input read by a patch (convolutional) side holds images, and gradients with respect to "
            "images are not supported: its grad_inputs entry must be NULL");
  CHECK_ARG(gx.ds->M == M, "sgp_elbo_grad: xz spec columns != number of inducing points");
  CHECK_ARG(M >= 1 && N >= 1, "sgp_elbo_grad: empty inputs");
  const long m_pad = rup(M, TILE), n_rows = rup(N, TILE);
  const long ld = m_pad + n_rows + m_pad;   // [Kzz + Sigma_z ; K(x,z) Lambda ; I]
  const long ldg = m_pad + TILE + m_pad;    // [A A' + I ; (A delta)' ; I]
  hipStream_t s = ctx->stream;
  // (include/sthenomi_stencil_wo.h; no-ops throughout when no table is asked for, as on every sharded call -- the entry
  // refuses the stencil leave on a multi-GPU context)
  StencilWo wo_zz, wo_xz;
  wo_zz.gw = a.grad_weights_zz, wo_zz.go = a.grad_offsets_zz, wo_xz.gw = a.grad_weights_xz, wo_xz.go = a.grad_offsets_xz;
  CHECK_RC(wo_zz.prepare(gz.ds, "sgp_elbo_grad_stencil_wo", false, s));
  CHECK_RC(wo_xz.prepare(gx.ds, "sgp_elbo_grad_stencil_wo", false, s));
  DevBuf dA, dG, dB, dBinv, dZ, dS, dRZ, dT1, dGzz, dy, dmean, dvar, ddelta, drsig, dots, sq, du, dut, dgy, dgsy,
      dpart, dgcz, dgsz, dgcx, dgsx, dgpz, dgpx;
  NoiseDev ndx, ndz;
  CHECK_RC(dA.alloc((size_t)ld * m_pad));
  CHECK_RC(dG.alloc((size_t)ldg * m_pad));
  CHECK_RC(dB.alloc((size_t)m_pad * m_pad));
  CHECK_RC(dBinv.alloc((size_t)m_pad * m_pad));
  CHECK_RC(dZ.alloc((size_t)m_pad * m_pad));
  CHECK_RC(dS.alloc((size_t)m_pad * m_pad));
  CHECK_RC(dT1.alloc((size_t)m_pad * m_pad));
  CHECK_RC(dGzz.alloc((size_t)m_pad * m_pad));
  CHECK_RC(dRZ.alloc((size_t)n_rows * m_pad));
  CHECK_RC(dy.upload(a.y, N));
  if (a.mean_x) CHECK_RC(dmean.upload(a.mean_x, N));
  CHECK_RC(dvar.upload(a.var_x, N));
  CHECK_RC(upload_noise(ndx, a.noise_kind, a.noise_x, N));
  CHECK_RC(upload_noise(ndz, a.z_noise_kind, a.z_noise, M));
  CHECK_RC(ddelta.alloc(n_rows));
  CHECK_RC(drsig.alloc(n_rows));
  CHECK_RC(dots.alloc(m_pad));
  CHECK_RC(sq.alloc(m_pad));
  CHECK_RC(du.alloc(m_pad));
  CHECK_RC(dut.alloc(m_pad));
  CHECK_RC(dgy.alloc(N));
  CHECK_RC(dgsy.alloc(N));
  const size_t ntz = std::max<size_t>(1, gz.ds->h_terms.size()), ntx = std::max<size_t>(1, gx.ds->h_terms.size());
  CHECK_RC(dgcz.alloc(ntz));
  CHECK_RC(dgsz.alloc(ntz));
  CHECK_RC(dgcx.alloc(ntx));
  CHECK_RC(dgsx.alloc(ntx));
  SGP_HIP(hipMemsetAsync(dgcz.p, 0, sizeof(double) * ntz, s));
  SGP_HIP(hipMemsetAsync(dgsz.p, 0, sizeof(double) * ntz, s));
  SGP_HIP(hipMemsetAsync(dgcx.p, 0, sizeof(double) * ntx, s));
  SGP_HIP(hipMemsetAsync(dgsx.p, 0, sizeof(double) * ntx, s));
  if (a.grad_param_zz) {
    CHECK_RC(dgpz.alloc(ntz));
    SGP_HIP(hipMemsetAsync(dgpz.p, 0, sizeof(double) * ntz, s));
  }
  if (a.grad_param_xz) {
    CHECK_RC(dgpx.alloc(ntx));
    SGP_HIP(hipMemsetAsync(dgpx.p, 0, sizeof(double) * ntx, s));
  }
  double* d_o = ctx->d_scal + 1;  // h[0..2]; h[3] at +4, h[4] at +5, h[5] at +6
  SGP_HIP(hipMemsetAsync(ctx->d_info, 0, sizeof(int), s));
  SGP_HIP(hipMemsetAsync(ddelta.p, 0, sizeof(double) * n_rows, s));
  SGP_HIP(hipMemsetAsync(drsig.p, 0, sizeof(double) * n_rows, s));
  CHECK_RC(launch_elbo_scalars(ctx, dy.p, a.mean_x ? dmean.p : nullptr, dvar.p,
                     ndx.kind, ndx.sigma2, ndx.diag.p, N, ddelta.p, drsig.p, d_o, s));
  // ---- factor 1: [Kzz + Sigma_z ; K(x,z) Lambda ; I]  ->  Lz, R = A', J = Lz^-T
  double* Rw = dA.p + m_pad;
  double* Jm = dA.p + m_pad + n_rows;
  CHECK_RC(assemble(gz.ds, dA.p, ld, 0, m_pad / TILE, 0, m_pad / TILE, 1, ndz.kind == SGP_NOISE_DENSE ? -1 : ndz.kind,
                    ndz.sigma2, ndz.diag.p, s));
  if (ndz.kind == SGP_NOISE_DENSE) CHECK_RC(launch_add_dense(dA.p, ld, ndz.dense.p, M, M, 1, s));   // dense Sigma_z (M x M, ld M)
  CHECK_RC(launch_fill_pad(dA.p, ld, M, m_pad, 0, m_pad, ld, 0, s));
  if (n_rows > N)
    SGP_HIP(hipMemset2DAsync(Rw + N, sizeof(double) * ld, 0, sizeof(double) * (n_rows - N), (size_t)m_pad, s));
  CHECK_RC(assemble(gx.ds, Rw, ld, 0, n_rows / TILE, 0, m_pad / TILE, 0, -1, 0.0, nullptr, s));
  CHECK_RC(launch_scale_rows(Rw, ld, N, m_pad, drsig.p, s));
  SGP_HIP(hipMemset2DAsync(Jm, sizeof(double) * ld, 0, sizeof(double) * m_pad, (size_t)m_pad, s));
  hipLaunchKernelGGL(add_identity_kernel, dim3((unsigned)((m_pad + 255) / 256)), dim3(256), 0, s, Jm, ld, m_pad);
  SGP_HIP(hipGetLastError());
  CHECK_RC(chol_bordered(ctx, dA.p, ld, m_pad, ld, nullptr, s, m_pad + n_rows));
  int info = fetch_info(ctx, s);
  if (info < 0) return -3;
  if (info > 0) {
    set_error("vfe: Kzz + Sigma_z is not positive definite (leading minor " + std::to_string(info) + ")");
    return info;
  }
  const double* R = Rw;
  hipLaunchKernelGGL(coldot_kernel, dim3((unsigned)m_pad), dim3(256), 0, s, R, ld, n_rows, ddelta.p, dots.p, sq.p);
  SGP_HIP(hipGetLastError());
  CHECK_RC(launch_sum_array(sq.p, m_pad, ctx->d_scal + 4, s));
  // ---- B = A A' + I (transpose + split-K Gram, as in the forward pass), kept full in dB
  SGP_HIP(hipMemsetAsync(dG.p, 0, sizeof(double) * ldg * m_pad, s));
  {
    DevBuf dAt, dPart;
    CHECK_RC(dAt.alloc((size_t)m_pad * n_rows));
    CHECK_RC(launch_transpose_add(R, ld, n_rows, m_pad, dAt.p, m_pad, nullptr, s));
    long tiles = (m_pad / TILE) * (m_pad / TILE + 1) / 2;
    int nsplit = 1;
    while (tiles * nsplit < 4096 && nsplit < 64 && (n_rows % (16L * nsplit * 2)) == 0 &&
           n_rows / (nsplit * 2) >= 2048)
      nsplit *= 2;
    long stride = ldg * m_pad;
    CHECK_RC(dPart.alloc((size_t)splitk_slabs(m_pad, n_rows, nsplit) * stride));
    CHECK_RC(launch_gemm_nt_splitk(dAt.p, m_pad, dAt.p, m_pad, dPart.p, ldg, m_pad, m_pad, n_rows, nsplit, stride, 1,
                                   s));
    CHECK_RC(launch_splitk_reduce(dPart.p, stride, nsplit, dG.p, ldg, m_pad, m_pad, 1.0, 0.0, 1, s, n_rows));
    SGP_HIP(hipStreamSynchronize(s));
  }
  if (shard) {
    // the slice's sums, packed: A A' (m_pad x m_pad, lower), A delta (m_pad), h[0..3] -> summed over the ranks -> back
    const long mm = m_pad * m_pad, len = mm + m_pad + 8;
    DevBuf dP;
    CHECK_RC(dP.alloc((size_t)len));
    SGP_HIP(hipMemsetAsync(dP.p + mm + m_pad, 0, sizeof(double) * 8, s));
    SGP_HIP(hipMemcpy2DAsync(dP.p, sizeof(double) * m_pad, dG.p, sizeof(double) * ldg, sizeof(double) * m_pad, (size_t)m_pad,
                             hipMemcpyDeviceToDevice, s));
    SGP_HIP(hipMemcpyAsync(dP.p + mm, dots.p, sizeof(double) * m_pad, hipMemcpyDeviceToDevice, s));
    SGP_HIP(hipMemcpyAsync(dP.p + mm + m_pad, ctx->d_scal + 1, sizeof(double) * 4, hipMemcpyDeviceToDevice, s));
    SGP_HIP(hipStreamSynchronize(s));
    CHECK_RC(shard->reduce(dP.p, len));   // collective: returns on every rank with the total in place, visible to `s`
    SGP_HIP(hipMemcpy2DAsync(dG.p, sizeof(double) * ldg, dP.p, sizeof(double) * m_pad, sizeof(double) * m_pad, (size_t)m_pad,
                             hipMemcpyDeviceToDevice, s));
    SGP_HIP(hipMemcpyAsync(dots.p, dP.p + mm, sizeof(double) * m_pad, hipMemcpyDeviceToDevice, s));
    SGP_HIP(hipMemcpyAsync(ctx->d_scal + 1, dP.p + mm + m_pad, sizeof(double) * 4, hipMemcpyDeviceToDevice, s));
    SGP_HIP(hipStreamSynchronize(s));   // dP goes out of scope
  }
  hipLaunchKernelGGL(add_identity_kernel, dim3((unsigned)((m_pad + 255) / 256)), dim3(256), 0, s, dG.p, ldg, m_pad);
  SGP_HIP(hipMemcpy2DAsync(dB.p, sizeof(double) * m_pad, dG.p, sizeof(double) * ldg, sizeof(double) * m_pad,
                           (size_t)m_pad, hipMemcpyDeviceToDevice, s));
  CHECK_RC(launch_mirror_lower(dB.p, m_pad, m_pad, s));
  hipLaunchKernelGGL(set_row_kernel, dim3((unsigned)((m_pad + 255) / 256)), dim3(256), 0, s, dG.p, ldg, m_pad, dots.p,
                     m_pad);
  double* Je = dG.p + m_pad + TILE;
  hipLaunchKernelGGL(add_identity_kernel, dim3((unsigned)((m_pad + 255) / 256)), dim3(256), 0, s, Je, ldg, m_pad);
  SGP_HIP(hipGetLastError());
  // ---- factor 2: [B ; (A delta)' ; I]  ->  Le, b' = (Le^-1 A delta)', Je = Le^-T
  SGP_HIP(hipMemsetAsync(ctx->d_info, 0, sizeof(int), s));
  CHECK_RC(chol_bordered(ctx, dG.p, ldg, m_pad, ldg, nullptr, s, m_pad + TILE));
  CHECK_RC(launch_sum_array(ctx->d_slots, m_pad / TILE, ctx->d_scal + 5, s));
  CHECK_RC(launch_rowsumsq(dG.p + m_pad, ldg, m_pad, 1, ctx->d_scal + 6, 0, s));
  double h[6];
  SGP_HIP(hipMemcpyAsync(h, ctx->d_scal + 1, sizeof(double) * 6, hipMemcpyDeviceToHost, s));
  info = fetch_info(ctx, s);
  if (info < 0) return -3;
  if (info > 0) {
    set_error("vfe: A A' + I is not positive definite (leading minor " + std::to_string(info) + ")");
    return info;
  }
  {
    double tmp = h[0] + h[4] + h[1] - h[5];
    double dtc = -0.5 * ((double)(shard ? shard->n_total : N) * 1.8378770664093453 + tmp);
    a.elbo_out[0] = dtc - 0.5 * (h[2] - h[3]);
  }
  // ---- M x M stage
  CHECK_RC(launch_gemv_rows(Je, ldg, m_pad, m_pad, dG.p + m_pad, ldg, nullptr, du.p, s, 1));   // u = Le^-T b
  CHECK_RC(launch_gemm_nt_uut(Je, ldg, dBinv.p, m_pad, m_pad, s));                               // B^-1
  CHECK_RC(launch_mirror_lower(dBinv.p, m_pad, m_pad, s));
  CHECK_RC(launch_vfe_zs(dB.p, dBinv.p, du.p, dZ.p, dS.p, m_pad, s));
  CHECK_RC(launch_gemv_rows(Jm, ld, m_pad, m_pad, du.p, 1, nullptr, dut.p, s, 1));               // J u
  // ---- data-point stage: R Z, row statistics, G_xz
  CHECK_RC(launch_gemm_nt(R, ld, dZ.p, m_pad, dRZ.p, n_rows, n_rows, m_pad, m_pad, 1.0, 0.0, NOMASK, 0, 0, s));
  CHECK_RC(launch_vfe_rowstats(R, ld, dRZ.p, n_rows, du.p, ddelta.p, drsig.p, dvar.p, N, m_pad, dgy.p, dgsy.p, s));
  // E = (R Z) J' overwrites R's storage?  no: keep R intact, reuse the Gram scratch-sized dRZ -> new buffer
  DevBuf dE;
  CHECK_RC(dE.alloc((size_t)n_rows * m_pad));
  CHECK_RC(launch_gemm_nt(dRZ.p, n_rows, Jm, ld, dE.p, n_rows, n_rows, m_pad, m_pad, 1.0, 0.0, NOMASK, 0, 0, s));
  CHECK_RC(launch_vfe_gxz(dE.p, n_rows, ddelta.p, dut.p, drsig.p, n_rows, m_pad, s));
  // ---- G_zz = -1/2 J S J' (a sharded call: on the primary rank only)
  if (!shard || shard->primary) {
    CHECK_RC(launch_gemm_nt(Jm, ld, dS.p, m_pad, dT1.p, m_pad, m_pad, m_pad, m_pad, 1.0, 0.0, NOMASK, 0, 0, s));
    CHECK_RC(launch_gemm_nt(dT1.p, m_pad, Jm, ld, dGzz.p, m_pad, m_pad, m_pad, m_pad, -0.5, 0.0, NOMASK, 0, 0, s));
  }
  // ---- contractions against the flattened terms
  if (a.grad_coef_xz || a.grad_inscale_xz || a.grad_param_xz)
    CHECK_RC(contract_spec(gx.ds, dE.p, n_rows, nullptr, n_rows / TILE, m_pad / TILE, dpart, dgcx.p, dgsx.p, s, a.leave,
                           dgpx.p));
  if (a.grad_coef_zz || a.grad_inscale_zz || a.grad_param_zz)
    CHECK_RC(contract_spec(gz.ds, dGzz.p, m_pad, nullptr, m_pad / TILE, m_pad / TILE, dpart, dgcz.p, dgsz.p, s, a.leave,
                           dgpz.p));
  // ---- input points: zz is symmetric (twice the row side, as in logpdf_grad_core); xz is
  // rectangular: row side for the x inputs, and the transposed contraction for the z inputs.  Function-valued scales
  // sigma(x) * f (product.jl:25-48) ride along: the row side gives d / d rs (scales at x), the transposed pass d / d cs (at z)
  TermGradBufs bufs_zz, bufs_xz;
  CHECK_RC(bufs_zz.init(gz.ds, a.grad_inputs_zz, a.grad_rowscale_zz, nullptr, s));
  CHECK_RC(input_pass(gz.ds, {dGzz.p, m_pad, nullptr, true, &bufs_zz}, s));
  CHECK_RC(bufs_xz.init(gx.ds, a.grad_inputs_xz, a.grad_rowscale_xz, a.grad_colscale_xz, s));
  CHECK_RC(input_pass(gx.ds, {dE.p, n_rows, nullptr, false, &bufs_xz}, s));
  // ---- the stencils' own weights and offsets: G_zz is symmetric, the xz cotangent is read transposed for its column side
  CHECK_RC(wo_zz.contract(gz.ds, dGzz.p, m_pad, nullptr, true, s));
  CHECK_RC(wo_xz.contract(gx.ds, dE.p, n_rows, nullptr, false, s));
  SGP_HIP(hipStreamSynchronize(s));
  CHECK_RC(wo_zz.fetch());
  CHECK_RC(wo_xz.fetch());
  // ---- results
  std::vector<double> hy(N), hs(N);
  SGP_HIP(hipMemcpy(hy.data(), dgy.p, sizeof(double) * N, hipMemcpyDeviceToHost));
  SGP_HIP(hipMemcpy(hs.data(), dgsy.p, sizeof(double) * N, hipMemcpyDeviceToHost));
  if (a.grad_y)
    for (long i = 0; i < N; ++i) a.grad_y[i] = hy[i];
  if (a.grad_mean)
    for (long i = 0; i < N; ++i) a.grad_mean[i] = -hy[i];
  if (a.grad_noise) {
    if (a.noise_kind == SGP_NOISE_DIAG) {
      for (long i = 0; i < N; ++i) a.grad_noise[i] = hs[i];
    } else {
      double acc = 0.0;
      for (long i = 0; i < N; ++i) acc += hs[i];  // fixed order
      a.grad_noise[0] = acc;
    }
  }
  if (a.grad_var_x) {
    for (long i = 0; i < N; ++i) {
      double s2 = a.noise_kind == SGP_NOISE_SCALAR ? a.noise_x[0] : a.noise_x[i];
      a.grad_var_x[i] = -0.5 / s2;
    }
  }
  if (a.grad_z_noise && a.z_noise_kind == SGP_NOISE_DENSE) {
    // dense Sigma_z: the cotangent of Kzz + Sigma_z itself, M x M (ld M) -- as sgp_logpdf_grad returns G for a dense Sigma_y
    SGP_HIP(hipMemcpy2D(a.grad_z_noise, sizeof(double) * M, dGzz.p, sizeof(double) * m_pad, sizeof(double) * M, (size_t)M,
                        hipMemcpyDeviceToHost));
  } else if (a.grad_z_noise) {
    std::vector<double> dg(M);
    SGP_HIP(hipMemcpy2D(dg.data(), sizeof(double), dGzz.p, sizeof(double) * (m_pad + 1), sizeof(double), (size_t)M,
                        hipMemcpyDeviceToHost));
    if (a.z_noise_kind == SGP_NOISE_DIAG) {
      for (long i = 0; i < M; ++i) a.grad_z_noise[i] = dg[i];
    } else {
      double acc = 0.0;
      for (long i = 0; i < M; ++i) acc += dg[i];
      a.grad_z_noise[0] = acc;
    }
  }
  CHECK_RC(fetch_terms(gz.ds, a.grad_coef_zz, dgcz.p));
  CHECK_RC(fetch_terms(gz.ds, a.grad_inscale_zz, dgsz.p));
  CHECK_RC(fetch_terms(gz.ds, a.grad_param_zz, dgpz.p));
  CHECK_RC(fetch_terms(gx.ds, a.grad_coef_xz, dgcx.p));
  CHECK_RC(fetch_terms(gx.ds, a.grad_inscale_xz, dgsx.p));
  CHECK_RC(fetch_terms(gx.ds, a.grad_param_xz, dgpx.p));
  CHECK_RC(bufs_zz.fetch());
  CHECK_RC(bufs_xz.fetch());
  return 0;
}

// the front door of the family (driver.h): the leave checks, then a multi-GPU context shards the data points over its ranks
// (round 6).  The C entry points here and in the libraries beside this one fill a record and call it
int sgp::elbo_grad_entry(sgp_ctx* ctx, const ElboGradArgs& a) {
  CHECK_ARG(ctx, "sgp_elbo_grad: NULL context");
  CHECK_RC(check_grad_leave(ctx, "sgp_elbo_grad", a.leave, a.zz, a.xz));
  CHECK_ARG(a.leave.kprod || (!spec_has_kprod(a.zz) && !spec_has_kprod(a.xz)),
            "sgp_elbo_grad: gradients through product chains and the RQ / LINEAR kinds are not supported: call "
            "sgp_elbo_grad_param (include/sthenomi_kprod_grad.h)");
  CHECK_ARG(!(a.leave.kprod && ctx->multi), "sgp_elbo_grad_param: not supported on a multi-GPU context");
  if (ctx->multi && ctx->multi_nranks > 1) return sgp_multi_elbo_grad(ctx, a);
  return drv_elbo_grad(ctx, a, nullptr);
}

extern "C" int sgp_elbo_grad(sgp_ctx* ctx, const sgp_cov_spec* zz, const sgp_cov_spec* xz, const double* var_x,
                             const double* mean_x, int noise_kind, const double* noise_x, int z_noise_kind,
                             const double* z_noise, const double* y, double* elbo_out, double* grad_y,
                             double* grad_mean, double* grad_noise, double* grad_var_x, double* grad_z_noise,
                             double* grad_coef_zz, double* grad_inscale_zz, double* grad_coef_xz,
                             double* grad_inscale_xz) {
  return elbo_grad_entry(ctx, elbo_grad_args(zz, xz, var_x, mean_x, noise_kind, noise_x, z_noise_kind, z_noise, y, elbo_out,
                                             grad_y, grad_mean, grad_noise, grad_var_x, grad_z_noise, grad_coef_zz,
                                             grad_inscale_zz, grad_coef_xz, grad_inscale_xz));
}

extern "C" int sgp_elbo_grad_x(sgp_ctx* ctx, const sgp_cov_spec* zz, const sgp_cov_spec* xz, const double* var_x,
                               const double* mean_x, int noise_kind, const double* noise_x, int z_noise_kind,
                               const double* z_noise, const double* y, double* elbo_out, double* grad_y,
                               double* grad_mean, double* grad_noise, double* grad_var_x, double* grad_z_noise,
                               double* grad_coef_zz, double* grad_inscale_zz, double* grad_coef_xz,
                               double* grad_inscale_xz, double* const* grad_inputs_zz,
                               double* const* grad_inputs_xz) {
  CHECK_ARG(grad_inputs_zz && grad_inputs_xz, "sgp_elbo_grad_x: grad_inputs_* is NULL");
  ElboGradArgs a = elbo_grad_args(zz, xz, var_x, mean_x, noise_kind, noise_x, z_noise_kind, z_noise, y, elbo_out, grad_y,
                                  grad_mean, grad_noise, grad_var_x, grad_z_noise, grad_coef_zz, grad_inscale_zz, grad_coef_xz,
                                  grad_inscale_xz);
  a.grad_inputs_zz = grad_inputs_zz, a.grad_inputs_xz = grad_inputs_xz;
  return elbo_grad_entry(ctx, a);
}

extern "C" int sgp_elbo_grad_xs(sgp_ctx* ctx, const sgp_cov_spec* zz, const sgp_cov_spec* xz, const double* var_x,
                                const double* mean_x, int noise_kind, const double* noise_x, int z_noise_kind,
                                const double* z_noise, const double* y, double* elbo_out, double* grad_y,
                                double* grad_mean, double* grad_noise, double* grad_var_x, double* grad_z_noise,
                                double* grad_coef_zz, double* grad_inscale_zz, double* grad_coef_xz,
                                double* grad_inscale_xz, double* const* grad_inputs_zz,
                                double* const* grad_inputs_xz, double* const* grad_rowscale_zz,
                                double* const* grad_rowscale_xz, double* const* grad_colscale_xz) {
  ElboGradArgs a = elbo_grad_args(zz, xz, var_x, mean_x, noise_kind, noise_x, z_noise_kind, z_noise, y, elbo_out, grad_y,
                                  grad_mean, grad_noise, grad_var_x, grad_z_noise, grad_coef_zz, grad_inscale_zz, grad_coef_xz,
                                  grad_inscale_xz);
  a.grad_inputs_zz = grad_inputs_zz, a.grad_inputs_xz = grad_inputs_xz, a.grad_rowscale_zz = grad_rowscale_zz;
  a.grad_rowscale_xz = grad_rowscale_xz, a.grad_colscale_xz = grad_colscale_xz;
  return elbo_grad_entry(ctx, a);
}

// sum_i w[i] d var_i / d theta over the diagonal of `spec` (the blocks (I, I) kernelmatrix_diag reads)
static int diag_grad_core(sgp_ctx* ctx, const DiagGradArgs& a) {
  // (a.leave.kprod: sgp_kernelmatrix_diag_grad_param, include/sthenomi_kprod_grad.h -- every output may be NULL there, and
  // the conv / stencil families set it too; a.leave.patch: sgp_kernelmatrix_diag_grad_conv, include/sthenomi_conv_grad.h;
  // a.leave.stencil: sgp_kernelmatrix_diag_grad_stencil, include/sthenomi_stencil_grad.h)
  CHECK_ARG(ctx && a.spec && a.w && (a.leave.kprod || (a.grad_coef && a.grad_inscale)),
            "sgp_kernelmatrix_diag_grad: NULL argument");
  CHECK_ARG(!spec_has_deriv(a.spec),
            "sgp_kernelmatrix_diag_grad: gradients of the diagonal through derivative terms are not supported");
  CHECK_RC(check_grad_leave(ctx, "sgp_kernelmatrix_diag_grad", a.leave, a.spec));
  CHECK_ARG(a.leave.kprod || !spec_has_kprod(a.spec),
            "sgp_kernelmatrix_diag_grad: gradients through product chains and the RQ / LINEAR kinds are not supported: call "
            "sgp_kernelmatrix_diag_grad_param (include/sthenomi_kprod_grad.h)");
  CHECK_ARG(!(a.leave.kprod && ctx->multi), "sgp_kernelmatrix_diag_grad_param: not supported on a multi-GPU context");
  CtxScope scope(ctx);
  SpecGuard g;
  CHECK_RC(dspec_create(ctx, a.spec, &g.ds));
  const sgp_dspec* ds = g.ds;
  CHECK_ARG(ds->nrb == ds->ncb, "kernelmatrix_diag_grad: row / col block counts differ");
  CHECK_ARG(images_unasked(ds, a.grad_inputs),
            "sgp_kernelmatrix_diag_grad_stencil: an input read by a patch (convolutional) side holds images, and gradients with "
            "respect to images are not supported: its grad_inputs entry must be NULL");
  StencilWo wo;   // (include/sthenomi_stencil_wo.h; a no-op throughout when neither table is asked for)
  wo.gw = a.grad_weights, wo.go = a.grad_offsets;
  CHECK_RC(wo.prepare(ds, "sgp_kernelmatrix_diag_grad_stencil_wo", true, ctx->stream));
  size_t nt = ds->h_terms.size();
  for (size_t t = 0; t < nt; ++t) {
    if (a.grad_coef) a.grad_coef[t] = 0.0;
    if (a.grad_inscale) a.grad_inscale[t] = 0.0;
    if (a.grad_param) a.grad_param[t] = 0.0;
  }
  if (ds->N == 0 || nt == 0) {
    if (wo.asked()) {
      SGP_HIP(hipStreamSynchronize(ctx->stream));
      CHECK_RC(wo.fetch());
    }
    return 0;
  }
  DevBuf dw, dgc, dgs, dgp;
  CHECK_RC(dw.upload(a.w, ds->N));
  CHECK_RC(dgc.alloc(nt));
  CHECK_RC(dgs.alloc(nt));
  hipStream_t s = ctx->stream;
  SGP_HIP(hipMemsetAsync(dgc.p, 0, sizeof(double) * nt, s));
  SGP_HIP(hipMemsetAsync(dgs.p, 0, sizeof(double) * nt, s));
  if (a.grad_param) {
    CHECK_RC(dgp.alloc(nt));
    SGP_HIP(hipMemsetAsync(dgp.p, 0, sizeof(double) * nt, s));
  }
  // Only the diagonal pairs are read, class by class over all of them (PairSegs, spec_segments.h): the patch and stencil
  // terms' coefficients and scales, the plain terms', the input points, the plain terms' function scales, then the chains.
  auto diag_segs = [&](int I) { return pair_segments(ds, I * ds->ncb + I); };
  DevBuf dpart;
  if (ds->n_patch || ds->n_stencil) CHECK_RC(dpart.alloc((size_t)2 * ds->N));
  for (int I = 0; (ds->n_patch || ds->n_stencil) && I < ds->nrb; ++I) {
    const PairSegs g = diag_segs(I);
    if (ds->row_len[I] == 0 || ds->row_len[I] != ds->col_len[I]) continue;
    for (int t = g.tp; t < g.ts; ++t)   // (conv.hip)
      CHECK_RC(launch_diag_grad_conv(dw.p + ds->row_off[I], ds->row_len[I], ds->h_terms[t], ds->d_terms + t, dpart.p,
                                     dgc.p + t, dgs.p + t, s));
    for (int t = g.ts; t < g.tk; ++t)   // (stencil.hip)
      CHECK_RC(launch_diag_grad_stencil(dw.p + ds->row_off[I], ds->row_len[I], ds->h_terms[t], ds->d_terms + t, dpart.p,
                                        dgc.p + t, dgs.p + t, s));
  }
  for (int I = 0; I < ds->nrb; ++I) {
    CHECK_ARG(ds->row_len[I] == ds->col_len[I], "kernelmatrix_diag_grad: block lengths differ");
    const PairSegs g = diag_segs(I);
    if (ds->row_len[I] == 0 || g.tp == g.t0) continue;
    CHECK_RC(launch_diag_grad(dw.p + ds->row_off[I], ds->row_len[I], ds->d_terms + g.t0, g.tp - g.t0, dgc.p + g.t0,
                              dgs.p + g.t0, s));
    for (int t = g.t0; a.grad_param && t < g.tp; ++t)   // d / d param of a plain term: SGP_CONST alone, as a chain of length one
      if (ds->h_terms[t].kind == SGP_CONST)
        CHECK_RC(launch_diag_grad_kprod(dw.p + ds->row_off[I], ds->row_len[I], &ds->h_terms[t], 1, nullptr, nullptr,
                                        dgp.p + t, nullptr, nullptr, nullptr, nullptr, s));
  }
  TermGradBufs bufs;
  CHECK_RC(bufs.init(ds, a.grad_inputs, a.grad_rowscale, a.grad_colscale, s));
  for (int I = 0; a.grad_inputs && I < ds->nrb; ++I) {
    const PairSegs g = diag_segs(I);
    if (ds->row_len[I] == 0) continue;
    for (int t = g.t0; t < g.tp; ++t)
      CHECK_RC(launch_diag_grad_inputs(dw.p + ds->row_off[I], ds->row_len[I], ds->h_terms[t],
                                       bufs.input(ds->term_row_input[t]), bufs.input(ds->term_col_input[t]), s));
    for (int t = g.tp; t < g.ts; ++t) {   // patch terms: the plain side of a one-sided one is not formed here
      const DevTerm& T = ds->h_terms[t];
      CHECK_ARG((T.hr && T.hc) || !a.grad_inputs[T.hr ? ds->term_col_input[t] : ds->term_row_input[t]],
                "sgp_kernelmatrix_diag_grad_stencil: the input-point gradient of a one-sided patch (convolutional) term on "
                "the diagonal is not supported: the grad_inputs entry of its plain side must be NULL");
    }
    for (int t = g.ts; t < g.tk; ++t)   // stencil terms: + on the row input, - on the column input (stencil.hip)
      CHECK_RC(launch_diag_grad_stencil_points(dw.p + ds->row_off[I], ds->row_len[I], ds->h_terms[t],
                                               bufs.input(ds->term_row_input[t]), bufs.input(ds->term_col_input[t]), s));
  }
  for (int I = 0; (a.grad_rowscale || a.grad_colscale) && I < ds->nrb; ++I) {
    const PairSegs g = diag_segs(I);
    const long len = ds->row_len[I];
    for (int t = g.t0; t < g.tp; ++t) {
      double *o_r, *o_c;
      CHECK_RC(bufs.scale(t, 0, ds->h_terms[t].rs, len, &o_r));
      CHECK_RC(bufs.scale(t, 1, ds->h_terms[t].cs, len, &o_c));
      if (!o_r && !o_c) continue;
      CHECK_RC(launch_diag_scale_grad(dw.p + ds->row_off[I], len, ds->h_terms[t], o_r, o_c, s));
    }
  }
  // product chains: every gradient of a chain in one launch (kprod.hip)
  for (int I = 0; I < ds->nrb; ++I) {
    const PairSegs g = diag_segs(I);
    const long len = ds->row_len[I];
    if (len == 0) continue;
    for (int t = g.tk; t < g.t1;) {
      const int e = chain_end(ds, t, g.t1);
      double *o_r, *o_c, *gxr[SGP_KPROD_MAX_FACTORS], *gxc[SGP_KPROD_MAX_FACTORS];
      CHECK_RC(bufs.scale(t, 0, ds->h_terms[t].rs, len, &o_r));
      CHECK_RC(bufs.scale(t, 1, ds->h_terms[t].cs, len, &o_c));
      for (int f = t; f < e; ++f) gxr[f - t] = bufs.input(ds->term_row_input[f]), gxc[f - t] = bufs.input(ds->term_col_input[f]);
      CHECK_RC(launch_diag_grad_kprod(dw.p + ds->row_off[I], len, &ds->h_terms[t], e - t, dgc.p + t, dgs.p + t,
                                      a.grad_param ? dgp.p + t : nullptr, gxr, gxc, o_r, o_c, s));
      t = e;
    }
  }
  CHECK_RC(wo.contract_diag(ds, dw.p, s));   // the stencils' own weights and offsets (stencil.hip)
  SGP_HIP(hipStreamSynchronize(s));
  CHECK_RC(wo.fetch());
  CHECK_RC(fetch_terms(ds, a.grad_coef, dgc.p));
  CHECK_RC(fetch_terms(ds, a.grad_inscale, dgs.p));
  CHECK_RC(fetch_terms(ds, a.grad_param, dgp.p));
  CHECK_RC(bufs.fetch());
  return 0;
}

// the front door of the family (driver.h): the C entry points here and in the libraries beside this one fill a record, call it
int sgp::drv_diag_grad(sgp_ctx* ctx, const DiagGradArgs& a) { return diag_grad_core(ctx, a); }

extern "C" int sgp_kernelmatrix_diag_grad(sgp_ctx* ctx, const sgp_cov_spec* spec, const double* w,
                                          double* grad_coef, double* grad_inscale) {
  DiagGradArgs a;
  a.spec = spec, a.w = w, a.grad_coef = grad_coef, a.grad_inscale = grad_inscale;
  return drv_diag_grad(ctx, a);
}

extern "C" int sgp_kernelmatrix_diag_grad_x(sgp_ctx* ctx, const sgp_cov_spec* spec, const double* w,
                                            double* grad_coef, double* grad_inscale,
                                            double* const* grad_inputs) {
  CHECK_ARG(grad_inputs != nullptr, "sgp_kernelmatrix_diag_grad_x: grad_inputs is NULL");
  DiagGradArgs a;
  a.spec = spec, a.w = w, a.grad_coef = grad_coef, a.grad_inscale = grad_inscale, a.grad_inputs = grad_inputs;
  return drv_diag_grad(ctx, a);
}

extern "C" int sgp_kernelmatrix_diag_grad_xs(sgp_ctx* ctx, const sgp_cov_spec* spec, const double* w,
                                             double* grad_coef, double* grad_inscale, double* const* grad_inputs,
                                             double* const* grad_rowscale, double* const* grad_colscale) {
  DiagGradArgs a;
  a.spec = spec, a.w = w, a.grad_coef = grad_coef, a.grad_inscale = grad_inscale, a.grad_inputs = grad_inputs;
  a.grad_rowscale = grad_rowscale, a.grad_colscale = grad_colscale;
  return drv_diag_grad(ctx, a);
}

static int sgp_sparse_posterior_create_impl(sgp_ctx* ctx, const sgp_cov_spec* zz,
                                           const sgp_cov_spec* xz, const double* mean_x,
                                           int noise_kind, const double* noise_x, int z_noise_kind,
                                           const double* z_noise, const double* y,
                                           sgp_sparse_post** out) {
  CHECK_ARG(ctx && zz && xz && noise_x && z_noise && y && out, "sgp_sparse_posterior_create: NULL argument");
  REFUSE_KPROD_MULTI(ctx, zz);
  REFUSE_KPROD_MULTI(ctx, xz);
  CtxScope scope(ctx);
  sgp_sparse_post* p = new sgp_sparse_post();
  double h[6];
  if (ctx->multi && ctx->multi_nranks > 1) {
    // data points sharded over the ranks; the M x M factors of the posterior are kept on devices[0]
    const long M = spec_rows_host(zz), m_pad = rup(M, TILE);
    p->ctx = ctx;
    p->ctx_serial = ctx->serial;
    p->M = M;
    p->m_pad = m_pad;
    p->ldg = m_pad + TILE;
    int rc = 0;
    if (hipMalloc(&p->dLz, sizeof(double) * m_pad * m_pad) != hipSuccess ||
        hipMalloc(&p->d_wz, sizeof(double) * (m_pad / TILE) * INVD_STRIDE) != hipSuccess ||
        hipMalloc(&p->dG, sizeof(double) * vfe_part_len(m_pad)) != hipSuccess ||
        hipMalloc(&p->d_wg, sizeof(double) * (m_pad / TILE) * INVD_STRIDE) != hipSuccess) {
      (void)hipGetLastError();
      set_error("sgp_sparse_posterior_create: hipMalloc failed");
      rc = -2;
    }
    if (!rc)
      rc = sgp_multi_vfe(ctx, zz, xz, nullptr, mean_x, noise_kind, noise_x, z_noise_kind, z_noise, y, h, p->dLz, p->d_wz,
                         p->dG, p->d_wg);
    if (rc) {
      sgp_sparse_posterior_destroy(p);
      return rc;
    }
    *out = p;
    return 0;
  }
  int rc = vfe_pipeline(ctx, zz, xz, nullptr, mean_x, noise_kind, noise_x, z_noise_kind, z_noise, y,
                        h, p);
  if (rc) {
    sgp_sparse_posterior_destroy(p);
    return rc;
  }
  *out = p;
  return 0;
}
extern "C" int sgp_sparse_posterior_create(sgp_ctx* ctx, const sgp_cov_spec* zz,
                                           const sgp_cov_spec* xz, const double* mean_x,
                                           int noise_kind, const double* noise_x, int z_noise_kind,
                                           const double* z_noise, const double* y,
                                           sgp_sparse_post** out) {
  return with_df_fallback(ctx, [&]() { return sgp_sparse_posterior_create_impl(ctx, zz, xz, mean_x, noise_kind, noise_x, z_noise_kind, z_noise, y, out); });
}

// B' = K(x*, z) Lz^-T, C' = B' Le^-T (always solved);  mean* = m* + K*z alpha, alpha = Lz^-T Le^-T (Le^-1 A delta)
// =>  mean* = m* + C' (Le^-1 A delta);  var* = k** - |B|^2 + |C|^2
extern "C" int sgp_sparse_posterior_predict(sgp_sparse_post* post, const sgp_cov_spec* cross,
                                            const sgp_cov_spec* prior_ss, const double* mean_s,
                                            double* mean_out, double* var_out, double* cov_out,
                                            int64_t ldcov) {
  CHECK_RC(kept_door(post, cross, "sgp_sparse_posterior_predict"));
  sgp_ctx* ctx = post->ctx;
  CtxScope scope(ctx);
  SpecGuard gc, gp;
  CHECK_RC(dspec_create(ctx, cross, &gc.ds));
  if (prior_ss) CHECK_RC(dspec_create(ctx, prior_ss, &gp.ds));
  long Ns = gc.ds->N;
  CHECK_ARG(gc.ds->M == post->M, "sparse predict: cross spec columns != number of inducing points");
  CHECK_ARG(!gp.ds || gp.ds->N == Ns, "sparse predict: prior_ss size != number of x*");
  CHECK_ARG(!cov_out || ldcov >= Ns, "sparse predict: ldcov < Ns");
  if (Ns == 0) return 0;
  const Kept k = PostRef(post).kept();
  CrossRows R;
  CHECK_RC(R.solve(ctx, k, CrossSource{gc.ds, nullptr, 0, Ns, mean_s}, rup(Ns, TILE), ctx->stream));
  return predict_read(ctx, k, R, gp.ds, nullptr, nullptr, 0, PredictOut{mean_out, var_out, cov_out, ldcov}, ctx->stream);
}

// ---------------------------------------------------------------------------------------
// multi-GPU building blocks (device pointers)
// ---------------------------------------------------------------------------------------
extern "C" int sgp_dev_assemble_cols(sgp_ctx* ctx, const sgp_dspec* ds, int64_t N, int64_t c0,
                                     int64_t nc, double* d_dst, int64_t ldd, int64_t m_tot,
                                     const double* d_mean, int noise_kind, const double* noise_host,
                                     const double* d_noise, const double* d_Y, int64_t ldy,
                                     int64_t ncols, void* stream) {
  CHECK_ARG(ctx && ds && d_dst, "sgp_dev_assemble_cols: NULL argument");
  CHECK_ARG(ds->symmetric && ds->N == N, "sgp_dev_assemble_cols: spec must be symmetric of size N");
  CHECK_ARG(c0 % TILE == 0 && nc % TILE == 0, "sgp_dev_assemble_cols: c0, nc must be multiples of 128");
  CHECK_ARG(noise_kind == SGP_NOISE_SCALAR || noise_kind == SGP_NOISE_DIAG, "bad noise kind");
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);  // ctx scratch (logdet slots, inverse blocks) is shared
  SGP_HIP(hipSetDevice(ctx->device));
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  int64_t n_pad, mt;
  sgp_geometry(N, ncols, &n_pad, &mt);
  // ldd >= m_tot - c0: a panel may be stored packed (rows c0 .. m_tot only); the caller then passes the
  // virtual address of global row 0 (first stored row minus c0), which is never dereferenced above row c0
  // m_tot > mt: the caller appends more bordered rows below the observation rows (sgp_dev_assemble_cross_rows)
  CHECK_ARG(mt <= m_tot && m_tot % TILE == 0 && ldd >= m_tot - c0, "sgp_dev_assemble_cols: geometry mismatch");
  double* Kv = d_dst - c0 * ldd;  // virtual base: global column index
  double s2 = noise_host ? noise_host[0] : 0.0;
  CHECK_RC(assemble(ds, Kv, ldd, c0 / TILE, n_pad / TILE, c0 / TILE, (c0 + nc) / TILE, 1, noise_kind,
                    s2, d_noise, s));
  CHECK_RC(launch_fill_pad(d_dst, ldd, N, n_pad, c0, nc, m_tot, c0, s));
  CHECK_RC(launch_border_rows(d_dst, ldd, n_pad, N, c0, nc, d_Y, ldy, ncols, d_mean, s));
  return 0;
}

// Sharded posterior (AbstractGPs.posterior + mean / var / cov of the PosteriorGP [EXT], App. A.5):
// K(x*, x) rides through the sharded factorisation as extra bordered rows and comes out as V' = K(x*, x) L^-T,
// next to the observation row z' = (L^-1 (y - m))'; then  mean* = m* + V' z,  var* = k** - rowsumsq(V'),
// cov* = K** - V' V  are sums over columns = over ranks: one all-reduce of 2 n* (+ n*^2) doubles.
extern "C" int sgp_dev_assemble_cross_rows(sgp_ctx* ctx, const sgp_dspec* cross, int64_t c0, int64_t nc,
                                           double* d_dst, int64_t ldd, int64_t row0, void* stream) {
  CHECK_ARG(ctx && cross && d_dst, "sgp_dev_assemble_cross_rows: NULL argument");
  CHECK_ARG(!cross->symmetric, "sgp_dev_assemble_cross_rows: needs a cross-covariance spec (rows x*, columns x)");
  CHECK_ARG(c0 % TILE == 0 && nc % TILE == 0 && row0 % TILE == 0 && row0 >= c0 + nc,
            "sgp_dev_assemble_cross_rows: c0, nc, row0 must be multiples of 128, rows below the square part");
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  SGP_HIP(hipSetDevice(ctx->device));
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  const long ns = cross->N, Nx = cross->M;
  const long ns_pad = (ns + TILE - 1) / TILE * TILE;
  CHECK_ARG(ldd >= row0 + ns_pad - c0, "sgp_dev_assemble_cross_rows: leading dimension too small");
  const long nc_valid = std::max<long>(0, std::min<long>(nc, Nx - c0));   // columns >= Nx are identity padding
  if (nc_valid > 0) {
    double* Kv = d_dst + row0 - c0 * ldd;   // element (r, c) of K(x*, x) at Kv[r + c * ldd]
    CHECK_RC(assemble(cross, Kv, ldd, 0, ns_pad / TILE, c0 / TILE, (c0 + nc) / TILE, 0, -1, 0.0, nullptr, s));
    CHECK_RC(launch_zero_rows(d_dst, ldd, row0 + ns, row0 + ns_pad, nc_valid, s));
  }
  if (nc_valid < nc) CHECK_RC(launch_zero_rows(d_dst + nc_valid * ldd, ldd, row0, row0 + ns_pad, nc - nc_valid, s));
  return 0;
}

extern "C" int sgp_dev_rows_dot(sgp_ctx* ctx, const double* d_rows, int64_t ld, int64_t nrows, int64_t nc,
                                const double* d_zrow, double* d_sumsq, double* d_dot, void* stream) {
  CHECK_ARG(ctx && d_rows && d_zrow && d_sumsq && d_dot, "sgp_dev_rows_dot: NULL argument");
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  SGP_HIP(hipSetDevice(ctx->device));
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  return launch_rows_dot(d_rows, ld, nrows, nc, d_zrow, d_sumsq, d_dot, s);
}

// G (nrows_pad x nrows_pad, ld ldg, all tiles) += R R' over the nc columns of the bordered rows R
extern "C" int sgp_dev_rows_gram(sgp_ctx* ctx, const double* d_rows, int64_t ld, int64_t nrows_pad, int64_t nc,
                                 double* d_G, int64_t ldg, void* stream) {
  CHECK_ARG(ctx && d_rows && d_G, "sgp_dev_rows_gram: NULL argument");
  CHECK_ARG(nrows_pad % TILE == 0 && nc % 16 == 0 && ldg >= nrows_pad, "sgp_dev_rows_gram: bad sizes");
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  SGP_HIP(hipSetDevice(ctx->device));
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  return launch_gemm_nt(d_rows, ld, d_rows, ld, d_G, ldg, nrows_pad, nrows_pad, nc, 1.0, 1.0, NOMASK, 0, 0, s);
}

extern "C" int sgp_dev_panel_factor(sgp_ctx* ctx, double* d_P, int64_t ld, int64_t m, int64_t w,
                                    int64_t g0, double* d_logdet, int* d_info, void* stream) {
  CHECK_ARG(ctx && d_P && d_logdet && d_info, "sgp_dev_panel_factor: NULL argument");
  CHECK_ARG(w % TILE == 0 && m % TILE == 0 && m >= w, "sgp_dev_panel_factor: bad sizes");
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);  // ctx scratch (logdet slots, inverse blocks) is shared
  SGP_HIP(hipSetDevice(ctx->device));
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  // per-block logdet slots live in ctx scratch; accumulate their sum into d_logdet[0]
  FuseScope fuse_scope(ctx, fuse_mode(ctx, m));   // inner fused launches by the panel's height
  CHECK_RC(panel_factor(ctx, d_P, ld, m, w, g0, ctx->d_slots, d_info, nullptr, s));
  CHECK_RC(launch_sum_array(ctx->d_slots, w / TILE, ctx->d_scal + 8, s));
  hipLaunchKernelGGL(accum_kernel, dim3(1), dim3(1), 0, s, d_logdet, ctx->d_scal + 8);
  SGP_HIP(hipGetLastError());
  return 0;
}

extern "C" int sgp_dev_panel_update_batch(sgp_ctx* ctx, const sgp_panel_src* srcs, int nsrc, const sgp_panel_dst* dsts,
                                          int ndst, int64_t m_tot, void* stream) {
  CHECK_ARG(ctx && (srcs || nsrc == 0) && (dsts || ndst == 0), "sgp_dev_panel_update_batch: NULL argument");
  CHECK_ARG(nsrc >= 0 && nsrc <= SEG_MAX_SRC && ndst >= 0, "sgp_dev_panel_update_batch: at most 8 source panels");
  if (ndst == 0 || nsrc == 0) return 0;
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  SGP_HIP(hipSetDevice(ctx->device));
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  SegBatch b;
  b.m_tot = m_tot;
  for (int q = 0; q < nsrc; ++q) {
    CHECK_ARG(srcs[q].base && srcs[q].w > 0 && srcs[q].w % 16 == 0 && srcs[q].w < (1 << 30),
              "sgp_dev_panel_update_batch: bad source panel");
    b.src[q] = SegSrc{srcs[q].base, (long)srcs[q].ld, (long)srcs[q].row0, (int)srcs[q].w};
  }
  for (int q = nsrc; q < SEG_MAX_SRC; ++q) b.src[q] = SegSrc{nullptr, 0, 0, 0};
  for (int d0 = 0; d0 < ndst; d0 += SEG_MAX_DST) {
    b.n_dst = 0;
    for (int d = d0; d < std::min(ndst, d0 + SEG_MAX_DST); ++d) {
      const sgp_panel_dst& D = dsts[d];
      CHECK_ARG(D.base && D.src_first >= 0 && D.src_count >= 0 && D.src_first + D.src_count <= nsrc && D.w < (1 << 30),
                "sgp_dev_panel_update_batch: bad destination panel");
      if (D.src_count == 0) continue;
      b.dst[b.n_dst++] = SegDst{D.base, (long)D.ld, (long)D.c0, (int)D.w, D.src_first, D.src_count, 0u};
    }
    CHECK_RC(launch_gemm_nt_seg(b, s));
  }
  return 0;
}

extern "C" int sgp_dev_panel_update(sgp_ctx* ctx, const double* d_P, int64_t ldp, int64_t p_row0,
                                    int64_t w, double* d_C, int64_t ldc, int64_t c0, int64_t nc,
                                    int64_t m_tot, void* stream) {
  CHECK_ARG(ctx && d_P && d_C, "sgp_dev_panel_update: NULL argument");
  CHECK_ARG(c0 % TILE == 0 && nc % TILE == 0 && w % 16 == 0 && c0 >= p_row0, "sgp_dev_panel_update: bad sizes");
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);  // ctx scratch (logdet slots, inverse blocks) is shared
  SGP_HIP(hipSetDevice(ctx->device));
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  const double* A = d_P + (c0 - p_row0);  // panel rows c0.. (global)
  // d_C column 0 == global column c0; rows are global
  CHECK_RC(launch_gemm_nt_update(A, ldp, d_C + c0, ldc, m_tot - c0, nc, w, s));
  return 0;
}

extern "C" int sgp_dev_rowsumsq(sgp_ctx* ctx, const double* d_rows, int64_t ld, int64_t nc,
                                int64_t nrows, double* d_out, void* stream) {
  CHECK_ARG(ctx && d_rows && d_out, "sgp_dev_rowsumsq: NULL argument");
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);  // ctx scratch (logdet slots, inverse blocks) is shared
  SGP_HIP(hipSetDevice(ctx->device));
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  return launch_rowsumsq(d_rows, ld, nc, nrows, d_out, 1, s);
}

// ---------------------------------------------------------------------------------------
// driver.h: the routines above for the multi-GPU driver (multi.hip)
// ---------------------------------------------------------------------------------------
__global__ void axpy_block_kernel(double* C, long ldc, const double* S, long lds, long nr, long nc, double a) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= nr * nc) return;
  const long r = idx % nr, c = idx / nr;
  C[r + c * ldc] += a * S[r + c * lds];
}

namespace sgp {
int drv_assemble(const sgp_dspec* ds, double* Kv, long ld, long tile_r_lo, long tile_r_hi, long tile_c_lo,
                 long tile_c_hi, int lower_only, int noise_kind, double sigma2, const double* d_noise_diag,
                 hipStream_t s) {
  return assemble(ds, Kv, ld, tile_r_lo, tile_r_hi, tile_c_lo, tile_c_hi, lower_only, noise_kind, sigma2,
                  d_noise_diag, s);
}
// Factor a PACKED panel of the sharded factorisation (w columns over m rows, element [0] = (row g0, column g0) of the matrix).
// df != 0 (round 6: the hybrid schedule carried into the sharded sweep): ONE launch of the dataflow kernel -- the diagonal
// chain and the row solves below it as tile tasks, the pattern d_nz read at the panel's offset; px (optional): factor only
// the first px->n_fact columns and update the others with them, external source panels applied first (chol_df.hip).
// df == 0: the launch-based chain of rounds 2 - 5 (px must be empty; the caller issues the updates as launches of its own).
int drv_panel_factor(sgp_ctx* ctx, double* P, long ld, long m, long w, long g0, double* d_logdet, int* d_info,
                     double* d_invstore, hipStream_t s, int df, const sz_word* d_nz, int nz_words, const DfPanel* px, int lean) {
  CHECK_ARG(w % TILE == 0 && m % TILE == 0 && m >= w, "drv_panel_factor: bad sizes");
  long n_fact = w;
  if (df) {
    if (px) n_fact = px->n_fact;
    CHECK_ARG(n_fact / TILE <= ctx->n_slots, "drv_panel_factor: panel too wide for the logdet slot buffer");
    CHECK_RC(df_scratch(ctx, m, 1, d_invstore ? 0 : n_fact, s));
    // lean: two workgroups per CU (the panel kernel of ranks that SHARE a GPU: it must fit beside other ranks' update launches)
    CHECK_RC(launch_chol_dataflow(P, ld, w, m, ctx->d_df_state, d_invstore ? d_invstore : ctx->d_df_inv, ctx->d_slots, d_info,
                                  lean ? ctx->df_wgs : ctx->hybrid_wgs, ctx->df_timeout_s, s, nullptr, nullptr,
                                  lean ? 0 : ctx->hybrid_fat, d_nz, nz_words, g0, px));
  } else {
    CHECK_ARG(!px || (px->n_ext == 0 && px->n_fact == w), "drv_panel_factor: the launch-based chain takes whole panels only");
    FuseScope fuse_scope(ctx, fuse_mode(ctx, m));
    if (d_nz) gemm_set_structure(P, ld, d_nz, nz_words, w, nullptr, 0, g0 / TILE);
    const int rc = panel_factor(ctx, P, ld, m, w, g0, ctx->d_slots, d_info, d_invstore, s);
    if (d_nz) gemm_set_structure(nullptr, 0, nullptr, 0);
    CHECK_RC(rc);
  }
  CHECK_RC(launch_sum_array(ctx->d_slots, n_fact / TILE, ctx->d_scal + 8, s));
  hipLaunchKernelGGL(accum_kernel, dim3(1), dim3(1), 0, s, d_logdet, ctx->d_scal + 8);
  SGP_HIP(hipGetLastError());
  return 0;
}
int drv_row_trsm(sgp_ctx* ctx, double* R, long ldr, long nrows, const double* L, long ldl, const double* d_invall,
                 long n, hipStream_t s) {
  return row_trsm(ctx, R, ldr, nrows, L, ldl, d_invall, n, s);
}
int drv_back_substitute(const double* Lv, long ld, const double* wall_v, long k_first, long k_last, long n_end,
                        double* d_z, double* d_alpha, hipStream_t s) {
  return back_substitute_range(Lv, ld, wall_v, k_first, k_last, n_end, d_z, d_alpha, s);
}
int drv_diag_of_spec(sgp_ctx* ctx, const sgp_dspec* ds, double* d_out, hipStream_t s) {
  return diag_of_spec(ctx, ds, d_out, s);
}
int drv_dspec_create(sgp_ctx* ctx, const sgp_cov_spec* sp, sgp_dspec** out) { return dspec_create(ctx, sp, out); }
int drv_row_trsm_block(double* R, long ldr, long nrows, const double* L, long ldl, const double* d_invall, long c, long w,
                       hipStream_t s) {
  return row_trsm_block(R, ldr, nrows, L, ldl, d_invall, c, w, 512, s);
}
int drv_chol_sub(sgp_ctx* ctx, double* A, long ld, long n_cols, long m_rows, double* d_wall, hipStream_t s) {
  return chol_bordered(ctx, A, ld, n_cols, m_rows, d_wall, s);
}
int drv_fetch_info(sgp_ctx* ctx, hipStream_t s) { return fetch_info(ctx, s); }
bool drv_ctx_is_live(const sgp_ctx* ctx, long serial) { return ctx_is_live(ctx, serial); }
int drv_with_df_fallback(sgp_ctx* ctx, const std::function<int()>& run) { return with_df_fallback(ctx, run); }
int drv_conv_geom(sgp_ctx* ctx, int h, int w, int ph, int pw, int32_t* id_out) {
  CHECK_ARG(ctx && id_out, "sgp_conv_geom: NULL argument");
  CtxScope scope(ctx);
  CHECK_ARG(!ctx->multi, "sgp_conv_geom: patch (convolutional) terms are not supported on a multi-GPU context");
  CHECK_ARG(h >= 1 && w >= 1 && ph >= 1 && pw >= 1 && ph <= h && pw <= w, "sgp_conv_geom: need 1 <= patch_h <= height, 1 <= patch_w <= width");
  CHECK_ARG((long)h * w <= CONV_MAX_PIXELS, "sgp_conv_geom: images of more than 3072 pixels are not supported");
  CHECK_ARG(ph * pw <= CONV_MAX_PATCH, "sgp_conv_geom: patches of more than 64 pixels are not supported");
  for (size_t k = 0; k < ctx->conv_geoms.size(); ++k) {
    const PatchGeom& g = ctx->conv_geoms[k];
    if (g.h == h && g.w == w && g.ph == ph && g.pw == pw) {
      *id_out = (int32_t)(k + 1);
      return 0;
    }
  }
  CHECK_ARG(ctx->conv_geoms.size() < 0xffff, "sgp_conv_geom: too many geometries on this context");
  ctx->conv_geoms.push_back(PatchGeom{h, w, ph, pw});
  *id_out = (int32_t)ctx->conv_geoms.size();
  return 0;
}
int drv_stencil_register(sgp_ctx* ctx, int dim, int npoints, const double* offsets, const double* weights, int32_t* id_out) {
  CHECK_ARG(ctx && id_out, "sgp_stencil_register: NULL argument");
  CtxScope scope(ctx);
  CHECK_ARG(!ctx->multi, "sgp_stencil_register: stencil terms are not supported on a multi-GPU context");
  CHECK_ARG(dim >= 1 && dim <= STENCIL_MAX_DIM, "sgp_stencil_register: stencil dim must be in 1 .. 16");
  CHECK_ARG(npoints >= 1 && npoints <= STENCIL_MAX_POINTS, "sgp_stencil_register: stencil npoints must be in 1 .. 64");
  CHECK_ARG(offsets && weights, "sgp_stencil_register: NULL offsets / weights");
  std::vector<double> host((size_t)dim * npoints + npoints);
  memcpy(host.data(), offsets, sizeof(double) * (size_t)dim * npoints);
  memcpy(host.data() + (size_t)dim * npoints, weights, sizeof(double) * (size_t)npoints);
  for (double v : host) CHECK_ARG(std::isfinite(v), "sgp_stencil_register: stencil offsets and weights must be finite");
  for (size_t k = 0; k < ctx->conv_geoms.size(); ++k) {
    const int st = ctx->conv_geoms[k].st;
    if (st <= 0) continue;
    const StencilDesc& e = ctx->stencils[st - 1];
    if (e.dim == dim && e.npoints == npoints && !memcmp(e.host.data(), host.data(), sizeof(double) * host.size())) {
      *id_out = (int32_t)(k + 1);   // bitwise-equal: the same id
      return 0;
    }
  }
  CHECK_ARG(ctx->conv_geoms.size() < 0xffff, "sgp_stencil_register: too many geometries and stencils on this context");
  StencilDesc d;
  d.dim = dim;
  d.npoints = npoints;
  d.host = std::move(host);
  SGP_HIP(hipMalloc((void**)&d.dev, sizeof(double) * d.host.size()));
  if (hipMemcpy(d.dev, d.host.data(), sizeof(double) * d.host.size(), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    hipFree(d.dev);
    set_error("sgp_stencil_register: upload failed");
    return -2;
  }
  ctx->stencils.push_back(std::move(d));
  PatchGeom e{0, 0, 0, 0};
  e.st = (int)ctx->stencils.size();
  ctx->conv_geoms.push_back(e);
  *id_out = (int32_t)ctx->conv_geoms.size();
  return 0;
}
void drv_dspec_free(sgp_dspec* ds) { dspec_free(ds); }
long drv_invd_stride() { return INVD_STRIDE; }
int drv_copy_strided(const double* src, long stride, long n, double* dst, hipStream_t s) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(copy_strided_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, stride, n, dst);
  SGP_HIP(hipGetLastError());
  return 0;
}
int drv_axpy_block(double* C, long ldc, const double* S, long lds, long nr, long nc, double a, hipStream_t s) {
  if (nr <= 0 || nc <= 0) return 0;
  hipLaunchKernelGGL(axpy_block_kernel, dim3((unsigned)((nr * nc + 255) / 256)), dim3(256), 0, s, C, ldc, S, lds, nr, nc,
                     a);
  SGP_HIP(hipGetLastError());
  return 0;
}
int drv_fill_mean_cols(double* dst, long ld, long nrows, long ncols, long N, const double* mean, hipStream_t s) {
  if (nrows <= 0 || ncols <= 0) return 0;
  hipLaunchKernelGGL(fill_mean_cols_kernel, dim3((unsigned)((nrows * ncols + 255) / 256)), dim3(256), 0, s, dst, ld,
                     nrows, ncols, N, mean);
  SGP_HIP(hipGetLastError());
  return 0;
}
long drv_vfe_part_len(long m_pad) { return vfe_part_len(m_pad); }
int drv_vfe_partial(sgp_ctx* ctx, const sgp_cov_spec* zz, const sgp_cov_spec* xz, const double* var_x,
                    const double* mean_x, int noise_kind, const double* noise_x, int z_noise_kind, const double* z_noise,
                    const double* y, double* dLz, double* d_wz, double* d_part, long part_len) {
  return elbo_partial_core(ctx, zz, xz, var_x, mean_x, noise_kind, noise_x, z_noise_kind, z_noise, y, dLz, d_wz, d_part,
                           part_len);
}
int drv_elbo_grad(sgp_ctx* ctx, const ElboGradArgs& a, const ElboGradShard* shard) {
  auto run = [&]() { return elbo_grad_core(ctx, a, shard); };
  // (a rank of a sharded call cannot rerun on its own -- the reduction is collective: multi.hip reruns all of them)
  return shard ? run() : with_df_fallback(ctx, run);
}
int drv_vfe_finish(sgp_ctx* ctx, long M, double* d_part, double* d_wg, double* h6) {
  return elbo_finish_core(ctx, M, d_part, d_wg, h6);
}
int drv_vfe_rows_append(sgp_ctx* ctx, const sgp_dspec* dx, long M, const double* var_x, const double* mean_x, int noise_kind,
                        const double* noise_x, const double* y, const double* dLz, const double* d_wz, double* d_part,
                        StageTimer& tm) {
  VfeRows rows(ctx, dx, M, d_part, 1);
  CHECK_RC(rows.upload(var_x, mean_x, noise_kind, noise_x, y));
  CHECK_RC(rows.alloc_rows());
  tm.mark(0);
  CHECK_RC(rows.scalars(mean_x != nullptr, var_x != nullptr));
  return rows.chunks(dLz, d_wz, tm);
}
// the multi-GPU driver's view (multi.hip): rank 0's context computes the pattern, every rank uploads it
int drv_sz_pattern(sgp_ctx* ctx, const sgp_dspec* ds, int noise_kind, long n_pad, long m_tot, int* words) {
  return ::sz_pattern(ctx, ds, noise_kind, n_pad, m_tot, words);
}
int drv_sz_upload(sgp_ctx* ctx, const sgp_ctx* from, int words, hipStream_t s, const sz_word** d_nz) {
  SzMask m;
  CHECK_RC(::sz_upload(ctx, from->h_sz, words, s, &m));
  *d_nz = m.d_nz;
  return 0;
}
// fraction of the lower tiles of destination columns [c0, c0 + w) (rows c0 .. m_tot) that the k tiles [kt0, kt1) touch
double drv_sz_live_fraction(const sgp_ctx* ctx, int words, long c0, long w, long m_tot, long kt0, long kt1) {
  if (words <= 0) return 1.0;
  const long t0 = c0 / TILE, n_tc = w / TILE, n_tr = (m_tot - c0) / TILE;
  double live = 0, all = 0;
  for (long tc = 0; tc < n_tc; ++tc)
    for (long tr = tc; tr < n_tr; ++tr) {
      const sz_word* ra = &ctx->h_sz[(size_t)(t0 + tr) * words];
      const sz_word* rb = &ctx->h_sz[(size_t)(t0 + tc) * words];
      bool on = false;
      for (long k = kt0; k < kt1 && !on; ++k) on = ((ra[k >> 6] & rb[k >> 6]) >> (k & 63)) & 1;
      all += 1;
      live += on ? 1 : 0;
    }
  return all > 0 ? live / all : 1.0;
}

}  // namespace sgp
