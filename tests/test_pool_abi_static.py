"""The ragged-pool extension of the C boundary without a GPU: include/sthenomi_pool.h is plain C and declares exactly what
libsthenomi_pool.so exports (and the ctypes table types), its names are disjoint from the product header's and the batch
extension's, the extension resolves its product-library dependency, and the Julia shim's `@ccall`s into it pass the declared
argument kinds."""
import os
import re
import subprocess

import stheno_jl_amd as P
from test_capi_symbols import _c_exports, _symbols_of
from test_julia_shim_static import SRC, _ctypes_kind, _julia_kind, _split_top

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sgp_logpdf_grad_pool", "sgp_logpdf_pool"]


def test_extension_header_and_library_agree():
    syms = _symbols_of("sthenomi_pool.h")
    assert syms == NAMES == P.lib.pool_symbols()
    assert _c_exports(P.lib.POOL_LIB_PATH) == syms
    for other in ("sthenomi.h", "sthenomi_batch.h"):
        assert not set(syms) & set(_symbols_of(other))
    assert not set(syms) & set(_c_exports(P.lib.LIB_PATH))
    assert not set(syms) & set(_c_exports(P.lib.BATCH_LIB_PATH))
    lib = P.lib.pool_lib()
    assert all(hasattr(lib, s) for s in syms)


def test_extension_header_is_plain_c_and_resolves(tmp_path):
    src = tmp_path / "pool_consumer.c"
    src.write_text(r'''
#include <stdio.h>
#include <dlfcn.h>
#include "sthenomi_pool.h"
int main(int argc, char** argv) {
  /* the declared prototypes, checked by the compiler without linking (sizeof is unevaluated) */
  typedef int (*val_t)(sgp_ctx*, int, const sgp_cov_spec* const*, const double* const*, const int*, const double* const*,
                       const double* const*, double*, int*, sgp_pool_report*);
  typedef int (*grad_t)(sgp_ctx*, int, const sgp_cov_spec* const*, const double* const*, const int*, const double* const*,
                        const double* const*, double*, double* const*, double* const*, double* const*, double* const*,
                        double* const*, int*, sgp_pool_report*);
  val_t pv = 0;
  grad_t pg = 0;
  sgp_pool_report rep;
  void* h;
  rep.pool_launches = rep.pooled_members = rep.single_members = rep.distinct_sizes = 0;
  printf("fnptr %d %d report %d\n", (int)sizeof(pv = &sgp_logpdf_pool), (int)sizeof(pg = &sgp_logpdf_grad_pool),
         (int)sizeof(rep) + rep.pool_launches);
  if (argc < 2) return 1;
  h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!h) { printf("dlopen failed: %s\n", dlerror()); return 2; }
  printf("%s\n", dlsym(h, "sgp_logpdf_pool") && dlsym(h, "sgp_logpdf_grad_pool") ? "resolved" : "missing");
  return 0;
}
''')
    exe = str(tmp_path / "pool_consumer")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           str(src), "-o", exe + ".o"])
    subprocess.check_call(["gcc", "-o", exe, exe + ".o", "-ldl"])
    out = subprocess.run([exe, P.lib.POOL_LIB_PATH], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split() == ["fnptr", "8", "8", "report", "16", "resolved"], (out.stdout, out.stderr)


def test_julia_at_ccall_matches_the_declared_signatures():
    calls = list(re.finditer(r"@ccall\s+LIB_POOL\.(\w+)\(", SRC))
    assert sorted(m.group(1) for m in calls) == NAMES
    assert re.search(r"^const LIB_POOL\s*=", SRC, re.M)
    for m in calls:
        depth, i = 0, m.end() - 1
        while True:
            depth += {"(": 1, ")": -1}.get(SRC[i], 0)
            i += 1
            if depth == 0:
                break
        args = _split_top(SRC[m.end():i - 1])
        ret = re.match(r"::\s*(\w+)", SRC[i:]).group(1)
        res, ctypes_args = P.lib._SIGS_POOL[m.group(1)]
        assert _julia_kind(ret) == _ctypes_kind(res)
        assert len(args) == len(ctypes_args), m.group(1)
        for a, ct in zip(args, ctypes_args):
            assert _julia_kind(a.split("::", 1)[1]) == _ctypes_kind(ct), (m.group(1), a, ct)
