"""The posterior rand / logpdf part of the C boundary without a GPU: include/sthenomi_postfx.h is plain C and declares exactly
what libsthenomi_postfx.so exports (and the ctypes table types), the product library keeps exporting exactly
include/sthenomi.h, the new library resolves its product-library dependency, and the Julia shim's `@ccall`s into it pass the
declared argument types."""
import os
import re
import subprocess

import stheno_jl_amd as P
from test_capi_symbols import _c_exports, _symbols_of
from test_julia_shim_static import SRC, _ctypes_kind, _julia_kind, _matching, _split_top

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ["sgp_posterior_logpdf", "sgp_posterior_rand", "sgp_sparse_posterior_logpdf", "sgp_sparse_posterior_rand"]


def test_header_and_library_agree():
    syms = _symbols_of("sthenomi_postfx.h")
    assert syms == SYMS == P.lib.postfx_symbols()
    assert _c_exports(P.lib.POSTFX_LIB_PATH) == syms                    # nm -D: exactly its four names
    assert not set(syms) & set(_c_exports(P.lib.LIB_PATH))
    assert not set(syms) & set(_symbols_of("sthenomi.h"))
    assert _c_exports(P.lib.LIB_PATH) == _symbols_of("sthenomi.h")      # the product library exports what it did
    lib = P.lib.postfx_lib()
    assert all(hasattr(lib, s) for s in syms)
    assert isinstance(P.lib.Context.postfx, property)


def test_header_is_plain_c_and_resolves(tmp_path):
    src = tmp_path / "postfx_consumer.c"
    src.write_text(r'''
#include <stdio.h>
#include <dlfcn.h>
#include "sthenomi_postfx.h"
int main(int argc, char** argv) {
  /* the declared prototypes, checked by the compiler without linking (sizeof is unevaluated) */
  typedef int (*rand_t)(sgp_post*, const sgp_cov_spec*, const sgp_cov_spec*, const double*, int, const double*, const double*,
                        int64_t, int64_t, double*, int64_t);
  typedef int (*logpdf_t)(sgp_post*, const sgp_cov_spec*, const sgp_cov_spec*, const double*, int, const double*, const double*,
                          int64_t, int64_t, double*);
  typedef int (*srand_t)(sgp_sparse_post*, const sgp_cov_spec*, const sgp_cov_spec*, const double*, int, const double*,
                         const double*, int64_t, int64_t, double*, int64_t);
  typedef int (*slogpdf_t)(sgp_sparse_post*, const sgp_cov_spec*, const sgp_cov_spec*, const double*, int, const double*,
                           const double*, int64_t, int64_t, double*);
  rand_t a = 0; logpdf_t b = 0; srand_t c = 0; slogpdf_t d = 0;
  const char* names[4] = {"sgp_posterior_rand", "sgp_posterior_logpdf", "sgp_sparse_posterior_rand", "sgp_sparse_posterior_logpdf"};
  void* h;
  int i;
  printf("fnptr %d\n", (int)(sizeof(a = &sgp_posterior_rand) + sizeof(b = &sgp_posterior_logpdf) +
                             sizeof(c = &sgp_sparse_posterior_rand) + sizeof(d = &sgp_sparse_posterior_logpdf)));
  if (argc < 2) return 1;
  h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!h) { printf("dlopen failed: %s\n", dlerror()); return 2; }
  for (i = 0; i < 4; ++i) printf("%s\n", dlsym(h, names[i]) ? "resolved" : "missing");
  return 0;
}
''')
    exe = str(tmp_path / "postfx_consumer")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           str(src), "-o", exe + ".o"])
    subprocess.check_call(["gcc", "-o", exe, exe + ".o", "-ldl"])
    out = subprocess.run([exe, P.lib.POSTFX_LIB_PATH], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split() == ["fnptr", "32"] + ["resolved"] * 4, (out.stdout, out.stderr)


def test_ctypes_table_types_the_declared_arguments():
    """argument by argument against the header's prototypes"""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sthenomi_postfx.h")).read(), flags=re.S)
    for name in SYMS:
        proto = re.search(r"int\s+" + name + r"\s*\((.*?)\)\s*;", txt, flags=re.S).group(1)
        kinds = []
        for arg in proto.split(","):
            arg = " ".join(arg.split())
            kinds.append("ptr" if "*" in arg else "i64" if arg.startswith("int64_t") else "i32" if arg.startswith("int ") else "?")
        res, args = P.lib._SIGS_POSTFX[name]
        assert _ctypes_kind(res) == "i32"
        assert [_ctypes_kind(a) for a in args] == kinds, name


def test_julia_at_ccalls_match_the_declared_signatures():
    calls = list(re.finditer(r"@ccall\s+LIB_POSTFX\.(\w+)\(", SRC))
    assert sorted(m.group(1) for m in calls) == SYMS
    for m in calls:
        end = _matching(SRC, m.end() - 1)
        args = _split_top(SRC[m.end():end - 1])
        ret = re.match(r"::\s*(\w+)", SRC[end:]).group(1)
        res, ctypes_args = P.lib._SIGS_POSTFX[m.group(1)]
        assert _julia_kind(ret) == _ctypes_kind(res)
        assert len(args) == len(ctypes_args), m.group(1)
        for a, ct in zip(args, ctypes_args):
            assert _julia_kind(a.rsplit("::", 1)[1]) == _ctypes_kind(ct), (m.group(1), a, ct)
