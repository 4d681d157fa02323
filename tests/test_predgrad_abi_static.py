"""The prediction-gradient part of the C boundary without a GPU: include/sthenomi_predgrad.h is plain C and declares exactly
what libsthenomi_predgrad.so exports (and the ctypes table types), the product library keeps exporting exactly
include/sthenomi.h, the new library resolves its product-library dependency, the header's chunk width is the host's, and the
Julia shim's `@ccall`s into it pass the declared argument types."""
import os
import re
import subprocess

import stheno_jl_amd as P
from test_capi_symbols import _c_exports, _symbols_of
from test_julia_shim_static import SRC, _ctypes_kind, _julia_kind, _matching, _split_top

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ["sgp_posterior_predict_grad_x", "sgp_sparse_posterior_predict_grad_x"]


def test_header_and_library_agree():
    syms = _symbols_of("sthenomi_predgrad.h")
    assert syms == SYMS == P.lib.predgrad_symbols()
    assert _c_exports(P.lib.PREDGRAD_LIB_PATH) == syms                  # nm -D: exactly its two names
    assert not set(syms) & set(_c_exports(P.lib.LIB_PATH))
    assert not set(syms) & set(_symbols_of("sthenomi.h"))
    assert _c_exports(P.lib.LIB_PATH) == _symbols_of("sthenomi.h")      # the product library exports what it did
    assert isinstance(P.lib.Context.predgrad, property)
    assert P.mean_and_var_and_gradient is P.finite_gp.mean_and_var_and_gradient


def test_the_chunk_width_is_a_constant_of_the_header():
    txt = open(os.path.join(ROOT, "include", "sthenomi_predgrad.h")).read()
    m = re.search(r"#define\s+SGP_PREDGRAD_COL_CHUNK\s+(\d+)", txt)
    assert m and int(m.group(1)) == P.lib.PREDGRAD_COL_CHUNK
    assert 128 <= P.lib.PREDGRAD_COL_CHUNK <= 512 and P.lib.PREDGRAD_COL_CHUNK % 128 == 0


def test_header_is_plain_c_and_resolves(tmp_path):
    src = tmp_path / "predgrad_consumer.c"
    src.write_text(r'''
#include <stdio.h>
#include <dlfcn.h>
#include "sthenomi_predgrad.h"
int main(int argc, char** argv) {
  /* the declared prototypes, checked by the compiler without linking (sizeof is unevaluated) */
  typedef int (*dense_t)(sgp_post*, const sgp_cov_spec*, const sgp_cov_spec*, const double*, double*, double*,
                         double* const*, double* const*, double* const*);
  typedef int (*sparse_t)(sgp_sparse_post*, const sgp_cov_spec*, const sgp_cov_spec*, const double*, double*, double*,
                          double* const*, double* const*, double* const*);
  dense_t a = 0; sparse_t b = 0;
  const char* names[2] = {"sgp_posterior_predict_grad_x", "sgp_sparse_posterior_predict_grad_x"};
  void* h;
  int i;
  printf("fnptr %d chunk %d\n", (int)(sizeof(a = &sgp_posterior_predict_grad_x) + sizeof(b = &sgp_sparse_posterior_predict_grad_x)),
         SGP_PREDGRAD_COL_CHUNK);
  if (argc < 2) return 1;
  h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!h) { printf("dlopen failed: %s\n", dlerror()); return 2; }
  for (i = 0; i < 2; ++i) printf("%s\n", dlsym(h, names[i]) ? "resolved" : "missing");
  return 0;
}
''')
    exe = str(tmp_path / "predgrad_consumer")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           str(src), "-o", exe + ".o"])
    subprocess.check_call(["gcc", "-o", exe, exe + ".o", "-ldl"])
    out = subprocess.run([exe, P.lib.PREDGRAD_LIB_PATH], capture_output=True, text=True)
    want = ["fnptr", "16", "chunk", str(P.lib.PREDGRAD_COL_CHUNK)] + ["resolved"] * 2
    assert out.returncode == 0 and out.stdout.split() == want, (out.stdout, out.stderr)


def test_ctypes_table_types_the_declared_arguments():
    """argument by argument against the header's prototypes"""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sthenomi_predgrad.h")).read(), flags=re.S)
    for name in SYMS:
        proto = re.search(r"int\s+" + name + r"\s*\((.*?)\)\s*;", txt, flags=re.S).group(1)
        kinds = []
        for arg in proto.split(","):
            arg = " ".join(arg.split())
            kinds.append("ptr" if "*" in arg else "i64" if arg.startswith("int64_t") else "i32" if arg.startswith("int ") else "?")
        res, args = P.lib._SIGS_PREDGRAD[name]
        assert _ctypes_kind(res) == "i32"
        assert [_ctypes_kind(a) for a in args] == kinds and len(kinds) == 9, name


def test_julia_at_ccalls_match_the_declared_signatures():
    calls = list(re.finditer(r"@ccall\s+LIB_PREDGRAD\.(\w+)\(", SRC))
    assert sorted(m.group(1) for m in calls) == SYMS
    for m in calls:
        end = _matching(SRC, m.end() - 1)
        args = _split_top(SRC[m.end():end - 1])
        ret = re.match(r"::\s*(\w+)", SRC[end:]).group(1)
        res, ctypes_args = P.lib._SIGS_PREDGRAD[m.group(1)]
        assert _julia_kind(ret) == _ctypes_kind(res)
        assert len(args) == len(ctypes_args), m.group(1)
        for a, ct in zip(args, ctypes_args):
            assert _julia_kind(a.rsplit("::", 1)[1]) == _ctypes_kind(ct), (m.group(1), a, ct)
