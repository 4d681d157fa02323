"""The sparse-posterior update part of the C boundary without a GPU: include/sthenomi_vfe_update.h is plain C and declares
exactly what libsthenomi_vfe_update.so exports (and the ctypes table types), the product library keeps exporting exactly
include/sthenomi.h, the new library resolves its product-library dependency, and the Julia shim's `@ccall`s into it pass
the declared argument types."""
import os
import re
import subprocess

import stheno_jl_amd as P
from test_capi_symbols import _c_exports, _symbols_of
from test_julia_shim_static import SRC, _ctypes_kind, _julia_kind, _matching, _split_top

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ["sgp_sparse_posterior_count", "sgp_sparse_posterior_update"]


def test_header_and_library_agree():
    syms = _symbols_of("sthenomi_vfe_update.h")
    assert syms == SYMS == P.lib.vfe_update_symbols()
    assert _c_exports(P.lib.VFE_UPDATE_LIB_PATH) == syms                # nm -D: exactly its two names
    assert not set(syms) & set(_c_exports(P.lib.LIB_PATH))
    assert not set(syms) & set(_symbols_of("sthenomi.h"))
    assert _c_exports(P.lib.LIB_PATH) == _symbols_of("sthenomi.h")      # the product library exports what it did
    lib = P.lib.vfe_update_lib()
    assert all(hasattr(lib, s) for s in syms)
    assert isinstance(P.lib.Context.vfe_update, property)


def test_header_is_plain_c_and_resolves(tmp_path):
    src = tmp_path / "vfe_update_consumer.c"
    src.write_text(r'''
#include <stdio.h>
#include <dlfcn.h>
#include "sthenomi_vfe_update.h"
int main(int argc, char** argv) {
  /* the declared prototypes, checked by the compiler without linking (sizeof is unevaluated) */
  typedef int (*update_t)(sgp_sparse_post*, const sgp_cov_spec*, const double*, const double*, int, const double*,
                          const double*, double*);
  typedef int (*count_t)(sgp_sparse_post*, int64_t*);
  update_t a = 0; count_t b = 0;
  const char* names[2] = {"sgp_sparse_posterior_update", "sgp_sparse_posterior_count"};
  void* h;
  int i;
  printf("fnptr %d\n", (int)(sizeof(a = &sgp_sparse_posterior_update) + sizeof(b = &sgp_sparse_posterior_count)));
  if (argc < 2) return 1;
  h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!h) { printf("dlopen failed: %s\n", dlerror()); return 2; }
  for (i = 0; i < 2; ++i) printf("%s\n", dlsym(h, names[i]) ? "resolved" : "missing");
  return 0;
}
''')
    exe = str(tmp_path / "vfe_update_consumer")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           str(src), "-o", exe + ".o"])
    subprocess.check_call(["gcc", "-o", exe, exe + ".o", "-ldl"])
    out = subprocess.run([exe, P.lib.VFE_UPDATE_LIB_PATH], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split() == ["fnptr", "16"] + ["resolved"] * 2, (out.stdout, out.stderr)


def test_ctypes_table_types_the_declared_arguments():
    """argument by argument against the header's prototypes"""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sthenomi_vfe_update.h")).read(), flags=re.S)
    for name in SYMS:
        proto = re.search(r"int\s+" + name + r"\s*\((.*?)\)\s*;", txt, flags=re.S).group(1)
        kinds = []
        for arg in proto.split(","):
            arg = " ".join(arg.split())
            kinds.append("ptr" if "*" in arg else "i64" if arg.startswith("int64_t") else "i32" if arg.startswith("int ") else "?")
        res, args = P.lib._SIGS_VFE_UPDATE[name]
        assert _ctypes_kind(res) == "i32"
        assert [_ctypes_kind(a) for a in args] == kinds, name


def test_julia_at_ccalls_match_the_declared_signatures():
    calls = list(re.finditer(r"@ccall\s+LIB_VFE_UPDATE\.(\w+)\(", SRC))
    assert sorted(m.group(1) for m in calls) == SYMS
    for m in calls:
        end = _matching(SRC, m.end() - 1)
        args = _split_top(SRC[m.end():end - 1])
        ret = re.match(r"::\s*(\w+)", SRC[end:]).group(1)
        res, ctypes_args = P.lib._SIGS_VFE_UPDATE[m.group(1)]
        assert _julia_kind(ret) == _ctypes_kind(res)
        assert len(args) == len(ctypes_args), m.group(1)
        for a, ct in zip(args, ctypes_args):
            assert _julia_kind(a.rsplit("::", 1)[1]) == _ctypes_kind(ct), (m.group(1), a, ct)
