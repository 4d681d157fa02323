"""The posterior-extension part of the C boundary without a GPU: include/sthenomi_extend.h is plain C and declares exactly
what libsthenomi_extend.so exports (and the ctypes table types), the product library keeps exporting exactly
include/sthenomi.h, the extension resolves its product-library dependency, and the Julia shim's `@ccall` into it passes the
declared argument types."""
import os
import re
import subprocess

import stheno_jl_amd as P
from test_capi_symbols import _c_exports, _symbols_of
from test_julia_shim_static import SRC, _ctypes_kind, _julia_kind, _split_top

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ["sgp_posterior_extend"]


def test_extension_header_and_library_agree():
    syms = _symbols_of("sthenomi_extend.h")
    assert syms == SYMS == P.lib.extend_symbols()
    assert _c_exports(P.lib.EXTEND_LIB_PATH) == syms
    assert not set(syms) & set(_c_exports(P.lib.LIB_PATH))
    assert not set(syms) & set(_symbols_of("sthenomi.h"))
    assert _c_exports(P.lib.LIB_PATH) == _symbols_of("sthenomi.h")      # the product library exports what it did
    hook = _symbols_of("sthenomi_extend_bench.h")
    assert hook == ["sgp_bench_extend_row_solve"] == sorted(P.lib._SIGS_EXTEND_BENCH)
    assert _c_exports(P.lib.EXTEND_BENCH_LIB_PATH) == hook
    lib = P.lib.extend_lib()
    assert all(hasattr(lib, s) for s in syms)
    assert isinstance(P.lib.Context.extend, property)


def test_extension_header_is_plain_c_and_resolves(tmp_path):
    src = tmp_path / "extend_consumer.c"
    src.write_text(r'''
#include <stdio.h>
#include <dlfcn.h>
#include "sthenomi_extend.h"
int main(int argc, char** argv) {
  /* the declared prototypes, checked by the compiler without linking (sizeof is unevaluated) */
  typedef int (*fn_t)(sgp_post*, const sgp_cov_spec*, const double*, int, const double*, const double*, int64_t, int64_t,
                      double*, double*);
  fn_t probe = 0;
  void* h;
  printf("fnptr %d\n", (int)sizeof(probe = &sgp_posterior_extend));
  if (argc < 2) return 1;
  h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!h) { printf("dlopen failed: %s\n", dlerror()); return 2; }
  printf("%s\n", dlsym(h, "sgp_posterior_extend") ? "resolved" : "missing");
  return 0;
}
''')
    exe = str(tmp_path / "extend_consumer")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           str(src), "-o", exe + ".o"])
    subprocess.check_call(["gcc", "-o", exe, exe + ".o", "-ldl"])
    out = subprocess.run([exe, P.lib.EXTEND_LIB_PATH], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split() == ["fnptr", "8", "resolved"], (out.stdout, out.stderr)


def test_ctypes_table_types_the_declared_arguments():
    """argument by argument against the header's prototype"""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sthenomi_extend.h")).read(), flags=re.S)
    for name in SYMS:
        proto = re.search(r"int\s+" + name + r"\s*\((.*?)\)\s*;", txt, flags=re.S).group(1)
        kinds = []
        for arg in proto.split(","):
            arg = " ".join(arg.split())
            kinds.append("ptr" if "*" in arg else "i64" if arg.startswith("int64_t") else "i32" if arg.startswith("int ") else "?")
        res, args = P.lib._SIGS_EXTEND[name]
        assert _ctypes_kind(res) == "i32"
        assert [_ctypes_kind(a) for a in args] == kinds, name


def test_julia_at_ccall_matches_the_declared_signature():
    calls = list(re.finditer(r"@ccall\s+LIB_EXTEND\.(\w+)\(", SRC))
    assert [m.group(1) for m in calls] == ["sgp_posterior_extend"]
    m = calls[0]
    depth, i = 0, m.end() - 1
    while True:
        depth += {"(": 1, ")": -1}.get(SRC[i], 0)
        i += 1
        if depth == 0:
            break
    args = _split_top(SRC[m.end():i - 1])
    ret = re.match(r"::\s*(\w+)", SRC[i:]).group(1)
    res, ctypes_args = P.lib._SIGS_EXTEND["sgp_posterior_extend"]
    assert _julia_kind(ret) == _ctypes_kind(res)
    assert len(args) == len(ctypes_args)
    for a, ct in zip(args, ctypes_args):
        assert _julia_kind(a.rsplit("::", 1)[1]) == _ctypes_kind(ct), (a, ct)
