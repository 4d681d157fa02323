"""The batched-gradient extension of the C boundary without a GPU: include/sthenomi_batch.h is plain C and declares exactly
what libsthenomi_batch.so exports (and the ctypes table types), the product library keeps exporting exactly
include/sthenomi.h, the extension resolves its product-library dependency, and the Julia shim's `@ccall` into it passes the
declared argument types."""
import os
import re
import subprocess

import stheno_jl_amd as P
from test_capi_symbols import _c_exports, _symbols_of
from test_julia_shim_static import SRC, _ctypes_kind, _julia_kind, _split_top

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_extension_header_and_library_agree():
    syms = _symbols_of("sthenomi_batch.h")
    assert syms == ["sgp_logpdf_grad_batch"] == P.lib.batch_symbols()
    assert _c_exports(P.lib.BATCH_LIB_PATH) == syms
    assert not set(syms) & set(_c_exports(P.lib.LIB_PATH))
    assert not set(syms) & set(_symbols_of("sthenomi.h"))
    lib = P.lib.batch_lib()
    assert hasattr(lib, "sgp_logpdf_grad_batch")


def test_extension_header_is_plain_c_and_resolves(tmp_path):
    src = tmp_path / "batch_consumer.c"
    src.write_text(r'''
#include <stdio.h>
#include <dlfcn.h>
#include "sthenomi_batch.h"
int main(int argc, char** argv) {
  /* the declared prototype, checked by the compiler without linking (sizeof is unevaluated) */
  typedef int (*fn_t)(sgp_ctx*, int, const sgp_cov_spec* const*, const double* const*, int, const double* const*,
                      const double* const*, double*, double* const*, double* const*, double* const*, double* const*,
                      double* const*, int*);
  fn_t probe = 0;
  void* h;
  printf("fnptr %d\n", (int)sizeof(probe = &sgp_logpdf_grad_batch));
  if (argc < 2) return 1;
  h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
  if (!h) { printf("dlopen failed: %s\n", dlerror()); return 2; }
  printf("%s\n", dlsym(h, "sgp_logpdf_grad_batch") ? "resolved" : "missing");
  return 0;
}
''')
    exe = str(tmp_path / "batch_consumer")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           str(src), "-o", exe + ".o"])
    subprocess.check_call(["gcc", "-o", exe, exe + ".o", "-ldl"])
    out = subprocess.run([exe, P.lib.BATCH_LIB_PATH], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split() == ["fnptr", "8", "resolved"], (out.stdout, out.stderr)


def test_julia_at_ccall_matches_the_declared_signature():
    calls = list(re.finditer(r"@ccall\s+LIB_BATCH\.(\w+)\(", SRC))
    assert [m.group(1) for m in calls] == ["sgp_logpdf_grad_batch"]
    m = calls[0]
    depth, i = 0, m.end() - 1
    while True:
        depth += {"(": 1, ")": -1}.get(SRC[i], 0)
        i += 1
        if depth == 0:
            break
    args = _split_top(SRC[m.end():i - 1])
    ret = re.match(r"::\s*(\w+)", SRC[i:]).group(1)
    res, ctypes_args = P.lib._SIGS_BATCH["sgp_logpdf_grad_batch"]
    assert _julia_kind(ret) == _ctypes_kind(res)
    assert len(args) == len(ctypes_args)
    for a, ct in zip(args, ctypes_args):
        assert _julia_kind(a.split("::", 1)[1]) == _ctypes_kind(ct), (a, ct)
