"""The table of sibling libraries (lib.FAMILIES): every row against its header, its built library and the Makefile's list, and
the one loader behind all of them."""
import os
import re

import pytest

import stheno_jl_amd as P
from test_capi_symbols import _c_exports, _symbols_of

L = P.lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bench", "batch", "pool", "conv", "conv_grad", "stencil", "stencil_grad", "stencil_wo", "kprod", "kprod_grad", "extend",
         "extend_bench", "postfx", "predgrad", "vfe_update"]


def test_the_table_has_the_fifteen_families():
    assert sorted(L.FAMILIES) == sorted(NAMES)


def test_every_row_is_its_header_and_its_library():
    for name in L.FAMILIES:
        header = f"sthenomi_{name}.h"
        assert os.path.exists(os.path.join(ROOT, "include", header)), header
        assert L.family_path(name) == os.path.join(os.path.dirname(L.LIB_PATH), f"libsthenomi_{name}.so")
        assert _symbols_of(header) == L.family_symbols(name) == _c_exports(L.family_path(name)), name
        assert L.family_symbols(name), name


def test_no_two_libraries_export_one_name():
    """the product library included: sixteen libraries, pairwise disjoint"""
    exports = {"product": _c_exports(L.LIB_PATH), **{name: _c_exports(L.family_path(name)) for name in L.FAMILIES}}
    assert len(exports) == 16
    seen = {}
    for lib, syms in exports.items():
        for s in syms:
            assert s not in seen, f"{s}: exported by {seen[s]} and {lib}"
            seen[s] = lib
    assert sorted(seen) == sorted(set(L.exported_symbols()) | {s for name in L.FAMILIES for s in L.family_symbols(name)})


def test_the_makefile_builds_the_table():
    src = open(os.path.join(ROOT, "stheno.jl_amd", "csrc", "Makefile")).read()
    words = re.search(r"^FAMILIES\s*=\s*(.*)$", src, flags=re.M).group(1).split()
    assert len(words) == len(set(words)) == 14
    assert sorted(words + ["bench"]) == sorted(L.FAMILIES)


def test_every_family_is_a_property_of_the_context():
    for name in L.FAMILIES:
        assert isinstance(getattr(L.Context, name), property), name


def test_one_handle_per_family_and_the_old_names_reach_it():
    for name in L.FAMILIES:
        lib = L.family_lib(name)
        assert lib is L.family_lib(name) is getattr(L, f"{name}_lib")()
        assert all(hasattr(lib, s) for s in L.family_symbols(name))
        assert getattr(L, f"{name.upper()}_LIB_PATH") == L.family_path(name)
        assert getattr(L, f"{name}_symbols")() == L.family_symbols(name)


def test_a_missing_library_is_named(tmp_path, monkeypatch):
    missing = str(tmp_path / "libsthenomi_batch.so")
    monkeypatch.setattr(L, "_family_libs", {})
    monkeypatch.setattr(L, "family_path", lambda name: missing)
    with pytest.raises(P.SthenoMIError) as ei:
        L.family_lib("batch")
    assert missing in str(ei.value) and "is missing: build it with" in str(ei.value)
