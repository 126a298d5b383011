"""Boundary checks that need no GPU: the shared library loads, exports every symbol
include/eggsim.h declares, refuses to run without a device (no CPU fallback), and the
host-side mirror validates configs and arguments like the reference."""
import os
import re
import warnings

import pytest

from conftest import ROOT


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "eggsim.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(egg_[a-z_0-9]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    from egg_fluid_simulation_amd import _ffi
    if not os.path.exists(_ffi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _ffi.load()


def test_library_exports_every_declared_symbol(lib):
    from egg_fluid_simulation_amd import _ffi
    declared = _declared_symbols()
    assert len(declared) >= 20
    for name in declared:
        assert hasattr(lib, name), "libeggsim.so does not export " + name
    assert sorted(_ffi.EXPORTED_SYMBOLS) == declared  # the ctypes binding covers the whole header


def test_default_config_values(lib):
    import ctypes as C
    from egg_fluid_simulation_amd import _ffi
    from egg_fluid_simulation_amd.default_config import default_configs
    w, y = default_configs()
    for which, ref in ((0, w), (1, y)):
        c = _ffi.EggConfig()
        assert lib.egg_default_config(which, C.byref(c)) == 0
        for k in ("damping", "follow_strength", "cohesion_strength", "cohesion_interaction_distance_factor",
                  "collision_strength", "collision_overlap_factor", "min_mass", "max_mass", "min_radius",
                  "max_radius"):
            assert getattr(c, k) == float(ref[k]), k
        assert (c.max_collision_fraction, c.mass_distribution_variance, c.eps) == (0.05, 4.0, 1e-8)


def test_no_device_means_loud_failure_not_cpu_fallback(lib):
    from egg_fluid_simulation_amd import EggError, SimulationHandler
    try:
        SimulationHandler()
    except EggError as e:
        assert "no CPU path" in str(e)
    else:
        pytest.skip("a GPU is present")


def test_product_package_does_not_import_the_oracle():
    import subprocess
    import sys
    code = ("import sys; import egg_fluid_simulation_amd; "
            "bad=[m for m in sys.modules if m.startswith('oracle')]; print(bad); sys.exit(1 if bad else 0)")
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0
    for dirpath, _, files in os.walk(os.path.join(ROOT, "egg_fluid_simulation_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", ".lua")):
                src = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in src and "from oracle" not in src and "eggsim_oracle" not in src, f


class _Bare:
    """SimulationHandler without a device: only the host-side config logic"""

    def __new__(cls):
        from egg_fluid_simulation_amd import SimulationHandler
        h = SimulationHandler.__new__(SimulationHandler)
        h._white_config, h._yolk_config, h._h = {}, {}, None
        return h


def test_load_config_validation_matches_reference():
    from egg_fluid_simulation_amd import EggError, EggWarning
    from egg_fluid_simulation_amd.default_config import default_configs
    w, _ = default_configs()
    h = _Bare()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        h._load_config(dict(w, damping=1.5, bogus=3, follow_strength=float("nan"), min_mass=-1), True)
    msgs = " | ".join(str(r.message) for r in rec)
    assert all(isinstance(r.message, EggWarning) for r in rec)
    assert "unrecognized config key `bogus`" in msgs and "`follow_strength` is NaN" in msgs
    assert h._white_config["damping"] == 1 and h._white_config["min_mass"] == 0  # clamped (L:1303-1309)
    assert "bogus" not in h._white_config and "follow_strength" not in h._white_config  # ignored
    with pytest.raises(EggError, match="wrong type for config key `damping`"):
        h._load_config({"damping": "x"}, True)
    with pytest.raises(EggError, match="does not have 4 components"):
        h._load_config({"color": [1, 1, 1]}, False)


def test_argument_type_errors_are_thrown():
    from egg_fluid_simulation_amd import EggError
    h = _Bare()
    with pytest.raises(EggError, match=r"argument #1: expected `number`, got `string`"):
        h.set_target_position("a", 1, 2)
    with pytest.raises(EggError, match=r"expected `number`, got `nil`"):
        h.get_position(None)
    with pytest.raises(EggError, match=r"expected `table`"):
        h.set_white_config(3)


def _build_c_caller(tmp_path):
    """tests/c/abi_roundtrip.c against include/eggsim.h and the built library, as strict C99"""
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    lib_dir = os.path.join(ROOT, "egg_fluid_simulation_amd")
    exe = str(tmp_path / "abi_roundtrip")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    "-o", exe, os.path.join(ROOT, "tests", "c", "abi_roundtrip.c"), "-L", lib_dir, "-leggsim",
                    "-Wl,-rpath," + lib_dir], check=True)
    return exe


def test_header_is_plain_c_and_library_links_from_c(tmp_path):
    """the boundary is a C ABI: the header compiles as pedantic C99, a C program links against libeggsim.so, and
    without a GPU egg_create reports EGG_ERR_NO_DEVICE (-3) instead of falling back to anything"""
    import subprocess
    exe = _build_c_caller(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    assert out.splitlines()[0] in ("create -3", "create 0")  # -3 = EGG_ERR_NO_DEVICE on a box without a GPU


def _prototypes(text):
    """{name: normalised parameter-type list} of the `egg_*` prototypes in a piece of C"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(?:int|void|const char \*)\s*(egg_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", text):
        params = []
        for prm in m.group(2).split(","):
            prm = " ".join(prm.split())
            prm = re.sub(r"\b[a-zA-Z_][a-zA-Z_0-9]*$", "", prm).strip()  # drop the parameter name
            params.append(prm.replace(" *", "*"))
        out[m.group(1)] = params
    return out


def test_lua_binding_declares_the_header_prototypes():
    """the LuaJIT wrapper cannot run here, but its ffi.cdef block can be held against include/eggsim.h: every
    function it binds must have exactly the header's parameter types"""
    lua = open(os.path.join(ROOT, "egg_fluid_simulation_amd", "lua", "egg_fluid_simulation", "simulation_handler.lua")).read()
    cdef = re.search(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S).group(1)
    header = _prototypes(open(os.path.join(ROOT, "include", "eggsim.h")).read())
    bound = _prototypes(cdef)
    assert len(bound) >= 12
    for name, params in bound.items():
        assert name in header, name
        assert params == header[name], (name, params, header[name])
    # and the two structs it passes by pointer have the header's field order
    for struct in ("egg_config", "egg_environment", "egg_render_config", "egg_render_params"):
        def fields(text):
            body = re.search(r"typedef struct\s*\{([^}]*)\}\s*" + struct + r"\s*;", re.sub(r"/\*.*?\*/", " ", text, flags=re.S), flags=re.S).group(1)
            return re.findall(r"[a-z_]+(?=\s*[,;])", body)
        assert fields(cdef) == fields(open(os.path.join(ROOT, "include", "eggsim.h")).read()), struct


def _header_text():
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "eggsim.h")).read(), flags=re.S)


def test_cell_hash_option_and_counter_are_appended():
    """EGG_OPT_FORCE_CELL_HASH is the last option (the earlier ones keep their numbers) and egg_stats ends with
    int64_t cell_hash[2]; the ctypes binding mirrors both, and a C program sees the struct size ctypes computes"""
    import ctypes as C
    from egg_fluid_simulation_amd import _ffi
    body = re.search(r"enum\s*\{\s*(EGG_OPT_CLAIM_MARGIN_CELLS\b[^}]*)\}", _header_text(), flags=re.S).group(1)
    names = [item.strip() for item in body.split(",") if item.strip()]
    assert all("=" not in n for n in names[1:]) and names[0].replace(" ", "") == "EGG_OPT_CLAIM_MARGIN_CELLS=0"
    names[0] = "EGG_OPT_CLAIM_MARGIN_CELLS"
    assert names[-2:] == ["EGG_OPT_COHESION", "EGG_OPT_FORCE_CELL_HASH"]
    assert names.index("EGG_OPT_FORCE_CELL_HASH") == _ffi.OPT_FORCE_CELL_HASH == _ffi.OPT_COHESION + 1 == 16
    for k, name in enumerate(names):  # every option of the header has its number in the binding
        assert getattr(_ffi, name[len("EGG_"):]) == k, name
    stats = re.search(r"typedef struct\s*\{((?:(?!typedef).)*?)\}\s*egg_stats\s*;", _header_text(), flags=re.S).group(1)
    assert re.search(r"int64_t\s+cohesion_solves\s*;\s*int64_t\s+cell_hash\s*\[\s*2\s*\]\s*;\s*$", stats)
    assert _ffi.EggStats._fields_[-1][0] == "cell_hash" and _ffi.EggStats._fields_[-1][1] is C.c_int64 * 2
    assert _ffi.EggStats.cell_hash.offset == C.sizeof(_ffi.EggStats) - 16 == _ffi.EggStats.cohesion_solves.offset + 8


def test_stats_struct_size_matches_the_c_compiler(tmp_path):
    """sizeof(egg_stats) and the offset of its last field as a C compiler lays the header out == the ctypes mirror"""
    import ctypes as C
    import shutil
    import subprocess
    from egg_fluid_simulation_amd import _ffi
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    src = tmp_path / "stats_layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "eggsim.h"\n'
                   'int main(void) { printf("%zu %zu %d\\n", sizeof(egg_stats), offsetof(egg_stats, cell_hash), (int)EGG_OPT_FORCE_CELL_HASH); return 0; }\n')
    exe = str(tmp_path / "stats_layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [C.sizeof(_ffi.EggStats), _ffi.EggStats.cell_hash.offset, _ffi.OPT_FORCE_CELL_HASH]
