"""The surface of the collider surfaces (egg_set_collider_surfaces, DESIGN.md section 2.7 "Collider surfaces") as far as it
can be checked without a device: the six entry points and the 24-byte struct in the header and in the ctypes binding, the
three methods on all three Python classes and in the Lua wrapper -- and that neither the option enum nor egg_stats grew."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
from test_cohesion_surface import _enum_values, _header

PROTOS = {
    "egg_set_collider_surfaces": "int egg_set_collider_surfaces(egg_handle *h, int32_t n, const egg_collider_surface *s);",
    "egg_get_collider_surfaces": "int egg_get_collider_surfaces(const egg_handle *h, int32_t cap, egg_collider_surface *s, int32_t *n);",
    "egg_get_collider_grips": "int egg_get_collider_grips(egg_handle *h, int64_t grips[2]);",
    "egg_group_set_collider_surfaces": "int egg_group_set_collider_surfaces(egg_group *g, int32_t n, const egg_collider_surface *s);",
    "egg_group_get_collider_surfaces": "int egg_group_get_collider_surfaces(const egg_group *g, int32_t cap, egg_collider_surface *s, int32_t *n);",
    "egg_group_get_collider_grips": "int egg_group_get_collider_grips(egg_group *g, int64_t grips[2]);",
}


def test_header_declares_the_six_entry_points_and_the_struct():
    from egg_fluid_simulation_amd import _ffi
    text = _header()
    for name, proto in PROTOS.items():
        assert proto in text, name
        assert name in _ffi._SIGNATURES and name in _ffi.EXPORTED_SYMBOLS, name
        assert len(_ffi._SIGNATURES[name][1]) == proto.count(",") + 1, name
    assert re.search(r"typedef struct\s*\{\s*double friction;[^}]*double vx, vy;[^}]*\}\s*egg_collider_surface;", text)
    assert C.sizeof(_ffi.EggColliderSurface) == 24
    assert [(n, getattr(_ffi.EggColliderSurface, n).offset) for n, _ in _ffi.EggColliderSurface._fields_] == \
        [("friction", 0), ("vx", 8), ("vy", 16)]
    # the kernel's record is the ABI's, and the collider fields stayed as they were
    device_h = open(os.path.join(ROOT, "egg_fluid_simulation_amd", "csrc", "eggsim_device.h")).read()
    assert re.search(r"struct EggSurface \{\s*double friction, vx, vy;\s*\};", device_h)
    assert re.search(r"struct EggRxSurfaceFields \{[^}]*const EggSurface \*list;[^}]*double sub_delta;[^}]*unsigned long long \*grips;", device_h)
    fields = re.search(r"struct EggRxColliderFields \{([^}]*)\}", device_h).group(1)
    assert re.findall(r"(\w+);", re.sub(r"//[^\n]*", "", fields)) == ["list", "count", "type_bit", "hits"]


def test_surface_struct_size_matches_the_c_compiler(tmp_path):
    """sizeof(egg_collider_surface) and the offsets of its fields as a C compiler lays the header out == the ctypes mirror"""
    from egg_fluid_simulation_amd import _ffi
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    src = tmp_path / "surface_layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "eggsim.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(egg_collider_surface), offsetof(egg_collider_surface, friction), '
                   'offsetof(egg_collider_surface, vx), offsetof(egg_collider_surface, vy)); return 0; }\n')
    exe = str(tmp_path / "surface_layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    S = _ffi.EggColliderSurface
    assert [int(v) for v in out] == [C.sizeof(S), S.friction.offset, S.vx.offset, S.vy.offset] == [24, 0, 8, 16]


def test_the_library_exports_the_symbols():
    from egg_fluid_simulation_amd import _ffi
    path = os.path.join(ROOT, "egg_fluid_simulation_amd", "libeggsim.so")
    if not os.path.exists(path):
        pytest.skip("libeggsim.so is not built")
    lib = C.CDLL(path)
    for name in PROTOS:
        assert hasattr(lib, name), name
    # every entry point links and refuses a null handle
    assert lib.egg_set_collider_surfaces(None, 0, None) == _ffi.EGG_ERR_INVALID_ARGUMENT
    assert lib.egg_get_collider_grips(None, None) == _ffi.EGG_ERR_INVALID_ARGUMENT


def test_python_classes_have_the_three_methods():
    from egg_fluid_simulation_amd import EggError, SimulationGroup, SimulationHandler
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler
    for cls in (SimulationHandler, SimulationGroup, ShardedSimulationHandler):
        assert list(inspect.signature(cls.set_collider_surfaces).parameters) == ["self", "surfaces"], cls
        assert list(inspect.signature(cls.get_collider_surfaces).parameters) == ["self"], cls
        assert list(inspect.signature(cls.collider_grips).parameters) == ["self"], cls
    # what only the host can check is refused before any device call
    for cls in (SimulationHandler, SimulationGroup):
        bare = cls.__new__(cls)
        for bad in (["rough"], [(1.0, 2.0)], [(1.0, 2.0, 3.0, 4.0)], [object()], [("a", 0, 0)]):
            with pytest.raises(EggError, match="collider surface 0"):
                bare.set_collider_surfaces(bad)
    n, arr = SimulationHandler._c_surfaces([None, 0.5, (0.25, 3, -4)])
    assert n == 3
    assert [(s.friction, s.vx, s.vy) for s in arr[:n]] == [(0.0, 0.0, 0.0), (0.5, 0.0, 0.0), (0.25, 3.0, -4.0)]
    assert SimulationHandler._c_surfaces([])[0] == 0


def test_lua_wrapper_names_the_methods():
    lua = open(os.path.join(ROOT, "egg_fluid_simulation_amd", "lua", "egg_fluid_simulation", "simulation_handler.lua")).read()
    for name in ("set_collider_surfaces(surfaces)", "get_collider_surfaces()", "collider_grips()"):
        assert "function SimulationHandler:" + name in lua, name
    for name in ("egg_set_collider_surfaces", "egg_get_collider_surfaces", "egg_get_collider_grips"):
        assert PROTOS[name] in lua and "lib." + name + "(self._h" in lua, name
    assert "typedef struct { double friction; double vx, vy; } egg_collider_surface;" in lua
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("egg_set_collider_surfaces", "egg_get_collider_surfaces", "egg_get_collider_grips"):
        assert PROTOS[name] in integration, name


def test_the_option_enum_and_the_stats_are_unchanged():
    from egg_fluid_simulation_amd import _ffi
    opts = _enum_values(_header(), "EGG_OPT_CLAIM_MARGIN_CELLS")
    assert max(opts, key=opts.get) == "EGG_OPT_FORCE_CELL_HASH" and opts["EGG_OPT_FORCE_CELL_HASH"] == _ffi.OPT_FORCE_CELL_HASH == 16
    body = re.search(r"typedef struct\s*\{((?:(?!typedef).)*?)\}\s*egg_stats\s*;", re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S),
                     flags=re.S).group(1)
    fields = re.findall(r"([a-z_]+)(?:\[[^;]*\])*\s*;", body)
    assert fields[-2:] == ["cohesion_solves", "cell_hash"]
    assert [f[0] for f in _ffi.EggStats._fields_] == fields
    assert _ffi.EggStats.cell_hash.offset == C.sizeof(_ffi.EggStats) - 16
