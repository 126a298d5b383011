"""The surface of the force fields (egg_set_forces, DESIGN.md section 2.7 "Forces") as far as it can be checked without a
device: the four entry points and the 40-byte struct in the header and in the ctypes binding, the two methods on all
three Python classes and in the Lua wrapper -- and that neither the option enum nor egg_stats grew."""
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
    "egg_set_forces": "int egg_set_forces(egg_handle *h, int32_t n, const egg_force *f);",
    "egg_get_forces": "int egg_get_forces(const egg_handle *h, int32_t cap, egg_force *f, int32_t *n);",
    "egg_group_set_forces": "int egg_group_set_forces(egg_group *g, int32_t n, const egg_force *f);",
    "egg_group_get_forces": "int egg_group_get_forces(const egg_group *g, int32_t cap, egg_force *f, int32_t *n);",
}


def test_header_declares_the_four_entry_points_and_the_struct():
    from egg_fluid_simulation_amd import _ffi
    text = _header()
    for name, proto in PROTOS.items():
        assert proto in text, name
        assert name in _ffi._SIGNATURES and name in _ffi.EXPORTED_SYMBOLS, name
        assert len(_ffi._SIGNATURES[name][1]) == proto.count(",") + 1, name
    assert re.search(r"typedef struct\s*\{\s*int32_t kind;[^}]*int32_t type_mask;[^}]*double p\[4\];\s*\}\s*egg_force;", text)
    assert C.sizeof(_ffi.EggForce) == 40
    assert [(n, C.sizeof(t)) for n, t in _ffi.EggForce._fields_] == [("kind", 4), ("type_mask", 4), ("p", 32)]
    # the same layout as egg_collider
    assert [(n, t) for n, t in _ffi.EggForce._fields_] == [(n, t) for n, t in _ffi.EggCollider._fields_]
    kinds = _enum_values(text, "EGG_FORCE_UNIFORM")
    assert kinds == {"EGG_FORCE_UNIFORM": 0, "EGG_FORCE_RADIAL": 1, "EGG_FORCE_VORTEX": 2}
    assert _ffi.FORCE_KINDS == ("uniform", "radial", "vortex")
    assert (_ffi.FORCE_UNIFORM, _ffi.FORCE_RADIAL, _ffi.FORCE_VORTEX) == (0, 1, 2)
    assert re.search(r"#define EGG_MAX_FORCES 16\b", text) and _ffi.MAX_FORCES == 16
    # the kernel's record is the ABI's
    device_h = open(os.path.join(ROOT, "egg_fluid_simulation_amd", "csrc", "eggsim_device.h")).read()
    assert re.search(r"#define EGG_RX_MAX_FORCES 16\b", device_h)
    for k, name in enumerate(("UNIFORM", "RADIAL", "VORTEX")):
        assert re.search(r"#define EGG_RX_FORCE_%s %d\b" % (name, k), device_h), name


def test_force_struct_size_matches_the_c_compiler(tmp_path):
    """sizeof(egg_force) and the offsets of its fields as a C compiler lays the header out == the ctypes mirror"""
    from egg_fluid_simulation_amd import _ffi
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    src = tmp_path / "force_layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "eggsim.h"\n'
                   'int main(void) { printf("%zu %zu %zu %d %zu\\n", sizeof(egg_force), offsetof(egg_force, type_mask), '
                   'offsetof(egg_force, p), (int)EGG_MAX_FORCES, sizeof(egg_collider)); return 0; }\n')
    exe = str(tmp_path / "force_layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [40, _ffi.EggForce.type_mask.offset, _ffi.EggForce.p.offset, 16, 40] == [40, 4, 8, 16, 40]


def test_python_classes_have_the_two_methods():
    from egg_fluid_simulation_amd import EggError, SimulationGroup, SimulationHandler
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler
    for cls in (SimulationHandler, SimulationGroup, ShardedSimulationHandler):
        assert list(inspect.signature(cls.set_forces).parameters) == ["self", "forces"], cls
        assert list(inspect.signature(cls.get_forces).parameters) == ["self"], cls
    # what only the host can check is refused before any device call
    for cls in (SimulationHandler, SimulationGroup):
        bare = cls.__new__(cls)
        for bad in ([("gravity", 0, 1)], [("uniform", 0)], [("uniform", 0, 1, 2)], [("radial", 0, 0, 1)], [("vortex", 0, 0, 1, 2, 3)],
                    [("radial", 0, 0, 1, 2, "red")], [("uniform", 0, "x")], [{"kind": "uniform", "gx": 0}],
                    [{"kind": "radial", "cx": 0, "cy": 0, "strength": 1, "R": 1, "gx": 2}], [()]):
            with pytest.raises(EggError, match="field 0"):
                bare.set_forces(bad)
    n, arr = SimulationHandler._c_forces([("uniform", 0, 980), {"kind": "vortex", "cx": 1, "cy": 2, "strength": 3, "R": 4, "types": "yolk"},
                                          ("radial", 1, 2, -3, 4, "white")])
    assert n == 3
    assert [(f.kind, f.type_mask, list(f.p)) for f in arr[:n]] == [(0, 3, [0, 980, 0, 0]), (2, 2, [1, 2, 3, 4]), (1, 1, [1, 2, -3, 4])]
    assert SimulationHandler._c_forces([])[0] == 0


def test_lua_wrapper_names_the_methods():
    lua = open(os.path.join(ROOT, "egg_fluid_simulation_amd", "lua", "egg_fluid_simulation", "simulation_handler.lua")).read()
    for name in ("set_forces(forces)", "get_forces()"):
        assert "function SimulationHandler:" + name in lua, name
    for name in ("egg_set_forces", "egg_get_forces"):
        assert PROTOS[name] in lua and "lib." + name + "(self._h" in lua, name
    assert "typedef struct { int32_t kind; int32_t type_mask; double p[4]; } egg_force;" in lua
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("egg_set_forces", "egg_get_forces"):
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
