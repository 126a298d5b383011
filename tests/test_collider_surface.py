"""The surface of the static colliders (egg_set_colliders, DESIGN.md section 2.7 "Colliders") as far as it can be checked
without a device: the six entry points and the 40-byte struct in the header and in the ctypes binding, the three methods
on all three Python classes and in the Lua wrapper -- and that neither the option enum nor egg_stats grew."""
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
    "egg_set_colliders": "int egg_set_colliders(egg_handle *h, int32_t n, const egg_collider *c);",
    "egg_get_colliders": "int egg_get_colliders(const egg_handle *h, int32_t cap, egg_collider *c, int32_t *n);",
    "egg_get_collider_hits": "int egg_get_collider_hits(egg_handle *h, int64_t hits[2]);",
    "egg_group_set_colliders": "int egg_group_set_colliders(egg_group *g, int32_t n, const egg_collider *c);",
    "egg_group_get_colliders": "int egg_group_get_colliders(const egg_group *g, int32_t cap, egg_collider *c, int32_t *n);",
    "egg_group_get_collider_hits": "int egg_group_get_collider_hits(egg_group *g, int64_t hits[2]);",
}


def test_header_declares_the_six_entry_points_and_the_struct():
    from egg_fluid_simulation_amd import _ffi
    text = _header()
    for name, proto in PROTOS.items():
        assert proto in text, name
        assert name in _ffi._SIGNATURES and name in _ffi.EXPORTED_SYMBOLS, name
        assert len(_ffi._SIGNATURES[name][1]) == proto.count(",") + 1, name
    assert re.search(r"typedef struct\s*\{\s*int32_t kind;[^}]*int32_t type_mask;[^}]*double p\[4\];\s*\}\s*egg_collider;", text)
    assert C.sizeof(_ffi.EggCollider) == 40
    assert [(n, C.sizeof(t)) for n, t in _ffi.EggCollider._fields_] == [("kind", 4), ("type_mask", 4), ("p", 32)]
    kinds = _enum_values(text, "EGG_COLLIDER_HALF_PLANE")
    assert kinds == {"EGG_COLLIDER_HALF_PLANE": 0, "EGG_COLLIDER_DISC": 1, "EGG_COLLIDER_CONTAINER": 2, "EGG_COLLIDER_SEGMENT": 3}
    assert _ffi.COLLIDER_KINDS == ("half_plane", "disc", "container", "segment")
    assert re.search(r"#define EGG_MAX_COLLIDERS 64\b", text) and _ffi.MAX_COLLIDERS == 64
    # the kernel's record is the ABI's
    device_h = open(os.path.join(ROOT, "egg_fluid_simulation_amd", "csrc", "eggsim_device.h")).read()
    assert re.search(r"#define EGG_RX_MAX_COLLIDERS 64\b", device_h)


def test_collider_struct_size_matches_the_c_compiler(tmp_path):
    """sizeof(egg_collider) and the offsets of its fields as a C compiler lays the header out == the ctypes mirror"""
    from egg_fluid_simulation_amd import _ffi
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    src = tmp_path / "collider_layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "eggsim.h"\n'
                   'int main(void) { printf("%zu %zu %zu %d\\n", sizeof(egg_collider), offsetof(egg_collider, type_mask), '
                   'offsetof(egg_collider, p), (int)EGG_MAX_COLLIDERS); return 0; }\n')
    exe = str(tmp_path / "collider_layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [40, _ffi.EggCollider.type_mask.offset, _ffi.EggCollider.p.offset, 64] == [40, 4, 8, 64]


def test_python_classes_have_the_three_methods():
    from egg_fluid_simulation_amd import EggError, SimulationGroup, SimulationHandler
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler
    for cls in (SimulationHandler, SimulationGroup, ShardedSimulationHandler):
        assert list(inspect.signature(cls.set_colliders).parameters) == ["self", "colliders"], cls
        assert list(inspect.signature(cls.get_colliders).parameters) == ["self"], cls
        assert list(inspect.signature(cls.collider_hits).parameters) == ["self"], cls
    # what only the host can check is refused before any device call
    for cls in (SimulationHandler, SimulationGroup):
        bare = cls.__new__(cls)
        for bad in ([("box", 0, 0, 1)], [("disc", 0, 0)], [("segment", 0, 0, 1)], [("disc", 0, 0, 1, "red")], [("disc", 0, 0, "x")],
                    [{"kind": "disc", "cx": 0, "cy": 0}], [{"kind": "disc", "cx": 0, "cy": 0, "R": 1, "x0": 2}], [()]):
            with pytest.raises(EggError, match="collider 0"):
                bare.set_colliders(bad)
    n, arr = SimulationHandler._c_colliders([("half_plane", 0, 2, 5), {"kind": "segment", "x0": 1, "y0": 2, "x1": 3, "y1": 4, "types": "yolk"},
                                             ("container", 1, 2, 3, "white")])
    assert n == 3
    assert [(c.kind, c.type_mask, list(c.p)) for c in arr[:n]] == [(0, 3, [0, 2, 5, 0]), (3, 2, [1, 2, 3, 4]), (2, 1, [1, 2, 3, 0])]
    assert SimulationHandler._c_colliders([])[0] == 0


def test_lua_wrapper_names_the_methods():
    lua = open(os.path.join(ROOT, "egg_fluid_simulation_amd", "lua", "egg_fluid_simulation", "simulation_handler.lua")).read()
    for name in ("set_colliders(colliders)", "get_colliders()", "collider_hits()"):
        assert "function SimulationHandler:" + name in lua, name
    for name in ("egg_set_colliders", "egg_get_colliders", "egg_get_collider_hits"):
        assert PROTOS[name] in lua and "lib." + name + "(self._h" in lua, name
    assert "typedef struct { int32_t kind; int32_t type_mask; double p[4]; } egg_collider;" in lua
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("egg_set_colliders", "egg_get_colliders", "egg_get_collider_hits"):
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
