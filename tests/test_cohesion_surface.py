"""The surface of effective cohesion (EGG_OPT_COHESION, DESIGN.md section 2.7 "Cohesion") as far as it can be checked
without a device: the option's value and the new counter in the header and in the ctypes binding, the new group entry
point, the two methods on all three Python classes and in the Lua wrapper."""
import ctypes as C
import inspect
import os
import re

from conftest import ROOT


def _header():
    return open(os.path.join(ROOT, "include", "eggsim.h")).read()


def _enum_values(text, first):
    """{name: value} of the anonymous enum that starts with `first` (comments stripped; explicit values honoured)"""
    body = re.search(r"enum\s*\{\s*(" + first + r"\b[^}]*)\}", re.sub(r"/\*.*?\*/", " ", text, flags=re.S), flags=re.S).group(1)
    out, value = {}, -1
    for item in (s.strip() for s in body.split(",")):
        if not item:
            continue
        name, _, explicit = item.partition("=")
        value = int(explicit, 0) if explicit.strip() else value + 1
        out[name.strip()] = value
    return out


def test_option_value_and_modes():
    from egg_fluid_simulation_amd import _ffi
    opts = _enum_values(_header(), "EGG_OPT_CLAIM_MARGIN_CELLS")
    assert opts["EGG_OPT_COHESION"] == opts["EGG_OPT_RELAXATION"] + 1 == _ffi.OPT_COHESION == 15
    # (options appended since keep these numbers: the only one behind it is the cell-hash test hook, tests/test_abi.py)
    assert [k for k, v in opts.items() if v > opts["EGG_OPT_COHESION"]] == ["EGG_OPT_FORCE_CELL_HASH"]
    assert opts["EGG_OPT_SOLVER_ORDER"] == _ffi.OPT_SOLVER_ORDER and opts["EGG_OPT_RELAXATION"] == _ffi.OPT_RELAXATION
    defines = dict(re.findall(r"#define (EGG_COHESION_[A-Z]+) (\d+)", _header()))
    assert defines == {"EGG_COHESION_REFERENCE": "0", "EGG_COHESION_EFFECTIVE": "1"}
    assert (_ffi.COHESION_REFERENCE, _ffi.COHESION_EFFECTIVE) == (0, 1)


def test_stats_end_with_the_new_counter():
    from egg_fluid_simulation_amd import _ffi
    body = re.search(r"typedef struct\s*\{((?:(?!typedef).)*?)\}\s*egg_stats\s*;", re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S),
                     flags=re.S).group(1)
    fields = re.findall(r"([a-z_]+)(?:\[[^;]*\])*\s*;", body)
    # (fields appended since leave the counter where it was: only cell_hash[2] stands behind it, tests/test_abi.py)
    assert fields[-3:] == ["relaxed_steps", "cohesion_solves", "cell_hash"]
    assert [f[0] for f in _ffi.EggStats._fields_] == fields
    assert _ffi.EggStats._fields_[-2] == ("cohesion_solves", C.c_int64)
    assert _ffi.EggStats.cohesion_solves.offset == C.sizeof(_ffi.EggStats) - 8 - 16 == _ffi.EggStats.relaxed_steps.offset + 8


def test_group_entry_point_and_record_size():
    from egg_fluid_simulation_amd import _ffi
    assert re.search(r"int egg_group_set_cohesion\(egg_group \*g, int32_t mode\);", _header())
    assert _ffi._SIGNATURES["egg_group_set_cohesion"] == (C.c_int, [C.c_void_p, C.c_int32])
    assert "egg_group_set_cohesion" in _ffi.EXPORTED_SYMBOLS
    # the ghost record did not grow: the tag rides in the key word
    device_h = open(os.path.join(ROOT, "egg_fluid_simulation_amd", "csrc", "eggsim_device.h")).read()
    assert re.search(r"#define EGG_RX_WIRE_RECORD_WORDS 5\b", device_h)
    assert (_ffi.RX_RECORD_WORDS, _ffi.RX_RECORD_BYTES) == (5, 40)


def test_python_classes_have_the_two_methods():
    from egg_fluid_simulation_amd import EggError, SimulationGroup, SimulationHandler
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler
    import pytest
    for cls in (SimulationHandler, SimulationGroup, ShardedSimulationHandler):
        assert list(inspect.signature(cls.set_cohesion).parameters) == ["self", "mode"], cls
        assert list(inspect.signature(cls.get_cohesion).parameters) == ["self"], cls
        bare = cls.__new__(cls)
        assert bare.get_cohesion() == "reference"
    for cls in (SimulationHandler, SimulationGroup):  # a bad mode is refused before any device call
        bare = cls.__new__(cls)
        for bad in ("on", 1, None):
            with pytest.raises(EggError, match="cohesion must be"):
                bare.set_cohesion(bad)
        assert bare.get_cohesion() == "reference"
    assert SimulationHandler._COHESION_MODES == {"reference": 0, "effective": 1}


def test_lua_wrapper_names_the_methods():
    lua = open(os.path.join(ROOT, "egg_fluid_simulation_amd", "lua", "egg_fluid_simulation", "simulation_handler.lua")).read()
    assert re.search(r"function SimulationHandler:set_cohesion\(mode\)", lua)
    assert re.search(r"function SimulationHandler:get_cohesion\(\)", lua)
    assert "int egg_set_option(egg_handle *h, int option, double value);" in lua
    from egg_fluid_simulation_amd import _ffi
    m = re.search(r"function SimulationHandler:set_cohesion\(mode\)(.*?)\nend", lua, flags=re.S)
    assert "egg_set_option(self._h, %d," % _ffi.OPT_COHESION in m.group(1)
