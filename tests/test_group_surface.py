"""SimulationGroup is the reference's SimulationHandler class over a device group: the method names, the argument checks of
a device-less instance and the ctypes bindings of the `egg_group_*` entry points.  No device needed."""
import inspect
import os
import re
import warnings

import pytest

from conftest import ROOT

# the public methods of the reference's class (simulation_handler.lua:27-419), written out
REFERENCE_METHODS = ["add", "remove", "draw", "update", "set_white_config", "set_yolk_config", "get_white_config",
                     "get_yolk_config", "set_target_position", "get_target_position", "get_position", "list_ids",
                     "set_white_color", "set_yolk_color", "get_n_particles"]
# what this change adds to include/eggsim.h
NEW_ENTRY_POINTS = ["egg_group_set_config", "egg_group_get_config", "egg_group_get_target", "egg_group_list_ids",
                    "egg_group_get_n_particles", "egg_group_get_elapsed", "egg_group_download_particles",
                    "egg_group_get_environment", "egg_group_set_render_config", "egg_group_get_render_config",
                    "egg_group_set_render_flags", "egg_group_set_add_color", "egg_group_set_color", "egg_group_render",
                    "egg_group_render_canvas"]


def _bare():
    """SimulationGroup without a device: only the host-side logic"""
    from egg_fluid_simulation_amd import SimulationGroup
    g = SimulationGroup.__new__(SimulationGroup)
    g._white_config, g._yolk_config, g._g, g._batch_colors = {}, {}, None, {}
    return g


def test_group_has_the_reference_methods():
    from egg_fluid_simulation_amd import SimulationGroup, SimulationHandler
    for name in REFERENCE_METHODS + ["render_canvas", "get_environment", "download", "step"]:
        assert callable(getattr(SimulationGroup, name, None)), name
    for name in ("elapsed", "interpolation_alpha", "_use_particle_color", "_use_lighting"):
        assert isinstance(inspect.getattr_static(SimulationGroup, name), property), name
    for name in REFERENCE_METHODS:  # same parameters as the single handle (add also keeps white_n / yolk_n)
        want = list(inspect.signature(getattr(SimulationHandler, name)).parameters)
        got = list(inspect.signature(getattr(SimulationGroup, name)).parameters)
        assert got[:len(want)] == want, (name, got, want)
    assert list(inspect.signature(SimulationGroup.add).parameters)[-2:] == ["white_n", "yolk_n"]
    for name in ("add_many", "export_batch", "step_begin"):  # single-handle plumbing stays off the group
        assert not hasattr(SimulationGroup, name), name


def test_argument_checks_of_a_deviceless_group():
    from egg_fluid_simulation_amd import EggError, EggWarning
    g = _bare()
    with pytest.raises(EggError, match=r"argument #1: expected `number`, got `string`"):
        g.set_target_position("a", 1, 2)
    with pytest.raises(EggError, match=r"argument #1: expected `number`, got `string`"):
        g.add("a", 2)
    with pytest.raises(EggError, match=r"expected `number`, got `nil`"):
        g.get_position(None)
    with pytest.raises(EggError, match=r"expected `number`, got `nil`"):
        g.get_target_position(None)
    with pytest.raises(EggError, match=r"expected `number`, got `table`"):
        g.remove([1])
    with pytest.raises(EggError, match=r"expected `table`"):
        g.set_white_config(3)
    with pytest.raises(EggError, match=r"expected `table`"):
        g.set_yolk_config("x")
    with pytest.raises(EggError, match="In SimulationHandler.set_yolk_config: color `color` does not have 4 components"):
        g.set_yolk_config({"color": [1, 1, 1]})
    with pytest.raises(EggError, match="wrong type for config key `damping`"):
        g.set_white_config({"damping": "x"})
    with pytest.raises(EggError, match="white radius cannot be 0 or negative"):
        g.add(1, 2, 0)
    with pytest.raises(EggError, match="yolk particle count cannot be 1 or negative"):
        g.add(1, 2, 50, 15, None, None, 100, 1)
    with pytest.raises(EggError, match="yolk particle count cannot be 1 or negative"):
        g.add(1, 2, 50, 15, yolk_n=1)
    with pytest.raises(EggError, match="white color component `a` is not a number"):
        g.add(1, 2, 50, 15, [1, 1, 1])
    with pytest.raises(EggError, match=r"argument #2: expected `number`, got `string`"):
        g.set_white_color(1, 0.5, "g", 0.5)
    with pytest.raises(EggError, match="`n_substeps` is not a number > 0"):
        g.update(1 / 60, 1 / 60, float("nan"))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        g.set_yolk_color(7, 2.0, 0.5, 0.5)  # out of range and an id nobody issued: two warnings, no device call
    msgs = " | ".join(str(r.message) for r in rec)
    assert all(isinstance(r.message, EggWarning) for r in rec)
    assert "set_egg_yolk_color: color component is outside of [0, 1]" in msgs and "no batch with id `7`" in msgs


def _prototypes(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return {m.group(1): [p for p in m.group(2).split(",") if p.strip()]
            for m in re.finditer(r"\b(?:int|void|const char \*|int32_t|egg_handle \*)\s*(egg_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", text)}


def test_every_group_prototype_has_a_binding_of_the_same_arity():
    from egg_fluid_simulation_amd import _ffi
    protos = _prototypes(open(os.path.join(ROOT, "include", "eggsim.h")).read())
    group = sorted(n for n in protos if n.startswith("egg_group_"))
    assert len(group) >= 30
    for name in NEW_ENTRY_POINTS:
        assert name in group, name
    for name in group:
        assert name in _ffi._SIGNATURES and name in _ffi.EXPORTED_SYMBOLS, name
        assert len(_ffi._SIGNATURES[name][1]) == len(protos[name]), (name, protos[name])
    # every new entry point has a single-handle twin with the same parameters after the handle
    for name in NEW_ENTRY_POINTS:
        twin = name.replace("egg_group_", "egg_")
        assert twin in _ffi._SIGNATURES, twin
        assert _ffi._SIGNATURES[name][1][1:] == _ffi._SIGNATURES[twin][1][1:], name
