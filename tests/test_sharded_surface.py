"""ShardedSimulationHandler is the reference's SimulationHandler class over the ranks of a process group: the method
names and parameter lists, the argument checks of a device-less instance and the C entry points behind its draw.  No
device, no process group."""
import ctypes
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
NEW_ENTRY_POINTS = ["egg_draw_pack", "egg_draw_source_layout", "egg_draw_source_place", "egg_draw_source_render",
                    "egg_draw_source_render_canvas", "egg_draw_source_environment", "egg_draw_source_download"]


def _bare():
    """ShardedSimulationHandler without a device or a process group: only the host-side logic"""
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler
    s = ShardedSimulationHandler.__new__(ShardedSimulationHandler)
    s._white_config, s._yolk_config, s._batch_colors, s.owner, s.local = {}, {}, {}, {}, None
    return s


def test_sharded_handler_has_the_reference_methods():
    from egg_fluid_simulation_amd import SimulationHandler
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler
    for name in REFERENCE_METHODS + ["render_canvas", "get_environment", "download", "download_instance_data", "step",
                                     "draw_counters", "halo_counters", "positions", "particles", "set_solver_order"]:
        assert callable(getattr(ShardedSimulationHandler, name, None)), name
    for name in ("elapsed", "interpolation_alpha", "_use_particle_color", "_use_lighting"):
        assert isinstance(inspect.getattr_static(ShardedSimulationHandler, name), property), name
    for name in REFERENCE_METHODS:  # the single handle's parameters, in its order
        want = list(inspect.signature(getattr(SimulationHandler, name)).parameters)
        got = list(inspect.signature(getattr(ShardedSimulationHandler, name)).parameters)
        assert got[:len(want)] == want, (name, got, want)
    add = inspect.signature(ShardedSimulationHandler.add).parameters
    assert list(add)[1:5] == ["x", "y", "white_radius", "yolk_radius"]  # its current positional form comes first ...
    assert add["white_radius"].default == 50.0 and add["yolk_radius"].default == 15.0  # ... with its defaults
    assert all(add[k].default is None for k in list(add)[5:])  # everything new is optional
    assert list(add)[-2:] == ["white_n", "yolk_n"]
    assert "root" in inspect.signature(ShardedSimulationHandler.__init__).parameters
    for name in ("add_many", "export_batch", "step_begin"):  # single-handle plumbing stays off the sharded class
        assert not hasattr(ShardedSimulationHandler, name), name


def test_argument_checks_of_a_deviceless_sharded_handler():
    from egg_fluid_simulation_amd import EggError, EggWarning
    s = _bare()
    with pytest.raises(EggError, match=r"argument #1: expected `number`, got `string`"):
        s.set_target_position("a", 1, 2)
    with pytest.raises(EggError, match=r"argument #1: expected `number`, got `string`"):
        s.add("a", 2)
    with pytest.raises(EggError, match=r"expected `number`, got `nil`"):
        s.get_position(None)
    with pytest.raises(EggError, match=r"expected `number`, got `nil`"):
        s.get_target_position(None)
    with pytest.raises(EggError, match=r"expected `number`, got `table`"):
        s.remove([1])
    with pytest.raises(EggError, match=r"expected `table`"):
        s.set_white_config(3)
    with pytest.raises(EggError, match=r"expected `table`"):
        s.set_yolk_config("x")
    with pytest.raises(EggError, match="In SimulationHandler.set_yolk_config: color `color` does not have 4 components"):
        s.set_yolk_config({"color": [1, 1, 1]})
    with pytest.raises(EggError, match="wrong type for config key `damping`"):
        s.set_white_config({"damping": "x"})
    with pytest.raises(EggError, match="white radius cannot be 0 or negative"):
        s.add(1, 2, 0)
    with pytest.raises(EggError, match="yolk particle count cannot be 1 or negative"):
        s.add(1, 2, 50, 15, None, None, 100, 1)
    with pytest.raises(EggError, match="yolk particle count cannot be 1 or negative"):
        s.add(1, 2, 50, 15, yolk_n=1)
    with pytest.raises(EggError, match="yolk_n_particles and yolk_n are two names of one count and differ"):
        s.add(1, 2, 50, 15, None, None, 100, 6, yolk_n=7)
    with pytest.raises(EggError, match="white color component `a` is not a number"):
        s.add(1, 2, 50, 15, [1, 1, 1])
    with pytest.raises(EggError, match="position is not a finite number"):
        s.add(float("inf"), 2)
    with pytest.raises(EggError, match=r"argument #2: expected `number`, got `string`"):
        s.set_white_color(1, 0.5, "g", 0.5)
    with pytest.raises(EggError, match="`n_substeps` is not a number > 0"):
        s.update(1 / 60, 1 / 60, float("nan"))
    with pytest.raises(EggError, match="`step_delta` is 0"):
        s.update(1 / 60, 0)
    with pytest.raises(EggError, match="`n_collision_steps` is not a number > 0"):
        s.update(1 / 60, 1 / 60, 2, 0)
    for call, text in ((lambda: s.get_position(7), "In SimulationHandler.get_position: no batch with id `7`"),
                       (lambda: s.get_target_position(7), "In SimulationHandler.get_target_position: no batch with id `7`"),
                       (lambda: s.get_n_particles(7), "In SimulationHandler:get_n_particles: no batch with id `7`")):
        with pytest.raises(EggError, match=re.escape(text)):
            call()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        s.set_yolk_color(7, 2.0, 0.5, 0.5)  # out of range and an id nobody issued: two warnings, nothing else
        s.remove(7)
        s.set_target_position(7, 1.0, 2.0)
    msgs = " | ".join(str(r.message) for r in rec)
    assert all(isinstance(r.message, EggWarning) for r in rec) and len(rec) == 4
    assert "set_egg_yolk_color: color component is outside of [0, 1]" in msgs and "no batch with id `7`" in msgs
    assert "In SimulationHandler.remove: no batch with id `7`" in msgs
    assert "In SimulationHandler.set_target_position: no batch with id `7`" in msgs
    assert s.list_ids() == []
    with pytest.raises(EggError, match="only x, y, last_x, last_y, vx, vy, radius and batch_id"):
        s.download(0, "inv_mass")


def test_colour_tables_follow_the_reference_aliasing():
    """the per-id mirror of what the device library keeps per handle (egg_set_add_color / egg_set_color /
    egg_set_render_config): no device needed, the tables are host state"""
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler, SlabLayout

    class Local:  # the least a local handler must offer to add()
        n = 0

        def add_many_keyed(self, xs, ys, keys, white_radius=None, yolk_radius=None, **counts):
            self.n += 1
            self.counts = counts
            return [self.n]

        def set_solver_config(self, which, c):
            self.cfg = (which, c.damping)

        def remove(self, lid):
            self.removed = lid

    s = ShardedSimulationHandler(SlabLayout([0.0, 100.0]), 0, None, Local)
    white = list(s.get_white_config()["color"])
    s._use_particle_color = True
    a = s.add(10, 10)                                    # shares the config's tables
    b = s.add(20, 10, 50, 15, [0.1, 0.2, 0.3, 1.0], None, 12, 6)  # its own white table
    assert s.local.counts == dict(white_n_particles=12, yolk_n_particles=6)
    assert s._pcolor[a][0].tolist() == [ctypes.c_float(v).value for v in white]
    assert s._pcolor[b][0].tolist() == [ctypes.c_float(v).value for v in (0.1, 0.2, 0.3, 1.0)]
    s.set_white_color(b, 0.5, 0.5, 0.5)                  # an own table: the config keeps its colour
    assert list(s._rcfg[0].color) == [ctypes.c_float(v).value for v in white]
    s.set_white_color(a, 0.25, 0.5, 0.75)                # the shared table: retints the type
    assert list(s._rcfg[0].color) == [0.25, 0.5, 0.75, 1.0] and s.get_white_config()["color"] == [0.25, 0.5, 0.75, 1]
    s.set_white_config({"damping": 0.5})                 # set_*_config: the config's table is a new one from here on
    assert s.local.cfg == (0, 0.5)
    s.set_white_color(a, 1.0, 0.0, 0.0)
    assert list(s._rcfg[0].color) == [0.25, 0.5, 0.75, 1.0] and s._pcolor[a][0].tolist() == [1.0, 0.0, 0.0, 1.0]
    s._use_particle_color = False
    c = s.add(30, 10, 50, 15, [0.1, 0.2, 0.3, 1.0])
    assert s._pcolor[c].tolist() == [[1.0] * 4] * 2      # L:978-990: plain white unless the switch is set
    s.remove(a)
    assert s.list_ids() == [b, c] and a not in s._pcolor and s.get_target_position(b) == (20.0, 10.0)


def _prototypes(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return {m.group(1): [p for p in m.group(2).split(",") if p.strip()]
            for m in re.finditer(r"\b(?:int|void|const char \*|int32_t|egg_handle \*)\s*(egg_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", text)}


def test_the_draw_entry_points_are_declared_exported_and_bound():
    from egg_fluid_simulation_amd import _ffi
    header = open(os.path.join(ROOT, "include", "eggsim.h")).read()
    protos = _prototypes(header)
    if not os.path.exists(_ffi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _ffi.load()
    for name in NEW_ENTRY_POINTS:
        assert name in protos, name
        assert name in _ffi._SIGNATURES and name in _ffi.EXPORTED_SYMBOLS, name
        assert len(_ffi._SIGNATURES[name][1]) == len(protos[name]), (name, protos[name])
        assert hasattr(lib, name), "libeggsim.so does not export " + name
    # the draw entry points of the external source take egg_render's / egg_get_environment's / egg_render_canvas' parameters
    assert _ffi._SIGNATURES["egg_draw_source_render_canvas"][1] == _ffi._SIGNATURES["egg_render_canvas"][1]
    assert _ffi._SIGNATURES["egg_draw_source_download"][1] == _ffi._SIGNATURES["egg_download_particles"][1]
    assert _ffi.DRAW_RECORD_BYTES == 8 * len(_ffi.DRAW_FIELDS) == 56
    # and the ffi.cdef of the integration guide declares them with the header's parameters
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    bound = {}
    for cdef in re.findall(r"ffi\.cdef\[\[(.*?)\]\]", guide, flags=re.S):
        bound.update(_prototypes(cdef))
    for name in NEW_ENTRY_POINTS:
        assert name in bound, name
        assert [" ".join(p.split()) for p in bound[name]] == [" ".join(p.split()) for p in protos[name]], name
