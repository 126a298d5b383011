"""The surface of the wall collider (EGG_COLLIDER_WALL, DESIGN.md section 2.7 "Walls").  Without a device: the fifth kind (number 5; 4 stays no kind) in
the header, in the ctypes binding, in the kernel's header and in the Lua wrapper, its shape checked like a segment's by
the Python classes -- and that it added no entry point, option, stats field or argument struct.  On a device (marked gpu):
the kind round-trips through set and get, the library validates it like a segment, and the refusals of any collider
list hold for it (exact order, a step in flight).  The sharded class is covered from its ranks in
test_gpu_collider_walls.py."""
import ctypes as C
import inspect
import math
import os
import re

import pytest

from conftest import ROOT
from test_cohesion_surface import _enum_values, _header

CSRC = os.path.join(ROOT, "egg_fluid_simulation_amd", "csrc")


def test_header_and_binding_name_the_fifth_kind():
    from egg_fluid_simulation_amd import _ffi
    text = _header()
    # the four kinds there were keep their enum and their numbers; the wall has an enum of its own, and 4 stays no kind
    kinds = _enum_values(text, "EGG_COLLIDER_HALF_PLANE")
    assert kinds == {"EGG_COLLIDER_HALF_PLANE": 0, "EGG_COLLIDER_DISC": 1, "EGG_COLLIDER_CONTAINER": 2, "EGG_COLLIDER_SEGMENT": 3}
    assert _enum_values(text, "EGG_COLLIDER_WALL") == {"EGG_COLLIDER_WALL": 5}
    assert _ffi.COLLIDER_KINDS == ("half_plane", "disc", "container", "segment") and _ffi.COLLIDER_WALL == 5
    assert _ffi.COLLIDER_CODES == {"half_plane": 0, "disc": 1, "container": 2, "segment": 3, "wall": 5}
    assert _ffi.COLLIDER_NAMES == {0: "half_plane", 1: "disc", 2: "container", 3: "segment", 5: "wall"}
    assert sorted(_ffi.COLLIDER_PARAM_NAMES) == [0, 1, 2, 3, 5]
    assert _ffi.COLLIDER_PARAM_NAMES[5] == _ffi.COLLIDER_PARAM_NAMES[3] == _ffi.COLLIDER_PARAMS[3] == ("x0", "y0", "x1", "y1")
    assert C.sizeof(_ffi.EggCollider) == 40 and _ffi.MAX_COLLIDERS == 64  # (the record did not grow)
    # the rule is documented where the other kinds are
    doc = text[text.index("---- static colliders"):text.index("#define EGG_MAX_COLLIDERS")]
    for word in ("WALL", "a0 = ex (prev.y - y0) - ey (prev.x - x0)", "tc >= 0 && tc <= 1", "pen = m + d"):
        assert word in doc, word
    # the kernel's constant is the ABI's
    device_h = open(os.path.join(CSRC, "eggsim_device.h")).read()
    assert re.search(r"#define EGG_RX_COLLIDER_WALL 5\b", device_h)


def test_no_entry_point_option_stats_field_or_argument_struct_was_added():
    from egg_fluid_simulation_amd import _ffi
    assert not [s for s in _ffi.EXPORTED_SYMBOLS if "wall" in s.lower()]
    assert not re.search(r"\begg_\w*wall\w*\s*\(", _header(), flags=re.I)
    opts = _enum_values(_header(), "EGG_OPT_CLAIM_MARGIN_CELLS")
    assert max(opts, key=opts.get) == "EGG_OPT_FORCE_CELL_HASH" and opts["EGG_OPT_FORCE_CELL_HASH"] == 16
    body = re.search(r"typedef struct\s*\{((?:(?!typedef).)*?)\}\s*egg_stats\s*;", re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S),
                     flags=re.S).group(1)
    fields = re.findall(r"([a-z_]+)(?:\[[^;]*\])*\s*;", body)
    assert fields[-2:] == ["cohesion_solves", "cell_hash"] and [f[0] for f in _ffi.EggStats._fields_] == fields
    # four new gather instantiations, on the surface instantiations' argument structs
    device_h = open(os.path.join(CSRC, "eggsim_device.h")).read()
    assert not re.search(r"struct \w*Wall\w*", device_h)
    # (rows of the one kernel list: defined, declared to the host and put into its table by the list's expansions)
    import rx_kernel_list
    rows = rx_kernel_list.assert_expansions()
    walls = [name for name in rows if "wall" in name]
    assert walls == ["egg_rx_gather_col_wall_kernel", "egg_rx_gather_group_col_wall_kernel", "egg_rx_gather_coh_col_wall_kernel",
                     "egg_rx_gather_group_coh_col_wall_kernel"]
    assert [n for n, r in rows.items() if r["flavour"] == "EGG_RX_WALL"] == walls  # (in the table under the walls' flavour, nowhere else)
    for name in walls:  # the surface instantiations' arguments -- the same groups, no pointer more -- and W = true
        srf = rows[name.replace("_wall_", "_srf_")]
        assert rows[name] == dict(srf, flavour="EGG_RX_WALL", W=True) and not srf["W"], name
        assert (rows[name]["G"], rows[name]["K"]) == ("_group" in name, "_coh" in name), name
        assert rows[name]["D"] and rows[name]["S"] and not (rows[name]["Mo"] or rows[name]["Sp"] or rows[name]["Ld"]), name
    # a wall in the list outranks a friction and nothing else
    order = rx_kernel_list.flavour_precedence()
    assert order[order.index(("walls", "EGG_RX_WALL")) + 1] == ("surfaces", "EGG_RX_SRF")
    assert [f for _, f in order[:order.index(("walls", "EGG_RX_WALL"))]] == ["EGG_RX_LOAD", "EGG_RX_SPIN", "EGG_RX_MOV"]


def test_python_classes_take_the_kind_and_check_its_shape_like_a_segments():
    from egg_fluid_simulation_amd import EggError, SimulationGroup, SimulationHandler
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler
    for cls in (SimulationHandler, SimulationGroup, ShardedSimulationHandler):
        assert list(inspect.signature(cls.set_colliders).parameters) == ["self", "colliders"], cls
    assert "wall" in SimulationHandler.set_colliders.__doc__
    n, arr = SimulationHandler._c_colliders([("wall", 1, 2, 3, 4), ("wall", 5, 6, 7, 8, "white"),
                                             {"kind": "wall", "x0": 1.5, "y0": 2, "x1": 3, "y1": -4, "types": "yolk"}, ("segment", 1, 2, 3, 4)])
    assert n == 4
    assert [(c.kind, c.type_mask, list(c.p)) for c in arr[:n]] == [(5, 3, [1, 2, 3, 4]), (5, 1, [5, 6, 7, 8]), (5, 2, [1.5, 2, 3, -4]),
                                                                    (3, 3, [1, 2, 3, 4])]
    for cls in (SimulationHandler, SimulationGroup):
        bare = cls.__new__(cls)
        for kind in ("wall", "segment"):  # the same shapes are refused for both, before any device call
            for bad in ([(kind, 0, 0, 1)], [(kind, 0, 0, 1, 1, 1)], [(kind, 0, 0, 1, 1, "red")], [(kind, 0, 0, 1, "x")],
                        [{"kind": kind, "x0": 0, "y0": 0, "x1": 1}], [{"kind": kind, "x0": 0, "y0": 0, "x1": 1, "y1": 1, "R": 2}]):
                with pytest.raises(EggError, match="collider 0"):
                    bare.set_colliders(bad)
        with pytest.raises(EggError, match="collider 1"):
            bare.set_colliders([("disc", 0, 0, 1), ("walls", 0, 0, 1, 1)])


def test_lua_wrapper_and_documents_name_the_kind():
    lua = open(os.path.join(ROOT, "egg_fluid_simulation_amd", "lua", "egg_fluid_simulation", "simulation_handler.lua")).read()
    assert re.search(r"_collider_kinds = \{[^}]*segment = 3, wall = 5 \}", lua)
    assert re.search(r'_collider_names = \{ \[0\] = "half_plane", "disc", "container", "segment", \[5\] = "wall" \}', lua)
    assert re.search(r"_collider_n_params = \{ \[0\] = 3, 3, 3, 4, \[5\] = 4 \}", lua)
    for doc in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        assert re.search(r'"wall"|`wall`|EGG_COLLIDER_WALL', open(os.path.join(ROOT, doc)).read()), doc


@pytest.mark.gpu
def test_round_trip_validation_and_refusals_on_a_device():
    import egg_fluid_simulation_amd as egg
    INF = math.inf
    good = [("wall", 100.0, 380.0, 500.0, 380.0), ("wall", 3.0, 3.0, 3.0, 3.0, "white"), ("segment", 1.0, 2.0, 3.0, 4.0, "yolk")]
    stored = [("wall", 100.0, 380.0, 500.0, 380.0, "both"), ("wall", 3.0, 3.0, 3.0, 3.0, "white"), ("segment", 1.0, 2.0, 3.0, 4.0, "yolk")]
    nan, inf = float("nan"), float("inf")
    h = egg.SimulationHandler()
    g = egg.SimulationGroup([0, 0], cuts=[-INF, 0.0, INF])
    for o in (h, g):
        # refused in exact order, as any non-empty list
        with pytest.raises(egg.EggError, match="relaxed order"):
            o.set_colliders(good)
        assert o.get_colliders() == []
        o.set_solver_order("relaxed")
        o.set_colliders(good)
        assert o.get_colliders() == stored  # (a degenerate wall is accepted, as a degenerate segment is)
        assert o.get_collider_surfaces() == [(0.0, 0.0, 0.0)] * 3
        # validated like a segment: four finite parameters
        for q in range(4):
            for v in (nan, inf, -inf):
                for kind in ("wall", "segment"):
                    p = [1.0, 2.0, 3.0, 4.0]
                    p[q] = v
                    with pytest.raises(egg.EggError, match=r"collider 1 \(%s\): parameter %d is not finite" % (kind, q)):
                        o.set_colliders([good[0], (kind, *p)])
                    assert o.get_colliders() == stored
        with pytest.raises(egg.EggError, match="clear the list first"):
            o.set_solver_order("exact")
        o.set_collider_surfaces([0.5, None, (0.25, 1.0, 2.0)])  # a wall takes a surface as any collider
        assert o.get_collider_surfaces() == [(0.5, 0.0, 0.0), (0.0, 0.0, 0.0), (0.25, 1.0, 2.0)]
    # the raw ABI: kind 5 is the wall; 4 and 6 are no kinds (4 was refused before there were walls and stays refused); a
    # mask of 0 is refused for a wall too
    lib, EC = egg._ffi.load(), egg._ffi.EggCollider
    bad = egg._ffi.EGG_ERR_INVALID_ARGUMENT
    for kind, mask, rc in ((5, 3, egg._ffi.EGG_OK), (4, 3, bad), (6, 3, bad), (5, 0, bad)):
        arr = (EC * 1)()
        arr[0].kind, arr[0].type_mask = kind, mask
        arr[0].p[0], arr[0].p[1], arr[0].p[2], arr[0].p[3] = 1.0, 2.0, 3.0, 4.0
        assert lib.egg_set_colliders(h._h, 1, arr) == rc
        assert h.get_colliders() == ([("wall", 1.0, 2.0, 3.0, 4.0, "both")] if kind == 5 and mask == 3 else h.get_colliders())
    assert h.get_colliders() == [("wall", 1.0, 2.0, 3.0, 4.0, "both")]
    # while a step is in flight (split steps exist in exact order only; the in-flight refusal comes before every other check)
    e = egg.SimulationHandler()
    e.add(300.0, 300.0, 50, 15)
    e.step_begin(1 / 60, 2, 3)
    with pytest.raises(egg.EggError, match="egg_set_colliders.*in flight"):
        e.set_colliders(good)
    e.step_end(True)
    assert e.get_colliders() == []
    h.set_colliders(good)
    assert h.get_colliders() == stored
