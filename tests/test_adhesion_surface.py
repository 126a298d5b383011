"""The surface of white-yolk adhesion (egg_set_adhesion, DESIGN.md section 2.7 "Adhesion") as far as it can be checked
without a device: the three entry points in the header, the ctypes binding, the Lua wrapper and INTEGRATION.md, the three
methods on all three Python classes, the range check, and the refusals in the sources (what they do on a device is
tests/test_gpu_adhesion.py::test_rules)."""
import inspect
import os
import re

import pytest

from conftest import ROOT
from test_cohesion_surface import _header

PROTOS = {
    "egg_set_adhesion": "int egg_set_adhesion(egg_handle *h, double reach, double strength);",
    "egg_get_adhesion": "int egg_get_adhesion(const egg_handle *h, double *reach, double *strength);",
    "egg_get_adhesion_solves": "int egg_get_adhesion_solves(egg_handle *h, int64_t *solves);",
}
CSRC = os.path.join(ROOT, "egg_fluid_simulation_amd", "csrc")


def _read(*parts):
    return open(os.path.join(*parts)).read()


def test_header_and_binding_declare_the_three_entry_points():
    from egg_fluid_simulation_amd import _ffi
    text = _header()
    for name, proto in PROTOS.items():
        assert proto in text, name
        assert name in _ffi._SIGNATURES and name in _ffi.EXPORTED_SYMBOLS, name
        assert len(_ffi._SIGNATURES[name][1]) == proto.count(",") + 1, name
    # there is no group twin: a device group refuses adhesion
    assert not [s for s in _ffi.EXPORTED_SYMBOLS if "adhesion" in s and s.startswith("egg_group_")]
    # the block stands behind coupling's, whose own text is as it was
    assert text.index("int egg_get_coupling_solves(") < text.index("white-yolk adhesion (not in the reference") < text.index(PROTOS["egg_set_adhesion"])
    section = text[text.index("white-yolk adhesion (not in the reference"):text.index(PROTOS["egg_set_adhesion"])]
    # the three conditions, the band, the target and the limits
    for phrase in ("coupling acts", "reach > factor", "the solver order is relaxed", "d2 <= rd rd", "TARGET", "same batch",
                   "max(factor, reach)", "A single handle only", "EGG_ERR_UNSUPPORTED while reach > 0", "egg_get_coupling_solves keeps"):
        assert phrase in section, phrase


def test_python_classes_have_the_three_methods():
    from egg_fluid_simulation_amd import SimulationGroup, SimulationHandler
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler
    for cls in (SimulationHandler, SimulationGroup, ShardedSimulationHandler):
        sig = inspect.signature(cls.set_adhesion)
        assert list(sig.parameters) == ["self", "reach", "strength"], cls
        assert [p.default for p in sig.parameters.values()][1:] == [0.0, 1.0], cls
        assert list(inspect.signature(cls.adhesion).parameters) == ["self"], cls
        assert list(inspect.signature(cls.adhesion_solves).parameters) == ["self"], cls


def test_the_range_check():
    """reach finite and >= 0, strength in [0, 1]; anything else is refused before any device call"""
    from egg_fluid_simulation_amd import EggError, SimulationGroup, SimulationHandler
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler
    for good in ((0.0, 1.0), (3.0, 1.0), (0.5, 0.0), (-0.0, 0.5), (1, 1)):
        assert SimulationHandler._c_adhesion(*good) == (float(good[0]), float(good[1]))
    nan, inf = float("nan"), float("inf")
    for cls in (SimulationHandler, SimulationGroup, ShardedSimulationHandler):
        bare = cls.__new__(cls)  # (no handle: a device call would fail on it)
        for bad in ((nan, 1.0), (-1e-300, 1.0), (-1.0, 1.0), (inf, 1.0), (-inf, 1.0)):
            with pytest.raises(EggError, match="not a finite number >= 0"):
                bare.set_adhesion(*bad)
        for bad in ((1.0, nan), (1.0, -0.25), (1.0, 1.0000000000000002), (0.0, 2.0), (1.0, inf)):
            with pytest.raises(EggError, match="outside"):
                bare.set_adhesion(*bad)
        with pytest.raises(EggError, match="must be a number"):
            bare.set_adhesion("sticky", 1.0)
        with pytest.raises(EggError, match="must be a number"):
            bare.set_adhesion(1.0, None)
    # the library's own check is the same one
    abi = _read(CSRC, "eggsim_host_abi.hip")
    assert "if (!(reach >= 0.0 && std::isfinite(reach)))" in abi
    body = abi[abi.index("int egg_set_adhesion("):abi.index("int egg_get_adhesion(")]
    assert "if (!(strength >= 0.0 && strength <= 1.0))" in body


def test_group_and_sharded_accept_zero_only():
    """adhesion is a band in the coupling pass, which several handles do not run: reach 0 is accepted, anything else names
    the limit; the getters report the defaults"""
    from egg_fluid_simulation_amd import EggError, SimulationGroup
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler
    for cls in (SimulationGroup, ShardedSimulationHandler):
        bare = cls.__new__(cls)
        assert bare.set_adhesion() is None and bare.set_adhesion(0.0, 0.5) is None and bare.set_adhesion(-0.0) is None
        for reach in (3.0, 1e-300):
            with pytest.raises(EggError, match="single SimulationHandler only"):
                bare.set_adhesion(reach, 1.0)
        assert bare.adhesion() == (0.0, 1.0) and bare.adhesion_solves() == 0


def test_the_refusals_stand_in_the_sources():
    abi = _read(CSRC, "eggsim_host_abi.hip")
    # reach > 0 is refused on a handle in exact order ...
    assert re.search(r"reach > 0\.0 && h->opt_solver_order != EGG_SOLVER_RELAXED\)\s*return fail\(h, EGG_ERR_UNSUPPORTED", abi)
    # ... and exact order while reach > 0
    assert re.search(r"value == EGG_SOLVER_EXACT && h->adhesion_reach > 0\.0\)\s*return fail\(h, EGG_ERR_UNSUPPORTED", abi)
    # refused while a step is in flight
    assert 'REJECT_IN_FLIGHT(h, "egg_set_adhesion");' in abi
    # egg_rx_begin and a device group's relaxed step refuse while reach > 0, and say why
    wire = _read(CSRC, "eggsim_host_relaxed_wire.hip")
    assert re.search(r"if \(h->adhesion_reach > 0\.0\)[^\n]*\n\s*return fail\(h, EGG_ERR_UNSUPPORTED, \"egg_rx_begin: white-yolk adhesion runs on a "
                     r"single handle only", wire)
    group = _read(CSRC, "eggsim_host_relaxed_group.hip")
    assert "adhesion_reach > 0.0" in group and "white-yolk adhesion runs on a single handle only" in group
    # adhesion acts when coupling acts and reach > factor, decided per step
    host = _read(CSRC, "eggsim_host_relaxed.hip")
    assert "st.L.adhesion = st.L.coupling && h->adhesion_reach > h->coupling_factor;" in host
    # the pass is one body in two instantiations; the gather keeps its five template parameters
    kernels = _read(CSRC, "eggsim_relaxed.hip")
    assert "egg_rx_couple_kernel(EggRelaxedCoupleArgs K) { rx_couple<false>(" in kernels
    assert "egg_rx_couple_adh_kernel(EggRelaxedCoupleAdhArgs K) { rx_couple<true>(" in kernels
    assert "template <bool G, bool K, bool D, bool S, bool W>\n__device__ __forceinline__ void rx_gather(" in kernels


def test_lua_wrapper_and_documents_name_the_methods():
    lua = _read(ROOT, "egg_fluid_simulation_amd", "lua", "egg_fluid_simulation", "simulation_handler.lua")
    for name in ("set_adhesion(reach, strength)", "adhesion()", "adhesion_solves()"):
        assert "function SimulationHandler:" + name in lua, name
    for name, proto in PROTOS.items():
        assert proto in lua and "lib." + name + "(self._h" in lua, name
    integration = _read(ROOT, "INTEGRATION.md")
    for name, proto in PROTOS.items():
        assert proto in integration, name
    design = _read(ROOT, "DESIGN.md")
    assert re.search(r"^\*\*Adhesion\.\*\*|^#+ .*Adhesion", design, flags=re.M)
    assert "egg_rx_couple_adh_kernel" in design and "egg_set_adhesion" in design
    readme = _read(ROOT, "README.md")
    assert "set_adhesion" in readme and "egg_set_adhesion" in readme
