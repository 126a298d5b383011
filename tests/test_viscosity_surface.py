"""The surface of the viscosity (egg_set_viscosity, DESIGN.md section 2.7 "Viscosity") as far as it can be checked without a
device: the six entry points and the pass constant in the header and in the ctypes binding, the three methods on all three
Python classes and in the Lua wrapper, the range check, and the exact-order refusals in the sources (what they do on a
device is tests/test_gpu_viscosity.py::test_rules)."""
import inspect
import os
import re

import pytest

from conftest import ROOT
from test_cohesion_surface import _header

PROTOS = {
    "egg_set_viscosity": "int egg_set_viscosity(egg_handle *h, const double c[2]);",
    "egg_get_viscosity": "int egg_get_viscosity(const egg_handle *h, double c[2]);",
    "egg_get_viscosity_pairs": "int egg_get_viscosity_pairs(egg_handle *h, int64_t pairs[2]);",
    "egg_group_set_viscosity": "int egg_group_set_viscosity(egg_group *g, const double c[2]);",
    "egg_group_get_viscosity": "int egg_group_get_viscosity(const egg_group *g, double c[2]);",
    "egg_group_get_viscosity_pairs": "int egg_group_get_viscosity_pairs(egg_group *g, int64_t pairs[2]);",
}
CSRC = os.path.join(ROOT, "egg_fluid_simulation_amd", "csrc")


def test_header_declares_the_six_entry_points_and_the_pass_constant():
    from egg_fluid_simulation_amd import _ffi
    text = _header()
    for name, proto in PROTOS.items():
        assert proto in text, name
        assert name in _ffi._SIGNATURES and name in _ffi.EXPORTED_SYMBOLS, name
        assert len(_ffi._SIGNATURES[name][1]) == proto.count(",") + 1 == 2, name
    assert re.search(r"#define EGG_RX_VISCOSITY_PASS 0x40000000\b", text)
    assert _ffi.RX_VISCOSITY_PASS == 0x40000000 == 1 << 30
    # the sequence comment of the egg_rx_* calls documents the pass
    seq = text[text.index("egg_rx_set_keys (per type"):text.index("A MESSAGE is one contiguous run")]
    assert "EGG_RX_VISCOSITY_PASS + sub" in seq and "egg_rx_run_pass(v)" in seq
    # a record stays five words: the displacement travels in the words of inverse mass and radius
    device_h = open(os.path.join(CSRC, "eggsim_device.h")).read()
    assert re.search(r"#define EGG_RX_WIRE_RECORD_WORDS 5\b", device_h) and _ffi.RX_RECORD_WORDS == 5


def test_python_classes_have_the_three_methods():
    from egg_fluid_simulation_amd import SimulationGroup, SimulationHandler
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler
    for cls in (SimulationHandler, SimulationGroup, ShardedSimulationHandler):
        sig = inspect.signature(cls.set_viscosity)
        assert list(sig.parameters) == ["self", "white", "yolk"], cls
        assert [p.default for p in sig.parameters.values()][1:] == [0.0, 0.0], cls
        assert list(inspect.signature(cls.viscosity).parameters) == ["self"], cls
        assert list(inspect.signature(cls.viscosity_pairs).parameters) == ["self"], cls


def test_the_range_check():
    """[0, 1] is accepted; NaN, negative values and values above 1 are refused before any device call"""
    from egg_fluid_simulation_amd import EggError, SimulationGroup, SimulationHandler
    for good in ((0.0, 0.0), (1.0, 1.0), (0.25, 0.0), (0.0, 1.0), (-0.0, 0.5), (1, 0)):
        arr = SimulationHandler._c_viscosity(*good)
        assert (arr[0], arr[1]) == (float(good[0]), float(good[1]))
    nan = float("nan")
    for cls in (SimulationHandler, SimulationGroup):
        bare = cls.__new__(cls)
        for bad in ((nan, 0.0), (0.0, nan), (-0.25, 0.0), (0.0, -1e-300), (1.0000000000000002, 0.0), (0.0, 2.0), (float("inf"), 0.0),
                    (float("-inf"), 0.0)):
            with pytest.raises(EggError, match="outside"):
                bare.set_viscosity(*bad)
        with pytest.raises(EggError, match="must be a number"):
            bare.set_viscosity("thick", 0.0)
    # the library's own check is the same one
    abi = open(os.path.join(CSRC, "eggsim_host_abi.hip")).read()
    assert "if (!(c[w] >= 0.0 && c[w] <= 1.0))" in abi


def test_the_exact_order_refusals_stand_both_ways():
    abi = open(os.path.join(CSRC, "eggsim_host_abi.hip")).read()
    group = open(os.path.join(CSRC, "eggsim_group.cpp")).read()
    # a non-zero coefficient is refused on a handle in exact order ...
    assert re.search(r"\(c\[0\] != 0\.0 \|\| c\[1\] != 0\.0\) && h->opt_solver_order != EGG_SOLVER_RELAXED\)\s*return fail\(h, EGG_ERR_UNSUPPORTED", abi)
    # ... and exact order while a coefficient is not zero, on a handle and on a group
    assert re.search(r"value == EGG_SOLVER_EXACT && \(h->viscosity\[0\] != 0\.0 \|\| h->viscosity\[1\] != 0\.0\)\)\s*return fail\(h, EGG_ERR_UNSUPPORTED", abi)
    assert re.search(r"order == EGG_SOLVER_EXACT && \(g->viscosity\[0\] != 0\.0 \|\| g->viscosity\[1\] != 0\.0\)\)\s*return gfail\(g, EGG_ERR_UNSUPPORTED", group)
    # a group whose handles differ refuses to step
    assert "differ in their viscosity" in open(os.path.join(CSRC, "eggsim_host_relaxed_group.hip")).read()


def test_lua_wrapper_and_documents_name_the_methods():
    lua = open(os.path.join(ROOT, "egg_fluid_simulation_amd", "lua", "egg_fluid_simulation", "simulation_handler.lua")).read()
    for name in ("set_viscosity(white, yolk)", "viscosity()", "viscosity_pairs()"):
        assert "function SimulationHandler:" + name in lua, name
    for name in ("egg_set_viscosity", "egg_get_viscosity", "egg_get_viscosity_pairs"):
        assert PROTOS[name] in lua and "lib." + name + "(self._h" in lua, name
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("egg_set_viscosity", "egg_get_viscosity", "egg_get_viscosity_pairs"):
        assert PROTOS[name] in integration, name
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^\*\*Viscosity\.\*\*|^#+ .*Viscosity", design, flags=re.M)
    assert "set_viscosity" in open(os.path.join(ROOT, "README.md")).read()
