"""The surface of yolk containment (egg_set_containment, DESIGN.md section 2.7 "Containment") as far as it can be checked
without a device: the six entry points in the header, the ctypes binding, the Lua wrapper and INTEGRATION.md, the three
methods on all three Python classes, the range check, and the rule and the refusals in the sources (what they do on a
device is tests/test_gpu_containment.py)."""
import inspect
import os
import re

import pytest

from conftest import ROOT
from test_cohesion_surface import _header

PROTOS = {
    "egg_set_containment": "int egg_set_containment(egg_handle *h, double factor, double strength);",
    "egg_get_containment": "int egg_get_containment(const egg_handle *h, double *factor, double *strength);",
    "egg_get_containment_hits": "int egg_get_containment_hits(egg_handle *h, int64_t *hits);",
}
GROUP_PROTOS = {
    "egg_group_set_containment": "int egg_group_set_containment(egg_group *g, double factor, double strength);",
    "egg_group_get_containment": "int egg_group_get_containment(const egg_group *g, double *factor, double *strength);",
    "egg_group_get_containment_hits": "int egg_group_get_containment_hits(egg_group *g, int64_t *hits);",
}
CSRC = os.path.join(ROOT, "egg_fluid_simulation_amd", "csrc")


def _read(*parts):
    return open(os.path.join(*parts)).read()


def test_header_and_binding_declare_the_six_entry_points():
    from egg_fluid_simulation_amd import _ffi
    text = _header()
    for name, proto in dict(PROTOS, **GROUP_PROTOS).items():
        assert proto in text, name
        assert name in _ffi._SIGNATURES and name in _ffi.EXPORTED_SYMBOLS, name
        assert len(_ffi._SIGNATURES[name][1]) == proto.count(",") + 1, name
    # the header states the rule: the order in the sub-step, the summation order, the projection, the limits
    section = text[text.index("yolk containment"):text.index(PROTOS["egg_set_containment"])]
    for phrase in ("does not depend on coupling or adhesion", "3. containment; 4. the collision passes",
                   "a[l] = a[l] + a[l ^ d]", "d = 32, 16, 8, 4, 2, 1", "L = +inf", "keep = L + (1 - strength) (d - L)",
                   "No mass test", "the white is never moved", "device groups", "This summation order is part of the rule"):
        assert phrase in section, phrase


def test_python_classes_have_the_three_methods():
    from egg_fluid_simulation_amd import SimulationGroup, SimulationHandler
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler
    for cls in (SimulationHandler, SimulationGroup, ShardedSimulationHandler):
        sig = inspect.signature(cls.set_containment)
        assert list(sig.parameters) == ["self", "factor", "strength"], cls
        assert [p.default for p in sig.parameters.values()][1:] == [0.0, 1.0], cls
        assert list(inspect.signature(cls.containment).parameters) == ["self"], cls
        assert list(inspect.signature(cls.containment_hits).parameters) == ["self"], cls
    # a group calls its own entry points, a sharded handler its local handle and an all-reduce
    assert SimulationGroup._PREFIX == "egg_group_" and SimulationGroup.set_containment is SimulationHandler.set_containment
    src = inspect.getsource(ShardedSimulationHandler.containment_hits)
    assert "self.local.containment_hits()" in src and "all_reduce" in src


def test_the_range_check():
    """factor finite and >= 0, strength in [0, 1]; anything else is refused before any device call"""
    from egg_fluid_simulation_amd import EggError, SimulationGroup, SimulationHandler
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler
    for good in ((0.0, 1.0), (2.0, 1.0), (0.5, 0.0), (-0.0, 0.5), (1, 1)):
        assert SimulationHandler._c_containment(*good) == (float(good[0]), float(good[1]))
    nan, inf = float("nan"), float("inf")
    for cls in (SimulationHandler, SimulationGroup):
        bare = cls.__new__(cls)  # (no handle: a device call would fail on it)
        for bad in ((nan, 1.0), (-1e-300, 1.0), (-1.0, 1.0), (inf, 1.0), (-inf, 1.0)):
            with pytest.raises(EggError, match="not a finite number >= 0"):
                bare.set_containment(*bad)
        for bad in ((1.0, nan), (1.0, -0.25), (1.0, 1.0000000000000002), (0.0, 2.0), (1.0, inf)):
            with pytest.raises(EggError, match="outside"):
                bare.set_containment(*bad)
        with pytest.raises(EggError, match="must be a number"):
            bare.set_containment("tight", 1.0)
    # a sharded handler hands the values to its local handle, whose check it is
    bare = ShardedSimulationHandler.__new__(ShardedSimulationHandler)
    bare.local = SimulationHandler.__new__(SimulationHandler)
    for bad, text in (((nan, 1.0), "not a finite number >= 0"), ((1.0, 1.5), "outside"), (("tight", 1.0), "must be a number")):
        with pytest.raises(EggError, match=text):
            bare.set_containment(*bad)
    # the library's own check is the same one
    abi = _read(CSRC, "eggsim_host_abi.hip")
    body = abi[abi.index("int egg_set_containment("):abi.index("int egg_get_containment(")]
    assert "if (!(factor >= 0.0 && std::isfinite(factor)))" in body
    assert "if (!(strength >= 0.0 && strength <= 1.0))" in body


def test_the_rules_stand_in_the_sources():
    abi = _read(CSRC, "eggsim_host_abi.hip")
    # factor > 0 is refused on a handle in exact order ...
    assert re.search(r"factor > 0\.0 && h->opt_solver_order != EGG_SOLVER_RELAXED\)\s*return fail\(h, EGG_ERR_UNSUPPORTED, \"egg_set_containment", abi)
    # ... and exact order while factor > 0
    assert re.search(r"value == EGG_SOLVER_EXACT && h->containment_factor > 0\.0\)\s*return fail\(h, EGG_ERR_UNSUPPORTED", abi)
    assert 'REJECT_IN_FLIGHT(h, "egg_set_containment");' in abi
    # it acts with or without a halo: no refusal in egg_rx_begin or in the group step, which only wants equal values
    wire = _read(CSRC, "eggsim_host_relaxed_wire.hip")
    assert "launch_contain_sum(W.st[0], sub)" in wire and "launch_contain(W.st[1], W.st[0], sub)" in wire
    assert not re.search(r"containment_factor > 0\.0\)[^\n]*\n\s*return fail", wire)
    group = _read(CSRC, "eggsim_host_relaxed_group.hip")
    assert "the handles of the group differ in their containment (egg_group_set_containment sets all)" in group
    assert "launch_contain_sum(t[0], sub)" in group and "launch_contain(t[1], t[0], sub)" in group
    # the layout: acting is factor > 0 and both types populated; the word is the last one, on the yolk
    host = _read(CSRC, "eggsim_host_relaxed.hip")
    assert "st.L.containment = h->containment_factor > 0.0 && h->sys[0].n > 0 && h->sys[1].n > 0;" in host
    assert "st.L.contained_word = st.L.containment && st.w == 1;" in host
    hdr = _read(CSRC, "eggsim_host.h")
    assert "size_t contained() const { return adhered() + (adhered_word ? 1 : 0); }" in hdr
    assert "size_t words() const { return contained() + (contained_word ? 1 : 0); }" in hdr
    # one event per sub-step, recorded after the summary and waited for before the projection
    assert re.search(r"egg_rx_contain_sum_kernel[^;]*;\s*\+\+st\.launches;\s*HIP_TRY\(h, hipEventRecord\(h->contain_summed\[\(size_t\)sub\]", host)
    assert re.search(r"hipStreamWaitEvent\(s\.stream, h->contain_summed\[\(size_t\)sub\], 0\)\);", host)
    # the kernels are three of their own: the gather keeps its five template parameters
    kernels = _read(CSRC, "eggsim_relaxed.hip")
    for k in ("egg_rx_contain_sum_kernel(EggRxContainSumArgs K)", "egg_rx_contain_kernel(EggRxContainArgs K)",
              "egg_rx_contain_group_kernel(EggRxContainArgs K)"):
        assert "__launch_bounds__(256) " + k in kernels, k
    assert "template <bool G, bool K, bool D, bool S, bool W>\n__device__ __forceinline__ void rx_gather(" in kernels
    # the rule's arithmetic, in the kernel's words
    assert "for (int d = 32; d >= 1; d >>= 1) a = a + __shfl_xor(a, d, 64);" in kernels
    assert "for (int k = l; k < n; k += 64)" in kernels
    assert "if (d > L) {" in kernels and "const double keep = L + (1.0 - K.strength) * (d - L);" in kernels


def test_lua_wrapper_and_documents_name_the_methods():
    lua = _read(ROOT, "egg_fluid_simulation_amd", "lua", "egg_fluid_simulation", "simulation_handler.lua")
    for name in ("set_containment(factor, strength)", "containment()", "containment_hits()"):
        assert "function SimulationHandler:" + name in lua, name
    for name, proto in PROTOS.items():
        assert proto in lua and "lib." + name + "(self._h" in lua, name
    integration = _read(ROOT, "INTEGRATION.md")
    for name, proto in PROTOS.items():
        assert proto in integration, name
    for name in GROUP_PROTOS:
        assert name in integration, name
    design = _read(ROOT, "DESIGN.md")
    assert re.search(r"^#+ Containment", design, flags=re.M)
    section = design[design.index("#### Containment"):]
    for phrase in ("egg_rx_contain_sum_kernel", "egg_rx_contain_kernel", "egg_rx_contain_group_kernel", "superset", "wsum",
                   "230.44297079401801", "113.07708254124792", "115.76261943016195", "52.218422258496894"):
        assert phrase in section, phrase
    limits = design[design.index("yolk containment (`egg_set_containment`)"):]
    for phrase in ("one-way", "a disc, not the white's outline", "does not hold the white together"):
        assert phrase in limits[:1500], phrase
    readme = _read(ROOT, "README.md")
    assert "set_containment" in readme and "egg_set_containment" in readme
