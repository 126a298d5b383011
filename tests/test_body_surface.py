"""The surface of collider bodies (egg_set_collider_bodies, DESIGN.md section 2.7 "Collider bodies") as far as it can be
checked without a device: the two entry points and the 48-byte struct in the header and in the ctypes binding, the methods on
all three Python classes and in the Lua wrapper, the wrapper's own refusals, the limits of the group and sharded classes, the
kernel and its launch, the refusals where the sources state them, and the documents."""
import ctypes as C
import inspect
import os
import re

import pytest

from conftest import ROOT
from test_cohesion_surface import _header

CSRC = os.path.join(ROOT, "egg_fluid_simulation_amd", "csrc")
PROTOS = {
    "egg_set_collider_bodies": "int egg_set_collider_bodies(egg_handle *h, int32_t n, const egg_collider_body *b);",
    "egg_get_collider_bodies": "int egg_get_collider_bodies(const egg_handle *h, int32_t cap, egg_collider_body *b, int32_t *n);",
}
FIELDS = ["inv_mass", "inv_inertia", "ax", "ay", "drag", "spin_drag"]


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_header_declares_the_entry_points_and_the_struct():
    from egg_fluid_simulation_amd import _ffi
    text = _header()
    for name, proto in PROTOS.items():
        assert proto in text, name
        assert name in _ffi._SIGNATURES and name in _ffi.EXPORTED_SYMBOLS, name
        assert len(_ffi._SIGNATURES[name][1]) == proto.count(",") + 1, name
    assert not [s for s in _ffi.EXPORTED_SYMBOLS if "bodies" in s and s.startswith("egg_group_")]  # one handle only
    assert re.search(r"typedef struct\s*\{\s*double inv_mass, inv_inertia;[^}]*double ax, ay;[^}]*double drag, spin_drag;[^}]*\}\s*egg_collider_body;", text)
    B = _ffi.EggColliderBody
    assert C.sizeof(B) == 48 and [(n, getattr(B, n).offset) for n, _ in B._fields_] == [(n, 8 * k) for k, n in enumerate(FIELDS)]
    # the same shape as egg_set_collider_spin, and the device's record is the ABI's
    assert [type(a) for a in _ffi._SIGNATURES["egg_set_collider_bodies"][1][:2]] == [type(a) for a in _ffi._SIGNATURES["egg_set_collider_spin"][1][:2]]
    device_h = _read(CSRC, "eggsim_device.h")
    body = re.search(r"struct EggBody \{([^}]*)\}", device_h).group(1)
    assert re.findall(r"(\w+)[,;]", body) == FIELDS
    assert "sizeof(egg_collider_body) == 48 && sizeof(EggBody) == sizeof(egg_collider_body)" in _read(CSRC, "eggsim_host_colliders.hip")
    # the definition, where a C caller reads it
    for phrase in ("d = sums[k] - seen[k] (three int64), seen[k] = sums[k]", "Jx = ((double)dx / 2^20) / h", "vx = vx + Jx * inv_mass; vx = vx + h * ax",
                   "f = 1 - h * drag; if (!(f > 0)) f = 0", "u = 0.5 * (h * omega); den = 1 + u * u; c = (1 - u * u) / den; s = (u + u) / den",
                   "2 atan(h omega / 2)", "The kinematic colliders of the list advance too", "bit for bit at S = 1",
                   "egg_set_colliders resets the", "Refused while a step is in flight", "egg_rx_begin returns EGG_ERR_UNSUPPORTED while a handle holds a body",
                   "fails before anything is launched with EGG_ERR_UNSUPPORTED"):
        assert phrase in text, phrase


def test_the_kernel_exists_and_only_a_step_with_bodies_launches_it():
    kernels = _read(CSRC, "eggsim_relaxed.hip")
    host_h = _read(CSRC, "eggsim_host.h")
    host = _read(CSRC, "eggsim_host_relaxed.hip")
    assert 'extern "C" __global__ void __launch_bounds__(64) egg_rx_bodies_kernel(EggRxBodiesArgs A)' in kernels
    assert 'extern "C" __global__ void egg_rx_bodies_kernel(EggRxBodiesArgs A);' in host_h
    body = kernels[kernels.index("egg_rx_bodies_kernel(EggRxBodiesArgs A) {"):kernels.index("// ---- viscosity ----")]
    assert "atomic" not in body and "__shared__" not in body and "__shfl" not in body  # plain loads and stores, lane k = collider k
    assert "if (k >= A.count) return;" in body
    # one wave, one launch, from the bodies driver only; the driver is chosen by what the handle holds
    assert host.count("hipLaunchKernelGGL(egg_rx_bodies_kernel, dim3(1), dim3(64)") == 1
    assert host.count("launch_bodies(") == 2 and host.count("enqueue_substep(") == 2  # (each defined, and called from one place)
    assert "static bool bodies_act(const egg_handle *h) { return h->bodies_any && h->opt_loads && !h->colliders.empty(); }" in host
    step = host[host.index("int relaxed_step(egg_handle *h"):host.index("// a relaxed step whose launches are all enqueued")]
    assert step.index("if (h->bodies_any && !h->colliders.empty() && !h->opt_loads)") < step.index("prepare_step(")  # before anything is launched
    assert "egg_set_collider_loads" in step and "EGG_ERR_UNSUPPORTED" in step
    assert "const bool bodies = bodies_act(h);" in step and "enqueue_types(h, st, on, S, C, bodies);" in step
    assert step.index("if (bodies || (h->coupling_factor > 0.0 && on[0] && on[1])) {") < step.index("enqueue_types(h, st, on, S, C, bodies);")
    # the one driver: the sub-step body, the whole step of a set of types, and relaxed_step, which calls it
    driver = host[host.index("static int enqueue_substep(egg_handle *h, RelaxedStep st[2], const bool on[2], int sub, int C, bool bodies) {"):
                  host.index("// a relaxed step whose launches are all enqueued")]
    assert driver.index("static int enqueue_types(") < driver.index("int relaxed_step(egg_handle *h")
    substep = driver[:driver.index("static int enqueue_types(")]
    assert "if (rc != EGG_OK || !bodies) return rc;" in substep and substep.index("|| !bodies) return rc;") < substep.index("launch_bodies(st[lead])")
    assert "hipEventDisableTiming" in driver and "hipDeviceSynchronize" not in driver
    assert driver.count("hipStreamSynchronize") == 1  # (only for a handle without particles, after the last launch)
    # the commit reads the records back in place of advance_colliders; after a failed step the next one puts the host's
    # copies back: preparing the step marks the three tables the integrator rewrites, and only take_bodies clears the marks
    commit = host[host.index("void relaxed_commit("):]
    assert "if (h->bodies_step) take_bodies(h);" in commit
    assert "if (h->bodies_step) return;" in host[host.index("static void advance_colliders("):host.index("// Collider bodies at the commit")]
    prepare = host[host.index("static int prepare_bodies(egg_handle *h"):host.index("// Per step with contacts acting")]
    assert "h->collider_dirty |= kDirtyList | kDirtyMotions | kDirtySpins;" in prepare
    assert host.count("h->collider_dirty &= ~") == 1
    assert "h->collider_dirty &= ~(kDirtyList | kDirtyMotions | kDirtySpins);" in host[host.index("static void take_bodies("):host.index("// Collider contacts at the commit")]
    finish = host[host.index("static int relaxed_finish(egg_handle *h, RelaxedStep st[2], int S, int C) {"):host.index("static void advance_colliders(")]
    assert "collider_dirty" not in finish and "hipMemcpy" not in finish
    step = host[host.index("int prepare_step(egg_handle *h"):host.index("int prepare_type(RelaxedStep &st")]
    assert step.index("sync_collider_records(h)") < step.index("prepare_bodies(h, sub_delta)")
    assert "st.L.loads = st.L.colliders && h->opt_loads;" in host  # (how loads are derived has not changed)


def test_the_refusals_stand_in_the_sources():
    abi = _read(CSRC, "eggsim_host_colliders.hip")
    setter = abi[abi.index("int egg_set_collider_bodies("):abi.index("int egg_get_collider_bodies(")]
    # the in-flight refusal and the "n = %d without records" check stand in the preface every setter of records opens with
    preface = abi[abi.index("int check_records(egg_handle *h, const char *name"):abi.index("// The getters' answer")]
    assert "REJECT_IN_FLIGHT(h, name);" in preface and '"%s: n = %d without records", name' in preface
    assert 'check_records(h, "egg_set_collider_bodies", n, b);\n    if (rc != EGG_OK) return rc;' in setter
    assert setter.index("h->bodies.swap(list);") > max(setter.index(m) for m in ("is negative or not finite", "is not finite", "check_records("))
    assert setter.count("collider %d:") == 5 and "o.inv_mass = o.inv_mass + 0.0;" in setter
    assert "hipMemcpy" not in setter  # (a step in which bodies act uploads what it runs on)
    lists = abi[abi.index("int egg_set_colliders("):abi.index("int egg_get_colliders(")]
    assert "h->bodies.clear();" in lists and "h->bodies_any = false;" in lists
    for name in ("egg_set_collider_motion", "egg_set_collider_spin", "egg_set_collider_surfaces"):  # these leave the bodies alone
        other = abi[abi.index("int %s(" % name):]
        assert "bodies" not in other[:other.index("\nint egg_get_")], name
    assert "collider bodies run on a single handle only" in _read(CSRC, "eggsim_host_relaxed_group.hip")
    wire = _read(CSRC, "eggsim_host_relaxed_wire.hip")
    begin = wire[wire.index("int egg_rx_begin("):]
    assert "if (h->bodies_any)" in begin and "egg_rx_begin: collider bodies run on a single handle only" in begin


def test_python_classes_and_lua_have_the_methods():
    from egg_fluid_simulation_amd import SimulationGroup, SimulationHandler
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler
    for cls in (SimulationHandler, SimulationGroup, ShardedSimulationHandler):
        for name in ("set_collider_bodies", "get_collider_bodies"):
            assert callable(getattr(cls, name)), (cls.__name__, name)
        assert list(inspect.signature(cls.set_collider_bodies).parameters) == ["self", "bodies"]
    for cls in (SimulationGroup, ShardedSimulationHandler):  # the limit: their setter never reaches the library
        src = inspect.getsource(cls.set_collider_bodies)
        assert "_BODIES_LIMIT" in src and "_c(" not in src
        assert "single SimulationHandler only" in cls._BODIES_LIMIT
    assert '_c("set_collider_bodies")' in inspect.getsource(SimulationHandler.set_collider_bodies)
    lua = _read(ROOT, "egg_fluid_simulation_amd", "lua", "egg_fluid_simulation", "simulation_handler.lua")
    for name in ("set_collider_bodies", "get_collider_bodies"):
        assert "function SimulationHandler:%s(" % name in lua, name
        assert re.search(r"int egg_%s\(" % name, lua), name
    assert "typedef struct { double inv_mass, inv_inertia, ax, ay, drag, spin_drag; } egg_collider_body;" in lua


def test_the_wrapper_checks_before_any_device_call():
    from egg_fluid_simulation_amd import EggError, SimulationHandler
    from egg_fluid_simulation_amd.group import SimulationGroup
    c = SimulationHandler._c_bodies
    n, arr = c([None, (1, 2), (1, 2, -3, 4), (0.5, 0.25, 1, -1, 3, 4)])
    assert n == 4 and [[getattr(arr[k], f) for f in FIELDS] for k in range(4)] == \
        [[0.0] * 6, [1.0, 2.0, 0.0, 0.0, 0.0, 0.0], [1.0, 2.0, -3.0, 4.0, 0.0, 0.0], [0.5, 0.25, 1.0, -1.0, 3.0, 4.0]]
    assert c([])[0] == 0
    for bad, match in (([(1,)], "collider body 0: expected None or"), ([None, (1, 2, 3)], "collider body 1: expected"), ([None, "ab"], "collider body 1"),
                       ([(-1, 0)], "collider body 0: inv_mass -1.0 is negative"), ([None, (0, -2.0)], "collider body 1: inv_inertia -2.0 is negative"),
                       ([(1, 0, float("nan"), 0)], "collider body 0: ax nan is not finite"), ([(1, 0, 0, 0, -0.5, 0)], "collider body 0: drag -0.5 is negative"),
                       ([(1, 0, 0, 0, 0, float("inf"))], "collider body 0: spin_drag inf is not finite")):
        with pytest.raises(EggError, match=match):
            c(bad)
    # where several handles share a step: a list without a body is accepted and changes nothing, a body names the limit
    # (the shared method needs nothing of the instance but its limit text)
    class Shared:
        _BODIES_LIMIT = SimulationGroup._BODIES_LIMIT
        _c_bodies = staticmethod(c)
    assert SimulationGroup.set_collider_bodies(Shared(), [None, (0, 0, 5, 5)]) is None
    for body in ((1, 0), (0, 1)):
        with pytest.raises(EggError, match="single SimulationHandler only"):
            SimulationGroup.set_collider_bodies(Shared(), [None, body])
    with pytest.raises(EggError, match="collider body 0: drag"):  # (after the checks of the records)
        SimulationGroup.set_collider_bodies(Shared(), [(1, 0, 0, 0, -1, 0)])


def test_the_documents_describe_the_rule():
    design = _read(ROOT, "DESIGN.md")
    part = design[design.index("#### Collider bodies"):design.index("#### Forces")]
    for phrase in ("egg_rx_bodies_kernel", "enqueue_substep", "Cayley", "2 atan(h omega / 2)", "seen[k] = sums[k]", "body_ready", "body_done",
                   "The plate experiment", "explicit", "bit-equal at `S = 1`", "profiles/r24_bodies.md", "ONE handle only"):
        assert phrase in part, phrase
    limits = design[design.index("## 7. Limits"):]
    assert "collider bodies (`egg_set_collider_bodies`)" in limits and "no\n    collider the device integrates from its own load" not in limits
    assert "set_collider_bodies" in _read(ROOT, "README.md")
    integration = _read(ROOT, "INTEGRATION.md")
    assert "set_collider_bodies" in integration and "egg_get_collider_bodies" in integration
    assert os.path.exists(os.path.join(ROOT, "profiles", "r24_bodies.md")) and os.path.exists(os.path.join(ROOT, "scripts", "gpu_bodies_bench.py"))
