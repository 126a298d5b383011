"""The surface of collider contacts (egg_set_collider_contacts, DESIGN.md section 2.7 "Collider contacts") as far as it can be
checked without a device: the three entry points and the 16-byte struct in the header and in the ctypes binding, the methods
on all three Python classes and in the Lua wrapper, the wrapper's own refusals, the limits of the group and sharded classes,
the kernel and its launch, the refusals where the sources state them, and the documents."""
import ctypes as C
import inspect
import os
import re

import pytest

from conftest import ROOT
from test_cohesion_surface import _header

CSRC = os.path.join(ROOT, "egg_fluid_simulation_amd", "csrc")
PROTOS = {
    "egg_set_collider_contacts": "int egg_set_collider_contacts(egg_handle *h, int32_t n, const egg_collider_contact *c, int32_t iterations);",
    "egg_get_collider_contacts": "int egg_get_collider_contacts(const egg_handle *h, int32_t cap, egg_collider_contact *out, int32_t *n, int32_t *iterations);",
    "egg_get_collider_contact_solves": "int egg_get_collider_contact_solves(egg_handle *h, int64_t *solves);",
}
METHODS = ("set_collider_contacts", "get_collider_contacts", "collider_contact_solves")


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
    assert not [s for s in _ffi.EXPORTED_SYMBOLS if "contact" in s and s.startswith("egg_group_")]  # one handle only
    assert re.search(r"typedef struct\s*\{\s*double restitution;[^}]*int32_t on;[^}]*int32_t reserved;[^}]*\}\s*egg_collider_contact;", text)
    K = _ffi.EggColliderContact
    assert C.sizeof(K) == 16 and [(n, getattr(K, n).offset) for n, _ in K._fields_] == [("restitution", 0), ("on", 8), ("reserved", 12)]
    device_h = _read(CSRC, "eggsim_device.h")
    record = re.search(r"struct EggContact \{([^}]*)\}", device_h).group(1)
    assert re.findall(r"(\w+)[,;]", record) == ["restitution", "on", "reserved"]
    assert "sizeof(egg_collider_contact) == 16 && sizeof(EggContact) == sizeof(egg_collider_contact)" in _read(CSRC, "eggsim_host_colliders.hip")
    # the rule, its place in the sub-step and the limits, where a C caller reads them
    for phrase in ("behind step 4 of collider bodies", "exactly when bodies act (above) and some record is on",
                   "launches exactly the kernels it launches today, with the same arguments", "((ma + ia) + mb) + ib > 0",
                   "DIRS[(b - a) & 7]", "g = (Rc - R) - d", "the segment's left normal", "with a the smaller index",
                   "w > 0 and g + h * vn < 0", "q2 = m * m - s * s;  q2 < 0: q2 = 0;  g = sqrt(q2) - d", "e = max(ea, eb);  t1 = (-g) / h;  t2 = -(e * vn);  target = t1 > t2 ? t1 : t2;  lam = (target - vn) / w",
                   "in ascending", "vx = vx + (sx * mk) / count", "omega = omega + (sz * ik) / count", "recomputes its turn (c, s)",
                   "tests/contact_model.py is the definition", "no friction between bodies", "no pair without a disc", "stacks are soft",
                   "never moved", "ONE handle only", "egg_rx_begin returns EGG_ERR_UNSUPPORTED", "refuses exact order while one is set",
                   "or 0 for the default of 4", "clears the records", "Refused\n * while a step is in flight", "a failed step adds\n * nothing"):
        assert phrase in text, phrase
    assert "No body-body contact" not in text


def test_the_kernel_exists_and_only_a_step_with_contacts_launches_it():
    kernel = _read(CSRC, "eggsim_relaxed_contacts.hip")
    host_h = _read(CSRC, "eggsim_host.h")
    host = _read(CSRC, "eggsim_host_relaxed.hip")
    makefile = _read(CSRC, "Makefile")
    assert 'extern "C" __global__ void __launch_bounds__(64) egg_rx_contacts_kernel(EggRxContactsArgs A)' in kernel
    assert 'extern "C" __global__ void egg_rx_contacts_kernel(EggRxContactsArgs A);' in host_h
    assert "struct EggRxContactsArgs {" in _read(CSRC, "eggsim_device.h")
    assert makefile.count("eggsim_relaxed_contacts.hip") == 2 and "-ffp-contract=off" in makefile  # built, and listed for resource-usage
    assert "egg_rx_contacts_kernel" not in _read(CSRC, "eggsim_relaxed.hip")  # (a translation unit of its own)
    assert "atomic" not in kernel.lower().replace("no atomics", "") and "__shfl" not in kernel and "fma(" not in kernel
    assert "__shared__" in kernel and kernel.count("__syncthreads();") == 3
    assert "return;" not in kernel[kernel.index("egg_rx_contacts_kernel(EggRxContactsArgs A) {"):]  # every lane meets the barriers
    # one wave, one launch, directly behind the integrator, from the bodies driver only
    assert host.count("hipLaunchKernelGGL(egg_rx_contacts_kernel, dim3(1), dim3(64)") == 1
    assert host.count("launch_contacts(") == 2  # (defined, called)
    assert "static bool contacts_act(const egg_handle *h) { return bodies_act(h) && h->contacts_any; }" in host
    driver = host[host.index("static int enqueue_substep(egg_handle *h, RelaxedStep st[2], const bool on[2], int sub, int C, bool bodies) {"):
                  host.index("// a relaxed step whose launches are all enqueued")]
    behind = driver[driver.index("rc = launch_bodies(st[lead]);"):driver.index("hipEventRecord(h->body_done")]
    assert "if (rc == EGG_OK && h->contacts_step) rc = launch_contacts(st[lead]);" in behind and "hipStreamWaitEvent" not in behind
    assert "hipEventCreate" not in host[host.index("static int launch_contacts("):host.index("// Sub-step `sub` of the types in `on`")]
    # prepare_step uploads the records, the commit adds the counter, a failed step reads nothing
    prepare = host[host.index("int prepare_step(egg_handle *h"):host.index("int prepare_type(RelaxedStep &st")]
    assert "contacts_act(h) ? prepare_contacts(h) : rc" in prepare
    commit = host[host.index("void relaxed_commit("):]
    assert "if (h->contacts_step) take_contacts(h);" in commit
    assert "h->contact_solves += (int64_t)fires;" in host
    finish = host[host.index("static int relaxed_finish(egg_handle *h, RelaxedStep st[2], int S, int C) {"):host.index("static void advance_colliders(")]
    assert "h->bodies_step = h->contacts_step = false;" in finish


def test_the_refusals_stand_in_the_sources():
    abi = _read(CSRC, "eggsim_host_colliders.hip")
    setter = abi[abi.index("int egg_set_collider_contacts("):abi.index("int egg_get_collider_contacts(")]
    # the in-flight refusal and the "n = %d without records" check stand in the preface every setter of records opens with
    preface = abi[abi.index("int check_records(egg_handle *h, const char *name"):abi.index("// The getters' answer")]
    assert "REJECT_IN_FLIGHT(h, name);" in preface and '"%s: n = %d without records", name' in preface
    assert 'check_records(h, "egg_set_collider_contacts", n, c);\n    if (rc != EGG_OK) return rc;' in setter
    assert setter.index("h->contacts.swap(list);") > max(setter.index(m) for m in ("lies outside [0, 1]", "is not 0 or 1", "reserved = %d is not 0",
                                                                                      "check_records(", "iterations (1 .. 16", "need relaxed order"))
    assert "EGG_ERR_UNSUPPORTED" in setter and "iterations == 0 ? 4 : iterations" in setter
    assert "hipMemcpy" not in setter  # (a step in which contacts act uploads what it runs on)
    lists = abi[abi.index("int egg_set_colliders("):abi.index("int egg_get_colliders(")]
    assert "h->contacts.clear();" in lists and "h->contacts_any = false;" in lists
    assert lists.index("h->bodies.clear();") < lists.index("h->contacts.clear();")
    core = _read(CSRC, "eggsim_host_abi.hip")
    order = core[core.index("case EGG_OPT_SOLVER_ORDER:"):core.index("case EGG_OPT_RELAXATION:")]
    assert "value == EGG_SOLVER_EXACT && h->contacts_any" in order and "exact order has no collider contacts" in order
    for name in ("egg_set_collider_motion", "egg_set_collider_spin", "egg_set_collider_surfaces", "egg_set_collider_bodies"):  # these leave the records alone
        other = abi[abi.index("int %s(" % name):]
        assert "contacts" not in other[:other.index("\nint egg_get_")], name
    # bodies' wording, bodies' return code and bodies' place in the code
    group = _read(CSRC, "eggsim_host_relaxed_group.hip")
    assert "collider contacts run on a single handle only" in group
    assert group.index("collider bodies run on a single handle only") < group.index("collider contacts run on a single handle only") < group.index("same_pivots")
    wire = _read(CSRC, "eggsim_host_relaxed_wire.hip")
    begin = wire[wire.index("int egg_rx_begin("):]
    assert "if (h->contacts_any)" in begin and "egg_rx_begin: collider contacts run on a single handle only" in begin
    assert begin.index("if (h->bodies_any)") < begin.index("if (h->contacts_any)") < begin.index("WireStep &W = wire_of(h);")


def test_python_classes_and_lua_have_the_methods():
    from egg_fluid_simulation_amd import SimulationGroup, SimulationHandler
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler
    for cls in (SimulationHandler, SimulationGroup, ShardedSimulationHandler):
        for name in METHODS:
            assert callable(getattr(cls, name)), (cls.__name__, name)
        assert list(inspect.signature(cls.set_collider_contacts).parameters) == ["self", "contacts", "iterations"]
        assert inspect.signature(cls.set_collider_contacts).parameters["iterations"].default == 4
    for cls in (SimulationGroup, ShardedSimulationHandler):  # the limit: their setter never reaches the library
        src = inspect.getsource(cls.set_collider_contacts)
        assert "_CONTACTS_LIMIT" in src and "_c(" not in src
        assert "single SimulationHandler only" in cls._CONTACTS_LIMIT
        assert "_c(" not in inspect.getsource(cls.collider_contact_solves)
    for name in METHODS:
        assert '_c("%s")' % name.replace("collider_contact_solves", "get_collider_contact_solves") in inspect.getsource(getattr(SimulationHandler, name))
    lua = _read(ROOT, "egg_fluid_simulation_amd", "lua", "egg_fluid_simulation", "simulation_handler.lua")
    for name in METHODS:
        assert "function SimulationHandler:%s(" % name in lua, name
    for name in PROTOS:
        assert re.search(r"int %s\(" % name, lua), name
    assert "typedef struct { double restitution; int32_t on; int32_t reserved; } egg_collider_contact;" in lua


def test_the_wrapper_checks_before_any_device_call():
    from egg_fluid_simulation_amd import EggError, SimulationHandler
    from egg_fluid_simulation_amd.group import SimulationGroup
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler
    c = SimulationHandler._c_contacts
    n, arr, iterations = c([None, 0.5, True, 1, 0.0])
    assert (n, iterations) == (5, 4)
    assert [(arr[k].restitution, arr[k].on, arr[k].reserved) for k in range(5)] == [(0.0, 0, 0), (0.5, 1, 0), (0.0, 1, 0), (1.0, 1, 0), (0.0, 1, 0)]
    assert c([])[0] == 0 and c([], 0)[2] == 0 and c([None], 16)[2] == 16
    for bad, match in (([1.5], "collider contact 0: the restitution 1.5 lies outside"), ([None, -0.25], "collider contact 1: the restitution -0.25"),
                       ([float("nan")], "collider contact 0: the restitution nan"), ([None, "ab"], "collider contact 1: expected None, True or a restitution"),
                       ([False], "collider contact 0: expected None"), ([(0.5, 1)], "collider contact 0: expected None")):
        with pytest.raises(EggError, match=match):
            c(bad)
    for iterations in (-1, 17, 2.0, True, None):
        with pytest.raises(EggError, match="collider contacts: iterations"):
            c([None], iterations)
    # a handle that was never created: the checks raise before anything is asked of the library
    for cls in (SimulationHandler, SimulationGroup, ShardedSimulationHandler):
        bare = cls.__new__(cls)
        with pytest.raises(EggError, match="collider contact 0: the restitution 2.0"):
            bare.set_collider_contacts([2.0])
        with pytest.raises(EggError, match="collider contacts: iterations"):
            bare.set_collider_contacts([None], 40)
    # where several handles share a step: a list with nothing on is accepted and changes nothing, a contact names the limit
    for cls in (SimulationGroup, ShardedSimulationHandler):
        bare = cls.__new__(cls)
        assert bare.set_collider_contacts([None, None]) is None and bare.set_collider_contacts([]) is None
        assert bare.collider_contact_solves() == 0
        for on in (True, 0.0, 0.5):
            with pytest.raises(EggError, match="single SimulationHandler only"):
                bare.set_collider_contacts([None, on])
        with pytest.raises(EggError, match="collider contact 1: the restitution"):  # (after the checks of the records)
            bare.set_collider_contacts([True, 3.0])


def test_the_documents_describe_the_rule():
    design = _read(ROOT, "DESIGN.md")
    part = design[design.index("#### Collider contacts"):design.index("#### Collider styles")]
    assert design.index("#### Collider bodies") < design.index("#### Collider contacts")
    for phrase in ("egg_rx_contacts_kernel", "eggsim_relaxed_contacts.hip", "tests/contact_model.py", "speculative", "Jacobi", "LDS", "broadcast",
                   "body_ready", "body_done", "no friction between bodies", "no pair without a disc", "stacks are soft", "ONE handle only",
                   "profiles/r26_contacts.md", "1, 4 and 16 iterations", "container"):
        assert phrase in part, phrase
    limits = design[design.index("## 7. Limits"):]
    assert "collider contacts (`egg_set_collider_contacts`)" in limits and "there is no body-body contact" not in limits
    readme = _read(ROOT, "README.md")
    assert "set_collider_contacts" in readme and "158 entry points -- 101 on one device" in readme
    integration = _read(ROOT, "INTEGRATION.md")
    assert "set_collider_contacts" in integration and "egg_get_collider_contact_solves" in integration and "158 entry points" in integration
    assert os.path.exists(os.path.join(ROOT, "profiles", "r26_contacts.md"))
