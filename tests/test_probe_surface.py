"""The surface of the probes (egg_probe) as far as it can be checked without a device: the two entry
points, the constants and the two structs in the header and in the ctypes binding, field offsets included, the three methods
on all three Python classes with equal parameter lists, the wrappers' own argument checks on a device-less instance, the
Lua methods as text, the kernels and that no step unit names them, and the documents."""
import ctypes as C
import inspect
import math
import os
import re

import pytest

from conftest import ROOT
from test_abi import _prototypes

CSRC = os.path.join(ROOT, "egg_fluid_simulation_amd", "csrc")
PROTOS = {
    "egg_probe": "int egg_probe(egg_handle *h, int32_t n, const egg_probe_query *probes, "
                 "egg_probe_hit *hits /* [n][2]: [0] white, [1] yolk */);",
    "egg_group_probe": "int egg_group_probe(egg_group *g, int32_t n, const egg_probe_query *probes, egg_probe_hit *hits /* [n][2] */);",
}
METHODS = {"probe": ["self", "probes"], "pick": ["self", "x", "y", "reach", "types"],
           "raycast": ["self", "x0", "y0", "x1", "y1", "pad", "types"]}
KERNELS = {"egg_probe_scan_kernel": "EggProbeArgs", "egg_probe_finish_kernel": "EggProbeFinishArgs"}
STEP_UNITS = ("eggsim_step.hip", "eggsim_packed.hip", "eggsim_relaxed.hip", "eggsim_relaxed_contacts.hip", "eggsim_relaxed_wire.hip",
              "eggsim_host_step.hip", "eggsim_host_relaxed.hip", "eggsim_host_relaxed_group.hip", "eggsim_host_relaxed_wire.hip",
              "eggsim_sensors.hip")


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_header_declares_the_entry_points_the_constants_and_the_structs():
    from egg_fluid_simulation_amd import _ffi
    text = _read(ROOT, "include", "eggsim.h")
    for name, proto in PROTOS.items():
        assert proto in text, name
        assert name in _ffi._SIGNATURES and name in _ffi.EXPORTED_SYMBOLS, name
        assert len(_ffi._SIGNATURES[name][1]) == 4, name
    assert _ffi._SIGNATURES["egg_probe"][1] == _ffi._SIGNATURES["egg_group_probe"][1]  # (the group twin has its handle twin's parameters)
    assert re.search(r"typedef struct \{ int32_t kind; int32_t type_mask; double p\[5\]; \} egg_probe_query; +/\* 48 bytes \*/", text)
    assert re.search(r"typedef struct \{ int64_t id, key; int32_t index, found; double score, x, y, radius; \} egg_probe_hit; +/\* 56 bytes \*/", text)
    assert "#define EGG_MAX_PROBES 64" in text and "enum { EGG_PROBE_POINT = 0, EGG_PROBE_RAY = 1 };" in text
    Q, H = _ffi.EggProbeQuery, _ffi.EggProbeHit
    assert C.sizeof(Q) == 48 and [(n, getattr(Q, n).offset) for n, _ in Q._fields_] == [("kind", 0), ("type_mask", 4), ("p", 8)]
    assert C.sizeof(H) == 56 and [(n, getattr(H, n).offset) for n, _ in H._fields_] == [
        ("id", 0), ("key", 8), ("index", 16), ("found", 20), ("score", 24), ("x", 32), ("y", 40), ("radius", 48)]
    assert _ffi.MAX_PROBES == 64 and (_ffi.PROBE_POINT, _ffi.PROBE_RAY) == (0, 1) and _ffi.PROBE_KINDS == ("point", "ray")
    assert [len(p) for p in _ffi.PROBE_PARAMS] == [3, 5] and _ffi.PROBE_DEFAULTS == ((math.inf,), (0.0,))
    assert _ffi.PROBE_TYPES == {"white": 1, "yolk": 2, "both": 3}
    # the rule, where a C caller reads it
    for phrase in ("d2 = dx dx + dy dy; candidate iff d2 <= reach reach && r == r", "score = d2", "R = r + pad",
                   "c = (fx fx + fy fy) - R R", "If c <= 0.0 the ray starts in or on the disc", "a miss unless b < 0.0",
                   "q = b b - l2 c; a miss unless q >= 0.0; t = (-b - sqrt(q)) / l2; a miss unless t <= 1.0", "(x0 + t ex, y0 + t ey)",
                   "t is never negative", "Parameters a kind does not use are ignored", "a NaN position or radius is a candidate for nothing",
                   "the smallest score by < on doubles", "the smallest batch key", "the smallest index inside the batch's run",
                   "A call is STATELESS", "checks everything before it launches anything",
                   "hits untouched", "n == 0 succeeds and writes nothing", "launches nothing", "contributes no work",
                   "Refused while a step\n * is in flight", "Nothing is cached: every call measures", "no k-nearest",
                   "no probe that rides on a collider", "colliders\n * themselves are not hit", "launches exactly the kernels it launches without them",
                   "those of egg_get_stats included", "whichever device owns tied batches", "A failure on any handle writes\n * nothing"):
        assert phrase in text, phrase
    assert all(name in _prototypes(text) for name in PROTOS)


def test_a_c_compiler_lays_the_structs_out_as_ctypes_does(tmp_path):
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    src = tmp_path / "probe_layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "eggsim.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(egg_probe_query), offsetof(egg_probe_query, p), '
                   'sizeof(egg_probe_hit), offsetof(egg_probe_hit, index), offsetof(egg_probe_hit, found), offsetof(egg_probe_hit, score), '
                   'offsetof(egg_probe_hit, radius), (int)EGG_PROBE_RAY, (int)EGG_MAX_PROBES); return 0; }\n')
    exe = str(tmp_path / "probe_layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)],
                   check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["48", "8", "56", "16", "20", "24", "48", "1", "64"]


def test_the_kernels_exist_and_no_step_unit_names_them():
    kernels = _read(CSRC, "eggsim_probes.hip")
    host_h = _read(CSRC, "eggsim_host.h")
    host = _read(CSRC, "eggsim_host_probes.hip")
    device_h = _read(CSRC, "eggsim_device.h")
    for name, args in KERNELS.items():
        assert re.search(r'extern "C" __global__ void __launch_bounds__\(\w+\) %s\(%s A\)' % (name, args), kernels), name
        assert 'extern "C" __global__ void %s(%s A);' % (name, args) in host_h, name
        assert "hipLaunchKernelGGL(%s," % name in host, name
        assert "struct %s {" % args in device_h, name
    makefile = _read(CSRC, "Makefile")
    assert makefile.count("eggsim_probes.hip") == 2 and "eggsim_host_probes.hip" in makefile and "-ffp-contract=off" in makefile
    # a wave per workgroup, the ballot of what beats the running best, the reduction behind the wave-uniform branch, the tie
    # rule inside it; no LDS, no atomics and no inline assembly in the scan
    body = kernels[kernels.index("void pb_scan("):kernels.index('extern "C"')]
    assert "if (__ballot(cand) == 0ull) continue;" in body and "pb_wave_min(" in body and "__ffsll(" in body and "s < cur" in body
    assert body.index("if (__ballot(cand) == 0ull) continue;") < body.index("pb_wave_min(")
    assert "__shared__" not in body and "atomic" not in body and "asm" not in kernels
    assert "__shfl_xor(" in kernels and "blockIdx.y" in kernels[kernels.index("egg_probe_finish_kernel"):]  # (parallel over (probe, type))
    assert "#define EGG_PB_MAX_PROBES 64" in device_h and "EggProbe probes[EGG_PB_MAX_PROBES];" in device_h
    assert "sizeof(egg_probe_query) == 48" in host and "sizeof(egg_probe_hit) == 56" in host and "sizeof(EggProbeArgs) <= 4096" in host
    assert "EGG_MAX_PROBES == EGG_PB_MAX_PROBES" in host and "EGG_PROBE_RAY == EGG_PB_RAY" in host
    # the unit table is the shared builder's, and its state is this feature's own
    scan = _read(CSRC, "eggsim_host_scan.hip")
    assert re.search(r"struct ProbeState \{\n\s*UnitTable units;", host) and 'S.units.refresh(h, "egg_probe", cover, false)' in host
    refresh = scan[scan.index("int UnitTable::refresh("):]
    refresh = refresh[:refresh.index("\n}\n")]
    key = "if (cover == want && gen[0] == h->sys[0].atoms_gen && gen[1] == h->sys[1].atoms_gen) return EGG_OK;"
    assert key in refresh and "gen[0] = gen[1] = ~0ull;" in refresh and "push_units(a, w, units);" in refresh
    assert refresh.index(key) < refresh.index("gen[0] = gen[1] = ~0ull;") < refresh.index("push_units(a, w,")  # invalidated, then rebuilt
    assert "std::shared_ptr<egghost::ProbeState> probe_state;" in host_h
    # nothing of a step knows about probes: no step kernel, no step driver, no commit -- and no unit but the probes' own, the
    # two shared headers and the group
    for unit in set(os.listdir(CSRC)) | set(STEP_UNITS):
        if unit.endswith((".hip", ".cpp", ".h")) and unit not in ("eggsim_probes.hip", "eggsim_host_probes.hip", "eggsim_host.h",
                                                                   "eggsim_device.h", "eggsim_group.cpp"):
            text = _read(CSRC, unit)
            assert "egg_probe" not in text and "EggProbe" not in text and "probe_state" not in text and "ProbeState" not in text, unit
    # the refusals, where the source states them: everything is checked before the first launch and before hits is written
    assert 'REJECT_IN_FLIGHT(h, "egg_probe");' in host and "opt_solver_order" not in host  # (either order)
    last_check = max(m.start() for m in re.finditer(r'return fail\(h, EGG_ERR_INVALID_ARGUMENT', host))
    assert last_check < host.index("hipLaunchKernelGGL(") and last_check < host.index("memcpy(hits,")
    assert host.count("memcpy(hits,") == 1 and "kernel_launches" not in host.replace("stats.kernel_launches counts what steps", "")
    group = _read(CSRC, "eggsim_group.cpp")
    twin = group[group.index("int egg_group_probe("):]
    twin = twin[:twin.index("\n}\n")]
    assert "egg_probe(g->h[k], n, probes," in twin and "a.key < b.key" in twin and "a.index < b.index" in twin and "b.id = b.key" in twin
    assert twin.index("return gfail(") < twin.index("memcpy(hits,")  # (a failure on any handle writes nothing)


def test_python_classes_have_the_methods_with_equal_parameter_lists():
    from egg_fluid_simulation_amd import SimulationGroup, SimulationHandler
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler
    from egg_fluid_simulation_amd.simulation_handler import ProbeHit
    for cls in (SimulationHandler, SimulationGroup, ShardedSimulationHandler):
        for name, params in METHODS.items():
            assert list(inspect.signature(getattr(cls, name)).parameters) == params, (cls.__name__, name)
        assert inspect.signature(cls.pick).parameters["reach"].default == math.inf and inspect.signature(cls.pick).parameters["types"].default == 3
        assert inspect.signature(cls.raycast).parameters["pad"].default == 0.0 and inspect.signature(cls.raycast).parameters["types"].default == 3
    assert ProbeHit._fields == ("id", "index", "score", "x", "y", "radius")
    # a group calls its own entry point; a sharded handler asks its local handle, gathers once and selects by (score, key, index)
    assert SimulationGroup._PREFIX == "egg_group_" and SimulationGroup.probe is SimulationHandler.probe
    src = inspect.getsource(ShardedSimulationHandler.probe)
    assert "self.local._probe_table(" in src and src.count("all_gather(") == 1 and "all_reduce" not in src and "int64" in src
    assert "(key, index) < found[1:3]" in src and "score < found[0]" in src
    assert ShardedSimulationHandler.pick is SimulationHandler.pick and ShardedSimulationHandler.raycast is SimulationHandler.raycast


def test_the_wrappers_check_what_only_the_host_can():
    from egg_fluid_simulation_amd import EggError, SimulationGroup, SimulationHandler, _ffi
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler
    from egg_fluid_simulation_amd.simulation_handler import ProbeHit
    for cls in (SimulationHandler, SimulationGroup, ShardedSimulationHandler):
        h = cls.__new__(cls)  # no device: the checks below come before any call into the library
        if cls is ShardedSimulationHandler:
            h.local = SimulationHandler.__new__(SimulationHandler)
        for bad, text in (([("ring", 0, 0, 1)], "probe 0: kind must be one of point, ray"),
                          ([("point", 0, 0), ("point", 0)], r"probe 1 \(point\): expected \('point', x, y\[, reach\[, types\]\]\)"),
                          ([("ray", 0, 0, 1)], r"probe 0 \(ray\): expected \('ray', x0, y0, x1, y1\[, pad\[, types\]\]\)"),
                          ([("ray", 0, 0, 1, 1, 0, "both", 3)], r"probe 0 \(ray\): expected"),
                          ([("point", 0, 0, 1, "none")], "probe 0: types must be"), ([("point", 0, 0, 1, 4)], "probe 0: types must be"),
                          ([("point", 0, 0, 1, True)], "probe 0: types must be"),
                          ([("ray", 0, 0, 1, "x", 0, "both")], r"probe 0 \(ray\): the parameters must be numbers"),
                          ([None], "probe 0: kind must be one of"), ([("point", 0, 0)] * 65, "a call takes 0 .. 64 probes")):
            with pytest.raises(EggError, match=text):
                h.probe(bad)
        with pytest.raises(EggError, match="probe 0: types must be"):
            h.pick(0.0, 0.0, 1.0, "none")
        with pytest.raises(EggError, match=r"probe 0 \(ray\): the parameters must be numbers"):
            h.raycast(0.0, 0.0, 1.0, None)
    n, arr = SimulationHandler._c_probes([("point", 1, 2), ("point", 1, 2, 3.5, "yolk"), ("point", 1, 2, "white"), ("ray", 1, 2, 3, 4),
                                          ("ray", 1, 2, 3, 4, 0.5), ("ray", 1, 2, 3, 4, 0.5, 1), ["ray", 1, 2, 3, 4, "yolk"]])
    assert n == 7 and [q.kind for q in arr[:7]] == [0, 0, 0, 1, 1, 1, 1] and [q.type_mask for q in arr[:7]] == [3, 2, 1, 3, 3, 1, 2]
    assert list(arr[0].p) == [1.0, 2.0, math.inf, 0.0, 0.0] and list(arr[1].p) == [1.0, 2.0, 3.5, 0.0, 0.0] and list(arr[2].p)[2] == math.inf
    assert list(arr[3].p) == [1.0, 2.0, 3.0, 4.0, 0.0] and list(arr[4].p) == list(arr[5].p) == [1.0, 2.0, 3.0, 4.0, 0.5] and list(arr[6].p)[4] == 0.0
    assert SimulationHandler._c_probes([])[0] == 0
    # hits as records, and the first of a pair: the lower score, an exact tie to white
    a, b = (2.0, 5, 3, 7, 1.0, 1.5, 4.0), (2.0, 1, 0, 9, 0.0, 0.5, 4.0)  # (score, key, index, id, x, y, radius)
    (white, yolk), (none, _) = SimulationHandler._probe_hits([(a, b), (None, b)])
    assert white == ProbeHit(7, 3, 2.0, 1.0, 1.5, 4.0) and yolk == ProbeHit(9, 0, 2.0, 0.0, 0.5, 4.0) and none is None
    assert SimulationHandler._probe_first((white, yolk)) == ("white", white) and SimulationHandler._probe_first((None, yolk)) == ("yolk", yolk)
    assert SimulationHandler._probe_first((white, yolk._replace(score=1.5)))[0] == "yolk" and SimulationHandler._probe_first((None, None)) is None
    assert _ffi.PROBE_CODES == {"point": 0, "ray": 1}


def test_lua_has_the_methods_and_the_header_prototypes():
    lua = _read(ROOT, "egg_fluid_simulation_amd", "lua", "egg_fluid_simulation", "simulation_handler.lua")
    for name in METHODS:
        assert "function SimulationHandler:%s(" % name in lua, name
    cdef = _prototypes(re.search(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S).group(1))
    header = _prototypes(_read(ROOT, "include", "eggsim.h"))
    assert cdef["egg_probe"] == header["egg_probe"] and "lib.egg_probe(self._h, n, arr, hits)" in lua
    assert "typedef struct { int32_t kind; int32_t type_mask; double p[5]; } egg_probe_query;" in lua
    assert "typedef struct { int64_t id, key; int32_t index, found; double score, x, y, radius; } egg_probe_hit;" in lua
    assert "_probe_defaults = { [0] = math.huge, 0 }" in lua and "_max_probes = 64" in lua
    assert "not (one.yolk.score < one.white.score)" in lua  # (an exact tie goes to white)
    assert "x0 + hit.score * (x1 - x0), y0 + hit.score * (y1 - y0)" in lua


def test_the_documents_describe_the_rule_and_the_limits():
    design = _read(ROOT, "DESIGN.md")
    part = design[design.index("### 2.9 Probes"):design.index("## 3. Data layout in HBM")]
    assert design.index("### 2.8 Sensors") < design.index("### 2.9 Probes")
    for phrase in ("egg_probe", "d2 <= reach reach", "c <= 0.0", "b < 0.0", "q >= 0.0", "t <= 1.0", "STATELESS", "smallest batch\n`key`", "__ballot",
                   "__shfl_xor", "1,024", "egg_probe_scan_kernel", "egg_probe_finish_kernel", "parallel over (probe, type)", "all_gather",
                   "egg_group_probe", "no scratch", "profiles/r28_probes.md", "scripts/gpu_probes_bench.py"):
        assert phrase in part, phrase
    limits = design[design.index("## 7. Limits"):design.index("## 8.")]
    assert "probes (`egg_probe`)" in limits
    for phrase in ("centres for `POINT` and discs for `RAY`", "One winner per type", "no k-nearest", "rides on a collider", "Colliders themselves are not hit",
                   "At most 64 per call", "refused while a step is in flight"):
        assert phrase in limits[limits.index("probes (`egg_probe`)"):], phrase
    readme = _read(ROOT, "README.md")
    assert readme.index("* Sensors (") < readme.index("* Probes (") < readme.index("* `bench.py`, `profiles/`")
    for phrase in ("pick(x, y, reach, types)", "raycast(x0, y0, x1, y1, pad, types)", "`egg_probe` and\n  `egg_group_probe`", "168 in all",
                   "profiles/r28_probes.md", "tests/probe_model.py"):
        assert phrase in readme, phrase
    integration = _read(ROOT, "INTEGRATION.md")
    assert "168\nin all" in integration and "| probes (either order; one handle, device groups) | `egg_probe`, `egg_group_probe` |" in integration
    for proto in ("int egg_probe(egg_handle *h, int32_t n, const egg_probe_query *probes, egg_probe_hit *hits);",
                  "int egg_group_probe(egg_group *g, int32_t n, const egg_probe_query *probes, egg_probe_hit *hits);"):
        assert proto in integration, proto
    for phrase in ("h.pick(mouse_x, mouse_y, reach=32.0)", "handler:pick(mouse_x, mouse_y, 32)", "ProbeHit(id, index, score, x, y, radius)"):
        assert phrase in integration, phrase
    assert os.path.exists(os.path.join(ROOT, "profiles", "r28_probes.md")) and os.path.exists(os.path.join(ROOT, "profiles", "r28_probes.jsonl"))
    assert os.path.exists(os.path.join(ROOT, "scripts", "gpu_probes_bench.py"))
    entry = _read(ROOT, "__graft_entry__.py")
    assert "h.pick(px, py)" in entry and "smoke ok (probes)" in entry
