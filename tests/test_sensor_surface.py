"""The surface of the sensors (egg_set_sensors) as far as it can be checked without a device: the
eight entry points, the constants and the two structs in the header and in the ctypes binding, the five methods on all three
Python classes with equal parameter lists, the wrappers' own argument checks on a device-less instance, the Lua methods as
text, the kernels and that no step unit names them, and the documents."""
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
    "egg_set_sensors": "int egg_set_sensors(egg_handle *h, int32_t n, const egg_sensor *sensors);",
    "egg_get_sensors": "int egg_get_sensors(const egg_handle *h, int32_t cap, egg_sensor *out, int32_t *n);",
    "egg_read_sensors": "int egg_read_sensors(egg_handle *h, int32_t cap, egg_sensor_reading *readings, int64_t dropped[2], int32_t *n);",
    "egg_read_sensor_batches": "int egg_read_sensor_batches(egg_handle *h, int64_t n_ids, const int64_t *ids, "
                               "int32_t *counts /* [n_ids][n_sensors][2] */);",
    "egg_group_set_sensors": "int egg_group_set_sensors(egg_group *g, int32_t n, const egg_sensor *sensors);",
    "egg_group_get_sensors": "int egg_group_get_sensors(const egg_group *g, int32_t cap, egg_sensor *out, int32_t *n);",
    "egg_group_read_sensors": "int egg_group_read_sensors(egg_group *g, int32_t cap, egg_sensor_reading *readings, int64_t dropped[2], "
                              "int32_t *n);",
    "egg_group_read_sensor_batches": "int egg_group_read_sensor_batches(egg_group *g, int64_t n_ids, const int64_t *ids, "
                                     "int32_t *counts /* [n_ids][n_sensors][2] */);",
}
METHODS = {"set_sensors": ["self", "sensors"], "get_sensors": ["self"], "sensor_sums": ["self"], "sensors": ["self"],
           "sensor_batches": ["self", "ids"]}
KERNELS = {"egg_sensor_sums_kernel": "EggSensorArgs", "egg_sensor_units_kernel": "EggSensorArgs",
           "egg_sensor_finish_kernel": "EggSensorFinishArgs", "egg_sensor_batch_finish_kernel": "EggSensorBatchFinishArgs"}


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_header_declares_the_entry_points_the_constants_and_the_structs():
    from egg_fluid_simulation_amd import _ffi
    text = _read(ROOT, "include", "eggsim.h")
    for name, proto in PROTOS.items():
        assert proto in text, name
        assert name in _ffi._SIGNATURES and name in _ffi.EXPORTED_SYMBOLS, name
        assert len(_ffi._SIGNATURES[name][1]) == proto.count(",") + 1, name
    for name in ("set_sensors", "get_sensors", "read_sensors", "read_sensor_batches"):  # a group twin has its handle twin's parameters
        assert _ffi._SIGNATURES["egg_" + name][1] == _ffi._SIGNATURES["egg_group_" + name][1], name
    assert "typedef struct { int32_t kind; int32_t type_mask; double p[6]; } egg_sensor;   /* 56 bytes */" in text
    assert "typedef struct { int64_t count[2], sx[2], sy[2]; } egg_sensor_reading;         /* 48 bytes; [0] white, [1] yolk */" in text
    assert "#define EGG_SENSOR_POSITION_SCALE 65536.0 /* 2^16 */" in text and "#define EGG_MAX_SENSORS 64" in text
    assert "enum { EGG_SENSOR_HALF_PLANE = 0, EGG_SENSOR_DISC = 1, EGG_SENSOR_BOX = 2, EGG_SENSOR_CAPSULE = 3 };" in text
    Sn, Rd = _ffi.EggSensor, _ffi.EggSensorReading
    assert C.sizeof(Sn) == 56 and [(n, getattr(Sn, n).offset) for n, _ in Sn._fields_] == [("kind", 0), ("type_mask", 4), ("p", 8)]
    assert C.sizeof(Rd) == 48 and [(n, getattr(Rd, n).offset) for n, _ in Rd._fields_] == [("count", 0), ("sx", 16), ("sy", 32)]
    assert _ffi.MAX_SENSORS == 64 and _ffi.SENSOR_POSITION_SCALE == 2.0 ** 16
    assert _ffi.SENSOR_KINDS == ("half_plane", "disc", "box", "capsule") and [len(p) for p in _ffi.SENSOR_PARAMS] == [3, 3, 6, 5]
    # the rule, where a C caller reads it
    for phrase in ("s = (nx x + ny y) - off; inside iff s >= 0.0", "d2 = dx dx + dy dy; inside iff d2 <= R R",
                   "u = dx ux + dy uy, v = dy ux - dx uy; inside iff fabs(u) <= hx && fabs(v) <= hy",
                   "exactly as the SEGMENT collider defines them, l2 == 0 included", "a NaN\n * position is inside nothing",
                   "its radius is not read", "Parameters a kind does not use are stored as 0",
                   "sx[w] += llrint(x * EGG_SENSOR_POSITION_SCALE)", "reaches 2^53 in magnitude",
                   "ONE pair of counters per read, not one per sensor",
                   "((double)sx[w] / EGG_SENSOR_POSITION_SCALE) / (double)count[w]", "checks everything before it changes anything",
                   "refused while a step is in flight", "EGG_ERR_UNKNOWN_ID and nothing is written", "a repeated id is answered twice",
                   "are not cached: every call measures", "The sums wrap only beyond 2^63",
                   "launches exactly the kernels it launches without one", "no sensor that rides on a collider"):
        assert phrase in text, phrase
    # the prototypes parse as the rest of the header's do, and a C compiler agrees with the sizes
    assert all(name in _prototypes(text) for name in PROTOS)


def test_a_c_compiler_lays_the_structs_out_as_ctypes_does(tmp_path):
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    src = tmp_path / "sensor_layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "eggsim.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %d\\n", sizeof(egg_sensor), offsetof(egg_sensor, p), '
                   'sizeof(egg_sensor_reading), offsetof(egg_sensor_reading, sy), (int)EGG_SENSOR_CAPSULE); return 0; }\n')
    exe = str(tmp_path / "sensor_layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)],
                   check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["56", "8", "48", "32", "3"]


def test_the_kernels_exist_and_no_step_unit_names_them():
    kernels = _read(CSRC, "eggsim_sensors.hip")
    host_h = _read(CSRC, "eggsim_host.h")
    host = _read(CSRC, "eggsim_host_sensors.hip")
    device_h = _read(CSRC, "eggsim_device.h")
    for name, args in KERNELS.items():
        assert re.search(r'extern "C" __global__ void __launch_bounds__\(\w+\) %s\(%s A\)' % (name, args), kernels), name
        assert 'extern "C" __global__ void %s(%s A);' % (name, args) in host_h, name
        assert "hipLaunchKernelGGL(%s," % name in host, name
        assert "struct %s {" % args in device_h, name
    makefile = _read(CSRC, "Makefile")
    assert "eggsim_sensors.hip" in makefile and "eggsim_host_sensors.hip" in makefile and "-ffp-contract=off" in makefile
    # a wave per workgroup, ballots and popcounts, the reduction behind the wave-uniform branch, no LDS and no atomics in the body
    body = kernels[kernels.index("void sn_body("):kernels.index('extern "C"')]
    assert "__ballot(in)" in body and "__popcll(" in body and "if (inside == 0ull) continue;" in body
    assert "__shared__" not in body and "atomic" not in body
    assert "#define EGG_SN_SCALE 0x1p16" in device_h and "#define EGG_SN_LIMIT 0x1p53" in device_h and "#define EGG_SN_UNIT 1024" in device_h
    assert "EGG_SENSOR_POSITION_SCALE == EGG_SN_SCALE" in host and "sizeof(egg_sensor) == 56" in host
    # nothing of a step knows about sensors: no step kernel, no step driver, no commit
    for unit in os.listdir(CSRC):
        if unit.endswith((".hip", ".cpp", ".h")) and unit not in ("eggsim_sensors.hip", "eggsim_host_sensors.hip", "eggsim_host.h",
                                                                   "eggsim_device.h", "eggsim_group.cpp"):
            assert "sensor" not in _read(CSRC, unit).lower(), unit
    # the refusals, where the sources state them
    setter = host[host.index("int egg_set_sensors("):host.index("int egg_get_sensors(")]
    assert 'REJECT_IN_FLIGHT(h, "egg_set_sensors");' in setter and "opt_solver_order" not in setter  # (either order)
    assert setter.index("h->sensors.swap(list);") > max(m.start() for m in re.finditer(r"return fail\(", setter))  # checked, then changed
    assert 'REJECT_IN_FLIGHT(h, "egg_read_sensors");' in host and 'REJECT_IN_FLIGHT(h, "egg_read_sensor_batches");' in host


def test_python_classes_have_the_methods_with_equal_parameter_lists():
    from egg_fluid_simulation_amd import SimulationGroup, SimulationHandler
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler
    for cls in (SimulationHandler, SimulationGroup, ShardedSimulationHandler):
        for name, params in METHODS.items():
            assert list(inspect.signature(getattr(cls, name)).parameters) == params, (cls.__name__, name)
    # a group calls its own entry points, a sharded handler its local handle and one all-reduce of an int64 tensor per read
    assert SimulationGroup._PREFIX == "egg_group_" and SimulationGroup.sensor_sums is SimulationHandler.sensor_sums
    for name in ("sensor_sums", "sensor_batches"):
        src = inspect.getsource(getattr(ShardedSimulationHandler, name))
        assert "self.local.%s(" % name in src and src.count("self._all_reduce_sum(") + src.count("self._owner_table(") == 1 and "int64" in src, name
    assert "self.local.set_sensors(sensors)" in inspect.getsource(ShardedSimulationHandler.set_sensors)
    assert "_sensor_readings" in inspect.getsource(ShardedSimulationHandler.sensors)


def test_the_wrappers_check_what_only_the_host_can():
    from egg_fluid_simulation_amd import EggError, SimulationGroup, SimulationHandler, _ffi
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler
    for cls in (SimulationHandler, SimulationGroup, ShardedSimulationHandler):
        h = cls.__new__(cls)  # no device: the checks below come before any call into the library
        if cls is ShardedSimulationHandler:
            h.local = SimulationHandler.__new__(SimulationHandler)
        for bad, text in (([("ring", 0, 0, 1)], "sensor 0: kind must be one of half_plane, disc, box, capsule"),
                          ([("disc", 0, 0, 1), ("disc", 0, 0)], r"sensor 1 \(disc\): expected \('disc', cx, cy, R\[, types\]\)"),
                          ([("box", 0, 0, 1, 1)], r"sensor 0 \(box\): expected"), ([("disc", 0, 0, 1, "none")], "sensor 0: types must be"),
                          ([("capsule", 0, 0, 1, 1, "x", "both")], r"sensor 0 \(capsule\): the parameters must be numbers"),
                          ([{"kind": "disc", "cx": 0, "cy": 0}], r"sensor 0 \(disc\): expected the keys cx, cy, R"),
                          ([("disc", 0, 0, 1)] * 65, "a list holds 0 .. 64 sensors")):
            with pytest.raises(EggError, match=text):
                h.set_sensors(bad)
    n, arr = SimulationHandler._c_sensors([("box", 1, 2, 3, 4, math.pi / 3, "yolk"), {"kind": "box", "cx": 1, "cy": 2, "hx": 3, "hy": 4, "angle": 0.25},
                                           ("box", 1, 2, 3, 4, 0.0, 2.0), ("capsule", 1, 2, 3, 4, 5, "white"), {"kind": "half_plane", "nx": 0, "ny": 1, "off": 2}])
    assert n == 5 and [s.kind for s in arr[:5]] == [2, 2, 2, 3, 0] and [s.type_mask for s in arr[:5]] == [2, 3, 3, 1, 3]
    assert list(arr[0].p) == [1.0, 2.0, 3.0, 4.0, math.cos(math.pi / 3), math.sin(math.pi / 3)]  # (the host's cos / sin, as spin)
    assert list(arr[1].p)[4:] == [math.cos(0.25), math.sin(0.25)] and list(arr[2].p)[4:] == [0.0, 2.0]  # (an axis goes as given)
    assert list(arr[3].p) == [1.0, 2.0, 3.0, 4.0, 5.0, 0.0] and list(arr[4].p) == [0.0, 1.0, 2.0, 0.0, 0.0, 0.0]
    assert SimulationHandler._c_sensors([])[0] == 0
    readings = SimulationHandler._sensor_readings([((2, 3 * 65536, -65536), (0, 0, 0))])
    assert readings == [{"count": (2, 0), "centroid": ((1.5, -0.5), None)}] and _ffi.SENSOR_TYPES == {"white": 1, "yolk": 2, "both": 3}


def test_lua_has_the_methods_and_the_header_prototypes():
    lua = _read(ROOT, "egg_fluid_simulation_amd", "lua", "egg_fluid_simulation", "simulation_handler.lua")
    for name in METHODS:
        assert "function SimulationHandler:%s(" % name in lua, name
    cdef = _prototypes(re.search(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S).group(1))
    header = _prototypes(_read(ROOT, "include", "eggsim.h"))
    for name in ("egg_set_sensors", "egg_get_sensors", "egg_read_sensors", "egg_read_sensor_batches"):
        assert cdef[name] == header[name], name
        assert "lib.%s(self._h" % name in lua, name
    assert "typedef struct { int32_t kind; int32_t type_mask; double p[6]; } egg_sensor;" in lua
    assert "typedef struct { int64_t count[2], sx[2], sy[2]; } egg_sensor_reading;" in lua
    assert "math.cos(s[6]), math.sin(s[6])" in lua  # (a box by its angle)
    assert "(tonumber(rec[name][2]) / _sensor_scale) / count" in lua and "_sensor_scale = 65536" in lua


def test_the_documents_describe_the_rule_and_the_limits():
    design = _read(ROOT, "DESIGN.md")
    part = design[design.index("### 2.8 Sensors"):design.index("## 3. Data layout in HBM")]
    assert design.index("### 2.7 Relaxed order") < design.index("### 2.8 Sensors")  # (a section of its own, not under 2.7)
    for phrase in ("egg_set_sensors", "d2 <= R R", "s >= 0.0", "llrint", "2^53", "2^63", "dropped", "__ballot", "1,024", "egg_sensor_finish_kernel",
                   "all_reduce", "profiles/r27_sensors.md"):
        assert phrase in part, phrase
    limits = design[design.index("## 7. Limits"):design.index("## 8.")]
    assert "sensors (`egg_set_sensors`)" in limits
    for phrase in ("centres only", "no velocity or mass sums", "rides on a collider", "at most 64", "2^63"):
        assert phrase in limits[limits.index("sensors (`egg_set_sensors`)"):], phrase
    readme = _read(ROOT, "README.md")
    assert "set_sensors" in readme and "sensor_batches" in readme and "profiles/r27_sensors.md" in readme
    assert "158 entry points -- 101 on one device" in readme  # (the pinned sentence stands as it was)
    integration = _read(ROOT, "INTEGRATION.md")
    assert "158 entry points" in integration
    for name in PROTOS:
        assert name in integration and name in readme + integration, name
    for proto in ("int egg_set_sensors(egg_handle *h, int32_t n, const egg_sensor *sensors);",
                  "int egg_read_sensors(egg_handle *h, int32_t cap, egg_sensor_reading *readings, int64_t dropped[2], int32_t *n);"):
        assert proto in integration, proto
    assert os.path.exists(os.path.join(ROOT, "profiles", "r27_sensors.md")) and os.path.exists(os.path.join(ROOT, "profiles", "r27_sensors.jsonl"))
    assert os.path.exists(os.path.join(ROOT, "scripts", "gpu_sensors_bench.py"))
