"""The measures (egg_measure) as far as their surface can be checked without a device: the prototypes
and structs of include/eggsim_measure.h against the ctypes binding and a C compiler, the kernel and its host side as text,
the methods of the three Python classes, the Lua wrapper as text and the documents."""
import ctypes as C
import inspect
import os
import re

import pytest

import measure_model as mm
from conftest import ROOT
from scan_surface import in_flight_messages_have_one_home
from test_abi import _prototypes

CSRC = os.path.join(ROOT, "egg_fluid_simulation_amd", "csrc")
PROTOS = {
    "egg_measure": "int egg_measure(egg_handle *h, const egg_measure_spec *spec, int64_t n_ids, const int64_t *ids, egg_measure_record *out /* host [n][2] */);",
    "egg_measure_to": "int egg_measure_to(egg_handle *h, const egg_measure_spec *spec, int64_t n_ids, const int64_t *ids, void *device_out, int64_t capacity_bytes);",
    "egg_group_measure": "int egg_group_measure(egg_group *g, const egg_measure_spec *spec, int64_t n_ids, const int64_t *ids, egg_measure_record *out);",
}


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_header_and_binding_agree_on_the_entry_points_and_the_structs():
    from egg_fluid_simulation_amd import _ffi
    text = _read(ROOT, "include", "eggsim_measure.h")
    for name, proto in PROTOS.items():
        assert proto in text, name
        assert name in _ffi._MEASURE_SIGNATURES and name in _ffi.MEASURE_SYMBOLS and name in _prototypes(text), name
    # the binding covers the whole of this header; the three tables are disjoint: 173 + 2 + 3 entry points
    assert sorted(_prototypes(text)) == _ffi.MEASURE_SYMBOLS == sorted(PROTOS)
    assert not set(_ffi.MEASURE_SYMBOLS) & set(_ffi.EXPORTED_SYMBOLS) and not set(_ffi.MEASURE_SYMBOLS) & set(_ffi.IMPULSE_SYMBOLS)
    assert len(_ffi.EXPORTED_SYMBOLS) + len(_ffi.IMPULSE_SYMBOLS) + len(_ffi.MEASURE_SYMBOLS) == 178
    assert _ffi._MEASURE_SIGNATURES["egg_measure"] == _ffi._MEASURE_SIGNATURES["egg_group_measure"]
    assert _ffi._MEASURE_SIGNATURES["egg_measure_to"][1][:4] == _ffi._MEASURE_SIGNATURES["egg_measure"][1][:4]
    main = _read(ROOT, "include", "eggsim.h")
    assert main.count('#include "eggsim_measure.h"') == 1 and main.index('#include "eggsim_measure.h"') > main.index('#include "eggsim_impulse.h"')
    declared = set(re.findall(r"\b(egg_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", main, flags=re.S)))
    assert declared == set(_ffi.EXPORTED_SYMBOLS) and len(declared) == 173  # (the main header's list stays as it was)
    if os.path.exists(_ffi.LIB_PATH):
        lib = _ffi.load()
        assert all(hasattr(lib, name) and getattr(lib, name).argtypes == _ffi._MEASURE_SIGNATURES[name][1] for name in _ffi.MEASURE_SYMBOLS)
    entry = _read(ROOT, "__graft_entry__.py")
    assert "_ffi.MEASURE_SYMBOLS" in entry and "_MEASURE_SIGNATURES.items()" in _read(ROOT, "egg_fluid_simulation_amd", "_ffi.py")
    # the record, field for field, and the spec
    R, P = _ffi.EggMeasureRecord, _ffi.EggMeasureSpec
    assert C.sizeof(R) == 192 and [(n, getattr(R, n).offset) for n, _ in R._fields_] == [(n, 8 * k) for k, n in enumerate(mm.FIELDS)]
    assert all(t is C.c_int64 for _, t in R._fields_) and _ffi.MEASURE_FIELDS == mm.FIELDS and len(mm.FIELDS) == 24
    assert C.sizeof(P) == 64 and [(n, getattr(P, n).offset) for n, _ in P._fields_] == [("region", 0), ("flags", 56), ("type_mask", 60)]
    body = re.search(r"typedef struct \{([^}]*)\} egg_measure_record;", text).group(1)
    assert tuple(re.findall(r"[a-z_0-9]+(?=\s*[,;])", body.replace("int64_t", ""))) == mm.FIELDS
    assert "typedef struct { egg_sensor region; int32_t flags, type_mask; } egg_measure_spec;" in text
    for line in ("#define EGG_MEASURE_SCALE 65536.0", "#define EGG_MEASURE_MASS_SCALE 4294967296.0", "#define EGG_MEASURE_FIELDS 24",
                 "enum { EGG_MEASURE_REGION = 1 };"):
        assert line in text, line
    assert (_ffi.MEASURE_SCALE, _ffi.MEASURE_MASS_SCALE, _ffi.MEASURE_REGION) == (mm.S, mm.SM, 1) == (65536.0, 4294967296.0, 1)
    # the rule, where a C caller reads it
    for phrase in ("m = 1.0 / inv_mass", "x*S, y*S, m*SM, (m*x)*S, (m*y)*S, (m*vx)*S, (m*vy)*S", "v2 = vx*vx + vy*vy then (m*v2)*S and v2*S",
                   "(x - radius)*S, (y - radius)*S, (x + radius)*S, (y + radius)*S", "truncation toward zero", "(m*(dx*vy - dy*vx))*S",
                   "(sqrt(d2) + radius)*S", "dropped_central", "never on doubles", "With kept == 0 the\n * fields 3 to 23 are 0",
                   "with kept == dropped_central the fields 19 to 23 are 0", "the whole record is 0", "Everything is checked before anything is launched or written",
                   "egg_step_begin or egg_rx_begin open", "EGG_ERR_UNKNOWN_ID", "tests/measure_model.py", "no contraction",
                   "no per-region measure without a batch list", "no measure that rides on a collider", "one region per call", "per type\n * only"):
        assert phrase in text, phrase


def test_a_c_compiler_lays_the_structs_out_as_ctypes_does(tmp_path):
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    src = tmp_path / "measure_layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "eggsim.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(egg_measure_spec), offsetof(egg_measure_spec, flags), '
                   'offsetof(egg_measure_spec, type_mask), sizeof(egg_measure_record), offsetof(egg_measure_record, lo_x), '
                   'offsetof(egg_measure_record, dropped_central), offsetof(egg_measure_record, max_reach), (int)EGG_MEASURE_FIELDS, '
                   '(int)EGG_MEASURE_REGION); return 0; }\n')
    exe = str(tmp_path / "measure_layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)],
                   check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["64", "56", "60", "192", "88", "144", "184", "24", "1"]


def test_the_kernel_exists_and_nothing_else_names_it():
    kernels, host, host_h, device_h = (_read(CSRC, f) for f in ("eggsim_measures.hip", "eggsim_host_measures.hip", "eggsim_host.h", "eggsim_device.h"))
    assert 'extern "C" __global__ void __launch_bounds__(EGG_MS_BLOCK) egg_measure_kernel(EggMeasureArgs A)' in kernels
    assert 'extern "C" __global__ void egg_measure_kernel(EggMeasureArgs A);' in host_h and "hipLaunchKernelGGL(egg_measure_kernel," in host
    for line in ("#define EGG_MS_FIELDS 24", "#define EGG_MS_SCALE 0x1p16", "#define EGG_MS_MASS_SCALE 0x1p32", "#define EGG_MS_LIMIT 0x1p53",
                 "#define EGG_MS_BLOCK 256", "#define EGG_MS_WAVE_ATOM 1024", "struct EggMeasureRow {", "struct EggMeasureArgs {"):
        assert line in device_h, line
    makefile = _read(CSRC, "Makefile")
    assert makefile.count("eggsim_measures.hip") == 2 and makefile.count("eggsim_host_measures.hip") == 1 and "-ffp-contract=off" in makefile
    assert "../../include/eggsim_measure.h" in makefile
    # the rule in the header's order; the shared region test; one reduction per pass; no global atomics, no inline assembly, no
    # single precision; lanes below the record's length write it
    for line in ("f[3] = (p.m * p.x) * EGG_MS_SCALE;", "const double v2 = p.vx * p.vx + p.vy * p.vy;", "f[7] = (p.m * v2) * EGG_MS_SCALE;",
                 "ok = ok && fabs(f[k]) < EGG_MS_LIMIT;", "p.m = 1.0 / ", "sn_test(A.region, p.x, p.y, d2, R)", "a[MS_SX] / kept_n",
                 "(double)ox_q / EGG_MS_SCALE", "g[3] = (p.m * (dx * p.vy - dy * p.vx)) * EGG_MS_SCALE;", "g[4] = (sqrt(d2) + p.r) * EGG_MS_SCALE;",
                 "if (lane < EGG_MS_FIELDS) A.out[(size_t)row.slot * EGG_MS_FIELDS + lane] = mine;"):
        assert line in kernels, line
    assert not re.search(r"atomic\w*\(", kernels) and "asm" not in kernels and "float" not in kernels and "bool sn_test(" not in kernels
    assert kernels.count("ms_wave_sum(a[k])") == 1 and kernels.count("ms_wave_sum(c[k])") == 1 and "__shfl_xor(" in kernels
    assert kernels.count("A.out[") == 1 and not re.findall(r"\bA\.(x|y|vx|vy|radius|inv_mass)\[w\]\[\w+\] *=[^=]", kernels)  # (read-only)
    # the host side: the ABI's constants are the kernel's, the table is kept by the atoms, the mask and the list, the checks
    # come before the first launch and before anything is written, only kernel_launches moves
    for line in ("sizeof(egg_measure_spec) == 64", "sizeof(egg_measure_record) == 192", "EGG_MEASURE_SCALE == EGG_MS_SCALE",
                 "struct MeasureState {", "atoms_gen", "check_region(h, what.c_str(), 0, region)", "device_range_fits(h, out, bytes)"):
        assert line in host, line
    scan = _read(CSRC, "eggsim_host_scan.hip")
    fits = scan[scan.index("bool device_range_fits("):]
    assert "on_device_of(h, p)" in fits[:fits.index("\n}\n")] and "hipMemGetAddressRange(" in fits[:fits.index("\n}\n")]
    assert host.index("REJECT_IN_FLIGHT(h, name);") < host.index("return fail(")  # (the first refusal of a call)
    in_flight_messages_have_one_home()
    assert "std::shared_ptr<egghost::MeasureState> measure_state;" in host_h and "opt_solver_order" not in host
    last_check = max(m.start() for m in re.finditer(r"return fail\(h, EGG_ERR_(INVALID_ARGUMENT|UNKNOWN_ID)", host))
    assert last_check < host.index("hipLaunchKernelGGL(") and last_check < host.index("hipMemsetAsync(") and last_check < host.index("upload_atoms(")
    assert last_check < host.index("hipMemcpyAsync(out,")
    assert host.count("h->stats.kernel_launches += 1;") == 1 and "h->stats." not in host.replace("h->stats.kernel_launches += 1;", "")
    # nothing of a step knows about measures -- and no unit but the measures' own, the two shared headers and the group
    for unit in os.listdir(CSRC):
        if unit.endswith((".hip", ".cpp", ".h")) and unit not in ("eggsim_measures.hip", "eggsim_host_measures.hip", "eggsim_host.h",
                                                                   "eggsim_device.h", "eggsim_group.cpp"):
            text = _read(CSRC, unit)
            assert "egg_measure" not in text and "EggMeasure" not in text and "measure_state" not in text and "EGG_MS_" not in text, unit
    group = _read(CSRC, "eggsim_group.cpp")
    twin = group[group.index("int egg_group_measure("):]
    twin = twin[:twin.index("\n}\n")]
    assert "egg_measure(g->h[k], spec," in twin and "route_to_owners<" in twin and twin.rindex("return gfail(") < twin.index("route_to_owners<")
    route = group[group.index("int route_to_owners("):]
    route = route[:route.index("\n}\n")]
    assert "r.owner != (int)k" in route and route.rindex("return gfail(") < route.index("memcpy(out,")  # (written after every handle answered)


def test_python_classes_have_the_methods():
    from egg_fluid_simulation_amd import EggError, SimulationGroup, SimulationHandler, _ffi
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler
    from egg_fluid_simulation_amd.simulation_handler import Measure
    for cls in (SimulationHandler, SimulationGroup, ShardedSimulationHandler):
        for name, params in (("measure", ["self", "ids", "region", "types"]), ("measure_table", ["self", "ids", "region", "types"]),
                             ("at_rest", ["self", "id", "speed", "types"])):
            assert list(inspect.signature(getattr(cls, name)).parameters) == params, (cls.__name__, name)
        assert inspect.signature(cls.measure).parameters["types"].default == "both" and inspect.signature(cls.measure).parameters["ids"].default is None
    assert list(inspect.signature(SimulationHandler.measure_to).parameters) == ["self", "out", "ids", "region", "types"]
    assert not hasattr(SimulationGroup, "measure_to") and not hasattr(ShardedSimulationHandler, "measure_to")
    assert SimulationGroup._PREFIX == "egg_group_" and SimulationGroup.measure_table is SimulationHandler.measure_table
    src = inspect.getsource(ShardedSimulationHandler.measure_table)
    assert src.count("self._owner_table(") == 1 and "self.dist" not in src and "self.local._measure_table(" in src and "self.local._measure_check(" in src
    assert ShardedSimulationHandler.measure is SimulationHandler.measure and ShardedSimulationHandler.at_rest is SimulationHandler.at_rest
    assert Measure._fields == mm.FIELDS
    for name in ("kept", "mass", "centroid", "center_of_mass", "momentum", "velocity", "kinetic_energy", "bounds", "max_speed", "origin", "reach", "spin"):
        assert isinstance(getattr(Measure, name), property), name
    spec = SimulationHandler._c_measure_spec(("disc", 1.0, 2.0, 3.0, "yolk"), "white")
    assert (spec.flags, spec.type_mask, spec.region.kind, spec.region.type_mask, list(spec.region.p)[:3]) == (1, 1, 1, 2, [1.0, 2.0, 3.0])
    spec = SimulationHandler._c_measure_spec(None, 3)
    assert (spec.flags, spec.type_mask) == (0, 3)
    for kw, text in ((dict(region=("ring", 0, 0, 1), types="both"), "measure: region"), (dict(region=None, types="none"), "types must be")):
        with pytest.raises(EggError, match=text):
            SimulationHandler._c_measure_spec(**kw)
    assert _ffi.MEASURE_SYMBOLS == ["egg_group_measure", "egg_measure", "egg_measure_to"]


def test_lua_has_the_functions_and_the_header_prototype():
    lua = _read(ROOT, "egg_fluid_simulation_amd", "lua", "egg_fluid_simulation", "simulation_handler.lua")
    for line in ("function SimulationHandler:measure(ids, region, types)", "function SimulationHandler:at_rest(id, speed, types)"):
        assert line in lua, line
    blocks = re.findall(r"ffi\.cdef\[(=*)\[(.*?)\]\1\]", lua, flags=re.S)
    assert len(blocks) == 3 and "egg_measure" not in blocks[0][1] and "egg_measure" not in blocks[1][1]  # (a block per header)
    assert _prototypes(blocks[2][1]) == {"egg_measure": _prototypes(_read(ROOT, "include", "eggsim_measure.h"))["egg_measure"]}
    assert "typedef struct { egg_sensor region; int32_t flags, type_mask; } egg_measure_spec;" in blocks[2][1]
    body = re.search(r"typedef struct \{([^}]*)\} egg_measure_record;", blocks[2][1]).group(1)
    assert tuple(re.findall(r"[a-z_0-9]+(?=\s*[,;])", body.replace("int64_t", ""))) == mm.FIELDS
    names = re.search(r"local _measure_fields = \{(.*?)\}", lua, flags=re.S).group(1)
    assert tuple(re.findall(r'"(\w+)"', names)) == mm.FIELDS
    assert "lib.egg_measure(self._h, spec, n, c_ids, out)" in lua and "_measure_scale = 65536" in lua and "_measure_mass_scale = 4294967296" in lua
    for phrase in ("one.mass = one.sm / _measure_mass_scale", "one.kinetic_energy = 0.5 * one.se / S", "one.max_speed = math.sqrt(one.max_v2 / S)",
                   "one.spin = one.sl / S", "res[1].white.max_speed <= speed"):
        assert phrase in lua, phrase


def test_the_documents_describe_the_call():
    design = _read(ROOT, "DESIGN.md")
    assert design.index("### 2.12 Impulses") < design.index("### 2.13 Measures") < design.index("## 3. Data layout in HBM")
    part = design[design.index("### 2.13 Measures"):design.index("## 3. Data layout in HBM")]
    for phrase in ("egg_measure", "egg_measure_to", "egg_group_measure", "egg_measure_kernel", "sn_test", "check_region", "tests/measure_model.py",
                   "scripts/gpu_measures_bench.py", "profiles/r32_measures.md", "all_reduce", "atoms_gen", "one launch per call", "No per-region measure without a batch list",
                   "no measure that rides on a collider", "one region per call", "per type\nonly", "never on doubles", "make resource-usage"):
        assert phrase in part, phrase
    readme, integration = _read(ROOT, "README.md"), _read(ROOT, "INTEGRATION.md")
    assert readme.index("* Impulses (") < readme.index("* Measures (") < readme.index("* `bench.py`, `profiles/`")
    assert "three more entry points for measures: 178" in " ".join(readme.split()) and "profiles/r32_measures.md" in readme
    assert "(the row \"measures\"): 178" in integration and "h.measure(" in integration and "handler:measure(" in integration
    assert "| measures (either order; one handle, device groups) | `egg_measure`, `egg_measure_to`, `egg_group_measure` |" in integration
    for proto in PROTOS.values():
        assert " ".join(proto.split()) in " ".join(integration.split()), proto
    for phrase in ("no per-region measure without a batch list", "no measure that rides on a collider", "one region per call", "per type only"):
        assert phrase in " ".join(integration.split()), phrase
    entry = _read(ROOT, "__graft_entry__.py")
    assert "h.measure_table()" in entry and "smoke ok (measures)" in entry
    profile = _read(ROOT, "profiles", "r32_measures.md")
    for phrase in ("measure_table", "measure_to", "yardstick", "VGPRs", "bench.py"):
        assert phrase in profile, phrase
