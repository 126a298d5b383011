"""The surface of the fields (egg_field) as far as it can be checked without a device: the three
entry points, the constants and the three structs in the header and in the ctypes binding, field offsets included, the
methods on the three Python classes with equal parameter lists, the wrappers' own argument checks on a device-less
instance, the Lua method as text, the kernels and that no step unit names them, and the documents."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from scan_surface import OBSERVER_UNITS, in_flight_messages_have_one_home, sources
from test_abi import _prototypes

CSRC = os.path.join(ROOT, "egg_fluid_simulation_amd", "csrc")
PROTOS = {
    "egg_field": "int egg_field(egg_handle *h, const egg_field_spec *spec, const egg_field_planes *host_out, egg_field_totals *totals);",
    "egg_field_to": "int egg_field_to(egg_handle *h, const egg_field_spec *spec, const egg_field_planes *device_out, egg_field_totals *totals);",
    "egg_group_field": "int egg_group_field(egg_group *g, const egg_field_spec *spec, const egg_field_planes *host_out, egg_field_totals *totals);",
}
FIELD_PARAMS = ["self", "origin", "cell", "shape", "types", "velocity", "path"]
FIELD_TO_PARAMS = ["self", "origin", "cell", "shape", "count", "svx", "svy", "types", "path"]
KERNELS = ("egg_field_count_kernel", "egg_field_velocity_kernel")
STEP_UNITS = ("eggsim_step.hip", "eggsim_packed.hip", "eggsim_relaxed.hip", "eggsim_relaxed_contacts.hip", "eggsim_relaxed_wire.hip",
              "eggsim_host_step.hip", "eggsim_host_relaxed.hip", "eggsim_host_relaxed_group.hip", "eggsim_host_relaxed_wire.hip",
              "eggsim_sensors.hip", "eggsim_probes.hip")


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
    assert _ffi._SIGNATURES["egg_field"][1] == _ffi._SIGNATURES["egg_field_to"][1] == _ffi._SIGNATURES["egg_group_field"][1]
    assert re.search(r"typedef struct \{ double x0, y0, cell; int32_t nx, ny, type_mask, path; \} egg_field_spec; +/\* 40 bytes \*/", text)
    assert re.search(r"typedef struct \{ int32_t \*count; int64_t \*svx, \*svy; \} egg_field_planes; +/\* each \[2\]\[ny\]\[nx\], row-major", text)
    assert re.search(r"typedef struct \{ int64_t inside\[2\], outside\[2\], dropped\[2\]; int32_t units_tiled, units_direct; \} egg_field_totals; /\* 56 bytes \*/", text)
    assert "#define EGG_FIELD_MAX_CELLS (1 << 20)" in text and "#define EGG_FIELD_VELOCITY_SCALE 65536.0" in text
    assert "enum { EGG_FIELD_PATH_AUTO = 0, EGG_FIELD_PATH_DIRECT = 1 };" in text
    S, P, T = _ffi.EggFieldSpec, _ffi.EggFieldPlanes, _ffi.EggFieldTotals
    assert C.sizeof(S) == 40 and [(n, getattr(S, n).offset) for n, _ in S._fields_] == [
        ("x0", 0), ("y0", 8), ("cell", 16), ("nx", 24), ("ny", 28), ("type_mask", 32), ("path", 36)]
    assert C.sizeof(P) == 3 * C.sizeof(C.c_void_p) and [n for n, _ in P._fields_] == ["count", "svx", "svy"]
    assert C.sizeof(T) == 56 and [(n, getattr(T, n).offset) for n, _ in T._fields_] == [
        ("inside", 0), ("outside", 16), ("dropped", 32), ("units_tiled", 48), ("units_direct", 52)]
    assert _ffi.FIELD_MAX_CELLS == 1 << 20 and _ffi.FIELD_VELOCITY_SCALE == 65536.0 and (_ffi.FIELD_PATH_AUTO, _ffi.FIELD_PATH_DIRECT) == (0, 1)
    assert _ffi.FIELD_PATHS == {"auto": 0, "direct": 1} and _ffi.FIELD_TYPES == {"white": 1, "yolk": 2, "both": 3}
    # the rule, where a C caller reads it
    for phrase in ("inv = 1.0 / cell, computed ONCE on the host", "fx = (x - x0) * inv", "fy = (y - y0) * inv",
                   "fx >= 0.0 && fx < (double)nx && fy >= 0.0 && fy < (double)ny", "a NaN position is outside", "ix = (int)fx, iy = (int)fy",
                   "-0.0 is\n * cell 0", "index iy * nx + ix", "Only the particle's centre counts", "outside[w] += 1 and nothing else",
                   "dropped[w] += 1 and nothing else", "reaches 2^53 in magnitude", "llrint(vx * EGG_FIELD_VELOCITY_SCALE)",
                   "ties to even", "svx and svy are given together or not at\n * all", "dropped is 0", "are all zero",
                   "inside[w] + outside[w] + dropped[w] = the particles of type w", "((double)svx / EGG_FIELD_VELOCITY_SCALE) / (double)count",
                   "wraps only beyond 2^63", "A call is STATELESS", "nothing is cached", "only kernel_launches moves",
                   "checks everything before it launches or writes anything", "planes and totals untouched", "Refused while a step is in flight",
                   "zero-fills the planes and launches nothing", "not aligned to its word", "returns after the stream is idle",
                   "no splat by radius, no area or mass plane", "no per-batch planes", "no field that rides on a collider",
                   "no egg_field_to for groups or sharded ranks", "A failure on any handle writes nothing", "There is no\n * egg_group_field_to"):
        assert phrase in text, phrase
    assert all(name in _prototypes(text) for name in PROTOS)


def test_a_c_compiler_lays_the_structs_out_as_ctypes_does(tmp_path):
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    src = tmp_path / "field_layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "eggsim.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %.1f\\n", sizeof(egg_field_spec), offsetof(egg_field_spec, cell), '
                   'offsetof(egg_field_spec, nx), offsetof(egg_field_spec, path), sizeof(egg_field_planes) / sizeof(void *), '
                   'offsetof(egg_field_planes, svy) / sizeof(void *), sizeof(egg_field_totals), offsetof(egg_field_totals, outside), '
                   'offsetof(egg_field_totals, dropped), offsetof(egg_field_totals, units_direct), (int)EGG_FIELD_PATH_DIRECT, '
                   '(int)EGG_FIELD_MAX_CELLS, EGG_FIELD_VELOCITY_SCALE); return 0; }\n')
    exe = str(tmp_path / "field_layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)],
                   check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == [
        "40", "16", "24", "36", "3", "2", "56", "16", "32", "52", "1", "1048576", "65536.0"]


def test_the_kernels_exist_and_no_step_unit_names_them():
    kernels = _read(CSRC, "eggsim_fields.hip")
    host_h = _read(CSRC, "eggsim_host.h")
    host = _read(CSRC, "eggsim_host_fields.hip")
    device_h = _read(CSRC, "eggsim_device.h")
    for name in KERNELS:
        assert re.search(r'extern "C" __global__ void __launch_bounds__\(64\) %s\(EggFieldArgs A\)' % name, kernels), name
        assert 'extern "C" __global__ void %s(EggFieldArgs A);' % name in host_h, name
        assert "hipLaunchKernelGGL(%s," % name in host, name
    assert "struct EggFieldArgs {" in device_h and "#define EGG_FD_TILE_CELLS 1024" in device_h and "#define EGG_FD_LIMIT 0x1p53" in device_h
    makefile = _read(CSRC, "Makefile")
    assert makefile.count("eggsim_fields.hip") == 2 and makefile.count("eggsim_host_fields.hip") == 1 and "-ffp-contract=off" in makefile
    # one kernel body in two instantiations; a wave per workgroup; the rule in the order the header states; the first pass
    # reduces the rectangle, the tile path sums in LDS and flushes non-zero words, the direct path adds per lane; no
    # inline assembly
    body = kernels[kernels.index("void fd_body("):kernels.index('extern "C"')]
    assert "template <bool VELOCITY>" in kernels and "fd_body<false>(A)" in kernels and "fd_body<true>(A)" in kernels
    assert "(x - A.x0) * A.inv" in kernels and "(y - A.y0) * A.inv" in kernels and "fx >= 0.0 && fx < (double)A.nx && fy >= 0.0 && fy < (double)A.ny" in kernels
    assert "__shared__ int32_t t_count[EGG_FD_TILE_CELLS];" in body and "__shared__ unsigned long long t_svx[" in body
    assert "__popcll(__ballot(live && !in))" in body and "fd_wave_min(" in body and "fd_wave_max(" in body and "__shfl_xor(" in kernels
    assert "rect <= (long long)A.tile_cells" in body and "atomicAdd(&t_count[i], 1);" in body and "if (n != 0) atomicAdd(&g_count[c], n);" in body
    assert "if (sx != 0ull) atomicAdd(&g_svx[c], sx);" in body and "atomicAdd(&g_count[c], 1);" in body
    assert "fabs(sx) < EGG_FD_LIMIT && fabs(sy) < EGG_FD_LIMIT" in body and "llrint(" in body
    assert body.index("fd_wave_min(") < body.index("atomicAdd(&t_count[i], 1);") < body.index("if (n != 0) atomicAdd(&g_count[c], n);")
    assert "atomicAdd(&A.totals[lane]" in body and "asm" not in kernels and "float" not in body
    assert "sizeof(egg_field_spec) == 40" in host and "sizeof(egg_field_totals) == 56" in host and "EGG_FIELD_VELOCITY_SCALE == EGG_FD_SCALE" in host
    assert "<= (int)kLdsMax" in host and "constexpr int kWavesPerCu = 8;" in host  # (the wave cap per compute unit fits its LDS)
    # the unit table is the shared builder's, and its state is this feature's own
    scan = _read(CSRC, "eggsim_host_scan.hip")
    assert re.search(r"struct FieldState \{\n\s*UnitTable units;", host) and "->units.refresh(h, name, cover, false)" in host
    refresh = scan[scan.index("int UnitTable::refresh("):]
    refresh = refresh[:refresh.index("\n}\n")]
    key = "if (cover == want && gen[0] == h->sys[0].atoms_gen && gen[1] == h->sys[1].atoms_gen) return EGG_OK;"
    assert key in refresh and "gen[0] = gen[1] = ~0ull;" in refresh and "push_units(a, w, units);" in refresh
    assert refresh.index(key) < refresh.index("gen[0] = gen[1] = ~0ull;") < refresh.index("push_units(a, w,")  # invalidated, then rebuilt
    assert refresh.index("hipMemcpy(d_units.p") < refresh.index("gen[0] = h->sys[0].atoms_gen;")              # remembered last
    assert "std::shared_ptr<egghost::FieldState> field_state;" in host_h
    # nothing of a step knows about fields: no step kernel, no step driver, no commit -- and no unit but the fields' own, the
    # two shared headers and the group
    for unit in set(os.listdir(CSRC)) | set(STEP_UNITS):
        if unit.endswith((".hip", ".cpp", ".h")) and unit not in ("eggsim_fields.hip", "eggsim_host_fields.hip", "eggsim_host.h",
                                                                   "eggsim_device.h", "eggsim_group.cpp"):
            text = _read(CSRC, unit)
            assert "egg_field" not in text and "EggField" not in text and "field_state" not in text and "FieldState" not in text, unit
            assert "EGG_FD_" not in text, unit
    # the refusals, where the source states them: everything is checked before the first launch and before anything is written
    assert host.index("REJECT_IN_FLIGHT(h, name);") < host.index("return fail(")  # (the first refusal of a call)
    in_flight_messages_have_one_home()
    assert "opt_solver_order" not in host  # (either order)
    last_check = max(m.start() for m in re.finditer(r'return fail\(h, EGG_ERR_INVALID_ARGUMENT', host))
    assert last_check < host.index("hipLaunchKernelGGL(") and last_check < host.index("hipMemsetAsync(") and last_check < host.index("memset(out->count")
    assert host.count("h->stats.kernel_launches += 1;") == 1 and "h->stats." not in host.replace("h->stats.kernel_launches += 1;", "")
    for name in ("spec is NULL", "planes is NULL", "count is NULL", "svx and svy are given together or not at all", "unknown path",
                 "is not aligned to 4 bytes", "is not aligned to 8 bytes"):
        assert name in host, name
    group = _read(CSRC, "eggsim_group.cpp")
    twin = group[group.index("int egg_group_field("):]
    twin = twin[:twin.index("\n}\n")]
    assert "egg_field(g->h[k], spec," in twin and twin.index("return gfail(") < twin.index("memcpy(host_out->count")


def test_what_the_observers_share_has_one_home():
    units = sources()
    scan = units["eggsim_host_scan.hip"]
    in_flight_messages_have_one_home()
    assert sum(source.count("egg_rx_begin without egg_rx_end)") for source in units.values()) == 1
    assert sum(source.count("hipMemGetAddressRange(") for source in units.values()) == 1 and "hipMemGetAddressRange(" in scan
    for unit in OBSERVER_UNITS:
        assert "multiProcessorCount" not in units[unit], unit
        assert "REJECT_IN_FLIGHT(h, " in units[unit] and "refuse_in_flight" not in units[unit], unit
    assert "multiProcessorCount" in scan[scan.index("int grid_cap("):scan.index("bool device_range_fits(")]
    # the map from a batch to its atom is filled in one function, and every other unit asks that function
    assigned = [(unit, m.start()) for unit, source in units.items() for m in re.finditer(r"atom_of_batch\[[^;]*\] = ", source)]
    assert len(assigned) == 1 and assigned[0][0] == "eggsim_host_scan.hip", assigned
    start = scan.index("atom_of_batch(const egg_handle *h) {")
    assert start < assigned[0][1] < start + scan[start:].index("\n}\n")
    # the unit builder, the unit table and the id lists: defined once (the walk over a list's atoms as a template in the
    # header), named by no feature
    for line in ("void push_units(const Atom &a, int w, std::vector<EggScanUnit> &units) {", "int UnitTable::refresh(", "int covered_types(",
                 "int check_batch_ids(", "std::vector<int64_t> live_batch_ids(", "int upload_atoms(egg_handle *h) {"):
        assert sum(source.count(line) for unit, source in units.items() if not unit.endswith(".h")) == 1 and line in scan, line
    assert sum(source.count("int for_each_requested_atom(") for source in units.values()) == 1
    assert "int for_each_requested_atom(" in units["eggsim_host.h"]
    makefile = _read(CSRC, "Makefile")
    assert makefile.count("eggsim_host_scan.hip") == 1


def test_python_classes_have_the_methods_with_equal_parameter_lists():
    from egg_fluid_simulation_amd import SimulationGroup, SimulationHandler
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler
    from egg_fluid_simulation_amd.simulation_handler import Field, FieldTotals
    for cls in (SimulationHandler, SimulationGroup, ShardedSimulationHandler):
        sig = inspect.signature(cls.field)
        assert list(sig.parameters) == FIELD_PARAMS, cls.__name__
        assert (sig.parameters["types"].default, sig.parameters["velocity"].default, sig.parameters["path"].default) == ("both", False, "auto")
    sig = inspect.signature(SimulationHandler.field_to)
    assert list(sig.parameters) == FIELD_TO_PARAMS
    assert [sig.parameters[n].default for n in ("svx", "svy", "types", "path")] == [None, None, "both", "auto"]
    assert not hasattr(SimulationGroup, "field_to") and not hasattr(ShardedSimulationHandler, "field_to")
    assert Field._fields == ("count", "svx", "svy", "inside", "outside", "dropped", "units_tiled", "units_direct")
    assert FieldTotals._fields == Field._fields[3:]
    # a group calls its own entry point; a sharded handler asks its local handle and reduces once per plane and once for the totals
    assert SimulationGroup._PREFIX == "egg_group_" and SimulationGroup.field is SimulationHandler.field
    src = inspect.getsource(ShardedSimulationHandler.field)
    assert "self.local._field_planes(" in src and src.count("self._all_reduce_sum(") == 1 and "self.dist" not in src and "all_gather" not in src
    assert "for plane in (count, svx, svy, flat):" in src


def test_field_velocity_follows_the_stated_formula():
    from egg_fluid_simulation_amd import EggError
    from egg_fluid_simulation_amd.simulation_handler import Field
    count = np.array([[[2, 0]], [[0, 3]]], dtype=np.int32)
    svx = np.array([[[3, 0]], [[0, -65536 * 3]]], dtype=np.int64)
    svy = np.array([[[2 ** 53 - 1, 0]], [[0, 1]]], dtype=np.int64)
    v = Field(count, svx, svy, (2, 3), (0, 0), (0, 0), 2, 0).velocity()
    assert v.shape == (2, 1, 2, 2) and v.dtype == np.float64
    assert tuple(v[0, 0, 0]) == ((3.0 / 65536.0) / 2.0, (float(2 ** 53 - 1) / 65536.0) / 2.0) and tuple(v[1, 0, 1]) == (-1.0, (1.0 / 65536.0) / 3.0)
    assert np.isnan(v[0, 0, 1]).all() and np.isnan(v[1, 0, 0]).all()
    with pytest.raises(EggError, match="without velocity=True"):
        Field(count, None, None, (2, 3), (0, 0), (0, 0), 2, 0).velocity()


def test_the_wrappers_check_what_only_the_host_can():
    from egg_fluid_simulation_amd import EggError, SimulationGroup, SimulationHandler
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler
    good = dict(origin=(0.0, 0.0), cell=4.0, shape=(8, 8))
    for cls in (SimulationHandler, SimulationGroup, ShardedSimulationHandler):
        h = cls.__new__(cls)  # no device: the checks below come before any call into the library
        if cls is ShardedSimulationHandler:
            h.local = SimulationHandler.__new__(SimulationHandler)
        for bad, text in ((dict(origin=(0.0,)), r"origin must be \(x0, y0\)"), (dict(origin=None), r"origin must be \(x0, y0\)"),
                          (dict(shape=(8,)), r"shape must be \(nx, ny\)"), (dict(shape=8), r"shape must be \(nx, ny\)"),
                          (dict(shape=(8.0, 8)), "shape must be two integers"), (dict(shape=(True, 8)), "shape must be two integers"),
                          (dict(shape=(0, 8)), "nx and ny are at least 1"), (dict(shape=(8, -1)), "nx and ny are at least 1"),
                          (dict(shape=(1024, 1025)), "nx \\* ny at most 1048576"), (dict(origin=("a", 0.0)), "origin and cell must be numbers"),
                          (dict(cell=None), "origin and cell must be numbers"), (dict(cell=0.0), "cell must be finite and above 0"),
                          (dict(cell=-2.0), "cell must be finite and above 0"), (dict(cell=float("inf")), "cell must be finite and above 0"),
                          (dict(cell=float("nan")), "cell must be finite and above 0"), (dict(cell=5e-324), "with a finite inverse"),
                          (dict(origin=(float("nan"), 0.0)), "is not finite"), (dict(origin=(0.0, float("inf"))), "is not finite"),
                          (dict(types="none"), "field: types must be"), (dict(types=0), "field: types must be"), (dict(types=True), "field: types must be"),
                          (dict(path="fast"), "path must be 'auto' or 'direct'"), (dict(path=1), "path must be 'auto' or 'direct'")):
            with pytest.raises(EggError, match=text):
                h.field(**dict(good, **bad))
    h = SimulationHandler.__new__(SimulationHandler)

    class Plane:
        def __init__(self, ptr, dtype="torch.int32", n=128, contiguous=True):
            self.ptr, self.dtype, self.n, self.contiguous = ptr, dtype, n, contiguous

        def data_ptr(self):
            return self.ptr

        def numel(self):
            return self.n

        def is_contiguous(self):
            return self.contiguous
    big = Plane(4096, "torch.int64")
    for kw, text in ((dict(count=None), "count is required"), (dict(count=Plane(4096), svx=big), "svx and svy are given together"),
                     (dict(count=Plane(4096), svy=big), "svx and svy are given together"), (dict(count=Plane(4098)), "count is not aligned to 4 bytes"),
                     (dict(count=4097), "count is not aligned to 4 bytes"), (dict(count=Plane(4096), svx=Plane(4100, "torch.int64"), svy=big), "svx is not aligned to 8 bytes"),
                     (dict(count=Plane(4096), svx=big, svy=4100), "svy is not aligned to 8 bytes"), (dict(count=Plane(4096, "torch.int64")), "count must hold int32"),
                     (dict(count=Plane(4096), svx=Plane(4096, "torch.float64"), svy=big), "svx must hold int64"), (dict(count=Plane(4096, n=64)), "count must hold 2 x 8 x 8 elements, not 64"),
                     (dict(count=Plane(4096, contiguous=False)), "count must be contiguous"), (dict(count="x"), "an object with data_ptr\\(\\) or an address"),
                     (dict(count=0), "an object with data_ptr\\(\\) or an address"), (dict(count=Plane(4096), shape=(0, 1)), "nx and ny are at least 1")):
        with pytest.raises(EggError, match=text):
            h.field_to(**dict(good, **kw))
    spec = SimulationHandler._c_field_spec((1, 2.5), 3, (np.int64(4), 5), 2, "direct")
    assert (spec.x0, spec.y0, spec.cell, spec.nx, spec.ny, spec.type_mask, spec.path) == (1.0, 2.5, 3.0, 4, 5, 2, 1)
    assert SimulationHandler._c_field_spec([0, 0], 1.0, [1024, 1024], "yolk", "auto").type_mask == 2


def test_lua_has_the_method_and_the_header_prototype():
    lua = _read(ROOT, "egg_fluid_simulation_amd", "lua", "egg_fluid_simulation", "simulation_handler.lua")
    assert "function SimulationHandler:field(x0, y0, cell, nx, ny, options)" in lua and "function SimulationHandler:field_velocity(field, w, ix, iy)" in lua
    cdef = _prototypes(re.search(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S).group(1))
    header = _prototypes(_read(ROOT, "include", "eggsim.h"))
    assert cdef["egg_field"] == header["egg_field"] and "lib.egg_field(self._h, spec, planes, totals)" in lua
    assert "typedef struct { double x0, y0, cell; int32_t nx, ny, type_mask, path; } egg_field_spec;" in lua
    assert "typedef struct { int32_t *count; int64_t *svx, *svy; } egg_field_planes;" in lua
    assert "typedef struct { int64_t inside[2], outside[2], dropped[2]; int32_t units_tiled, units_direct; } egg_field_totals;" in lua
    assert "_field_max_cells = 1048576" in lua and "_field_velocity_scale = 65536" in lua and "_field_paths = { auto = 0, direct = 1 }" in lua
    assert "(w * field.ny + iy) * field.nx + ix" in lua and "(tonumber(field.svx[i]) / _field_velocity_scale) / n" in lua


def test_the_documents_describe_the_rule_and_the_limits():
    design = _read(ROOT, "DESIGN.md")
    assert design.index("### 2.9 Probes") < design.index("### 2.10 Fields") < design.index("## 3. Data layout in HBM")
    part = design[design.index("### 2.10 Fields"):design.index("## 3. Data layout in HBM")]
    for phrase in ("egg_field", "egg_field_to", "egg_group_field", "(x - x0) * inv", "STATELESS", "egg_field_count_kernel", "egg_field_velocity_kernel",
                   "EGG_FD_TILE_CELLS", "1,024", "push_units", "__ballot", "atomicAdd", "FLOAT atomics", "Integer adds have no order", "2^63",
                   "all_reduce", "no scratch", "VGPRs", "LDS", "NOT MEASURED", "profiles/r29_fields.md", "scripts/gpu_fields_bench.py",
                   "tests/field_model.py"):
        assert phrase in part, phrase
    limits = design[design.index("## 7. Limits"):design.index("## 8.")]
    assert limits.index("probes (`egg_probe`)") < limits.index("fields (`egg_field`)")
    for phrase in ("bin centres only", "no splat by radius", "no area or\n    mass plane", "No per-batch planes", "rides on a\n    collider",
                   "No `field_to` on a `SimulationGroup` or a `ShardedSimulationHandler`", "At most 2^20 cells", "refused while a step is in flight"):
        assert phrase in limits[limits.index("fields (`egg_field`)"):], phrase
    readme = _read(ROOT, "README.md")
    assert readme.index("* Probes (") < readme.index("* Fields (") < readme.index("* `bench.py`, `profiles/`")
    for phrase in ("field(origin, cell, shape, types, velocity, path)", "field_to(origin, cell, shape, count, svx, svy, types, path)",
                   "three more entry points for fields: 171", "profiles/r29_fields.md", "tests/field_model.py", "158 entry points -- 101 on one device",
                   "168 in all"):
        assert phrase in readme, phrase
    integration = _read(ROOT, "INTEGRATION.md")
    assert "168\nin all" in integration and "(the row \"fields\"): 171" in integration and "158 entry points" in integration
    assert "| fields (either order; one handle, device groups) | `egg_field`, `egg_field_to`, `egg_group_field` |" in integration
    for proto in PROTOS.values():
        assert proto in integration, proto
    for phrase in ("h.field((pan_x, pan_y), 4.0, (256, 256), velocity=True)", "handler:field(pan_x, pan_y, 4, 256, 256, { velocity = true })",
                   "Field(count, svx, svy, inside, outside, dropped, units_tiled, units_direct)"):
        assert phrase in integration, phrase
    assert os.path.exists(os.path.join(ROOT, "profiles", "r29_fields.md")) and os.path.exists(os.path.join(ROOT, "profiles", "r29_fields.jsonl"))
    assert os.path.exists(os.path.join(ROOT, "scripts", "gpu_fields_bench.py"))
    entry = _read(ROOT, "__graft_entry__.py")
    assert "h.field((x0, y0), cell, (nx, ny), velocity=True)" in entry and "smoke ok (fields)" in entry
