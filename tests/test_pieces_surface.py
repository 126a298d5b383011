"""The surface of the pieces (egg_pieces) as far as it can be checked without a device: the two entry
points, the constant and the two structs in the header and in the ctypes binding, field offsets included, the methods on
the three Python classes, the wrappers' own argument checks on a device-less instance, the Lua functions as text, the
kernels and that no step unit names them, and the documents."""
import ctypes as C
import inspect
import os
import re

import pytest

from conftest import ROOT
from scan_surface import in_flight_messages_have_one_home
from test_abi import _prototypes

CSRC = os.path.join(ROOT, "egg_fluid_simulation_amd", "csrc")
PROTOS = {
    "egg_pieces": "int egg_pieces(egg_handle *h, const egg_pieces_spec *spec, int64_t n_ids, const int64_t *ids,\n"
                  "               egg_piece_summary *out /* [n][2] */, int32_t *white_labels, int32_t *yolk_labels);",
    "egg_group_pieces": "int egg_group_pieces(egg_group *g, const egg_pieces_spec *spec, int64_t n_ids, const int64_t *ids, "
                        "egg_piece_summary *out /* [n][2] */);",
}
KERNELS = {"egg_pieces_wave_kernel": "EGG_WAVE", "egg_pieces_block_kernel": "EGG_PC_BLOCK"}
STEP_UNITS = ("eggsim_step.hip", "eggsim_packed.hip", "eggsim_relaxed.hip", "eggsim_relaxed_contacts.hip", "eggsim_relaxed_wire.hip",
              "eggsim_host_step.hip", "eggsim_host_relaxed.hip", "eggsim_host_relaxed_group.hip", "eggsim_host_relaxed_wire.hip",
              "eggsim_sensors.hip", "eggsim_probes.hip", "eggsim_fields.hip")


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_header_declares_the_entry_points_the_constant_and_the_structs():
    from egg_fluid_simulation_amd import _ffi
    text = _read(ROOT, "include", "eggsim.h")
    for name, proto in PROTOS.items():
        assert proto in text, name
        assert name in _ffi._SIGNATURES and name in _ffi.EXPORTED_SYMBOLS and name in _prototypes(text), name
    assert len(_ffi._SIGNATURES["egg_pieces"][1]) == 7 and len(_ffi._SIGNATURES["egg_group_pieces"][1]) == 5
    assert _ffi._SIGNATURES["egg_pieces"][1][:5] == _ffi._SIGNATURES["egg_group_pieces"][1]
    assert len(_ffi.EXPORTED_SYMBOLS) == 173
    assert re.search(r"typedef struct \{ double reach\[2\]; int32_t type_mask; int32_t reserved; \} egg_pieces_spec; +/\* 24 bytes \*/", text)
    assert re.search(r"typedef struct \{ int32_t n, pieces, largest, first, singles, dropped; int64_t sx, sy; \} egg_piece_summary; +/\* 40 bytes \*/", text)
    assert "#define EGG_PIECES_MAX_ATOM 4096" in text and _ffi.PIECES_MAX_ATOM == 4096
    S, R = _ffi.EggPiecesSpec, _ffi.EggPieceSummary
    assert C.sizeof(S) == 24 and [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("reach", 0), ("type_mask", 16), ("reserved", 20)]
    assert C.sizeof(R) == 40 and [(n, getattr(R, n).offset) for n, _ in R._fields_] == [
        ("n", 0), ("pieces", 4), ("largest", 8), ("first", 12), ("singles", 16), ("dropped", 20), ("sx", 24), ("sy", 32)]
    assert _ffi.PIECES_TYPES == {"white": 1, "yolk": 2, "both": 3}
    # the rule, where a C caller reads it
    for phrase in ("LINKED iff d2 <= L * L", "dx = x[i] - x[j]; dy = y[i] - y[j]; d2 = dx * dx + dy * dy; L = reach[type] * (radius[i] + radius[j])",
                   "no contraction", "false when anything in it is a NaN", "different batches or types are never linked",
                   "the lowest index in its piece", "the one with the lower label", "EGG_SENSOR_POSITION_SCALE", "reaches 2^53 in magnitude",
                   "(double)(largest - dropped)", "every live batch in egg_list_ids order", "an id may\n * repeat", "-1 for a particle of an atom that was not asked for",
                   "A call is STATELESS", "only kernel_launches moves, by at most 2 per call", "Everything is checked before anything is launched or written",
                   "EGG_ERR_UNKNOWN_ID for an unknown id", "EGG_ERR_UNSUPPORTED, naming the batch and\n * its count", "egg_step_begin or egg_rx_begin open",
                   "no path for larger atoms", "no neighbour grid", "labels on one\n * handle only", "tests/pieces_model.py",
                   "A failure on any handle writes nothing", "The records equal one handle's bit for bit"):
        assert phrase in text, phrase


def test_a_c_compiler_lays_the_structs_out_as_ctypes_does(tmp_path):
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    src = tmp_path / "pieces_layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "eggsim.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(egg_pieces_spec), offsetof(egg_pieces_spec, type_mask), '
                   'sizeof(egg_piece_summary), offsetof(egg_piece_summary, first), offsetof(egg_piece_summary, dropped), '
                   'offsetof(egg_piece_summary, sx), offsetof(egg_piece_summary, sy), sizeof(((egg_piece_summary *)0)->sx), '
                   '(int)EGG_PIECES_MAX_ATOM); return 0; }\n')
    exe = str(tmp_path / "pieces_layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)],
                   check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["24", "16", "40", "12", "20", "24", "32", "8", "4096"]


def test_the_kernels_exist_and_no_step_unit_names_them():
    kernels = _read(CSRC, "eggsim_pieces.hip")
    host_h = _read(CSRC, "eggsim_host.h")
    host = _read(CSRC, "eggsim_host_pieces.hip")
    device_h = _read(CSRC, "eggsim_device.h")
    for name, threads in KERNELS.items():
        assert 'extern "C" __global__ void __launch_bounds__(%s) %s(EggPiecesArgs A)' % (threads, name) in kernels, name
        assert 'extern "C" __global__ void %s(EggPiecesArgs A);' % name in host_h, name
        assert "hipLaunchKernelGGL(%s," % name in host, name
    for line in ("#define EGG_PC_MAX_ATOM 4096", "#define EGG_PC_WAVE_ATOM 512", "#define EGG_PC_BLOCK 256", "#define EGG_PC_LDS_PER_PARTICLE 32",
                 "struct EggPiecesTask {", "struct EggPieceSummary {", "struct EggPiecesArgs {"):
        assert line in device_h, line
    makefile = _read(CSRC, "Makefile")
    assert makefile.count("eggsim_pieces.hip") == 2 and makefile.count("eggsim_host_pieces.hip") == 1 and "-ffp-contract=off" in makefile
    # the rule in the order the header states; the atom in dynamic LDS; labels only fall; the finish in the same kernel; no
    # global atomics, no inline assembly, no single precision
    assert "extern __shared__" in kernels and "const double dx = xi[k] - p.x, dy = yi[k] - p.y;" in kernels and "const double d2 = dx * dx + dy * dy;" in kernels
    assert "const double L = reach * (ri[k] + rj);" in kernels and "const double L = reach * (ri[0] + ri[0]);" in kernels and kernels.count("l2 = L * L;") == 1
    assert "const bool linked = d2 <= l2;" in kernels and "for (int32_t q = label[m]; q < m; q = label[m]) m = q;" in kernels
    assert "__syncthreads_or(" in kernels and "atomicAdd(&size[label[i]], 1);" in kernels and "__ballot(lead)" in kernels and "pc_wave_max(" in kernels
    assert "fabs(fx) < EGG_SN_LIMIT && fabs(fy) < EGG_SN_LIMIT" in kernels and "* EGG_SN_SCALE" in kernels and "llrint(" in kernels
    assert "asm" not in kernels and "float" not in kernels and "A.out[task.slot] = rec;" in kernels
    for word in re.findall(r"atomic\w+\(&(\w+)", kernels):
        assert word in ("size", "tail"), word  # (LDS words only)
    assert "sizeof(egg_pieces_spec) == 24" in host and "sizeof(egg_piece_summary) == 40" in host and "EGG_PIECES_MAX_ATOM == EGG_PC_MAX_ATOM" in host
    assert "<= kLdsMax" in host and "constexpr int kGroupsPerCu = 16;" in host and "hipFuncAttributeMaxDynamicSharedMemorySize" in host
    assert "struct PiecesState {" in host and "atoms_gen" in host and "std::shared_ptr<egghost::PiecesState> pieces_state;" in host_h
    # nothing of a step knows about pieces -- and no unit but the pieces' own, the two shared headers and the group
    for unit in set(os.listdir(CSRC)) | set(STEP_UNITS):
        if unit.endswith((".hip", ".cpp", ".h")) and unit not in ("eggsim_pieces.hip", "eggsim_host_pieces.hip", "eggsim_host.h",
                                                                   "eggsim_device.h", "eggsim_group.cpp"):
            text = _read(CSRC, unit)
            assert "egg_pieces" not in text and "EggPiece" not in text and "pieces_state" not in text and "PiecesState" not in text, unit
            assert "EGG_PC_" not in text, unit
    # the refusals, where the source states them: everything is checked before the first launch and before anything is written
    assert host.index('REJECT_IN_FLIGHT(h, "egg_pieces");') < host.index("return fail(")  # (the first refusal of a call)
    in_flight_messages_have_one_home()
    assert "opt_solver_order" not in host  # (either order)
    last_check = max(m.start() for m in re.finditer(r"return fail\(h, EGG_ERR_(INVALID_ARGUMENT|UNKNOWN_ID|UNSUPPORTED), \"egg_pieces: (?!the device)", host))
    assert last_check < host.index("hipLaunchKernelGGL(") and last_check < host.index("hipMemsetAsync(") and last_check < host.index("memcpy(out,")
    assert last_check < host.index("upload_atoms(") and host.index("memcpy(out,") > host.index("hipStreamSynchronize(W.stream)")
    assert host.count("h->stats.kernel_launches += 1;") == 1 and "h->stats." not in host.replace("h->stats.kernel_launches += 1;", "")
    for name in ("spec is NULL", "out is NULL", 'check_batch_ids(h, "egg_pieces", n_ids, ids)', "it is finite and above 0", "type_mask %d",
                 "an atom holds at most %d"):
        assert name in host, name
    assert 'return fail(h, EGG_ERR_UNKNOWN_ID, "%s: no batch with id `%lld`", name, (long long)ids[i]);' in _read(CSRC, "eggsim_host_scan.hip")
    assert host.index("check_batch_ids(") < host.index("reach[%d] = %g")  # (an unknown id is refused before the reach and the mask)
    group = _read(CSRC, "eggsim_group.cpp")
    twin = group[group.index("int egg_group_pieces("):]
    twin = twin[:twin.index("\n}\n")]
    assert "egg_pieces(g->h[k], spec," in twin and "route_to_owners<" in twin and twin.rindex("return gfail(") < twin.index("route_to_owners<")
    route = group[group.index("int route_to_owners("):]
    route = route[:route.index("\n}\n")]
    assert "r.owner != (int)k" in route and route.rindex("return gfail(") < route.index("memcpy(out,")  # (written after every handle answered)


def test_python_classes_have_the_methods():
    from egg_fluid_simulation_amd import SimulationGroup, SimulationHandler
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler
    from egg_fluid_simulation_amd.simulation_handler import PieceSummary
    for cls in (SimulationHandler, SimulationGroup, ShardedSimulationHandler):
        sig = inspect.signature(cls.pieces)
        assert list(sig.parameters) == ["self", "ids", "reach", "types"], cls.__name__
        assert [sig.parameters[n].default for n in ("ids", "reach", "types")] == [None, None, "both"]
        sig = inspect.signature(cls.is_whole)
        assert list(sig.parameters) == ["self", "id", "reach", "types"] and [sig.parameters[n].default for n in ("reach", "types")] == [None, "both"]
    sig = inspect.signature(SimulationHandler.piece_labels)
    assert list(sig.parameters) == ["self", "reach", "types"] and [sig.parameters[n].default for n in ("reach", "types")] == [None, "both"]
    assert not hasattr(SimulationGroup, "piece_labels") and not hasattr(ShardedSimulationHandler, "piece_labels")
    assert PieceSummary._fields == ("n", "pieces", "largest", "first", "singles", "dropped", "x", "y")
    # a group calls its own entry point; a sharded handler asks its local handle and reduces one int64 table once
    assert SimulationGroup._PREFIX == "egg_group_" and SimulationGroup.pieces is SimulationHandler.pieces
    assert SimulationGroup.is_whole is SimulationHandler.is_whole is ShardedSimulationHandler.is_whole
    src = inspect.getsource(ShardedSimulationHandler.pieces)
    assert "self.local._piece_table(" in src and src.count("self._owner_table(") == 1 and "self.dist" not in src and "np.int64" in src
    assert "all_gather" not in src


def test_the_wrappers_check_what_only_the_host_can_and_derive_the_centroid():
    from egg_fluid_simulation_amd import EggError, SimulationGroup, SimulationHandler, default_configs
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler
    from egg_fluid_simulation_amd.simulation_handler import PieceSummary
    white, yolk = default_configs()
    for cls in (SimulationHandler, SimulationGroup, ShardedSimulationHandler):
        h = cls.__new__(cls)  # no device: the checks below come before any call into the library
        h._white_config, h._yolk_config = dict(white), dict(yolk)
        for kw, text in ((dict(reach=0.0), "reach must be finite and above 0"), (dict(reach=-1.0), "reach must be finite and above 0"),
                         (dict(reach=float("nan")), "reach must be finite and above 0"), (dict(reach=float("inf")), "reach must be finite and above 0"),
                         (dict(reach=(1.0, 0.0)), "reach must be finite and above 0"), (dict(reach=(1.0,)), "reach must be None, a number or"),
                         (dict(reach=(1.0, 2.0, 3.0)), "reach must be None, a number or"), (dict(reach="far"), "reach must be None, a number or"),
                         (dict(reach=(1.0, None)), "reach must be None, a number or"), (dict(types="none"), "pieces: types must be"),
                         (dict(types=0), "pieces: types must be"), (dict(types=True), "pieces: types must be")):
            with pytest.raises(EggError, match=text):
                h.pieces(**kw)
            with pytest.raises(EggError, match=text):
                h.is_whole(1, **kw)
        if cls is not ShardedSimulationHandler:
            with pytest.raises(EggError, match="ids must be None or a list of batch ids"):
                h.pieces(ids=[1, "a"])
            with pytest.raises(EggError, match="ids must be None or a list of batch ids"):
                h.pieces(ids=7)
        # the default reach: per type max(collision_overlap_factor, cohesion_interaction_distance_factor) of the config
        spec = h._c_pieces_spec(None, "both")
        assert (spec.reach[0], spec.reach[1], spec.type_mask) == (2.0, 3.0, 3)
        h._white_config["collision_overlap_factor"] = 4.5
        h._yolk_config["cohesion_interaction_distance_factor"] = 0.5
        spec = h._c_pieces_spec(None, "yolk")
        assert (spec.reach[0], spec.reach[1], spec.type_mask) == (4.5, yolk["collision_overlap_factor"], 2)
        spec = h._c_pieces_spec(1.25, 1)
        assert (spec.reach[0], spec.reach[1], spec.type_mask) == (1.25, 1.25, 1)
        spec = h._c_pieces_spec((1, 2.5), "both")
        assert (spec.reach[0], spec.reach[1]) == (1.0, 2.5)
    h = SimulationHandler.__new__(SimulationHandler)
    h._white_config, h._yolk_config = dict(white), dict(yolk)
    with pytest.raises(EggError, match="piece_labels: reach must be finite and above 0"):
        h.piece_labels(0.0)
    with pytest.raises(EggError, match="piece_labels: types must be"):
        h.piece_labels(None, "none")
    table = [[(3, 2, 2, 0, 1, 0, 6 * 65536, -3 * 65536), (0, 0, 0, 0, 0, 0, 0, 0)], [(2, 1, 2, 0, 0, 2, 0, 0), (1, 1, 1, 0, 1, 0, 2 ** 53 - 1, 1)]]
    got = SimulationHandler._piece_summaries(table)
    assert got == [(PieceSummary(3, 2, 2, 0, 1, 0, 3.0, -1.5), None),
                   (PieceSummary(2, 1, 2, 0, 0, 2, None, None), PieceSummary(1, 1, 1, 0, 1, 0, float(2 ** 53 - 1) / 65536.0, 1.0 / 65536.0))]


def test_lua_has_the_functions_and_the_header_prototype():
    lua = _read(ROOT, "egg_fluid_simulation_amd", "lua", "egg_fluid_simulation", "simulation_handler.lua")
    for line in ("function SimulationHandler:pieces(ids, reach, types)", "function SimulationHandler:is_whole(id, reach, types)",
                 "function SimulationHandler:piece_labels(reach, types)"):
        assert line in lua, line
    cdef = _prototypes(re.search(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S).group(1))
    header = _prototypes(_read(ROOT, "include", "eggsim.h"))
    assert cdef["egg_pieces"] == header["egg_pieces"]
    assert "lib.egg_pieces(self._h, spec, n, c_ids, out, nil, nil)" in lua and "lib.egg_pieces(self._h, spec, 0, nil, out, white, yolk)" in lua
    assert "typedef struct { double reach[2]; int32_t type_mask; int32_t reserved; } egg_pieces_spec;" in lua
    assert "typedef struct { int32_t n, pieces, largest, first, singles, dropped; int64_t sx, sy; } egg_piece_summary;" in lua
    assert "_pieces_max_atom = 4096" in lua and "(tonumber(rec.sx) / _sensor_scale) / kept" in lua
    assert "math.max(self._white_config.collision_overlap_factor, self._white_config.cohesion_interaction_distance_factor)" in lua


def test_the_documents_describe_the_rule_and_the_limits():
    design = _read(ROOT, "DESIGN.md")
    assert design.index("### 2.10 Fields") < design.index("### 2.11 Pieces") < design.index("## 3. Data layout in HBM")
    part = design[design.index("### 2.11 Pieces"):design.index("## 3. Data layout in HBM")]
    for phrase in ("egg_pieces", "egg_group_pieces", "d2 <= L * L", "reach[type] * (radius[i] + radius[j])", "STATELESS", "egg_pieces_wave_kernel",
                   "egg_pieces_block_kernel", "EGG_PIECES_MAX_ATOM", "4,096", "pointer jumping", "broadcast", "__ballot", "all_reduce", "no scratch",
                   "VGPRs", "LDS", "NOT MEASURED", "profiles/r30_pieces.md", "scripts/gpu_pieces_bench.py", "tests/pieces_model.py",
                   "| 0 | 0.89 | 0.89 |", "| 5 | 1.42 | 3.87 |", "| 120 | 1.28 | 1.91 |", "relaxed order", "The wall experiment"):
        assert phrase in part, phrase
    limits = design[design.index("## 7. Limits"):design.index("## 8.")]
    assert limits.index("fields (`egg_field`)") < limits.index("pieces (`egg_pieces`)")
    for phrase in ("4,096 particles", "EGG_ERR_UNSUPPORTED", "A path for larger atoms: not built", "A neighbour grid in LDS", "not built",
                   "Labels on one handle only", "refused while a step is in flight"):
        assert phrase in limits[limits.index("pieces (`egg_pieces`)"):], phrase
    readme = _read(ROOT, "README.md")
    assert readme.index("* Fields (") < readme.index("* Pieces (") < readme.index("* `bench.py`, `profiles/`")
    for phrase in ("pieces(ids, reach, types)", "piece_labels(reach, types)", "is_whole(id, reach, types)", "two more entry points for pieces: 173",
                   "profiles/r30_pieces.md", "tests/pieces_model.py", "158 entry points -- 101 on one device", "168 in all",
                   "three more entry points for fields: 171"):
        assert phrase in readme, phrase
    integration = _read(ROOT, "INTEGRATION.md")
    assert "168\nin all" in integration and "(the row \"fields\"): 171" in integration and "(the row \"pieces\"): 173" in integration
    assert "| pieces (either order; one handle, device groups) | `egg_pieces`, `egg_group_pieces` |" in integration
    for proto in PROTOS.values():
        assert " ".join(proto.split()) in " ".join(integration.split()), proto
    for phrase in ("h.pieces()", "h.is_whole(egg)", "handler:is_whole(egg)", "PieceSummary(n, pieces, largest, first, singles, dropped, x, y)"):
        assert phrase in integration, phrase
    assert os.path.exists(os.path.join(ROOT, "profiles", "r30_pieces.md")) and os.path.exists(os.path.join(ROOT, "profiles", "r30_pieces.jsonl"))
    assert os.path.exists(os.path.join(ROOT, "scripts", "gpu_pieces_bench.py"))
    entry = _read(ROOT, "__graft_entry__.py")
    assert "h.pieces(None, reach)" in entry and "h.piece_labels(reach)" in entry and "smoke ok (pieces)" in entry
