"""The touches (egg_touches) as far as their surface can be checked without a device: the prototypes and
structs of include/eggsim_touch.h against the ctypes binding, the kernels and their host side as text, the methods of the three
Python classes, the merge of record tables, the Lua wrapper as text, the documents and the Makefile lists."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import touch_model as tm
from conftest import ROOT
from test_abi import _prototypes

CSRC = os.path.join(ROOT, "egg_fluid_simulation_amd", "csrc")
PROTOS = {
    "egg_touches": "int egg_touches(egg_handle *h, const egg_touch_spec *spec, int64_t n_ids, const int64_t *ids, int64_t cap, egg_touch_record *out,\n"
                   "                int64_t *n_out);",
    "egg_touches_of": "int egg_touches_of(egg_handle *h, const egg_touch_spec *spec, int64_t n_queries, const egg_touch_query *queries, const double *x,\n"
                      "                   const double *y, const double *r, int64_t cap, egg_touch_record *out, int64_t *n_out);",
    "egg_group_touches": "int egg_group_touches(egg_group *g, const egg_touch_spec *spec, int64_t n_ids, const int64_t *ids, int64_t cap, egg_touch_record *out,\n"
                         "                      int64_t *n_out);",
}


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_header_and_binding_agree_on_the_entry_points_and_the_structs():
    from egg_fluid_simulation_amd import _ffi
    text = _read(ROOT, "include", "eggsim_touch.h")
    for name, proto in PROTOS.items():
        assert proto in text, name
        assert name in _ffi._TOUCH_SIGNATURES and name in _ffi.TOUCH_SYMBOLS and name in _prototypes(text), name
    # the binding covers the whole of this header; the five tables are disjoint: 173 + 2 + 3 + 3 + 3 entry points
    assert sorted(_prototypes(text)) == _ffi.TOUCH_SYMBOLS == sorted(PROTOS)
    tables = (_ffi.EXPORTED_SYMBOLS, _ffi.IMPULSE_SYMBOLS, _ffi.MEASURE_SYMBOLS, _ffi.COVER_SYMBOLS, _ffi.TOUCH_SYMBOLS)
    assert sum(len(t) for t in tables) == len(set().union(*tables)) == 184
    assert _ffi._TOUCH_SIGNATURES["egg_touches"][1] == _ffi._TOUCH_SIGNATURES["egg_group_touches"][1]
    main = _read(ROOT, "include", "eggsim.h")
    assert main.count('#include "eggsim_touch.h"') == 1 and main.index('#include "eggsim_touch.h"') > main.index('#include "eggsim_cover.h"')
    if os.path.exists(_ffi.LIB_PATH):
        lib = _ffi.load()
        assert all(hasattr(lib, name) and getattr(lib, name).argtypes == _ffi._TOUCH_SIGNATURES[name][1] for name in _ffi.TOUCH_SYMBOLS)
    entry = _read(ROOT, "__graft_entry__.py")
    assert "_ffi.TOUCH_SYMBOLS" in entry and "_TOUCH_SIGNATURES.items()" in _read(ROOT, "egg_fluid_simulation_amd", "_ffi.py")
    # the structs, field for field
    P, Q, R = _ffi.EggTouchSpec, _ffi.EggTouchQuery, _ffi.EggTouchRecord
    assert C.sizeof(P) == 24 and [(n, getattr(P, n).offset) for n, _ in P._fields_] == [("reach", 0), ("type_mask", 16), ("flags", 20)]
    assert C.sizeof(Q) == 16 and [(n, getattr(Q, n).offset) for n, _ in Q._fields_] == [("key", 0), ("type", 8), ("count", 12)]
    assert C.sizeof(R) == 40 and [(n, getattr(R, n).offset) for n, _ in R._fields_] == [
        ("slot", 0), ("pairs", 4), ("particles", 8), ("dropped", 12), ("other", 16), ("sx", 24), ("sy", 32)]
    for line in ("typedef struct { double reach[2]; int32_t type_mask, flags; } egg_touch_spec;", "typedef struct { int64_t key; int32_t type, count; } egg_touch_query;",
                 "typedef struct { int32_t slot, pairs, particles, dropped; int64_t other, sx, sy; } egg_touch_record;",
                 "enum { EGG_TOUCH_BY_KEYS = 1 };", "#define EGG_TOUCH_MAX_QUERY (1 << 20)"):
        assert line in text, line
    assert _ffi.TOUCH_BY_KEYS == 1 and _ffi.TOUCH_MAX_QUERY == 1 << 20 and tm.SCALE == _ffi.SENSOR_POSITION_SCALE
    from egg_fluid_simulation_amd.simulation_handler import _TOUCH_RECORD
    assert _TOUCH_RECORD.itemsize == 40 and [(n, _TOUCH_RECORD.fields[n][1]) for n in _TOUCH_RECORD.names] == [
        (n, getattr(R, n).offset) for n, _ in R._fields_]
    # the rule, where a C caller reads it, in the words of the model; and the limits at the end
    for phrase in ("dx = xa - xb; dy = ya - yb; d2 = dx*dx + dy*dy", "L = reach[type] * (ra + rb)", "d2 <= L * L", "anything in it is a NaN", "no contraction",
                   "collision_overlap_factor", "L:1632-1653", "never across types and never inside the query's own batch", "2 i + w",
                   "EGG_TOUCH_BY_KEYS", "distinct particles b of the other batch", "count\n *              in pairs and add nothing to the sums",
                   "q(xa) + q(xb)", "sx / (2 * (pairs - dropped)) / 65536", "ordered by (slot, other)", "additive over any split", "ask the reverse direction",
                   "*n_out is ALWAYS the number of records", "nothing is written to `out`", "naming both numbers", "Everything is checked before anything is launched or written",
                   "egg_step_begin or egg_rx_begin open", "EGG_ERR_UNKNOWN_ID", "tests/touch_model.py", "-1 excludes nothing", "a radius that is not finite",
                   "Handle 0 refuses a bad\n * spec; nothing is written before every handle has answered"):
        assert phrase in text, phrase
    limits = text[text.index(" * Limits:"):text.index("#define EGG_TOUCH_MAX_QUERY")]
    for phrase in ("same type only, no white-yolk touches", "colliders touch nothing", "no touch that rides on a collider", "no per-particle\n * partner lists",
                   "no depth of overlap", "must fit 31 bits", "no touches_to on a device tensor"):
        assert phrase in limits, phrase
    for name, doc in (("SCALE", 65536.0), ("LIMIT", 2.0 ** 53)):
        assert getattr(tm, name) == doc


def test_the_kernels_and_their_host_side_as_text():
    kernel = _read(CSRC, "eggsim_touches.hip")
    host = _read(CSRC, "eggsim_host_touches.hip")
    device = _read(CSRC, "eggsim_device.h")
    head = _read(CSRC, "eggsim_host.h")
    for name in ("egg_touch_gather_kernel", "egg_touch_kernel"):
        assert re.search(r'extern "C" __global__ void __launch_bounds__\(64\) %s\(' % name, kernel), name
        assert 'extern "C" __global__ void %s(' % name in head and "hipLaunchKernelGGL(%s," % name in host
    for define in ("#define EGG_TC_ROUND 64", "#define EGG_TC_FIRST_RECORDS 256", "#define EGG_TC_OWN (EGG_SN_UNIT / EGG_WAVE)"):
        assert define in device, define
    # FP64 and integers only, no LDS, one global atomic beside the developer's counter; the rule in the model's order
    assert "float " not in kernel and "__shared__" not in kernel and kernel.count("atomicAdd(") == 2 and "atomicAdd(A.cursor, 1)" in kernel
    for phrase in ("const double dx = d.x - px[j], dy = d.y - py[j];", "const double d2 = dx * dx + dy * dy;", "const double L = reach * (d.r + pr[j]);",
                   "if (!(d2 <= L * L)) continue;", "__ballot(pairs != 0) == 0ull", "at >= 0 && at < A.cap", "q.key != label", "llrint("):
        assert phrase in kernel, phrase
    # the cull's argument stands above the test
    cull = kernel[kernel.index("// THE CULL."):kernel.index("__device__ __forceinline__ bool tc_apart(")]
    for phrase in ("may only skip what the rule rejects", "rounding being monotone", "fl(dx * dx) <= fl(d2)", "fl(L * L) <= fl(Lmax * Lmax)",
                   "A comparison with a NaN is false", "touches nothing", "g0 * g0 > L2"):
        assert phrase in cull, phrase
    # the host: the shared layer, everything checked first, the one re-run, the merge
    for phrase in ("REJECT_IN_FLIGHT(h, name);", "UnitTable units, units_by_key;", "grid_cap(h, T.n_units, kWavesPerCu", "for_each_requested_atom(h, \"egg_touches\"",
                   "check_batch_ids(h, \"egg_touches\"", "size_t records = EGG_TC_FIRST_RECORDS;", "for (int run = 0; run < 2; ++run)", "sizeof(egg_touch_record) == 40",
                   "the answer holds %lld records, the buffer %lld", "h->stats.kernel_launches += 2;", "std::isfinite(r[i])"):
        assert phrase in host, phrase
    assert "touch_state" in head and "struct TouchState;" in head
    group = _read(CSRC, "eggsim_group.cpp")
    body = group[group.index("int egg_group_touches("):group.index("int egg_group_get_collider_grips(")]
    for phrase in ("keyed.flags |= EGG_TOUCH_BY_KEYS;", "egg_export_batch(", "egg_touches(g->h[k], &keyed", "egg_touches_of(g->h[k], &keyed", "group_alive(g, ids[i])"):
        assert phrase in body, phrase
    make = _read(CSRC, "Makefile")
    src = re.search(r"^SRC = (.*)$", make, flags=re.M).group(1).split()
    hdr = re.search(r"^HDR = (.*)$", make, flags=re.M).group(1).split()
    usage = re.search(r"^resource-usage:\n\tfor f in ([^;]*);", make, flags=re.M).group(1).split()
    assert "eggsim_touches.hip" in src and "eggsim_host_touches.hip" in src and "../../include/eggsim_touch.h" in hdr and "eggsim_touches.hip" in usage
    assert "-ffp-contract=off" in make


def test_the_three_classes_have_the_methods():
    from egg_fluid_simulation_amd import SimulationHandler
    from egg_fluid_simulation_amd.group import SimulationGroup
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler
    from egg_fluid_simulation_amd.simulation_handler import Touch
    assert Touch._fields == ("other", "pairs", "particles", "dropped", "x", "y")
    for cls in (SimulationHandler, SimulationGroup, ShardedSimulationHandler):
        assert list(inspect.signature(cls.touch_table).parameters) == ["self", "ids", "reach", "types"], cls
        assert list(inspect.signature(cls.touches).parameters) == ["self", "ids", "reach", "types"], cls
        assert list(inspect.signature(cls.touching).parameters) == ["self", "a", "b", "reach", "types"], cls
        assert list(inspect.signature(cls.touches_of).parameters) == ["self", "discs", "reach", "types", "key"], cls
        assert inspect.signature(cls.touches_of).parameters["types"].default == "white" and inspect.signature(cls.touches_of).parameters["key"].default == -1
        assert not hasattr(cls, "touches_to")
    assert SimulationHandler._TOUCH_OF_FLAGS == 0 and SimulationGroup._TOUCH_OF_FLAGS == ShardedSimulationHandler._TOUCH_OF_FLAGS == 1
    assert "_touch_table" in ShardedSimulationHandler.__dict__ and "_touch_table" not in SimulationGroup.__dict__
    sharded = inspect.getsource(ShardedSimulationHandler._touch_table)
    for phrase in ("export_batch", "st[0], st[1], st[7]", "_all_gather_rows", "_touch_of_table", "TOUCH_BY_KEYS", "_touch_gather"):
        assert phrase in sharded, phrase


def test_tables_of_several_handles_merge_into_one():
    """the rows of one (entry, type, other) are added, int64 sums wrap, and the order is (entry, type, other)"""
    from egg_fluid_simulation_amd import SimulationHandler
    a = np.array([[1, 0, 7, 2, 2, 0, 2 ** 62, -5], [0, 1, 3, 1, 1, 1, 0, 0]], dtype=np.int64)
    b = np.array([[1, 0, 7, 3, 1, 1, 2 ** 62, 9], [0, 0, 9, 1, 1, 0, 10, 20]], dtype=np.int64)
    with np.errstate(over="ignore"):
        got = SimulationHandler._merge_touch_tables([a, b, np.zeros((0, 8), dtype=np.int64)])
    assert got.tolist() == [[0, 0, 9, 1, 1, 0, 10, 20], [0, 1, 3, 1, 1, 1, 0, 0], [1, 0, 7, 5, 3, 1, -2 ** 63, 4]]
    assert SimulationHandler._merge_touch_tables([]).shape == (0, 8)
    lists = SimulationHandler._touch_lists(got, 2)
    assert [[tuple(t) for t in side] for side in lists[0]] == [[(9, 1, 1, 0, 5.0 / 65536.0, 10.0 / 65536.0)], [(3, 1, 1, 1, None, None)]]
    assert lists[1][0][0][:4] == (7, 5, 3, 1) and lists[1][1] == []
    # the model splits the same way: the records of a scene's halves add up to the whole's
    import test_touch_model as tt
    batches = tt.random_scene(4, n_batches=8, most=30, spread=30.0)
    parts = tm.labelled(tt.particles_of(batches))
    queries = [(i + 1, w, parts[w]["x"][parts[w]["label"] == i + 1], parts[w]["y"][parts[w]["label"] == i + 1], parts[w]["radius"][parts[w]["label"] == i + 1])
               for i in range(8) for w in (0, 1)]
    whole = tm.records_of(queries, parts, (1.1, 1.1))
    halves = []
    for keep in (lambda k: k % 2 == 0, lambda k: k % 2 == 1):  # (every other PARTICLE: a split inside the batches)
        half = tuple({f: v[[k for k in range(v.size) if keep(k)]] for f, v in p.items()} for p in parts)
        halves.append(np.array(tm.records_of(queries, half, (1.1, 1.1)), dtype=np.int64).reshape(-1, 8))
    assert whole and SimulationHandler._merge_touch_tables(halves).tolist() == [list(r) for r in whole]


def test_the_lua_wrapper_as_text():
    lua = _read(ROOT, "egg_fluid_simulation_amd", "lua", "egg_fluid_simulation", "simulation_handler.lua")
    for phrase in ("function SimulationHandler:touches(ids, reach, types)", "function SimulationHandler:touching(a, b, reach, types)",
                   "function SimulationHandler:touches_of(discs, reach, types, key)", "ffi.cdef(_touch_decls)", "lib.egg_touches(self._h, spec, n, c_ids, cap, out, n_out)",
                   "lib.egg_touches_of(self._h, spec, 1, query, x, y, r, cap, out, n_out)", "collision_overlap_factor",
                   "typedef struct { double reach[2]; int32_t type_mask, flags; } egg_touch_spec;",
                   "typedef struct { int32_t slot, pairs, particles, dropped; int64_t other, sx, sy; } egg_touch_record;",
                   "(tonumber(rec.sx) / (2 * kept)) / _sensor_scale", "tonumber(n_out[0]) > cap"):
        assert phrase in lua, phrase
    decls = lua[lua.index("local _touch_decls = [==["):lua.index("ffi.cdef(_touch_decls)")]
    header = _read(ROOT, "include", "eggsim_touch.h")
    squash = lambda t: re.sub(r"\s+", " ", t)
    for name in ("egg_touches", "egg_touches_of"):
        assert squash(PROTOS[name]) in squash(decls) and squash(PROTOS[name]) in squash(header), name


def test_the_documents():
    readme, integration, design = (_read(ROOT, name) for name in ("README.md", "INTEGRATION.md", "DESIGN.md"))
    profile = _read(ROOT, "profiles", "r36_touches.md")
    assert "* Touches (`touches(ids, reach, types)`" in readme and "three more entry points for touches: 184" in readme
    assert "three more entry points for the cover: 181" in readme and readme.index("* Touches (") > readme.index("* Cover (")
    assert "`profiles/r36_touches.md`" in readme and "NOT MEASURED" in readme[readme.index("* Touches ("):]
    assert "| touches (either order; one handle, device groups) | `egg_touches`, `egg_touches_of`, `egg_group_touches` |" in integration
    assert '(the row "touches"): 184' in integration and "**Touches (which eggs touch which, how much and where; either order).**" in integration
    section = design[design.index("### 2.15 Touches ("):design.index("## 3. Data layout in HBM")]
    for phrase in ("**The rule**", "**Rounds.**", "**The scan**", "**The cull**", "**The record buffer**", "**Groups and ranks.**", "**Limits.**",
                   "EGG_TC_FIRST_RECORDS = 256", "fl(g * g) > fl(Lmax * Lmax)", "monotonicity of rounding", "run once more", "L:1632-1653",
                   "no white-yolk touches", "Colliders touch nothing", "No per-particle\npartner lists", "no depth of overlap", "31 bits",
                   "No `touches_to` on a device tensor", "NOT MEASURED"):
        assert phrase in section, phrase
    assert design.index("### 2.15 Touches (") > design.index("### 2.14 Cover (")
    for phrase in ("NOT MEASURED", "config 3 (704,512 particles)", "16,384 separate batches", "alternating runs", "egg_touch_kernel", "| 228 |"):
        assert phrase in profile, phrase
