"""The cover (egg_cover) as far as its surface can be checked without a device: the prototypes and
structs of include/eggsim_cover.h against the ctypes binding and a C compiler, the kernels and their host side as text, the
group's merge helper compiled alone under a sanitizer, the methods of the three Python classes, the sharded merge on two gloo
ranks with stub planes, the Lua wrapper as text and the documents."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cover_model as cm
from conftest import ROOT
from scan_surface import in_flight_messages_have_one_home, sources
from test_abi import _prototypes

CSRC = os.path.join(ROOT, "egg_fluid_simulation_amd", "csrc")
PROTOS = {
    "egg_cover": "int egg_cover(egg_handle *h, const egg_cover_spec *spec, const egg_cover_planes *host_planes, egg_cover_totals *totals);",
    "egg_cover_to": "int egg_cover_to(egg_handle *h, const egg_cover_spec *spec, const egg_cover_planes *device_planes, egg_cover_totals *totals);",
    "egg_group_cover": "int egg_group_cover(egg_group *g, const egg_cover_spec *spec, const egg_cover_planes *host_planes, egg_cover_totals *totals);",
}
TOTALS = ["inside", "outside", "dropped", "hits", "covered", "covered_both", "covered_any", "units_lanes", "units_wave", "units_direct", "reserved"]


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_header_and_binding_agree_on_the_entry_points_and_the_structs():
    from egg_fluid_simulation_amd import _ffi
    text = _read(ROOT, "include", "eggsim_cover.h")
    for name, proto in PROTOS.items():
        assert proto in text, name
        assert name in _ffi._COVER_SIGNATURES and name in _ffi.COVER_SYMBOLS and name in _prototypes(text), name
    # the binding covers the whole of this header; the four tables are disjoint: 173 + 2 + 3 + 3 entry points
    assert sorted(_prototypes(text)) == _ffi.COVER_SYMBOLS == sorted(PROTOS)
    tables = (_ffi.EXPORTED_SYMBOLS, _ffi.IMPULSE_SYMBOLS, _ffi.MEASURE_SYMBOLS, _ffi.COVER_SYMBOLS)
    assert sum(len(t) for t in tables) == len(set().union(*tables)) == 181
    assert len(set(map(tuple, (_ffi._COVER_SIGNATURES[name][1] for name in PROTOS)))) == 1  # (the three calls take the same arguments)
    main = _read(ROOT, "include", "eggsim.h")
    assert main.count('#include "eggsim_cover.h"') == 1 and main.index('#include "eggsim_cover.h"') > main.index('#include "eggsim_measure.h"')
    if os.path.exists(_ffi.LIB_PATH):
        lib = _ffi.load()
        assert all(hasattr(lib, name) and getattr(lib, name).argtypes == _ffi._COVER_SIGNATURES[name][1] for name in _ffi.COVER_SYMBOLS)
    entry = _read(ROOT, "__graft_entry__.py")
    assert "_ffi.COVER_SYMBOLS" in entry and "_COVER_SIGNATURES.items()" in _read(ROOT, "egg_fluid_simulation_amd", "_ffi.py")
    # the structs, field for field
    P, L, T = _ffi.EggCoverSpec, _ffi.EggCoverPlanes, _ffi.EggCoverTotals
    assert C.sizeof(P) == 48 and [(n, getattr(P, n).offset) for n, _ in P._fields_] == [
        ("x0", 0), ("y0", 8), ("cell", 16), ("scale", 24), ("nx", 32), ("ny", 36), ("type_mask", 40), ("path", 44)]
    assert C.sizeof(L) == 16 and [n for n, _ in L._fields_] == ["cover", "owner"]
    assert C.sizeof(T) == 112 and [n for n, _ in T._fields_] == TOTALS and T.covered_both.offset == 80 and T.units_lanes.offset == 96
    assert "typedef struct { double x0, y0, cell, scale; int32_t nx, ny, type_mask, path; } egg_cover_spec;" in text
    assert "typedef struct { int32_t *cover; int32_t *owner; } egg_cover_planes;" in text
    body = re.search(r"typedef struct \{([^}]*)\} egg_cover_totals;", text).group(1)
    assert re.findall(r"([a-z_]+)(?:\[2\])?\s*[,;]", re.sub(r"int(64|32)_t", "", body)) == TOTALS
    for line in ("#define EGG_COVER_MAX_CELLS (1 << 20)", "#define EGG_COVER_MAX_SPAN 64.0",
                 "enum { EGG_COVER_PATH_AUTO = 0, EGG_COVER_PATH_DIRECT = 1, EGG_COVER_PATH_LANES = 2, EGG_COVER_PATH_WAVE = 3 };",
                 "enum { EGG_COVER_OWNER_KEYS = 0x100 };"):
        assert line in text, line
    assert (_ffi.COVER_MAX_CELLS, _ffi.COVER_MAX_SPAN) == (cm.MAX_CELLS, cm.MAX_SPAN) == (1 << 20, 64.0)
    assert _ffi.COVER_PATHS == {"auto": 0, "direct": 1, "lanes": 2, "wave": 3} and _ffi.COVER_OWNER_KEYS == 0x100
    # the rule, where a C caller reads it
    for phrase in ("inv = 1.0 / cell", "cx(ix) = x0 + ((double)ix + 0.5) * cell", "R = scale * radius", "!(isfinite(x) && isfinite(y))", "!(R >= 0.0)",
                   "!(R * inv <= EGG_COVER_MAX_SPAN)", "fxl = ((x - R) - x0) * inv", "fxh = ((x + R) - x0) * inv",
                   "fxh < 0.0 || fxl >= (double)nx || fyh < 0.0 || fyl >= (double)ny", "d2 = dx*dx + dy*dy", "d2 <= R*R",
                   "[floor(max(fxl, 0)), floor(min(fxh, nx-1))]", "clamped in double", "!(max(|x0|, |y0|, |x0 + nx*cell|, |y0 + ny*cell|) <= cell * 0x1p20)",
                   "preset to 0xFFFFFFFF", "does not fit 31 bits", "NOT ADDITIVE", "Everything is checked before anything is launched or written",
                   "egg_step_begin or egg_rx_begin\n * open", "tests/cover_model.py", "no contraction", "by at most 2 per call",
                   "no anti-aliased or fractional coverage", "no mass or velocity planes by disc", "no per-batch planes beyond owner",
                   "no cover that rides on a collider"):
        assert phrase in text, phrase


def test_a_c_compiler_lays_the_structs_out_as_ctypes_does(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    src = tmp_path / "cover_layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "eggsim.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(egg_cover_spec), sizeof(egg_cover_planes), '
                   'sizeof(egg_cover_totals), offsetof(egg_cover_spec, scale), offsetof(egg_cover_spec, path), offsetof(egg_cover_planes, owner), '
                   'offsetof(egg_cover_totals, covered_both), offsetof(egg_cover_totals, units_direct), (int)EGG_COVER_MAX_CELLS, '
                   '(int)EGG_COVER_PATH_WAVE); return 0; }\n')
    exe = str(tmp_path / "cover_layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)],
                   check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["48", "16", "112", "24", "44", "8", "80", "104", "1048576", "3"]


def test_the_kernels_exist_and_nothing_else_names_them():
    kernels, host, host_h, device_h = (_read(CSRC, f) for f in ("eggsim_cover.hip", "eggsim_host_cover.hip", "eggsim_host.h", "eggsim_device.h"))
    assert 'extern "C" __global__ void __launch_bounds__(64) egg_cover_kernel(EggCoverArgs A)' in kernels
    assert 'extern "C" __global__ void __launch_bounds__(EGG_CV_FINISH_THREADS) egg_cover_finish_kernel(EggCoverFinishArgs A)' in kernels
    for name, args in (("egg_cover_kernel", "EggCoverArgs"), ("egg_cover_finish_kernel", "EggCoverFinishArgs")):
        assert 'extern "C" __global__ void %s(%s A);' % (name, args) in host_h and "hipLaunchKernelGGL(%s," % name in host
    assert host.count("hipLaunchKernelGGL(") == 2  # (at most two launches per call)
    for line in ("#define EGG_CV_TILE_CELLS 4096", "#define EGG_CV_LANES_CELLS 784", "#define EGG_CV_WAVE_CELLS 784", "#define EGG_CV_MAX_SPAN 64.0", "#define EGG_CV_TOTALS 16",
                 "struct EggCoverArgs {", "struct EggCoverFinishArgs {"):
        assert line in device_h, line
    makefile = _read(CSRC, "Makefile")
    assert makefile.count("eggsim_cover.hip") == 2 and makefile.count("eggsim_host_cover.hip") == 1 and "-ffp-contract=off" in makefile
    assert "../../include/eggsim_cover.h" in makefile and "eggsim_cover_merge.h" in makefile
    # the rule in the header's order; static LDS within 64 KB; integer atomics only; no inline assembly, no single precision
    for line in ("const double R = A.scale * radius;", "if (!(isfinite(x) && isfinite(y)) || !(R >= 0.0) || !(R * A.inv <= EGG_CV_MAX_SPAN)) return CV_DROPPED;",
                 "const double fxl = ((x - R) - A.x0) * A.inv, fxh = ((x + R) - A.x0) * A.inv;",
                 "if (fxh < 0.0 || fxl >= (double)A.nx || fyh < 0.0 || fyl >= (double)A.ny) return CV_OUTSIDE;",
                 "d.ix0 = (int)floor(fmax(fxl, 0.0));", "d.ix1 = (int)floor(fmin(fxh, (double)(A.nx - 1)));",
                 "(A.x0 + ((double)ix + 0.5) * A.cell) - x", "const double d2 = dx * dx + dy * dy;", "return d2 <= R * R;",
                 "__shared__ int32_t t_cover[EGG_CV_TILE_CELLS];", "const bool fits = rect <= (long long)A.tile_cells;",
                 "const bool by_lanes = fits && foot <= A.lanes_cells;", "const bool tile = by_lanes || (fits && foot <= A.wave_cells);", "atomicMin(&g_owner[c], id);"):
        assert line in kernels, line
    assert "asm" not in kernels and "float" not in kernels and kernels.count("cv_classify(A,") == 2
    assert set(re.findall(r"\b(atomic\w+)\(", kernels)) == {"atomicAdd", "atomicMin"}
    assert not re.findall(r"\bA\.(x|y|radius)\[w\]\[[^\]]+\] *=[^=]", kernels) and not re.search(r"\b(X|Y|Rad)\[[^\]]+\] *=[^=]", kernels)  # (read-only)
    assert 4096 * 4 <= 64 * 1024
    # the host side: the ABI's constants are the kernel's, the checks come before the first launch and before anything is
    # written, only kernel_launches moves; the new units name nothing of another observer and share the host layer
    for line in ("sizeof(egg_cover_spec) == 48", "sizeof(egg_cover_totals) == 112", "sizeof(egg_cover_planes) == 16", "EGG_COVER_MAX_SPAN == EGG_CV_MAX_SPAN",
                 "struct CoverState {", "T.refresh(h, name, types, true)", "units_by_key.by_key = true;", "device_range_fits(h, out->cover, bytes)", "hipMemsetAsync(A.owner, 0xFF, bytes, W.stream)",
                 "spec->cell * 0x1p20", 'grid_cap(h, n_units, kWavesPerCu, "EGGSIM_COVER_WAVES_PER_CU")', '"EGGSIM_COVER_TILE_CELLS"', '"EGGSIM_COVER_LANES_CELLS"', '"EGGSIM_COVER_WAVE_CELLS"'):
        assert line in host, line
    assert host.index("REJECT_IN_FLIGHT(h, name);") < host.index("return fail(")  # (the first refusal of a call)
    in_flight_messages_have_one_home()
    assert "std::shared_ptr<egghost::CoverState> cover_state;" in host_h and "opt_solver_order" not in host
    last_check = max(m.start() for m in re.finditer(r"return fail\(h, EGG_ERR_INVALID_ARGUMENT", host))
    for first in ("hipLaunchKernelGGL(", "hipMemsetAsync(", "memset(", "upload_atoms(", "hipMemcpyAsync("):
        assert last_check < host.index(first), first
    assert host.count("h->stats.kernel_launches += 2;") == 1 and "h->stats." not in host.replace("h->stats.kernel_launches += 2;", "")
    # the labels of the owner plane are the shared builder's spare word: no second enumeration of the units in this unit
    scan = _read(CSRC, "eggsim_host_scan.hip")
    assert "push_units(" not in host and "by_key ? h->batches[(size_t)a.batch].key : h->batches[(size_t)a.batch].id" in scan
    assert "const uint32_t id = (uint32_t)un.reserved;" in kernels
    merge = _read(CSRC, "eggsim_cover_merge.h")
    for unit in (kernels, host, merge):
        for word in ("egg_field", "EggField", "EGG_FD_", "field_state", "FieldState", "egg_measure", "EGG_MS_", "egg_probe", "egg_pieces", "EGG_PC_",
                     "egg_impulse", "EGG_IM_", "hipMemGetAddressRange", "multiProcessorCount", "refuse_in_flight", "a step is in flight"):
            assert word not in unit, word
        assert "sensor" not in unit.lower()
    for unit, text in sources().items():
        if unit not in ("eggsim_cover.hip", "eggsim_host_cover.hip", "eggsim_host.h", "eggsim_device.h", "eggsim_group.cpp", "eggsim_cover_merge.h"):
            assert "egg_cover" not in text and "EggCover" not in text and "cover_state" not in text and "EGG_CV_" not in text and "eggcover" not in text, unit
    group = _read(CSRC, "eggsim_group.cpp")
    twin = group[group.index("int egg_group_cover("):]
    twin = twin[:twin.index("\n}\n")]
    assert "egg_cover(g->h[k], spec ? &keyed : nullptr," in twin and "keyed.path |= EGG_COVER_OWNER_KEYS;" in twin and twin.count("eggcover::merge_planes(") == 1 and twin.count("eggcover::recount(") == 1
    assert twin.rindex("return gfail(") < twin.index("memcpy(host_planes->cover")  # (written after every handle answered)
    assert "hip" not in merge.lower() and "#include \"" not in merge  # (plain C++: it compiles alone)


MERGE_MAIN = r"""
#include <cstdio>
#include <vector>
#include "eggsim_cover_merge.h"
int main() {
    const size_t cells = 6, words = 2 * cells;
    std::vector<int32_t> cover(words, 0);
    std::vector<uint32_t> owner(words, 0xFFFFFFFFu);
    // handle A holds the scene's batches 5 and 2, handle B the batches 3 and 0x7FFFFFFF (the largest key an owner word takes)
    const int32_t a_cover[] = {1, 0, 2, 0, 0, 7,  0, 1, 0, 0, 3, 0}, a_owner[] = {5, -1, 2, -1, -1, 5,  -1, 2, -1, -1, 5, -1};
    const int32_t b_cover[] = {1, 0, 1, 4, 0, 0,  0, 1, 0, 0, 0, 0}, b_owner[] = {3, -1, 3, 0x7FFFFFFF, -1, -1,  -1, 3, -1, -1, -1, -1};
    eggcover::merge_planes(words, cover.data(), owner.data(), a_cover, a_owner);
    eggcover::merge_planes(words, cover.data(), owner.data(), b_cover, b_owner);
    eggcover::merge_planes(words, cover.data(), nullptr, b_cover, nullptr);   // (no owner asked for: the planes alone)
    eggcover::merge_planes(0, nullptr, nullptr, nullptr, nullptr);
    int64_t covered[2], both, any;
    eggcover::recount(cells, cover.data(), covered, &both, &any);
    for (size_t q = 0; q < words; ++q) std::printf("%d ", (int)cover[q]);
    for (size_t q = 0; q < words; ++q) std::printf("%d ", (int)(int32_t)owner[q]);
    std::printf("%lld %lld %lld %lld\n", (long long)covered[0], (long long)covered[1], (long long)both, (long long)any);
    eggcover::recount(0, nullptr, covered, &both, &any);
    return (int)(covered[0] + covered[1] + both + any);
}
"""


def test_the_merge_helper_alone_under_a_sanitizer(tmp_path):
    """the group's merge and recount, compiled stand-alone with a main of its own under address and undefined-behaviour
    sanitizers on the host: added planes, the unsigned minimum over keys with -1 as the largest value, no owner, nothing at all"""
    compiler = shutil.which("g++") or shutil.which("clang++")
    if compiler is None:
        pytest.skip("no C++ compiler")
    src = tmp_path / "cover_merge_main.cpp"
    src.write_text(MERGE_MAIN)
    exe = str(tmp_path / "cover_merge_main")
    subprocess.run([compiler, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, "-o", exe, str(src)], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    got = [int(v) for v in run.stdout.split()]
    assert got[:12] == [3, 0, 4, 8, 0, 7, 0, 3, 0, 0, 3, 0]
    assert got[12:24] == [3, -1, 2, 0x7FFFFFFF, -1, 5, -1, 2, -1, -1, 5, -1]  # (min(5, 3); min(2, 3); any key beats "none")
    assert got[24:] == [4, 2, 0, 6]


def test_python_classes_have_the_methods():
    from egg_fluid_simulation_amd import EggError, SimulationGroup, SimulationHandler, _ffi
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler
    from egg_fluid_simulation_amd.simulation_handler import Cover, CoverTotals
    params = ["self", "origin", "cell", "shape", "scale", "types", "owner", "path"]
    for cls in (SimulationHandler, SimulationGroup, ShardedSimulationHandler):
        sig = inspect.signature(cls.cover).parameters
        assert list(sig) == params and [sig[k].default for k in params[4:]] == [1.0, "both", False, "auto"], cls.__name__
    assert list(inspect.signature(SimulationHandler.cover_to).parameters) == ["self", "origin", "cell", "shape", "cover", "owner", "scale", "types", "path"]
    assert not hasattr(SimulationGroup, "cover_to") and not hasattr(ShardedSimulationHandler, "cover_to")
    assert SimulationGroup._PREFIX == "egg_group_" and SimulationGroup.cover is SimulationHandler.cover
    src = inspect.getsource(ShardedSimulationHandler.cover)
    assert src.count("self._all_reduce_sum(") == 1 and src.count("self._all_reduce_min(") == 1 and "self.dist" not in src and "COVER_OWNER_KEYS" in src and "self.local._cover_planes(" in src
    assert Cover._fields == ("cover", "owner", "cell", "inside", "outside", "dropped", "hits", "covered", "covered_both", "covered_any",
                             "units_lanes", "units_wave", "units_direct") and CoverTotals._fields == Cover._fields[2:]
    c = Cover(None, None, 1.5, (1, 2), (0, 0), (0, 0), (30, 8), (10, 4), 3, 11, 0, 0, 0)
    assert c.area() == (22.5, 9.0, 6.75, 24.75) and c.depth() == (3.0, 2.0)
    spec = SimulationHandler._c_cover_spec((1.0, 2.0), 0.5, (3, 4), 12.0, "yolk", "wave")
    assert (spec.x0, spec.y0, spec.cell, spec.scale, spec.nx, spec.ny, spec.type_mask, spec.path) == (1.0, 2.0, 0.5, 12.0, 3, 4, 2, 3)
    for kw, text in ((dict(shape=(0, 4)), "nx and ny are at least 1"), (dict(shape=(1 << 10, (1 << 10) + 1)), "nx \\* ny at most 1048576"),
                     (dict(cell=0.0), "cell must be finite and above 0"), (dict(origin=(0.0,)), "origin must be"), (dict(scale=0.0), "scale must be finite and above 0"),
                     (dict(scale=float("inf")), "scale must be finite"), (dict(types="none"), "types must be"), (dict(path="fast"), "path must be")):
        with pytest.raises(EggError, match=text):
            SimulationHandler._c_cover_spec(**dict(dict(origin=(0.0, 0.0), cell=1.0, shape=(4, 4), scale=1.0, types="both", path="auto"), **kw))
    assert _ffi.COVER_SYMBOLS == ["egg_cover", "egg_cover_to", "egg_group_cover"]


# ------------------------------------------------------------------------------------------------ the sharded merge, on stubs
GRID = (0.0, 0.0, 1.0, 6, 4)
# global id -> (white, yolk) particles (x, y, radius); ranks own {1, 3} and {2}: rank 1's local id 1 is the global 2
SCENE = {1: ([(2.5, 1.5, 1.2)], [(2.5, 1.5, 0.5)]), 2: ([(3.5, 1.5, 1.2), (0.5, 3.5, 0.2)], [(3.5, 2.5, 0.5)]), 3: ([(3.5, 2.5, 1.6)], [(9.0, 9.0, 1.0)])}
OWNED = ({1: 2, 3: 1}, {2: 1})  # per rank: global id -> local id (rank 0 got its batches in the other order)


def _arrays(batches):
    out = [[[], [], [], []], [[], [], [], []]]
    for key, (white, yolk) in batches:
        for w, spots in ((0, white), (1, yolk)):
            for x, y, r in spots:
                for f, v in enumerate((x, y, r, key)):
                    out[w][f].append(v)
    return [[np.array(out[w][f], dtype=np.float64) for w in (0, 1)] for f in range(4)]


class _StubLocal:
    """what ShardedSimulationHandler.cover asks of its handle: the planes and totals of the batches this rank owns, labelled
    by their keys -- the global ids -- where the spec carries EGG_COVER_OWNER_KEYS and by the handle's own ids otherwise"""

    def __init__(self, local_id):
        self.local_id = local_id

    def _cover_planes(self, spec, owner):
        from egg_fluid_simulation_amd import _ffi
        keyed = bool(spec.path & _ffi.COVER_OWNER_KEYS)
        x, y, r, b = _arrays([(gid if keyed else lid, SCENE[gid]) for gid, lid in sorted(self.local_id.items())])
        got = cm.cover((spec.x0, spec.y0, spec.cell, spec.nx, spec.ny), spec.scale, x, y, r, b, spec.type_mask, owner)
        assert spec.path & ~_ffi.COVER_OWNER_KEYS == 0
        t = _ffi.EggCoverTotals()
        for w in (0, 1):
            t.inside[w], t.outside[w], t.dropped[w], t.hits[w], t.covered[w] = (got[k][w] for k in (2, 3, 4, 5, 6))
        t.covered_both, t.covered_any, t.units_lanes = got[7], got[8], 1
        return got[0], got[1], t


def _stub_rank(rank, world, port, q):
    import sys
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch
    import torch.distributed as dist
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        calls = []

        class Counting:
            ReduceOp = dist.ReduceOp

            @staticmethod
            def all_reduce(t, op):
                calls.append(str(op))
                return dist.all_reduce(t, op=op)
        sh = ShardedSimulationHandler.__new__(ShardedSimulationHandler)
        sh.world, sh.rank, sh.dist, sh.torch, sh.device = world, rank, Counting, torch, "cpu"
        sh.local_id = dict(OWNED[rank])
        sh.local = _StubLocal(sh.local_id)
        got = sh.cover(GRID[:2], GRID[2], GRID[3:], 1.0, owner=True)
        n_owned = len(calls)
        plain = sh.cover(GRID[:2], GRID[2], GRID[3:], 1.0, "white")
        q.put((rank, "ok", dict(owned=tuple(got), calls=calls[:n_owned], plain=tuple(plain), plain_calls=len(calls) - n_owned)))
    except Exception:
        import traceback
        q.put((rank, "error: " + traceback.format_exc(), None))
    finally:
        dist.destroy_process_group()


def test_sharded_merge_on_two_gloo_ranks_with_stub_planes():
    """the owner merge (local ids to global ones, none the largest) and the recount of covered* equal the single-table
    answer, with exactly two collectives -- one without the owner plane"""
    import socket

    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_stub_rank, args=(r, 2, port, q)) for r in (0, 1)]
    for p in procs:
        p.start()
    res = {}
    for _ in procs:
        rank, outcome, results = q.get(timeout=120)
        assert outcome == "ok", outcome
        res[rank] = results
    for p in procs:
        p.join(30)
        assert p.exitcode == 0
    x, y, r, b = _arrays(sorted(SCENE.items()))
    want = cm.cover(GRID, 1.0, x, y, r, b, "both", True)
    white = cm.cover(GRID, 1.0, x, y, r, b, "white", False)
    assert want[7] > 0 and set(np.unique(want[1])) == {-1, 1, 2, 3} and want[3] == (0, 1)
    for rank in (0, 1):
        got = res[rank]["owned"]
        assert cm.same(got[:2] + got[3:10], want) and got[2] == GRID[2] and got[10:] == (2, 0, 0), rank
        assert len(res[rank]["calls"]) == 2 and sorted(c.split(".")[-1] for c in res[rank]["calls"]) == ["MIN", "SUM"], res[rank]["calls"]
        plain = res[rank]["plain"]
        assert cm.same(plain[:2] + plain[3:10], white) and res[rank]["plain_calls"] == 1, rank
    # covered is not additive: the ranks' own counts add up to more than the merged plane holds
    own = [cm.cover(GRID, 1.0, *_arrays([(g, SCENE[g]) for g in sorted(OWNED[rank])]))[6][0] for rank in (0, 1)]
    assert sum(own) > want[6][0]


def test_a_one_rank_object_needs_no_process_group():
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler
    sh = ShardedSimulationHandler.__new__(ShardedSimulationHandler)
    sh.world, sh.rank, sh.dist, sh.torch, sh.device = 1, 0, None, None, "cpu"
    sh.local_id = {1: 3, 2: 2, 3: 1}
    sh.local = _StubLocal(sh.local_id)
    got = sh.cover(GRID[:2], GRID[2], GRID[3:], owner=True)
    x, y, r, b = _arrays(sorted(SCENE.items()))
    want = cm.cover(GRID, 1.0, x, y, r, b, "both", True)
    assert cm.same(tuple(got)[:2] + tuple(got)[3:10], want) and set(np.unique(got.owner)) == {-1, 1, 2, 3}


def test_lua_has_the_function_and_the_header_prototype():
    lua = _read(ROOT, "egg_fluid_simulation_amd", "lua", "egg_fluid_simulation", "simulation_handler.lua")
    assert "function SimulationHandler:cover(x0, y0, cell, nx, ny, options)" in lua and "ffi.cdef(_cover_decls)" in lua
    decls = re.search(r"local _cover_decls = \[==\[(.*?)\]==\]", lua, flags=re.S).group(1)
    header = _read(ROOT, "include", "eggsim_cover.h")
    assert _prototypes(decls) == {"egg_cover": _prototypes(header)["egg_cover"]}
    for struct in ("egg_cover_spec", "egg_cover_planes", "egg_cover_totals"):
        pattern = r"typedef struct \{([^}]*)\} %s;" % struct
        assert " ".join(re.search(pattern, decls).group(1).split()) == " ".join(re.search(pattern, header).group(1).split()), struct
    assert "lib.egg_cover(self._h, spec, planes, totals)" in lua and "_cover_paths = { auto = 0, direct = 1, lanes = 2, wave = 3 }" in lua
    assert "_cover_max_cells = 1048576" in lua and "area = { covered[1] * a, covered[2] * a, both * a, any * a }" in lua


def test_the_documents_describe_the_call():
    design = _read(ROOT, "DESIGN.md")
    assert design.index("### 2.13 Measures") < design.index("### 2.14 Cover") < design.index("## 3. Data layout in HBM")
    part = design[design.index("### 2.14 Cover"):design.index("## 3. Data layout in HBM")]
    for phrase in ("egg_cover", "egg_cover_to", "egg_group_cover", "egg_cover_kernel", "egg_cover_finish_kernel", "tests/cover_model.py",
                   "scripts/gpu_cover_bench.py", "profiles/r35_cover.md", "all_reduce", "EGG_CV_TILE_CELLS", "EGG_CV_LANES_CELLS", "LANES", "WAVE", "DIRECT",
                   "at most two launches", "not additive", "eggsim_cover_merge.h", "no anti-aliased or fractional coverage", "no cover that rides on a collider",
                   "make resource-usage"):
        assert phrase in part, phrase
    readme, integration = _read(ROOT, "README.md"), _read(ROOT, "INTEGRATION.md")
    assert readme.index("* Measures (") < readme.index("* Cover (") < readme.index("* `bench.py`, `profiles/`")
    assert "three more entry points for the cover: 181" in " ".join(readme.split()) and "profiles/r35_cover.md" in readme
    assert "(the row \"cover\"): 181" in integration and "h.cover(" in integration and "handler:cover(" in integration and "h.cover_to(" in integration
    assert "| cover (either order; one handle, device groups) | `egg_cover`, `egg_cover_to`, `egg_group_cover` |" in integration
    for proto in PROTOS.values():
        assert " ".join(proto.split()) in " ".join(integration.split()), proto
    for phrase in ("no anti-aliased or fractional coverage", "no mass or velocity planes by disc", "no cover that rides on a collider", "no `cover_to` on groups or ranks"):
        assert phrase in " ".join(integration.split()), phrase
    entry = _read(ROOT, "__graft_entry__.py")
    assert "h.cover(" in entry and "smoke ok (cover)" in entry
    profile = _read(ROOT, "profiles", "r35_cover.md")
    for phrase in ("cover_to", "downloads", "lanes", "wave", "direct", "VGPRs", "bench.py"):
        assert phrase in profile, phrase
