"""The impulses (egg_impulse) as far as they can be checked without a device: the numpy model
tests/impulse_model.py against a hand table over every action, flag and region kind and against the corner cases of the rule,
the refusals, the structs in the header and in the ctypes binding, the methods of the three Python classes and the Lua
wrapper as text.  tests/test_gpu_impulses.py holds the device against the same table."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import impulse_model as im
from conftest import ROOT
from test_abi import _prototypes

S16 = 65536

# name -> spots (white, yolk), velocities (white, yolk) before, inverse masses (white, yolk), the list, and by hand: the
# velocities after and per record (count, sdvx, sdvy, skipped) x (white, yolk)
CASES = {
    # a disc with a particle exactly on its edge (3, 4): d2 = 25 <= 25, it is in
    "kick_disc": dict(
        spots=([(0.0, 0.0), (3.0, 4.0), (6.0, 0.0)], [(0.0, 0.0)]), v=([(0.0, 0.0)] * 3, [(1.0, 1.0)]), inv_mass=([1.0] * 3, [1.0]),
        records=[("kick", ("disc", 0.0, 0.0, 5.0), 1.5, -2.0)],
        after=([(1.5, -2.0), (1.5, -2.0), (0.0, 0.0)], [(2.5, -1.0)]),
        results=[((2, 1), (3 * S16, 3 * S16 // 2), (-4 * S16, -2 * S16), (0, 0))]),
    # the same with the linear weight: on the edge w == 0, so the particle is counted with dv = 0
    "kick_disc_linear": dict(
        spots=([(0.0, 0.0), (3.0, 4.0), (6.0, 0.0)], [(0.0, 2.5)]), v=([(0.0, 0.0)] * 3, [(0.0, 0.0)]), inv_mass=([1.0] * 3, [1.0]),
        records=[("kick", ("disc", 0.0, 0.0, 5.0), 1.5, -2.0, dict(linear=True))],
        after=([(1.5, -2.0), (0.0, 0.0), (0.0, 0.0)], [(0.75, -1.0)]),
        results=[((2, 1), (3 * S16 // 2, 3 * S16 // 4), (-2 * S16, -S16), (0, 0))]),
    # a blast passes the particle at its own centre by: neither changed nor counted nor skipped; s < 0 sucks
    "blast_flat": dict(
        spots=([(0.0, 0.0), (3.0, 4.0), (0.0, -2.0)], [(100.0, 100.0)]), v=([(7.0, 7.0), (0.0, 0.0), (0.0, 1.0)], [(0.0, 0.0)]),
        inv_mass=([1.0] * 3, [1.0]),
        records=[("blast", ("disc", 0.0, 0.0, 10.0), 0.0, 0.0, 10.0), ("blast", ("disc", 0.0, 0.0, 10.0, "white"), 0.0, 0.0, -5.0)],
        after=([(7.0, 7.0), (3.0, 4.0), (0.0, -4.0)], [(0.0, 0.0)]),
        results=[((2, 0), (6 * S16, 0), (-2 * S16, 0), (0, 0)), ((2, 0), (-3 * S16, 0), (S16, 0), (0, 0))]),
    # a swirl about (1, 1) on the side x >= 0 of a half-plane: the sign of collider spin (counter-clockwise for omega > 0)
    "swirl_half_plane": dict(
        spots=([(2.0, 1.0), (-1.0, 0.0), (1.0, 3.0)], [(0.0, 1.0)]), v=([(0.0, 0.0)] * 3, [(0.5, 0.5)]), inv_mass=([1.0] * 3, [1.0]),
        records=[("swirl", ("half_plane", 2.0, 0.0, 0.0), 1.0, 1.0, 2.0)],
        after=([(0.0, 2.0), (0.0, 0.0), (-4.0, 0.0)], [(0.5, -1.5)]),
        results=[((2, 1), (-4 * S16, 0), (2 * S16, -2 * S16), (0, 0))]),
    # brake(0, 0, 1) in a turned box stops exactly; half a brake towards (2, 0) afterwards, for the yolk only
    "brake_box": dict(
        spots=([(1.0, 1.0), (3.0, 0.0)], [(0.0, 0.5)]), v=([(3.7, -1.3), (3.7, -1.3)], [(-8.0, 6.0)]), inv_mass=([1.0] * 2, [1.0]),
        records=[("brake", ("box", 0.0, 0.0, 2.0, 1.0, 1.0, 1.0), 0.0, 0.0, 1.0), ("brake", ("box", 0.0, 0.0, 2.0, 1.0, 0.0, "yolk"), 2.0, 0.0, 0.5)],
        after=([(0.0, 0.0), (3.7, -1.3)], [(1.0, 0.0)]),
        results=[((1, 1), (-242483, 8 * S16), (85197, -6 * S16), (0, 0)), ((0, 1), (0, S16), (0, 0), (0, 0))]),
    # a capsule with both weights: d = 2 of R = 4 gives 0.5, times the inverse masses 0.5, 2, 1
    "kick_capsule_linear_by_inv_mass": dict(
        spots=([(5.0, 2.0), (-2.0, 0.0), (12.0, 0.0), (5.0, 5.0)], [(5.0, 0.0)]), v=([(0.0, 0.0)] * 4, [(0.0, 0.0)]),
        inv_mass=([0.5, 2.0, 1.0, 1.0], [0.25]),
        records=[("kick", ("capsule", 0.0, 0.0, 10.0, 0.0, 4.0), 8.0, 0.0, dict(linear=True, by_inv_mass=True))],
        after=([(2.0, 0.0), (8.0, 0.0), (4.0, 0.0), (0.0, 0.0)], [(2.0, 0.0)]),
        results=[((3, 1), (14 * S16, 2 * S16), (0, 0), (0, 0))]),
    # a kick of 1e300 is skipped and leaves the velocity; the record after it still finds the old velocity
    "skipped": dict(
        spots=([(0.0, 0.0)], [(0.0, 0.0)]), v=([(1.0, 2.0)], [(3.0, 4.0)]), inv_mass=([1.0], [1.0]),
        records=[("kick", ("disc", 0.0, 0.0, 1.0), 1e300, 0.0), ("kick", ("disc", 0.0, 0.0, 1.0, "yolk"), 1.0, 1.0)],
        after=([(1.0, 2.0)], [(4.0, 5.0)]),
        results=[((0, 0), (0, 0), (0, 0), (1, 1)), ((0, 1), (0, S16), (0, S16), (0, 0))]),
}


# every type of a batch has at least two particles: a far one that nothing reaches keeps its velocity (9, 9)
FAR, FAR_V = (-1e4, -1e4), (9.0, 9.0)
for _case in CASES.values():
    for _t in (0, 1):
        if len(_case["spots"][_t]) < 2:
            _case["spots"][_t].append(FAR)
            _case["v"][_t].append(FAR_V)
            _case["inv_mass"][_t].append(1.0)
            _case["after"][_t].append(FAR_V)


def run_case(case, records=None):
    xs = [np.array([p[0] for p in s], dtype=np.float64) for s in case["spots"]]
    ys = [np.array([p[1] for p in s], dtype=np.float64) for s in case["spots"]]
    vx = [np.array([p[0] for p in s], dtype=np.float64) for s in case["v"]]
    vy = [np.array([p[1] for p in s], dtype=np.float64) for s in case["v"]]
    ims = [np.array(m, dtype=np.float64) for m in case["inv_mass"]]
    bid = [np.ones(len(s), dtype=np.int64) for s in case["spots"]]
    return im.apply(case["records"] if records is None else records, xs, ys, vx, vy, ims, bid)


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_case(name):
    case = CASES[name]
    nvx, nvy, results = run_case(case)
    for w in (0, 1):
        assert [tuple(p) for p in zip(nvx[w].tolist(), nvy[w].tolist())] == case["after"][w], (name, w)
    assert results == case["results"], name


def test_the_table_covers_every_action_flag_and_region_kind():
    canon = [r for case in CASES.values() for r in im.canonical(case["records"])]
    assert {r[0] for r in canon} == set(im.ACTIONS) and {r[1][0] for r in canon} == {"half_plane", "disc", "box", "capsule"}
    assert any(r[4] for r in canon) and any(r[5] for r in canon) and {r[1][1] for r in canon} == {1, 2, 3}


def test_brake_stops_exactly_and_order_matters():
    case = CASES["brake_box"]
    nvx, nvy, _ = run_case(case, [("brake", ("disc", 1.0, 1.0, 0.1), 0.0, 0.0, 1.0)])
    assert nvx[0][0] == 0.0 and nvy[0][0] == 0.0 and not np.signbit(nvx[0][0]) and not np.signbit(nvy[0][0])
    disc = ("disc", 0.0, 0.0, 50.0)
    kick, brake = ("kick", disc, 2.0, 0.0), ("brake", disc, 0.0, 0.0, 0.5)
    a = run_case(case, [kick, brake])
    b = run_case(case, [brake, kick])
    assert a[0][0][0] == (3.7 + 2.0) + 0.5 * (0.0 - (3.7 + 2.0)) and b[0][0][0] == (3.7 + 0.5 * (0.0 - 3.7)) + 2.0
    assert a[0][0][0] != b[0][0][0] and a[2] != b[2]


def test_a_nan_position_is_in_nothing_and_id_filters_by_batch():
    nan = float("nan")
    xs, ys = [np.array([nan, 0.0, 0.0]), np.array([0.0])], [np.array([0.0, nan, 0.0]), np.array([0.0])]
    zeros = [np.zeros(3), np.zeros(1)]
    ones = [np.ones(3), np.ones(1)]
    bid = [np.array([1, 1, 2]), np.array([2])]
    for region in (("disc", 0.0, 0.0, 1e9), ("half_plane", 1.0, 0.0, -1e9), ("box", 0.0, 0.0, 1e9, 1e9, 0.0), ("capsule", -1.0, 0.0, 1.0, 0.0, 1e9)):
        nvx, nvy, res = im.apply([("kick", region, 1.0, 1.0)], xs, ys, zeros, zeros, ones, bid)
        assert nvx[0].tolist() == [0.0, 0.0, 1.0] and res == [((1, 1), (S16, S16), (S16, S16), (0, 0))], region
    nvx, _, res = im.apply([("kick", ("disc", 0.0, 0.0, 1.0), 1.0, 0.0, dict(id=1))], [np.zeros(3), np.zeros(1)], [np.zeros(3), np.zeros(1)],
                           zeros, zeros, ones, bid)
    assert nvx[0].tolist() == [1.0, 1.0, 0.0] and nvx[1].tolist() == [0.0] and res[0][0] == (2, 0)
    with pytest.raises(KeyError, match="record 0: no batch with id 9"):
        im.canonical([("kick", ("disc", 0.0, 0.0, 1.0), 1.0, 0.0, dict(id=9))], known_ids={1, 2})


BAD = [  # (record, what the refusal names)
    (("push", ("disc", 0.0, 0.0, 1.0), 1.0, 0.0), "unknown action"),
    (("kick", ("half_plane", 1.0, 0.0, 0.0), 1.0, 0.0, dict(linear=True)), "linear weight"),
    (("kick", ("box", 0.0, 0.0, 1.0, 1.0, 0.0), 1.0, 0.0, dict(linear=True)), "linear weight"),
    (("kick", ("disc", 0.0, 0.0, 0.0), 1.0, 0.0, dict(linear=True)), "linear weight"),
    (("kick", ("capsule", 0.0, 0.0, 1.0, 0.0, 0.0), 1.0, 0.0, dict(linear=True)), "linear weight"),
    (("swirl", ("disc", 0.0, 0.0, 1.0), 0.0, 0.0, 1.0, dict(by_inv_mass=True)), "inverse mass"),
    (("brake", ("disc", 0.0, 0.0, 1.0), 0.0, 0.0, 1.0, dict(by_inv_mass=True)), "inverse mass"),
    (("kick", ("disc", 0.0, 0.0, 1.0), float("inf"), 0.0), "not finite"),
    (("blast", ("disc", 0.0, 0.0, 1.0), 0.0, float("nan"), 1.0), "not finite"),
    (("brake", ("disc", 0.0, 0.0, 1.0), 0.0, 0.0, 1.5), "outside"),
    (("brake", ("disc", 0.0, 0.0, 1.0), 0.0, 0.0, -0.1), "outside"),
    (("kick", ("disc", 0.0, 0.0, -1.0), 1.0, 0.0), "negative"),
    (("kick", ("half_plane", 0.0, 1e-9, 0.0), 1.0, 0.0), "shorter than eps"),
    (("kick", ("disc", 0.0, float("nan"), 1.0), 1.0, 0.0), "not finite"),
]


@pytest.mark.parametrize("k", range(len(BAD)))
def test_the_model_refuses_what_the_header_lists(k):
    record, what = BAD[k]
    good = ("kick", ("disc", 0.0, 0.0, 1.0), 1.0, 0.0)
    with pytest.raises(ValueError, match=r"record 2.*" + what):
        im.canonical([good, good, record])
    with pytest.raises(ValueError, match="0 .. 64"):
        im.canonical([good] * 65)
    assert len(im.canonical([good] * 64)) == 64 and im.canonical([]) == []


# ------------------------------------------------------------------------------------------------ the surface
def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


PROTOS = {
    "egg_impulse": "int egg_impulse(egg_handle *h, int32_t n, const egg_impulse_record *list, egg_impulse_result *results /* [n] or NULL */);",
    "egg_group_impulse": "int egg_group_impulse(egg_group *g, int32_t n, const egg_impulse_record *list, egg_impulse_result *results /* [n] or NULL */);",
}


def test_header_and_binding_agree_on_the_entry_points_and_the_structs():
    from egg_fluid_simulation_amd import _ffi
    text = _read(ROOT, "include", "eggsim_impulse.h")
    for name, proto in PROTOS.items():
        assert proto in text, name
        assert name in _ffi._IMPULSE_SIGNATURES and name in _ffi.IMPULSE_SYMBOLS and name in _prototypes(text), name
    assert _ffi._IMPULSE_SIGNATURES["egg_impulse"] == _ffi._IMPULSE_SIGNATURES["egg_group_impulse"]
    # the binding covers the whole of this header as it covers the main one, which brings it along: 173 + 2 entry points
    assert sorted(_prototypes(text)) == _ffi.IMPULSE_SYMBOLS and not set(_ffi.IMPULSE_SYMBOLS) & set(_ffi.EXPORTED_SYMBOLS)
    assert len(_ffi.EXPORTED_SYMBOLS) + len(_ffi.IMPULSE_SYMBOLS) == 175
    main = _read(ROOT, "include", "eggsim.h")
    assert main.count('#include "eggsim_impulse.h"') == 1 and main.index('#include "eggsim_impulse.h"') > main.index("int egg_draw_source_instances(")
    if os.path.exists(_ffi.LIB_PATH):
        lib = _ffi.load()
        assert all(hasattr(lib, name) and getattr(lib, name).argtypes == _ffi._IMPULSE_SIGNATURES[name][1] for name in _ffi.IMPULSE_SYMBOLS)
    assert C.sizeof(_ffi.EggImpulse) == 96 and C.sizeof(_ffi.EggImpulseResult) == 64
    R = _ffi.EggImpulse
    assert [(n, getattr(R, n).offset) for n, _ in R._fields_] == [("region", 0), ("action", 56), ("flags", 60), ("id", 64), ("a", 72)]
    T = _ffi.EggImpulseResult
    assert [(n, getattr(T, n).offset) for n, _ in T._fields_] == [("count", 0), ("sdvx", 16), ("sdvy", 32), ("skipped", 48)]
    assert re.search(r"typedef struct \{ egg_sensor region; int32_t action, flags; int64_t id; double a\[3\]; \} egg_impulse_record; +/\* 96 bytes \*/", text)
    assert re.search(r"typedef struct \{ int64_t count\[2\], sdvx\[2\], sdvy\[2\], skipped\[2\]; \} egg_impulse_result; +/\* 64 bytes \*/", text)
    for line in ("#define EGG_MAX_IMPULSES 64", "#define EGG_IMPULSE_SCALE 65536.0", "#define EGG_IMPULSE_ALL_BATCHES ((int64_t)-1)",
                 "enum { EGG_IMPULSE_KICK = 0, EGG_IMPULSE_BLAST = 1, EGG_IMPULSE_SWIRL = 2, EGG_IMPULSE_BRAKE = 3 };",
                 "enum { EGG_IMPULSE_LINEAR = 1, EGG_IMPULSE_BY_INV_MASS = 2 };"):
        assert line in text, line
    assert (_ffi.MAX_IMPULSES, _ffi.IMPULSE_SCALE, _ffi.IMPULSE_ALL_BATCHES, _ffi.IMPULSE_NO_BATCH) == (64, 65536.0, -1, -2)
    assert _ffi.IMPULSE_ACTIONS == im.ACTIONS and (_ffi.IMPULSE_LINEAR, _ffi.IMPULSE_BY_INV_MASS) == (1, 2)
    assert {a: len(p) for a, p in zip(_ffi.IMPULSE_ACTIONS, _ffi.IMPULSE_PARAMS)} == im.N_PARAMS
    # the rule, where a C caller reads it
    for phrase in ("w = 1.0 - sqrt(d2) / R", "w = w * inv_mass", "nvx = vx + w * ax", "g = (w * s) / sqrt(d2)", "nvx = vx - g * dy, nvy = vy + g * dx",
                   "nvx = vx + g * (ux - vx)", "Unless d2 > 0.0 the record passes the\n *                              particle by",
                   "fabs(fx) < 2^53 && fabs(fy) < 2^53", "skipped[w] += 1", "Only vx and vy are ever written",
                   "smears by the new velocities, inside a padding that follows them too", "its max_velocity follows the edit and its other nine fields stay", "Everything is checked before anything is launched or changed",
                   "egg_step_begin or egg_rx_begin open", "tests/impulse_model.py", "no contraction", "EGG_ERR_UNKNOWN_ID", "one handle's, bit for bit"):
        assert phrase in text, phrase


def test_a_c_compiler_lays_the_structs_out_as_ctypes_does(tmp_path):
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    src = tmp_path / "impulse_layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "eggsim.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(egg_impulse_record), offsetof(egg_impulse_record, action), '
                   'offsetof(egg_impulse_record, id), offsetof(egg_impulse_record, a), sizeof(egg_impulse_result), '
                   'offsetof(egg_impulse_result, sdvx), offsetof(egg_impulse_result, skipped), (int)EGG_MAX_IMPULSES); return 0; }\n')
    exe = str(tmp_path / "impulse_layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)],
                   check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["96", "56", "64", "72", "64", "16", "48", "64"]


def test_the_kernels_exist_and_share_the_one_region_test():
    csrc = os.path.join(ROOT, "egg_fluid_simulation_amd", "csrc")
    kernels, host, host_h = _read(csrc, "eggsim_impulses.hip"), _read(csrc, "eggsim_host_impulses.hip"), _read(csrc, "eggsim_host.h")
    device_h, regions = _read(csrc, "eggsim_device.h"), _read(csrc, "eggsim_sensors.hip")
    for name, args in (("egg_impulse_kernel", "EggImpulseArgs"), ("egg_impulse_quiet_kernel", "EggImpulseArgs"),
                       ("egg_impulse_finish_kernel", "EggImpulseFinishArgs")):
        assert re.search(r'extern "C" __global__ void __launch_bounds__\(\w+\) %s\(%s A\)' % (name, args), kernels), name
        assert 'extern "C" __global__ void %s(%s A);' % (name, args) in host_h and "hipLaunchKernelGGL(%s," % name in host, name
    makefile = _read(csrc, "Makefile")
    assert makefile.count("eggsim_impulses.hip") == 2 and makefile.count("eggsim_host_impulses.hip") == 1 and "-ffp-contract=off" in makefile
    # ONE definition of the inside test, in the shared header
    assert device_h.count("bool sn_test(") == 1 and "bool sn_test(" not in regions and "bool sn_test(" not in kernels
    assert "sn_test(r.region, x, y, d2, R)" in kernels and "return sn_test(s, x, y, d2, R);" in device_h and "sn_inside(s, x, y)" in regions
    body = kernels[kernels.index("void im_body("):kernels.index('extern "C"')]
    assert "__shared__" not in body and "atomic" not in body and "asm" not in kernels and "float" not in kernels
    assert "__ballot(" in body and "__popcll(" in body and "if (taken != 0ull)" in body and "__shfl_xor(" in kernels
    stores = re.findall(r"\b(\w+)\[base \+ lane\] = ", body)
    assert sorted(stores) == ["VX", "VY"], stores  # only vx and vy are ever written
    assert "check_region(h, \"egg_impulse: record\", k, o.region)" in host and "check_region(h, \"egg_set_sensors: sensor\", k, o)" in _read(csrc, "eggsim_host_sensors.hip")
    last_check = max(m.start() for m in re.finditer(r"return fail\(h, EGG_ERR_(INVALID_ARGUMENT|UNKNOWN_ID)", host))
    assert last_check < host.index("hipLaunchKernelGGL(") and last_check < host.index("memset(results") and last_check < host.index("upload_atoms(")
    assert "opt_solver_order" not in host and host.count("h->stats.kernel_launches += 1;") == 2


def test_python_classes_have_the_methods_and_check_what_only_the_host_can():
    from egg_fluid_simulation_amd import EggError, SimulationGroup, SimulationHandler, _ffi
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler
    from egg_fluid_simulation_amd.simulation_handler import Impulse, ImpulseResult
    for cls in (SimulationHandler, SimulationGroup, ShardedSimulationHandler):
        assert list(inspect.signature(cls.impulse).parameters) == ["self", "records", "results"], cls.__name__
        for name, params in (("kick", ["self", "region", "ax", "ay", "id", "linear", "by_inv_mass"]),
                             ("blast", ["self", "cx", "cy", "R", "s", "id", "by_inv_mass", "types"]),
                             ("stir", ["self", "cx", "cy", "R", "omega", "id", "linear", "types"]),
                             ("brake", ["self", "region", "k", "ux", "uy", "id", "linear"])):
            assert list(inspect.signature(getattr(cls, name)).parameters) == params, (cls.__name__, name)
    assert SimulationGroup._PREFIX == "egg_group_" and SimulationGroup.impulse is SimulationHandler.impulse
    src = inspect.getsource(ShardedSimulationHandler.impulse)
    assert src.count("self._all_reduce_sum(") == 1 and "self.dist" not in src and "self.local._impulse_table(" in src and "IMPULSE_NO_BATCH" in src
    n, arr = SimulationHandler._c_impulses([Impulse("blast", ("disc", 1.0, 2.0, 3.0, "yolk"), (1.0, 2.0, -4.0), 7, True, True),
                                            ("brake", ("box", 0.0, 0.0, 2.0, 1.0, 0.0), 0.5, 0.25, 1.0), ("kick", ("half_plane", 0.0, 2.0, 1.0), 1.0, 2.0, {"id": 3})])
    assert n == 3 and (arr[0].action, arr[0].flags, arr[0].id, list(arr[0].a)) == (1, 3, 7, [1.0, 2.0, -4.0])
    assert (arr[0].region.kind, arr[0].region.type_mask, list(arr[0].region.p)[:3]) == (1, 2, [1.0, 2.0, 3.0])
    assert (arr[1].action, arr[1].flags, arr[1].id, list(arr[1].a)) == (3, 0, -1, [0.5, 0.25, 1.0]) and list(arr[1].region.p)[4:] == [1.0, 0.0]
    assert (arr[2].action, arr[2].id, list(arr[2].a)) == (0, 3, [1.0, 2.0, 0.0])
    for bad, text in (([("push", ("disc", 0, 0, 1), 1, 1)], "action must be one of"), ([("kick", ("disc", 0, 0, 1), 1)], "expected the parameters"),
                      ([("kick", ("ring", 0, 0, 1), 1, 1)], "record 0: region"), ([("kick",)], "expected \\(action, region"),
                      ([("kick", ("disc", 0, 0, 1), 1, 1, {"mass": 1})], "expected \\(action, region"),
                      ([("kick", ("disc", 0, 0, 1), 1, 1, {"id": 1.5})], "id must be None or a batch id"),
                      ([("kick", ("disc", 0, 0, 1), 1, "a")], "must be numbers"), ([("kick", ("disc", 0, 0, 1), 1, 1)] * 65, "0 .. 64 records")):
        with pytest.raises(EggError, match=text):
            SimulationHandler._c_impulses(bad)
    got = SimulationHandler._impulse_results(np.array([[2, 1, 3 * S16, -S16, 0, S16 // 2, 0, 4]], dtype=np.int64))
    assert got == [ImpulseResult((2, 1), (3 * S16, -S16), (0, S16 // 2), (0, 4))] and got[0].dv() == ((3.0, 0.0), (-1.0, 0.5))
    assert _ffi.IMPULSE_CODES == {"kick": 0, "blast": 1, "swirl": 2, "brake": 3}


def test_lua_has_the_functions_and_the_header_prototype():
    lua = _read(ROOT, "egg_fluid_simulation_amd", "lua", "egg_fluid_simulation", "simulation_handler.lua")
    for line in ("function SimulationHandler:impulse(records, want_results)", "function SimulationHandler:kick(region, ax, ay, opts)",
                 "function SimulationHandler:blast(cx, cy, R, s, opts)", "function SimulationHandler:stir(cx, cy, R, omega, opts)",
                 "function SimulationHandler:brake(region, k, ux, uy, opts)"):
        assert line in lua, line
    blocks = re.findall(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S)
    assert len(blocks) == 2 and "egg_impulse" not in blocks[0]  # (a block per header)
    assert _prototypes(blocks[1]) == {"egg_impulse": _prototypes(_read(ROOT, "include", "eggsim_impulse.h"))["egg_impulse"]}
    assert "typedef struct { egg_sensor region; int32_t action, flags; int64_t id; double a[3]; } egg_impulse_record;" in lua
    assert "typedef struct { int64_t count[2], sdvx[2], sdvy[2], skipped[2]; } egg_impulse_result;" in lua
    assert "lib.egg_impulse(self._h, n, arr, out)" in lua and "lib.egg_impulse(self._h, n, arr, nil)" in lua
    assert "_impulse_actions = { kick = 0, blast = 1, swirl = 2, brake = 3 }" in lua and "_impulse_scale = 65536" in lua
    assert "(r.linear and 1 or 0) + (r.by_inv_mass and 2 or 0)" in lua and "r.id or _impulse_all_batches" in lua
    assert 'linear = true' in lua[lua.index("function SimulationHandler:blast("):lua.index("function SimulationHandler:stir(")]


def test_the_documents_describe_the_call():
    design = _read(ROOT, "DESIGN.md")
    assert design.index("### 2.11 Pieces") < design.index("### 2.12 Impulses") < design.index("## 3. Data layout in HBM")
    part = design[design.index("### 2.12 Impulses"):design.index("## 3. Data layout in HBM")]
    for phrase in ("egg_impulse", "egg_group_impulse", "egg_impulse_kernel", "egg_impulse_finish_kernel", "EGG_IMPULSE_NO_BATCH", "sn_test",
                   "tests/impulse_model.py", "NOT MEASURED", "scripts/gpu_impulses_bench.py", "profiles/r31_impulses.md", "Only `vx` and `vy`", "all_reduce"):
        assert phrase in part, phrase
    readme, integration = _read(ROOT, "README.md"), _read(ROOT, "INTEGRATION.md")
    assert readme.index("* Pieces (") < readme.index("* Impulses (") and "two more entry points for impulses: 175" in " ".join(readme.split())
    assert "(the row \"impulses\"): 175" in integration and "h.blast(" in integration and "handler:blast(" in integration
    for proto in PROTOS.values():
        assert " ".join(proto.split()) in " ".join(integration.split()), proto
    entry = _read(ROOT, "__graft_entry__.py")
    assert "h.impulse(" in entry and "smoke ok (impulses)" in entry
