"""The surface of collider motion (egg_set_collider_motion, DESIGN.md section 2.7 "Collider motion") as far as it can be
checked without a device: the four entry points and the 16-byte struct in the header and in the ctypes binding, the two
methods on all three Python classes and in the Lua wrapper, the documents, and the four kernels with their launches."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
from test_cohesion_surface import _header

CSRC = os.path.join(ROOT, "egg_fluid_simulation_amd", "csrc")
PROTOS = {
    "egg_set_collider_motion": "int egg_set_collider_motion(egg_handle *h, int32_t n, const egg_collider_motion *m);",
    "egg_get_collider_motion": "int egg_get_collider_motion(const egg_handle *h, int32_t cap, egg_collider_motion *m, int32_t *n);",
    "egg_group_set_collider_motion": "int egg_group_set_collider_motion(egg_group *g, int32_t n, const egg_collider_motion *m);",
    "egg_group_get_collider_motion": "int egg_group_get_collider_motion(const egg_group *g, int32_t cap, egg_collider_motion *m, int32_t *n);",
}
# kernel: (G, K) of its row in the one kernel list -- its place in the host's table beside the motion flavour
KERNELS = {
    "egg_rx_gather_col_mov_kernel": (False, False),
    "egg_rx_gather_group_col_mov_kernel": (True, False),
    "egg_rx_gather_coh_col_mov_kernel": (False, True),
    "egg_rx_gather_group_coh_col_mov_kernel": (True, True),
}


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_header_declares_the_four_entry_points_and_the_struct():
    from egg_fluid_simulation_amd import _ffi
    text = _header()
    for name, proto in PROTOS.items():
        assert proto in text, name
        assert name in _ffi._SIGNATURES and name in _ffi.EXPORTED_SYMBOLS, name
        assert len(_ffi._SIGNATURES[name][1]) == proto.count(",") + 1, name
    # a group twin has its handle twin's arity
    for name in ("set_collider_motion", "get_collider_motion"):
        assert len(_ffi._SIGNATURES["egg_" + name][1]) == len(_ffi._SIGNATURES["egg_group_" + name][1])
    assert re.search(r"typedef struct\s*\{\s*double vx, vy;[^}]*\}\s*egg_collider_motion;", text)
    assert C.sizeof(_ffi.EggColliderMotion) == 16
    assert [(n, getattr(_ffi.EggColliderMotion, n).offset) for n, _ in _ffi.EggColliderMotion._fields_] == [("vx", 0), ("vy", 8)]
    # the kernel's record is the ABI's; motion has a fields struct of its own: the time of the pass, no counter
    device_h = _read(CSRC, "eggsim_device.h")
    assert re.search(r"struct EggMotion \{\s*double vx, vy;\s*\};", device_h)
    fields = re.search(r"struct EggRxMotionFields \{([^}]*)\}", device_h).group(1)
    assert re.findall(r"(\w+);", re.sub(r"//[^\n]*", "", fields)) == ["list", "t"]


def test_motion_struct_size_matches_the_c_compiler(tmp_path):
    """sizeof(egg_collider_motion) and the offsets of its fields as a C compiler lays the header out == the ctypes mirror"""
    from egg_fluid_simulation_amd import _ffi
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    src = tmp_path / "motion_layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "eggsim.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(egg_collider_motion), offsetof(egg_collider_motion, vx), '
                   'offsetof(egg_collider_motion, vy)); return 0; }\n')
    exe = str(tmp_path / "motion_layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    M = _ffi.EggColliderMotion
    assert [int(v) for v in out] == [C.sizeof(M), M.vx.offset, M.vy.offset] == [16, 0, 8]


def test_the_library_exports_the_symbols():
    from egg_fluid_simulation_amd import _ffi
    path = os.path.join(ROOT, "egg_fluid_simulation_amd", "libeggsim.so")
    if not os.path.exists(path):
        pytest.skip("libeggsim.so is not built")
    lib = C.CDLL(path)
    for name in PROTOS:
        assert hasattr(lib, name), name
    # every entry point links and refuses a null handle
    for name in PROTOS:
        args = (None, 0, None) if "_set_" in name else (None, 0, None, None)
        assert getattr(lib, name)(*args) == _ffi.EGG_ERR_INVALID_ARGUMENT, name


def test_python_classes_have_the_two_methods():
    from egg_fluid_simulation_amd import EggError, SimulationGroup, SimulationHandler
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler
    for cls in (SimulationHandler, SimulationGroup, ShardedSimulationHandler):
        assert list(inspect.signature(cls.set_collider_motion).parameters) == ["self", "motions"], cls
        assert list(inspect.signature(cls.get_collider_motion).parameters) == ["self"], cls
    # shape and finiteness are refused before any device call: a bare instance has no handle to call with
    for cls in (SimulationHandler, SimulationGroup):
        bare = cls.__new__(cls)
        for bad in (["fast"], [(1.0,)], [(1.0, 2.0, 3.0)], [object()], [("a", 0)], [3.0]):
            with pytest.raises(EggError, match="collider motion 0: expected"):
                bare.set_collider_motion(bad)
        for bad in ([None, (float("nan"), 0.0)], [None, (0.0, float("inf"))], [None, (-float("inf"), 0.0)]):
            with pytest.raises(EggError, match="collider motion 1: the velocity .* is not finite"):
                bare.set_collider_motion(bad)
    n, arr = SimulationHandler._c_motions([None, (3, -4), (0.5, 0.25)])
    assert n == 3
    assert [(m.vx, m.vy) for m in arr[:n]] == [(0.0, 0.0), (3.0, -4.0), (0.5, 0.25)]
    assert SimulationHandler._c_motions([])[0] == 0


def test_lua_wrapper_and_documents_name_the_methods():
    lua = _read(ROOT, "egg_fluid_simulation_amd", "lua", "egg_fluid_simulation", "simulation_handler.lua")
    for name in ("set_collider_motion(motions)", "get_collider_motion()"):
        assert "function SimulationHandler:" + name in lua, name
    for name in ("egg_set_collider_motion", "egg_get_collider_motion"):
        assert PROTOS[name] in lua and "lib." + name + "(self._h" in lua, name
    assert "typedef struct { double vx, vy; } egg_collider_motion;" in lua
    integration = _read(ROOT, "INTEGRATION.md")
    for name in ("egg_set_collider_motion", "egg_get_collider_motion"):
        assert PROTOS[name] in integration, name
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        text = _read(ROOT, doc)
        assert "set_collider_motion" in text and "get_collider_motion" in text, doc
    design = _read(ROOT, "DESIGN.md")
    assert "Collider motion" in design
    for rule in ("t  = (double)(sub + 1) * h", "off' = off + (nx*ox + ny*oy)", "pvx = prev.x + h*vx;  pvy = prev.y + h*vy",
                 "wx = sf.vx + vx;  wy = sf.vy + vy", "ex = (x - prev.x) - h*wx;  ey = (y - prev.y) - h*wy"):
        assert rule in design, rule
    assert "is not swept against a collider list the caller changes" not in design


def test_the_four_kernels_and_their_launches():
    import rx_kernel_list
    kernels = _read(CSRC, "eggsim_relaxed.hip")
    rows = rx_kernel_list.assert_expansions()  # (every row is defined, declared to the host and in its table once)
    for name, (G, K) in KERNELS.items():  # rx_gather<G, K, true, true, true> with the motion fields, without spin and load fields
        assert rows[name] == dict(G=G, K=K, flavour="EGG_RX_MOV", D=True, S=True, W=True, Mo=True, Sp=False, Ld=False), name
    # the motion instantiations are the only ones that are given the motion fields and nothing beyond them
    assert sorted(n for n, r in rows.items() if r["Mo"] and not r["Sp"]) == sorted(KERNELS)
    assert sorted(n for n, r in rows.items() if r["flavour"] == "EGG_RX_MOV") == sorted(n for n in rows if "mov" in n) == sorted(KERNELS)
    # a motion outranks walls, surfaces and colliders; a spin and loads outrank it
    order = rx_kernel_list.flavour_precedence()
    at = order.index(("motion", "EGG_RX_MOV"))
    assert [f for _, f in order[:at]] == ["EGG_RX_LOAD", "EGG_RX_SPIN"] and order[at + 1] == ("walls", "EGG_RX_WALL")
    # the gather keeps its five template parameters
    assert "template <bool G, bool K, bool D, bool S, bool W>\n__device__ __forceinline__ void rx_gather(" in kernels
