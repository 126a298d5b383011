"""The surface of collider spin (egg_set_collider_spin, DESIGN.md section 2.7 "Collider spin") as far as it can be
checked without a device: the four entry points and the 24-byte struct in the header and in the ctypes binding, the two
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
    "egg_set_collider_spin": "int egg_set_collider_spin(egg_handle *h, int32_t n, const egg_collider_spin *s);",
    "egg_get_collider_spin": "int egg_get_collider_spin(const egg_handle *h, int32_t cap, egg_collider_spin *s, int32_t *n);",
    "egg_group_set_collider_spin": "int egg_group_set_collider_spin(egg_group *g, int32_t n, const egg_collider_spin *s);",
    "egg_group_get_collider_spin": "int egg_group_get_collider_spin(const egg_group *g, int32_t cap, egg_collider_spin *s, int32_t *n);",
}
# kernel: (G, K) of its row in the one kernel list -- its place in the host's table beside the spin flavour
KERNELS = {
    "egg_rx_gather_col_spin_kernel": (False, False),
    "egg_rx_gather_group_col_spin_kernel": (True, False),
    "egg_rx_gather_coh_col_spin_kernel": (False, True),
    "egg_rx_gather_group_coh_col_spin_kernel": (True, True),
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
    for name in ("set_collider_spin", "get_collider_spin"):  # a group twin has its handle twin's arity
        assert len(_ffi._SIGNATURES["egg_" + name][1]) == len(_ffi._SIGNATURES["egg_group_" + name][1])
    assert re.search(r"typedef struct\s*\{\s*double px, py;[^}]*double omega;[^}]*\}\s*egg_collider_spin;", text)
    S = _ffi.EggColliderSpin
    assert C.sizeof(S) == 24
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("px", 0), ("py", 8), ("omega", 16)]
    # the kernel's record is the ABI's; spin has a fields struct of its own: the records, the host's sines and cosines of
    # the sub-step's end and of one sub-step, the sub-step's start; no counter
    device_h = _read(CSRC, "eggsim_device.h")
    assert re.search(r"struct EggSpin \{\s*double px, py, omega;\s*\};", device_h)
    fields = re.search(r"struct EggRxSpinFields \{([^}]*)\}", device_h).group(1)
    assert re.findall(r"(\w+);", re.sub(r"//[^\n]*", "", fields)) == ["list", "cs", "hcs", "ts"]
    import rx_kernel_list
    rows = rx_kernel_list.gather_rows()
    for name in KERNELS:  # everything a motion twin takes, and the spin fields (A.r of the one record)
        assert rows[name] == dict(rows[name.replace("_spin_", "_mov_")], flavour="EGG_RX_SPIN", Sp=True), name
    record = re.search(r"struct EggRxPassArgs \{([^}]*)\}", device_h).group(1)
    assert "EggRxMotionFields m;\n    EggRxSpinFields r;\n" in record
    # the rules of the setter, where a C caller reads them
    for phrase in ("egg_set_colliders resets every spin", "egg_set_collider_motion and egg_set_collider_surfaces leave them",
                   "A -0.0 is stored as +0.0 and counts as zero", "Refused while a step is in flight",
                   "with the collider's index in the message", "computed on the host (libm)"):
        assert phrase in re.sub(r"\s*\n \* ", " ", text), phrase


def test_spin_struct_size_matches_the_c_compiler(tmp_path):
    """sizeof(egg_collider_spin) and the offsets of its fields as a C compiler lays the header out == the ctypes mirror"""
    from egg_fluid_simulation_amd import _ffi
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    src = tmp_path / "spin_layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "eggsim.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(egg_collider_spin), offsetof(egg_collider_spin, px), '
                   'offsetof(egg_collider_spin, py), offsetof(egg_collider_spin, omega)); return 0; }\n')
    exe = str(tmp_path / "spin_layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    S = _ffi.EggColliderSpin
    assert [int(v) for v in out] == [C.sizeof(S), S.px.offset, S.py.offset, S.omega.offset] == [24, 0, 8, 16]


def test_the_library_exports_the_symbols():
    from egg_fluid_simulation_amd import _ffi
    path = os.path.join(ROOT, "egg_fluid_simulation_amd", "libeggsim.so")
    if not os.path.exists(path):
        pytest.skip("libeggsim.so is not built")
    lib = C.CDLL(path)
    for name in PROTOS:
        assert hasattr(lib, name), name
    for name in PROTOS:  # every entry point links and refuses a null handle
        args = (None, 0, None) if "_set_" in name else (None, 0, None, None)
        assert getattr(lib, name)(*args) == _ffi.EGG_ERR_INVALID_ARGUMENT, name


def test_python_classes_have_the_two_methods():
    from egg_fluid_simulation_amd import EggError, SimulationGroup, SimulationHandler
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler
    for cls in (SimulationHandler, SimulationGroup, ShardedSimulationHandler):
        assert list(inspect.signature(cls.set_collider_spin).parameters) == ["self", "spins"], cls
        assert list(inspect.signature(cls.get_collider_spin).parameters) == ["self"], cls
    # shape and finiteness are refused before any device call: a bare instance has no handle to call with
    for cls in (SimulationHandler, SimulationGroup):
        bare = cls.__new__(cls)
        for bad in (["fast"], [(1.0,)], [(1.0, 2.0)], [(1.0, 2.0, 3.0, 4.0)], [object()], [("a", 0, 0)], [3.0]):
            with pytest.raises(EggError, match="collider spin 0: expected"):
                bare.set_collider_spin(bad)
        for bad in ([None, (float("nan"), 0.0, 1.0)], [None, (0.0, float("inf"), 1.0)]):
            with pytest.raises(EggError, match="collider spin 1: the pivot .* is not finite"):
                bare.set_collider_spin(bad)
        for bad in ([None, (0.0, 0.0, float("nan"))], [None, (0.0, 0.0, -float("inf"))]):
            with pytest.raises(EggError, match="collider spin 1: omega .* is not finite"):
                bare.set_collider_spin(bad)
    n, arr = SimulationHandler._c_spins([None, (3, -4, 2), (0.5, 0.25, -0.125)])
    assert n == 3
    assert [(s.px, s.py, s.omega) for s in arr[:n]] == [(0.0, 0.0, 0.0), (3.0, -4.0, 2.0), (0.5, 0.25, -0.125)]
    assert SimulationHandler._c_spins([])[0] == 0


def test_lua_wrapper_and_documents_name_the_methods():
    lua = _read(ROOT, "egg_fluid_simulation_amd", "lua", "egg_fluid_simulation", "simulation_handler.lua")
    for name in ("set_collider_spin(spins)", "get_collider_spin()"):
        assert "function SimulationHandler:" + name in lua, name
    for name in ("egg_set_collider_spin", "egg_get_collider_spin"):
        assert PROTOS[name] in lua and "lib." + name + "(self._h" in lua, name
    assert "typedef struct { double px, py, omega; } egg_collider_spin;" in lua
    integration = _read(ROOT, "INTEGRATION.md")
    for name in ("egg_set_collider_spin", "egg_get_collider_spin"):
        assert PROTOS[name] in integration, name
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        text = _read(ROOT, doc)
        assert "set_collider_spin" in text and "get_collider_spin" in text, doc
    design = _read(ROOT, "DESIGN.md")
    assert "Collider spin" in design
    for rule in ("Px = px + ox;  Py = py + oy", "c  = cos(t*omega);  s = sin(t*omega)", "qx' = Px + (c*rx - s*ry);   qy' = Py + (s*rx + c*ry)",
                 "nx' = c*nx - s*ny;  ny' = s*nx + c*ny", "off' = (nx'*Px + ny'*Py) + (off - (nx*px + ny*py))",
                 "ux = prev.x - (px + ts*vx);  uy = prev.y - (py + ts*vy)", "pvx = Px + (ch*ux - sh*uy);  pvy = Py + (sh*ux + ch*uy)",
                 "wx = (sf.vx + vx) - omega*(y - Py)", "wy = (sf.vy + vy) + omega*(x - Px)"):
        assert rule in design, rule
    # the limits, in section 7 and in the subsection
    for limit in ("no angular acceleration", "Only walls sweep", "not renormalised"):
        assert limit in design, limit
    assert "egg_group_set_collider_spin" in design or "egg_group_set_collider_spin" in integration
    assert "Collider spin" in _read(ROOT, "README.md")


def test_the_four_kernels_and_their_launches():
    import rx_kernel_list
    kernels, driver = _read(CSRC, "eggsim_relaxed.hip"), _read(CSRC, "eggsim_host_relaxed.hip")
    rows = rx_kernel_list.assert_expansions()  # (every row is defined, declared to the host and in its table once)
    for name, (G, K) in KERNELS.items():  # rx_gather<G, K, true, true, true> with the motion and the spin fields, without load fields
        assert rows[name] == dict(G=G, K=K, flavour="EGG_RX_SPIN", D=True, S=True, W=True, Mo=True, Sp=True, Ld=False), name
    # the spin instantiations are the only ones that are given the spin fields and no load fields, and they get the motion fields too
    assert sorted(n for n, r in rows.items() if r["Sp"] and not r["Ld"]) == sorted(KERNELS)
    assert all(r["Mo"] for r in rows.values() if r["Sp"])
    assert sorted(n for n, r in rows.items() if r["flavour"] == "EGG_RX_SPIN") == sorted(n for n in rows if "spin" in n) == sorted(KERNELS)
    # a spin twin is picked in front of its motion twin, by a flag of its own; only loads outrank it
    order = rx_kernel_list.flavour_precedence()
    at = order.index(("spin", "EGG_RX_SPIN"))
    assert order[:at] == [("loads", "EGG_RX_LOAD")] and order[at + 1] == ("motion", "EGG_RX_MOV")
    # sines and cosines are the host's: the kernels call none
    assert not re.search(r"\b(sin|cos|sincos)\(", re.sub(r"//[^\n]*", "", kernels))
    assert "cos(a), sin(a)" in driver
    # the group refuses handles that differ, by the setter's name
    assert "egg_group_set_collider_spin sets all" in _read(CSRC, "eggsim_host_relaxed_group.hip")
