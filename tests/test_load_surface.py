"""The surface of collider loads (egg_set_collider_loads, DESIGN.md section 2.7 "Collider loads") as far as it can be
checked without a device: the seven entry points, the two scales and the 24-byte struct in the header and in the ctypes
binding, the methods on all three Python classes and in the Lua wrapper, the documents, the four kernels with their
launches, and the refusals where the sources state them."""
import ctypes as C
import inspect
import os
import re

from conftest import ROOT
from test_cohesion_surface import _header

CSRC = os.path.join(ROOT, "egg_fluid_simulation_amd", "csrc")
PROTOS = {
    "egg_set_collider_loads": "int egg_set_collider_loads(egg_handle *h, int on);",
    "egg_get_collider_loads_enabled": "int egg_get_collider_loads_enabled(const egg_handle *h, int *on);",
    "egg_get_collider_load_sums": "int egg_get_collider_load_sums(egg_handle *h, int32_t cap, int64_t *sums /* [n][3] */, int64_t *dropped, "
                                  "double *sub_delta, int32_t *n);",
    "egg_get_collider_loads": "int egg_get_collider_loads(egg_handle *h, int32_t cap, egg_collider_load *out, int32_t *n);",
    "egg_group_set_collider_loads": "int egg_group_set_collider_loads(egg_group *g, int on);",
    "egg_group_get_collider_load_sums": "int egg_group_get_collider_load_sums(egg_group *g, int32_t cap, int64_t *sums /* [n][3] */, "
                                        "int64_t *dropped, double *sub_delta, int32_t *n);",
    "egg_group_get_collider_loads": "int egg_group_get_collider_loads(egg_group *g, int32_t cap, egg_collider_load *out, int32_t *n);",
}
# kernel: (G, K) of its row in the one kernel list -- its place in the host's table beside the loads flavour
KERNELS = {
    "egg_rx_gather_col_load_kernel": (False, False),
    "egg_rx_gather_group_col_load_kernel": (True, False),
    "egg_rx_gather_coh_col_load_kernel": (False, True),
    "egg_rx_gather_group_coh_col_load_kernel": (True, True),
}


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_header_declares_the_entry_points_the_scales_and_the_struct():
    from egg_fluid_simulation_amd import _ffi
    text = _header()
    for name, proto in PROTOS.items():
        assert proto in text, name
        assert name in _ffi._SIGNATURES and name in _ffi.EXPORTED_SYMBOLS, name
        assert len(_ffi._SIGNATURES[name][1]) == proto.count(",") + 1, name
    for name in ("set_collider_loads", "get_collider_load_sums", "get_collider_loads"):  # a group twin has its handle twin's arity
        assert len(_ffi._SIGNATURES["egg_" + name][1]) == len(_ffi._SIGNATURES["egg_group_" + name][1])
    assert re.search(r"typedef struct\s*\{\s*double jx, jy;[^}]*double torque;[^}]*\}\s*egg_collider_load;", text)
    L = _ffi.EggColliderLoad
    assert C.sizeof(L) == 24 and [(n, getattr(L, n).offset) for n, _ in L._fields_] == [("jx", 0), ("jy", 8), ("torque", 16)]
    assert "#define EGG_COLLIDER_LOAD_IMPULSE_SCALE 1048576.0" in text and "#define EGG_COLLIDER_LOAD_TORQUE_SCALE 1024.0" in text
    assert _ffi.COLLIDER_LOAD_IMPULSE_SCALE == 2.0 ** 20 and _ffi.COLLIDER_LOAD_TORQUE_SCALE == 2.0 ** 10
    # the kernel's scales are the ABI's, and the host says so to the compiler
    device_h = _read(CSRC, "eggsim_device.h")
    assert "#define EGG_RX_LOAD_SCALE_IMPULSE 0x1p20" in device_h and "#define EGG_RX_LOAD_SCALE_TORQUE 0x1p10" in device_h
    assert "#define EGG_RX_LOAD_LIMIT 0x1p53" in device_h
    assert "EGG_COLLIDER_LOAD_IMPULSE_SCALE == EGG_RX_LOAD_SCALE_IMPULSE && EGG_COLLIDER_LOAD_TORQUE_SCALE == EGG_RX_LOAD_SCALE_TORQUE" in \
        _read(CSRC, "eggsim_host_colliders.hip")
    fields = re.search(r"struct EggRxLoadFields \{([^}]*)\}", device_h).group(1)
    assert re.findall(r"(\w+);", re.sub(r"//[^\n]*", "", fields)) == ["sums", "dropped", "eps", "moving", "turning", "pivots"]
    import rx_kernel_list
    rows = rx_kernel_list.gather_rows()
    for name in KERNELS:  # the load row passes everything its spin row passes, and beyond it the load fields (A.l of the one record) alone
        assert rows[name] == dict(rows[name.replace("_load_", "_spin_")], flavour="EGG_RX_LOAD", Ld=True), name
    record = re.search(r"struct EggRxPassArgs \{([^}]*)\}", device_h).group(1)
    assert "EggRxSpinFields r;\n    EggRxLoadFields l;\n" in record
    # the definition, where a C caller reads it
    for phrase in ("ux = m * (bx - ax),  uy = m * (by - ay)", "uz = (ax - Px) * uy - (ay - Py) * ux", "m  = 1.0 / im",
                   "qz = llrint(uz * EGG_COLLIDER_LOAD_TORQUE_SCALE)", "reaches 2^53 in magnitude, the contribution is dropped whole",
                   "step 5c's grip included", "also when omega == 0; (0, 0) when the handle", "The sums cover ONE step",
                   "egg_set_colliders keeps the switch and zeroes the", "refused while a step is in flight",
                   "jx = ((double)sx / EGG_COLLIDER_LOAD_IMPULSE_SCALE) / h", "The MEAN FORCE over a step of", "is j / delta",
                   "A group whose handles differ in the switch refuses to step"):
        assert phrase in text, phrase


def test_the_kernels_exist_and_only_a_step_with_loads_launches_them():
    kernels = _read(CSRC, "eggsim_relaxed.hip")
    host = _read(CSRC, "eggsim_host_relaxed.hip")
    import rx_kernel_list
    rows = rx_kernel_list.assert_expansions()  # (every row is defined, declared to the host and in its table once)
    for name, (G, K) in KERNELS.items():  # rx_gather<G, K, true, true, true> with the motion, spin and load fields
        assert rows[name] == dict(G=G, K=K, flavour="EGG_RX_LOAD", D=True, S=True, W=True, Mo=True, Sp=True, Ld=True), name
    assert sorted(n for n, r in rows.items() if r["Ld"]) == sorted(n for n, r in rows.items() if r["flavour"] == "EGG_RX_LOAD") == sorted(KERNELS)
    # only a step with loads launches them, and such a step launches no other gather: the switch is tested first
    order = rx_kernel_list.flavour_precedence()
    assert order[0] == ("loads", "EGG_RX_LOAD") and order[1] == ("spin", "EGG_RX_SPIN")
    assert [f for _, f in order].count("EGG_RX_LOAD") == 1
    assert "st.L.loads = st.L.colliders && h->opt_loads;" in host
    # no per-lane atomics on the sums: the three adds sit behind the wave's lane 0, and a wave nothing counted in returns
    tally = kernels[kernels.index("void rx_tally("):kernels.index("// Step 5b of the relaxed pass")]
    assert "if (__ballot(counts) == 0ull) return;" in tally
    assert tally.count("atomicAdd(") == 4 and tally.index("if ((threadIdx.x & 63) == 0)") < tally.index("atomicAdd(")
    assert "__shared__" not in tally
    # cleared before either stream starts, taken over in the commit only
    assert "hipMemcpy(h->d_loads.p, none.data()" in host[host.index("int prepare_step("):host.index("int prepare_type(")]
    commit = host[host.index("void relaxed_commit("):]
    assert "if (h->opt_loads && !h->colliders.empty()) take_loads(h, st[0].env.sub_delta);" in commit
    assert host.count("take_loads(") == 2  # (its definition and the commit)


def test_the_refusals_stand_in_the_sources():
    abi = _read(CSRC, "eggsim_host_colliders.hip")
    setter = abi[abi.index("int egg_set_collider_loads("):abi.index("int egg_get_collider_loads_enabled(")]
    assert 'REJECT_IN_FLIGHT(h, "egg_set_collider_loads");' in setter
    assert "opt_solver_order" not in setter and "colliders.empty()" not in setter  # (either order, any list: it only observes)
    group = _read(CSRC, "eggsim_host_relaxed_group.hip")
    assert ("relaxed order: the handles of the group differ in their collider loads (egg_group_set_collider_loads sets all)") in group
    assert "hs[0]->opt_loads != hs[k]->opt_loads" in group
    lists = abi[abi.index("int egg_set_colliders("):abi.index("int egg_get_colliders(")]
    assert "h->load_sums.assign(3 * h->colliders.size(), 0);" in lists and "opt_loads" not in lists  # (zeroed; the switch stays)


def test_python_classes_and_lua_have_the_methods():
    from egg_fluid_simulation_amd import SimulationGroup, SimulationHandler
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler
    for cls in (SimulationHandler, SimulationGroup, ShardedSimulationHandler):
        for name in ("set_collider_loads", "collider_loads", "collider_load_sums", "get_collider_loads_enabled"):
            assert callable(getattr(cls, name)), (cls.__name__, name)
        assert list(inspect.signature(cls.set_collider_loads).parameters) == ["self", "on"]
    src = inspect.getsource(ShardedSimulationHandler.collider_load_sums)
    assert "all_reduce" in src and "int64" in src  # a collective over the raw integers
    assert "_ffi.COLLIDER_LOAD_IMPULSE_SCALE" in inspect.getsource(ShardedSimulationHandler.collider_loads)
    lua = _read(ROOT, "egg_fluid_simulation_amd", "lua", "egg_fluid_simulation", "simulation_handler.lua")
    for name in ("set_collider_loads", "get_collider_loads_enabled", "collider_loads", "collider_load_sums"):
        assert "function SimulationHandler:%s(" % name in lua, name
    for name in ("egg_set_collider_loads", "egg_get_collider_loads_enabled", "egg_get_collider_load_sums", "egg_get_collider_loads"):
        assert re.search(r"int %s\(" % name, lua), name
    assert "typedef struct { double jx, jy, torque; } egg_collider_load;" in lua


def test_the_documents_describe_the_rule():
    design = _read(ROOT, "DESIGN.md")
    assert "Collider loads" in design
    part = design[design.index("#### Collider loads"):design.index("#### Forces")]
    for phrase in ("uz = (ax - Px) * uy - (ay - Py) * ux", "2^63", "2^53", "egg_rx_gather*_col_load_kernel", "dropped"):
        assert phrase in part, phrase
    readme = _read(ROOT, "README.md")
    assert "set_collider_loads" in readme
    integration = _read(ROOT, "INTEGRATION.md")
    assert "set_collider_loads" in integration and "collider_loads()" in integration
    assert os.path.exists(os.path.join(ROOT, "profiles", "r23_loads.md"))
