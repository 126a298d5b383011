"""The one list of the relaxed pass's flavoured kernels (EGG_RX_PASS_KERNELS in csrc/eggsim_device.h), read the way the
compiler reads it, for the surface tests of the features whose kernels are rows of it: what a row says, and that the
definitions (eggsim_relaxed.hip), the declarations (eggsim_host.h) and the host's table of gathers
(eggsim_host_relaxed.hip) are expansions of the list and of nothing else."""
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "egg_fluid_simulation_amd", "csrc")
FLAVOURS = ("EGG_RX_NONE", "EGG_RX_COL", "EGG_RX_SRF", "EGG_RX_WALL", "EGG_RX_MOV", "EGG_RX_SPIN", "EGG_RX_LOAD")
COLUMNS = ("G", "K", "flavour", "D", "S", "W", "Mo", "Sp", "Ld")


def read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def gather_rows():
    """{kernel: dict(G, K, flavour, D, S, W, Mo, Sp, Ld)} of the GATHER rows; the 0 / 1 columns as bools"""
    device_h = read("eggsim_device.h")
    body = device_h[device_h.index("#define EGG_RX_PASS_KERNELS(GATHER, OTHER)"):]
    body = body[:body.index("\n\n")] if "\n\n" in body else body
    rows = {}
    for name, cols in re.findall(r"^\s*GATHER\((\w+),([^)]*)\)", body, flags=re.M):
        cols = [c.strip() for c in cols.split(",")]
        assert len(cols) == len(COLUMNS) and name not in rows, name
        row = dict(zip(COLUMNS, cols))
        assert row["flavour"] in FLAVOURS and all(row[c] in ("0", "1") for c in COLUMNS if c != "flavour"), name
        rows[name] = {c: (v if c == "flavour" else v == "1") for c, v in row.items()}
    return rows


def other_rows():
    """{kernel: its body} of the OTHER rows"""
    device_h = read("eggsim_device.h")
    body = device_h[device_h.index("#define EGG_RX_PASS_KERNELS(GATHER, OTHER)"):]
    return {name: call.strip() for name, call in re.findall(r"^\s*OTHER\((\w+),\s*(.*?\))\)\s*\\?$", body, flags=re.M)}


def assert_expansions():
    """the list is the only place that names a flavoured kernel; the three expansions are what this module takes them for"""
    device_h, kernels, host_h, host = (read(f) for f in ("eggsim_device.h", "eggsim_relaxed.hip", "eggsim_host.h", "eggsim_host_relaxed.hip"))
    rows = gather_rows()
    # a gather's definition: rx_gather<G, K, D, S, W> over the groups and pointers the columns name, constants for the others
    assert re.search(r"#define EGG_RX_DEFINE_GATHER\(name, G, K, flavour, D, S, W, Mo, Sp, Ld\)\s*\\\n"
                     r'\s*extern "C" __global__ void __launch_bounds__\(256\) name\(EggRxPassArgs A\) \{\s*\\\n'
                     r"\s*rx_gather<G, K, D, S, W>\(A\.a, G \? A\.g : EggRxGroupFields\{\}, K \? A\.c : EggRxCohesionFields\{\},\s*\\\n"
                     r"\s*D \? A\.d : EggRxColliderFields\{\}, S \? A\.s : EggRxSurfaceFields\{\}, Mo \? &A\.m : nullptr,\s*\\\n"
                     r"\s*Sp \? &A\.r : nullptr, Ld \? &A\.l : nullptr\);\s*\\\n\s*\}", kernels)
    assert '#define EGG_RX_DEFINE_OTHER(name, ...) \\\n    extern "C" __global__ void __launch_bounds__(256) name(EggRxPassArgs A) { __VA_ARGS__; }' in kernels
    assert kernels.count("EGG_RX_PASS_KERNELS(EGG_RX_DEFINE_GATHER, EGG_RX_DEFINE_OTHER)") == 1
    # the declarations: every row, under its name, taking the one record
    assert '#define EGG_RX_DECLARE(name, ...) extern "C" __global__ void name(EggRxPassArgs A);\nEGG_RX_PASS_KERNELS(EGG_RX_DECLARE, EGG_RX_DECLARE)' in host_h
    # the table: a gather sits at [G][K][flavour], an OTHER row nowhere; launch_pass launches from it by (halo, cohesion, flavour)
    assert "#define EGG_RX_SLOT(name, G, K, flavour, ...) t.k[G][K][flavour] = name;\n#define EGG_RX_NO_SLOT(name, ...)\n" in host
    assert "RxPassKernel k[2][2][EGG_RX_FLAVOURS];" in host and "EGG_RX_PASS_KERNELS(EGG_RX_SLOT, EGG_RX_NO_SLOT)" in host
    assert host.count("hipLaunchKernelGGL(kRxGather.k[st.L.halo][st.L.cohesion][st.flavour], grid, block, 0, s.stream, a);") == 1
    assert host.count("kRxGather") == 2  # (the table and that launch)
    enum = re.search(r"enum EggRxFlavour \{([^}]*)\}", device_h).group(1)
    assert [w.strip() for w in enum.split(",")] == list(FLAVOURS) + ["EGG_RX_FLAVOURS"]
    # no slot is filled twice, none is left empty
    slots = [(r["G"], r["K"], r["flavour"]) for r in rows.values()]
    assert len(slots) == len(set(slots)) == 2 * 2 * len(FLAVOURS) == 28
    # a kernel of the list is named in the list and nowhere else in the four files
    for name in list(rows) + list(other_rows()):
        assert device_h.count(name) == 1, name
        assert kernels.count(name + "(") == 0 and host_h.count(name) == 0, name
    for name in rows:
        assert host.count(name) == 0, name
    return rows


def flavour_precedence():
    """the flavours in the order prepare_type tests the switches of RelaxedLayout: [(switch, flavour)], the last the default"""
    host = read("eggsim_host_relaxed.hip")
    expr = host[host.index("st.flavour = "):]
    expr = expr[:expr.index(";")]
    pairs = re.findall(r"st\.L\.(\w+)\s*\?\s*(EGG_RX_\w+)", expr)
    return pairs + [(None, re.search(r":\s*(EGG_RX_\w+)\s*$", expr).group(1))]
