"""Helpers of the surface tests that read the C++ sources as text: what the host sides of the between-step calls share
(csrc/eggsim_host_scan.hip) is checked from several test modules."""
import os

from conftest import ROOT

CSRC = os.path.join(ROOT, "egg_fluid_simulation_amd", "csrc")
IN_FLIGHT = ("a step is in flight (egg_step_begin without egg_step_end)", "a step is in flight (egg_rx_begin without egg_rx_end)")
OBSERVER_UNITS = tuple("eggsim_host_%s.hip" % name for name in ("sensors", "probes", "fields", "pieces", "impulses", "measures"))


def sources():
    """every C++ source and header under csrc, by file name"""
    units = {}
    for unit in os.listdir(CSRC):
        if unit.endswith((".hip", ".cpp", ".h")):
            with open(os.path.join(CSRC, unit)) as f:
                units[unit] = f.read()
    return units


def in_flight_messages_have_one_home():
    """Both refusals of a call while a step is in flight are written once, in refuse_in_flight of the shared host layer."""
    units = sources()
    scan = units["eggsim_host_scan.hip"]
    body = scan[scan.index("int refuse_in_flight(egg_handle *h, const char *name) {"):]
    body = body[:body.index("\n}\n")]
    for text in IN_FLIGHT:
        assert sum(source.count(text) for source in units.values()) == 1 and text in body, text
    macro = units["eggsim_host.h"]
    macro = macro[macro.index("#define REJECT_IN_FLIGHT(h, name)"):]
    assert "egghost::refuse_in_flight(h, name);" in macro[:macro.index("while (0)")]
