"""The observer sessions of tests/observer_session.py, without a GPU and without the library: the scripts are fixed, every
script contains the situations it is there for, and the layout model does what the library's add, egg_remove and
egg_import_batch do.

The layout model against the source, egg_fluid_simulation_amd/csrc/eggsim_host_abi.hip:
  egg_import_batch, lines 742-745: the position is the first whose key is not below the new one, an equal key is refused;
                    lines 750-767: the tail of both types moves up by the batch's count; line 775: the id is the number of
                    batches ever created plus one; line 787: next_key only rises;
  egg_remove,       lines 307-320: the tail moves down over the removed atom; line 326: the batch leaves the order;
  add_many_impl,    lines 259-272: id and key of an added batch, appended to the order.
The GPU test holds the same model against download(w, "batch_id") at every observe of every session."""
import pytest

import observer_session as osn


@pytest.mark.parametrize("name", osn.NAMES)
def test_a_script_is_fixed(name):
    a, b = osn.script(name), osn.script(name)
    assert a == b and a is not b and repr(a) == repr(b)
    kinds = {"add", "remove", "export_remove", "import_back", "import_front", "config", "order", "step", "discarded_step", "sensors", "observe",
             "impulse", "checkpoint"}
    assert {e[0] for e in a} <= kinds
    for e in a:
        if e[0] in ("add", "import_front"):
            assert e[1] in osn.COUNTS, e  # (the kernels' seams, all below the 4,096 of pieces)
            assert e[0] == "import_front" or e[1] > 1  # (add creates no batch of one)
        if e[0] == "observe":
            assert set(e[1]) == set(osn.BASE)
    assert any(e[0] == "observe" for e in a)


@pytest.mark.parametrize("name", osn.NAMES)
def test_a_script_contains_its_situations(name):
    events = osn.script(name)
    found = osn.situations(events)
    for want in osn.REQUIRED[name]:
        assert found.get(want), "script %r lacks situation %s" % (name, want)
    changes = osn.argument_changes(events)
    for want in osn.REQUIRED_CHANGES[name]:
        assert changes.get(want), "script %r lacks an observe with the change %s" % (name, want)
    # a situation is only one where an observe follows at once (e, i_* and j_* name the observe or the impulse itself)
    for situation, where in found.items():
        for k in where:
            if situation == "e" or situation.startswith("i_"):
                assert events[k][0] == "observe"
            elif situation in ("j_a", "j_c", "j_d"):
                assert events[k][0] == "impulse" and events[k - 1][0] == "observe" and events[k - 2][0] in osn.POPULATION
            elif situation == "k":
                assert events[k][0] in osn.POPULATION and events[k + 1][0] == "impulse"
            else:
                assert events[k + 1][0] == "observe", (situation, k)


def test_the_counts_sit_on_the_seams_and_the_one_particle_batch_is_imported():
    """the chunk of a wave (63, 64, 65), one particle, and one batch per script beyond the 1,024 of a unit; the pieces model
    costs the square of an atom's size, so that batch is the smallest one beyond the seam and leaves early"""
    for name in ("exact", "relaxed"):
        used = {e[1] for e in osn.script(name) if e[0] in ("add", "import_front")}
        assert {63, 64, 65, 1025} <= used <= set(osn.COUNTS), name
    assert ("import_front", 1) in osn.script("relaxed")


def test_only_the_relaxed_script_has_impulses_imports_and_order_switches():
    kinds = {e[0] for e in osn.script("exact")}
    assert not kinds & {"impulse", "order", "import_back", "import_front", "export_remove"}  # (the oracle has none of them)
    assert {"impulse", "order", "import_back", "import_front", "export_remove"} <= {e[0] for e in osn.script("relaxed")}
    assert "checkpoint" in kinds and "discarded_step" in kinds


def test_the_interleaved_scripts_sit_on_both_sides_of_the_wave_class_of_pieces():
    largest = {name: max(e[1] for e in osn.script(name) if e[0] == "add") for name in ("block", "wave")}
    assert largest["block"] > 512 > largest["wave"]


# ------------------------------------------------------------------------------------------------ the layout model
def _labels(layout):
    return [b["label"] for b in layout.batches]


def test_the_layout_model_orders_by_key_and_compacts():
    lay = osn.Layout()
    for n in (63, 2100, 64, 1025):
        lay.add(n)
    assert lay.ids() == [1, 2, 3, 4] and [b["key"] for b in lay.batches] == [1, 2, 3, 4]
    assert lay.offsets(0) == {0: 0, 1: 63, 2: 2163, 3: 2227} and lay.offsets(1) == {0: 0, 1: 15, 2: 30, 3: 45}
    assert lay.units(0) == 1 + 3 + 1 + 2 and lay.units(1) == 4
    # a removal compacts: everything behind moves down, by the count of each type
    assert lay.remove(1, export=True) == 1
    assert _labels(lay) == [0, 2, 3] and lay.offsets(0) == {0: 0, 2: 63, 3: 127} and lay.offsets(1) == {0: 0, 2: 15, 3: 30}
    assert lay.units(0) == 4
    # an added batch is appended with the next key and the next id, whatever was removed
    assert lay.add(65) == 3 and lay.ids() == [1, 3, 4, 5] and lay.batches[-1]["key"] == 5
    # the exported batch comes back by its key, into the middle, with a NEW id; the ones behind move up
    assert lay.import_back(1) == 1
    assert _labels(lay) == [0, 1, 2, 3, 4] and lay.ids() == [1, 6, 3, 4, 5] and [b["key"] for b in lay.batches] == [1, 2, 3, 4, 5]
    assert lay.offsets(0) == {0: 0, 1: 63, 2: 2163, 3: 2227, 4: 3252}
    # in front of everything: a key below every live key, next_key stays
    assert lay.front_key() == 0 and lay.import_front(1) == 0
    assert lay.ids() == [7, 1, 6, 3, 4, 5] and lay.offsets(0)[0] == 1 and lay.offsets(1)[0] == osn.N_YOLK_FRONT and lay.next_key == 6
    assert lay.front_key() == -1
    assert lay.batch_ids(0)[:3] == [7, 1, 1] and len(lay.batch_ids(0)) == 1 + 63 + 2100 + 64 + 1025 + 65
    with pytest.raises(AssertionError, match="already present"):
        lay._insert(99, 3, (5, 5))
    # down to nothing and back: the keys and ids go on
    for label in list(_labels(lay)):
        lay.remove(label)
    assert lay.ids() == [] and lay.units(0) == 0 and lay.front_key() == 5
    assert lay.add(64) == 0 and lay.ids() == [8] and lay.batches[0]["key"] == 6


def test_listed_ids():
    lay = osn.Layout()
    for n in (63, 64, 65, 513):
        lay.add(n)
    assert osn.listed_ids(lay, "all") is None and lay.ids() == [1, 2, 3, 4]
    assert osn.listed_ids(lay, "reversed") == [4, 3, 2, 1] and osn.listed_ids(lay, "rotated") == [2, 3, 4, 1]
    assert osn.listed_ids(lay, "head2") == [1, 2] and osn.listed_ids(lay, "tail2") == [3, 4]
    assert osn.listed_ids(lay, ("labels", (3, 0))) == [4, 1]
    lay.remove(1)
    assert osn.listed_ids(lay, ("labels", (3, 0))) == [4, 1] and osn.listed_ids(lay, "rotated") == [3, 4, 1]


def test_situations_on_hand_made_scripts():
    """what situations() finds and, as important, what it does not: a step between the change and the observe hides it"""
    o = osn.observe()
    r = ("observe", dict(o[1], repeat=True))
    adds = [("add", 63), ("add", 1025), ("add", 64), o]
    assert osn.situations(adds) == {}
    assert osn.situations(adds + [("remove", 1), r]) == {"a_middle": [4], "d_remove": [4], "i_a": [5], "i_d": [5]}
    assert osn.situations(adds + [("remove", 1), ("step", 2, 3), r]) == {}
    assert osn.situations(adds + [("remove", 0), o]) == {"a_first": [4]}
    assert osn.situations(adds + [("remove", 2), o, ("impulse", "gentle")]) == {"a_last": [4], "j_a": [6]}
    assert osn.situations(adds + [("remove", 1), ("add", 65), r]) == {"b": [5], "i_b": [6]}
    assert osn.situations(adds + [("add", 65), r]) == {}  # (no remove before it)
    back = adds + [("export_remove", 1), ("step", 2, 3), ("import_back", 1), r]
    assert osn.situations(back) == {"c_back": [6], "d_insert": [6], "i_c": [7], "i_d": [7]}
    assert osn.situations(adds + [("export_remove", 2), ("step", 2, 3), ("import_back", 2), r]) == {}  # (at the end: nothing moves)
    assert osn.situations(adds + [("import_front", 1), o]) == {"c_front": [4]}
    empty = adds + [("remove", 0), ("remove", 1), ("remove", 2), o]
    assert osn.situations(empty) == {} and osn.situations(empty + [("add", 63)]) == {"e": [7]}
    # e) wants removals down to one batch and then to none right before the observe, not an add in between
    assert osn.situations(adds + [("remove", 0), ("remove", 1), ("add", 65), ("remove", 2), ("remove", 3), o, ("add", 63)]) == {"e": [9]}
    assert osn.situations([("add", 63), ("remove", 0), o, ("add", 63)]) == {}  # (it never stood at two and at one)
    assert osn.situations(adds + [("remove", 1), ("impulse", "gentle")]) == {"k": [4]}
    assert osn.situations(adds + [("config", "white", "wide"), r, ("step", 2, 3), r]) == {"f": [4], "f_step": [4]}
    assert osn.situations(adds + [("config", "white", "wide"), o]) == {}  # (other arguments: a table may be rebuilt anyway)
    assert osn.situations(adds + [("config", "white", "default"), r]) == {}  # (no limit changes)
    assert osn.situations(adds + [("discarded_step",), o]) == {"g": [4]}
    sens = [("sensors", "white")] + adds + [("sensors", "both"), o, ("sensors", "white"), o]
    assert osn.situations(sens) == {"h_widen": [5], "h_narrow": [7]}
    assert osn.situations([("sensors", "white")] + adds + [("add", 64), ("sensors", "both"), o]) == {}  # (the atoms changed as well)
    assert osn.situations(adds + [("order", "relaxed"), o]) == {"j_order": [4]}


# ------------------------------------------------------------------------------------------------ the plan
@pytest.mark.parametrize("name", osn.NAMES)
def test_the_plan_counts_the_comparisons_from_the_script_alone(name):
    events = osn.script(name)
    plan = osn.plan(events, osn.ROTATION_START[name])
    observes = [k for k, e in enumerate(events) if e[0] == "observe"]
    impulses = [k for k, e in enumerate(events) if e[0] == "impulse"]
    assert sorted(plan) == sorted(observes + impulses)
    empty = [k for k in observes if not plan[k]["layout"]]
    assert [k for k in observes if plan[k]["empty"]] == empty and len(empty) == len(osn.situations(events).get("e", []))
    # one model comparison per observer and observe with particles, one per impulse; the empty handle's answers and the
    # second answers of a call made twice are counted apart
    want = 6 * (len(observes) - len(empty)) + len(impulses)
    assert osn.planned_comparisons(events) == want == osn.describe(name)["comparisons"] and want > 0
    assert osn.planned(events, "empty_checks") == 6 * len(empty)
    assert osn.planned(events, "second_answers") == 6 * sum(1 for k in observes if events[k][1]["twice"] and k not in empty) > 0
    for k in observes:
        p = plan[k]
        assert [len(b) for b in p["batch_ids"]] == [sum(n[1 + w] for n in p["layout"]) for w in (0, 1)]
        assert p["ids"] is None or set(p["ids"]) <= {i for i, _, _ in p["layout"]}
        assert sorted(p["order"]) == sorted(osn.OBSERVERS) and p["fresh"] == (events[k - 1][0] in osn.POPULATION)
    assert len({i for p in plan.values() if "layout" in p for i, _, _ in p["layout"]}) == sum(
        1 for e in events if e[0] in ("add", "import_front", "import_back"))  # (every batch ever created is observed: no id is reused)


def test_every_observer_is_the_first_call_behind_some_change():
    """download(w, "batch_id") rebuilds the atoms itself: only the FIRST call behind a population change finds atoms_dirty set,
    so the observers take turns at being it, and in the relaxed script an impulse is it once"""
    for name in ("exact", "relaxed"):
        first = osn.first_observers(osn.script(name), osn.ROTATION_START[name])
        assert set(first) == set(osn.OBSERVERS), (name, first)
        found = osn.situations(osn.script(name))
        behind = {k + 1 for s in ("a_first", "a_middle", "a_last", "b", "c_back", "c_front", "d_remove", "d_insert") for k in found.get(s, [])}
        assert all(behind & set(where) for where in first.values()), (name, first, behind)  # (each behind one of a) to d))
    both = {}
    for name in ("block", "wave"):
        both.update(osn.first_observers(osn.script(name), osn.ROTATION_START[name]))
    assert set(both) == set(osn.OBSERVERS)
    events = osn.script("relaxed")
    k = osn.situations(events)["k"][0]
    assert events[k][0] == "remove" and events[k + 1][0] == "impulse" and osn.plan(events)[k + 1]["first"]
    assert sum(1 for p in osn.plan(events).values() if p.get("first")) == 1


def test_a_listed_call_is_made_twice_in_a_row():
    """measures keeps its rows per id list: two identical listed calls in a row hit that cache"""
    for name in ("exact", "relaxed"):
        events = osn.script(name)
        plan = osn.plan(events)
        assert any(e[0] == "observe" and e[1]["twice"] and plan[k]["ids"] is not None and len(plan[k]["ids"]) > 1 for k, e in enumerate(events)), name
