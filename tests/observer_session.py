"""Sessions for the observers (sensors, probes, fields, pieces, impulses, measures) as data: a script is a fixed list of
events, a host-side layout model says where every batch lies after each of them, and situations() names the spots at which
an observer's cached table could go stale without the suite noticing.  Pure CPU: no library, no GPU.

The layout model restates three functions of egg_fluid_simulation_amd/csrc/eggsim_host_abi.hip:

* egg_import_batch (lines 735-791) inserts by KEY: the position is the first one whose key is not below the new key
  (742-745), the arrays of both types open a gap there and every later batch moves up (750-767), the batch gets the next id
  (775: ids are never reused) and next_key only rises (787).
* egg_remove (lines 292-329) compacts: the tail behind the removed atom moves down over it (307-320) and the batch leaves
  the order (326).
* add (add_many_impl, lines 220-285) appends: key = next_key (267-268), id = number of batches ever created + 1 (259).

upload_atoms (eggsim_host_state.hip, lines 131-172) lays the atoms out in that order, offset after offset, and bumps
atoms_gen; the unit tables of sensors, probes, fields and impulses split an atom into units of 1,024 particles.
tests/test_gpu_observer_session.py checks the model against download(w, "batch_id") at every observe.

A config event changes the radius and mass limits; the library re-derives radius and inverse mass in the next step
(eggsim_host_step.hip, lines 491-507), not in egg_set_config (eggsim_host_abi.hip, lines 184-190): so situation f) is
followed by a step and one more observe with the same arguments, reported as f_step.

Events (tuples; a batch is named by its label, the number of batches the script created before it):
  ("add", n_white)              ("remove", label)             ("export_remove", label)      ("import_back", label)
  ("import_front", n_white)     ("config", type, tweak)       ("order", "exact" | "relaxed") ("step", S, C)
  ("discarded_step",)           ("sensors", name)             ("observe", variant)          ("impulse", name)
  ("checkpoint",)
"""
INF = float("inf")
UNIT = 1024  # EGG_SN_UNIT and its twins: the particles of one unit of a unit table
# the kernels' seams, from COUNTS of tests/test_gpu_measures.py; its 1,024 and 2,100 are left out: the pieces model costs the
# square of an atom's size, and 1,025 is the smallest atom that crosses the unit boundary
COUNTS = (1, 63, 64, 65, 513, 1025)
N_YOLK = 15  # of an added batch
N_YOLK_FRONT = 2  # of a batch imported at the front
SPOTS = [(300.0 + 500.0 * (k % 4), 300.0 + 500.0 * (k // 4)) for k in range(12)]

# ------------------------------------------------------------------------------------------------ what the calls are given
SENSORS = {
    "white": [("disc", 300.0, 300.0, 80.0, "white"), ("half_plane", 1.0, 0.05, 815.0, "white"), ("capsule", 200.0, 800.0, 1900.0, 820.0, 60.0, "white")],
    "both": [("disc", 300.0, 300.0, 80.0), ("half_plane", 1.0, 0.05, 815.0, "white"), ("capsule", 200.0, 800.0, 1900.0, 820.0, 60.0, "yolk"),
             ("box", 1050.0, 550.0, 600.0, 200.0, 0.3)],
}
PROBES = {
    "a": [("point", 330.0, 300.0), ("point", 815.0, 320.0, 200.0), ("ray", 100.0, 310.0, 2000.0, 330.0), ("ray", 320.0, 100.0, 300.0, 1500.0, 2.0, "white"),
          ("point", 1300.0, 800.0, INF, "yolk")],
    "b": [("point", 1800.0, 300.0, INF, "white"), ("ray", 2000.0, 820.0, 100.0, 790.0, 1.0), ("point", 0.0, 0.0), ("ray", 1300.0, 100.0, 1310.0, 1500.0)],
}
GRIDS = {"a": (0.0, 0.0, 40.0, 56, 40), "b": (250.0, 250.0, 12.5, 64, 48)}
REGIONS = {None: None, "half": ("half_plane", 1.0, 0.05, 815.0), "capsule": ("capsule", 200.0, 800.0, 1900.0, 820.0, 60.0),
           "white_disc": ("disc", 1050.0, 550.0, 5000.0, "white")}
IMPULSES = {
    "gentle": [("kick", ("disc", 800.0, 300.0, 700.0), 30.0, -10.0, dict(by_inv_mass=True)), ("swirl", ("disc", 1300.0, 800.0, 600.0, "yolk"), 1300.0, 800.0, 1.5),
               ("brake", ("half_plane", 0.0, 1.0, 500.0), 5.0, 0.0, 0.25)],
    "blast": [("blast", ("disc", 800.0, 550.0, 900.0), 800.0, 550.0, 40.0, dict(linear=True)), ("kick", ("capsule", 200.0, 800.0, 1900.0, 820.0, 90.0, "white"), -3.0, 4.0)],
}
TWEAKS = {"wide": dict(min_radius=3.0, max_radius=5.5, min_mass=1.0, max_mass=2.5), "default": {}}

BASE = dict(ids="all", types="both", region=None, reach=None, probes="a", grid="a", twice=False, repeat=False)


def observe(**kw):
    assert not set(kw) - set(BASE), kw
    return ("observe", dict(BASE, **kw))


REPEAT = ("observe", "repeat")  # the previous observe's arguments exactly, once per call


# ------------------------------------------------------------------------------------------------ the scripts
def _exact():
    """the pieces model costs the square of an atom's size: the one batch above 1,024 is added, observed and removed at the
    start, and every later observe sees small atoms"""
    return [
        ("add", 63), ("add", 64), ("add", 1025), ("add", 65), ("add", 64),  # labels 0 .. 4
        ("sensors", "white"), observe(ids=("labels", (1, 3, 4))),  # before any step
        ("remove", 2), REPEAT,  # a) a middle one; d) 1,025 particles ahead of survivors; the same id list, labels 3 and 4 have moved
        ("step", 2, 3), ("checkpoint",), observe(twice=True),
        ("remove", 0), REPEAT,  # a) the first one in layout order
        ("remove", 4), REPEAT,  # a) the last one
        ("add", 65), REPEAT,  # b) label 5 gets id 6 and is appended
        ("add", 63), REPEAT,  # b) label 6
        ("step", 2, 3), ("checkpoint",),
        ("sensors", "both"), observe(ids="reversed", types="white", region="half", reach=1.0, probes="b", grid="b"),  # h) white -> both
        ("sensors", "white"), observe(ids="rotated", types="white", region="half", reach=1.0, probes="b", grid="b"),  # h) both -> white; permuted
        observe(ids="head2", types="yolk", region="capsule", reach=1.0, probes="b", grid="b"),  # mask and region change
        observe(ids="tail2", types="yolk", region="capsule", reach=1.5, probes="b", grid="b", twice=True),  # other ids, same length; reach; a listed call twice
        observe(),
        ("config", "white", "wide"), REPEAT,  # f) no table is rebuilt, nothing derived moved yet
        ("step", 2, 3), REPEAT, ("checkpoint",),  # f_step) radius and mass follow, still no table is rebuilt
        ("discarded_step",), REPEAT,  # g)
        ("step", 3, 1), ("checkpoint",),
        ("remove", 1), ("remove", 3), ("remove", 6),  # down to one batch (label 5)
        ("remove", 5), REPEAT,  # e) none
        ("add", 64), REPEAT,  # e) and back; b) as well
        ("step", 1, 1), ("checkpoint",),
    ]


def _relaxed():
    return [
        ("import_front", 1), ("add", 63), ("add", 1025), ("add", 64), ("add", 65),  # labels 0 .. 4
        ("sensors", "both"), observe(ids=("labels", (1, 3, 4))),
        ("export_remove", 2), REPEAT, ("impulse", "gentle"),  # a) a middle one; d) 1,025 particles ahead of survivors; j); the same id list
        ("step", 2, 3),
        ("import_back", 2), REPEAT, ("impulse", "blast"),  # c) strictly inside; d) an insertion; j); the same id list once more
        ("remove", 2), REPEAT,  # a) a middle one again: the large atom is gone for good
        ("step", 2, 3), observe(twice=True),
        ("import_front", 65), REPEAT, ("impulse", "gentle"),  # c) label 5 in front of everything; j)
        ("step", 1, 1),
        ("remove", 5), REPEAT,  # a) the first one
        ("remove", 4), REPEAT,  # a) the last one
        ("add", 64), REPEAT,  # b) label 6
        ("remove", 0), ("impulse", "gentle"),  # k) the impulse is the first call after the change: every offset moved by one white particle
        ("order", "exact"), REPEAT,  # j)
        ("step", 2, 3),
        ("order", "relaxed"), observe(ids="reversed", types="white", region="half", reach=1.0, probes="b", grid="b"),  # j)
        ("step", 2, 3),
        ("sensors", "white"), observe(ids="rotated", types="white", region="half", reach=1.0, probes="b", grid="b"),  # h) both -> white; permuted
        ("sensors", "both"), observe(ids="head2", types="yolk", region="white_disc", reach=1.0, probes="b", grid="b"),  # h) white -> both
        observe(ids="tail2", types="yolk", region="white_disc", reach=1.5, probes="b", grid="b", twice=True),
        observe(),
        ("config", "white", "wide"), REPEAT,  # f)
        ("step", 2, 3), REPEAT,  # f_step)
        ("remove", 1), ("remove", 3),  # down to one batch (label 6)
        ("remove", 6), REPEAT,  # e) none
        ("add", 65), REPEAT,  # e) and back
        ("step", 2, 3),
    ]


def _block():
    """the first of two interleaved handles: its largest atom is over 512 particles (the 256-thread class of pieces)"""
    return [
        ("add", 513), ("add", 64), ("add", 65), ("sensors", "both"), observe(twice=True),
        ("step", 2, 3),
        ("export_remove", 0), REPEAT,  # a) the first one
        ("import_back", 0), REPEAT,  # c) in front: the key is the lowest again
        ("remove", 1), REPEAT,  # a) a middle one
        ("step", 2, 3), observe(ids="reversed", reach=1.0, grid="b", probes="b"),
    ]


def _wave():
    """the second: every atom stays in the one-wave class of pieces"""
    return [
        ("add", 63), ("add", 65), ("add", 64), ("sensors", "white"), observe(twice=True),
        ("step", 2, 3),
        ("remove", 1), REPEAT,  # a) a middle one
        ("add", 65), REPEAT,  # b)
        ("remove", 0), REPEAT,  # a) the first one
        ("step", 2, 3), observe(ids="reversed", reach=1.0, grid="b", probes="b"),
    ]


_SCRIPTS = {"exact": _exact, "relaxed": _relaxed, "block": _block, "wave": _wave}
NAMES = tuple(sorted(_SCRIPTS))

COMMON = ("a_first", "a_middle", "a_last", "b", "d_remove", "e", "f", "f_step", "h_widen", "h_narrow", "i_a", "i_b", "i_d")
# what each script has to contain (the oracle has no import: c) and an insertion of d) are the relaxed script's; a relaxed
# handle refuses egg_step_begin: g) is the exact script's)
REQUIRED = {
    "exact": COMMON + ("g",),
    "relaxed": COMMON + ("c_back", "c_front", "d_insert", "i_c", "j_order", "j_a", "j_c", "j_d", "k"),
    "block": ("a_first", "a_middle", "c_front", "i_a", "i_c"),
    "wave": ("a_first", "a_middle", "b", "i_a", "i_b"),
}
# how the arguments of an observe differ from the previous one's
REQUIRED_CHANGES = {name: ("repeat", "repeat_listed", "twice", "other_ids", "permuted", "mask", "region", "reach") for name in ("exact", "relaxed")}
REQUIRED_CHANGES.update(block=("repeat", "twice"), wave=("repeat", "twice"))


def script(name):
    """the events of a named session, every ("observe", "repeat") written out as the previous observe's variant with
    repeat=True and twice=False"""
    events, last = [], None
    for e in _SCRIPTS[name]():
        if e == REPEAT:
            assert last is not None
            e = ("observe", dict(last, repeat=True, twice=False))
        if e[0] == "observe":
            last = e[1]
        events.append(e)
    return events


# ------------------------------------------------------------------------------------------------ the layout model
class Layout:
    """the live batches in key order: dicts of label, id, key and the counts n = (white, yolk)"""

    def __init__(self):
        self.batches, self.exported = [], {}
        self.created = 0  # batches ever created: the next id is created + 1
        self.labels = 0
        self.next_key = 1

    def copy(self):
        other = Layout()
        other.batches, other.exported = [dict(b) for b in self.batches], dict(self.exported)
        other.created, other.labels, other.next_key = self.created, self.labels, self.next_key
        return other

    def _insert(self, label, key, n):
        pos = 0
        while pos < len(self.batches) and self.batches[pos]["key"] < key:
            pos += 1
        assert pos == len(self.batches) or self.batches[pos]["key"] != key, "key %d is already present" % key
        self.created += 1
        self.batches.insert(pos, dict(label=label, id=self.created, key=key, n=tuple(n)))
        self.next_key = max(self.next_key, key + 1)
        return pos

    def _new_label(self):
        self.labels += 1
        return self.labels - 1

    def add(self, n_white):
        return self._insert(self._new_label(), self.next_key, (n_white, N_YOLK))

    def front_key(self):
        return min([b["key"] for b in self.batches] + [self.next_key]) - 1

    def import_front(self, n_white):
        return self._insert(self._new_label(), self.front_key(), (n_white, N_YOLK_FRONT))

    def position(self, label):
        return [b["label"] for b in self.batches].index(label)

    def remove(self, label, export=False):
        pos = self.position(label)
        b = self.batches.pop(pos)
        if export:
            self.exported[label] = b
        return pos

    def import_back(self, label):
        b = self.exported.pop(label)
        return self._insert(label, b["key"], b["n"])

    def ids(self):
        return [b["id"] for b in self.batches]

    def id_of(self, label):
        return self.batches[self.position(label)]["id"]

    def offsets(self, w):
        out, off = {}, 0
        for b in self.batches:
            out[b["label"]] = off
            off += b["n"][w]
        return out

    def units(self, w):
        return sum((b["n"][w] + UNIT - 1) // UNIT for b in self.batches)

    def batch_ids(self, w):
        """what download(w, "batch_id") holds"""
        return [b["id"] for b in self.batches for _ in range(b["n"][w])]


POPULATION = ("add", "remove", "export_remove", "import_back", "import_front")


def apply(layout, event):
    """one population event on the layout; returns the position it touched"""
    kind = event[0]
    if kind == "add":
        return layout.add(event[1])
    if kind == "import_front":
        return layout.import_front(event[1])
    if kind == "import_back":
        return layout.import_back(event[1])
    if kind in ("remove", "export_remove"):
        return layout.remove(event[1], kind == "export_remove")
    raise KeyError(kind)


def listed_ids(layout, selector):
    """the id list of an observe: None (every batch), a list made of the live ids in layout order, or the ids of
    ("labels", (label, ..))"""
    live = layout.ids()
    if selector == "all":
        return None
    if isinstance(selector, tuple) and selector[0] == "labels":
        return [layout.id_of(label) for label in selector[1]]
    return {"reversed": live[::-1], "rotated": live[1:] + live[:1], "head2": live[:2], "tail2": live[-2:]}[selector]


def walk(events):
    """per event (index, event, layout after it); the layouts are copies"""
    layout = Layout()
    for k, e in enumerate(events):
        if e[0] in POPULATION:
            apply(layout, e)
        yield k, e, layout.copy()


OBSERVERS = ("sensors", "probes", "field", "pieces", "labels", "measure")  # one model comparison each per observe
# which observer an observe calls first: the tuple above turned by this much, and by one more behind every population change
ROTATION_START = {"exact": 0, "relaxed": 2, "block": 0, "wave": 3}


def plan(events, start=0):
    """{event index: what the driver needs there}.  For an observe: the concrete id list, the live (id, n_white, n_yolk) in
    layout order, the order in which the observers are called (`order[0]` is the first call of the handle after the event
    before), whether an observe follows a population change at once (`fresh`), and the counts: `comparisons` with a model
    (one per observer; none on an empty handle, which has `empty_checks` instead) and `second_answers` (one per observer
    where twice is set).  For an impulse: 1 comparison, and `first` where it follows a population change at once."""
    out, turned = {}, start
    for k, e, layout in walk(events):
        if e[0] == "observe":
            n, empty = len(OBSERVERS), not layout.batches
            fresh = k > 0 and events[k - 1][0] in POPULATION
            order = tuple(OBSERVERS[(turned + j) % n] for j in range(n))
            out[k] = dict(ids=listed_ids(layout, e[1]["ids"]), layout=[(b["id"], b["n"][0], b["n"][1]) for b in layout.batches],
                          batch_ids=[layout.batch_ids(w) for w in (0, 1)], order=order, fresh=fresh, empty=empty,
                          comparisons=0 if empty else n, empty_checks=n if empty else 0, second_answers=n if e[1]["twice"] and not empty else 0)
            if fresh and not empty:
                turned += 1
        elif e[0] == "impulse":
            out[k] = dict(comparisons=1, empty_checks=0, second_answers=0, first=k > 0 and events[k - 1][0] in POPULATION)
    return out


def planned_comparisons(events):
    """how many comparisons with a model the session makes: from the script alone, never from a handle"""
    return sum(p["comparisons"] for p in plan(events).values())


def planned(events, what):
    """the sum of another count of plan(): `what` is "empty_checks" or "second_answers", for instance"""
    return sum(p[what] for p in plan(events).values())


def first_observers(events, start=0):
    """{observer: [event indices]}: the observes right behind a population change, by the observer they call first"""
    out = {}
    for k, p in sorted(plan(events, start).items()):
        if p.get("fresh") and not p["empty"]:
            out.setdefault(p["order"][0], []).append(k)
    return out


# ------------------------------------------------------------------------------------------------ situations
def situations(events):
    """{situation: [event indices]}: the index is that of the change, except for e) (the observe on the empty handle), i_*
    (the repeating observe) and j_a / j_c / j_d (the impulse).  A situation counts only where an observe is the NEXT event.

    a_first, a_middle, a_last: a removal of the first, a middle, the last batch in layout order (others survive);
    b: an add after a removal: a new id, appended;  c_back: import_back that lands strictly inside;  c_front: an import that
    lands in front of everything -- for both the first-particle offset of a survivor changes, for both types;
    d_remove, d_insert: a batch of more than 1,024 white particles leaves or enters ahead of a survivor: the unit count moves
    by more than one;  e: the observe on the handle that removals took down to one batch and then to none just before, with
    an add later on;  f: a config event that changes
    the radius and mass limits, then an observe with unchanged arguments;  f_step: the same followed by a step and such an
    observe again;  g: a discarded step;  h_widen, h_narrow: a sensor list that covers both types instead of white only, and
    the reverse, the atoms unchanged since the last observe;  i_a .. i_d: the observe behind a) .. d) repeats the previous
    one's arguments;  j_order: an order switch;  j_a, j_c, j_d: an impulse behind the observe that follows a), c), d);
    k: a population change with an impulse as the next event: the impulse is the handle's first call behind it."""
    found = {}

    def note(name, k):
        found.setdefault(name, []).append(k)

    def next_is_observe(k):
        return k + 1 < len(events) and events[k + 1][0] == "observe"

    layout = Layout()
    sizes = []  # the number of live batches after each population event
    removed_before = False
    cover = None  # of the sensor list
    population_since_observe = False
    for k, e in enumerate(events):
        kind = e[0]
        before = layout.copy()
        here = []  # the situations a) .. d) of this event
        if kind in POPULATION:
            pos = apply(layout, e)
            population_since_observe = True
            survivors = [b["label"] for b in layout.batches if b["label"] in before.offsets(0)]
            moved = [w for w in (0, 1) if any(before.offsets(w)[s] != layout.offsets(w)[s] for s in survivors)]
            if next_is_observe(k):
                if kind in ("remove", "export_remove") and len(before.batches) > 1:
                    here.append("a_first" if pos == 0 else "a_last" if pos == len(before.batches) - 1 else "a_middle")
                    n_white = before.batches[pos]["n"][0]
                    if n_white > UNIT and pos < len(before.batches) - 1 and before.units(0) - layout.units(0) > 1:
                        here.append("d_remove")
                if kind == "add" and removed_before and layout.batches[pos]["id"] == before.created + 1 and pos == len(layout.batches) - 1 \
                        and layout.batches[pos]["id"] not in before.ids():
                    here.append("b")
                if kind == "import_back" and 0 < pos < len(layout.batches) - 1 and moved == [0, 1]:
                    here.append("c_back")
                if kind in ("import_back", "import_front") and pos == 0 and len(layout.batches) > 1 and moved == [0, 1]:
                    here.append("c_front")
                if kind in ("import_back", "import_front") and layout.batches[pos]["n"][0] > UNIT and pos < len(layout.batches) - 1 \
                        and layout.units(0) - before.units(0) > 1:
                    here.append("d_insert")
            if kind in ("remove", "export_remove"):
                removed_before = True
        for name in here:
            note(name, k)
        if here:
            letters = sorted({name[0] for name in here})
            if events[k + 1][1]["repeat"]:
                for letter in letters:
                    note("i_" + letter, k + 1)
            if k + 2 < len(events) and events[k + 2][0] == "impulse":
                for letter in letters:
                    if letter != "b":
                        note("j_" + letter, k + 2)
        if kind in POPULATION:
            sizes.append(len(layout.batches))
            if k + 1 < len(events) and events[k + 1][0] == "impulse":
                note("k", k)
        if kind == "observe":
            # the last two population events were removals that left one batch and then none
            if events[k - 1][0] in ("remove", "export_remove") and sizes[-3:] == [2, 1, 0] and any(x[0] == "add" for x in events[k + 1:]):
                note("e", k)
            population_since_observe = False
        if kind == "config" and next_is_observe(k) and events[k + 1][1]["repeat"]:
            tweak = TWEAKS[e[2]]
            if {"min_radius", "max_radius", "min_mass", "max_mass"} <= set(tweak):
                note("f", k)
                if k + 3 < len(events) and events[k + 2][0] == "step" and events[k + 3][0] == "observe" and events[k + 3][1]["repeat"]:
                    note("f_step", k)
        if kind == "discarded_step" and next_is_observe(k):
            note("g", k)
        if kind == "sensors":
            new = 0
            for s in SENSORS[e[1]]:
                new |= {"white": 1, "yolk": 2}.get(s[-1], 3) if isinstance(s[-1], str) else 3
            if cover is not None and next_is_observe(k) and not population_since_observe and layout.batches:
                if cover == 1 and new == 3:
                    note("h_widen", k)
                if cover == 3 and new == 1:
                    note("h_narrow", k)
            cover = new
        if kind == "order" and next_is_observe(k):
            note("j_order", k)
    return found


def argument_changes(events):
    """{change: [event indices]} of the observes, each against the previous observe: repeat, repeat_listed (a repeat with a
    written-out id list right behind a population change: the list is the same, the offsets behind it are not), twice,
    other_ids (another list of the same length that is no permutation), permuted, mask, region, reach"""
    found, last = {}, None
    for k, e, layout in walk(events):
        if e[0] != "observe":
            continue
        v, ids = e[1], listed_ids(layout, e[1]["ids"])
        if v["twice"]:
            found.setdefault("twice", []).append(k)
        if last is not None:
            lv, lids = last
            if v["repeat"]:
                assert {key: v[key] for key in v if key not in ("repeat", "twice")} == {key: lv[key] for key in lv if key not in ("repeat", "twice")}
                assert ids == lids, (k, ids, lids)
                found.setdefault("repeat", []).append(k)
                if ids is not None and events[k - 1][0] in POPULATION:
                    found.setdefault("repeat_listed", []).append(k)
            if ids is not None and lids is not None and ids != lids and len(ids) == len(lids):
                found.setdefault("permuted" if sorted(ids) == sorted(lids) else "other_ids", []).append(k)
            for key, name in (("types", "mask"), ("region", "region"), ("reach", "reach")):
                if v[key] != lv[key]:
                    found.setdefault(name, []).append(k)
        last = (v, ids)
    return found


def describe(name):
    """the figures of a script for a report"""
    events = script(name)
    return dict(events=len(events), observes=sum(1 for e in events if e[0] == "observe"), comparisons=planned_comparisons(events),
                empty_checks=planned(events, "empty_checks"), second_answers=planned(events, "second_answers"),
                situations=situations(events), changes=argument_changes(events), first=first_observers(events, ROTATION_START[name]))


if __name__ == "__main__":
    for name in NAMES:
        d = describe(name)
        print("%s: %d events, %d observes, %d model comparisons, %d empty-answer checks, %d second answers" % (
            name, d["events"], d["observes"], d["comparisons"], d["empty_checks"], d["second_answers"]))
        print("  called first behind a change: " + ", ".join("%s@%s" % (s, d["first"][s]) for s in sorted(d["first"])))
        print("  situations: " + ", ".join("%s@%s" % (s, d["situations"][s]) for s in sorted(d["situations"])))
        print("  changes: " + ", ".join("%s@%s" % (s, d["changes"][s]) for s in sorted(d["changes"])))
