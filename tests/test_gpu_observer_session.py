"""The observers (sensors, probes, fields, pieces, impulses, measures; DESIGN.md sections 2.8 - 2.13) across sessions in
which the particle layout moves under them: batches are removed from the front, the middle and the end, added after a
removal, exported, removed and imported back by their key into the middle, imported in front of everything, the handle is
emptied and filled again, configs change live, steps are discarded, the sensor list changes its coverage, the solver order
switches, and batches are handed to another handle of a device group or to another rank.  Each observer keeps a table of
the layout that it rebuilds only when System::atoms_gen moved: a stale table reads the right arrays at the wrong offsets
and returns plausible integers, which only a comparison with a model evaluated on the handle's own downloads notices.

The scripts, the host-side layout model and the situations they contain are tests/observer_session.py (checked without a
GPU by tests/test_observer_session.py).  Every comparison is exact and goes through the helpers of the observers' own GPU
tests; the number of comparisons made must be the number the script plans.

download(w, "batch_id") and export_batch rebuild the atom table themselves (egg_download_particles and egg_export_batch call
upload_atoms), and every helper downloads before it calls its observer.  So at an observe the six observers are first called
on their own, before any download, in an order that turns by one behind every population change: each of them is the
handle's first call behind some change, where its own upload_atoms is what notices.  Those answers are kept, the helpers then
hold a later call against the model, and the kept answers have to equal the model's too."""
import warnings

import numpy as np
import pytest

import impulse_model as im
import observer_session as osn
import pieces_model as pcm
import sensor_model as sm
from conftest import ROOT
from test_gpu_fields import _as_model, _assert_field
from test_gpu_fuzz import _same as _same_as_oracle
from test_gpu_impulses import _assert_impulse
from test_gpu_impulses import _results as _impulse_results
from test_gpu_measures import _assert_measure
from test_gpu_pieces import _assert_labels, _assert_pieces
from test_gpu_probes import _assert_probes, _template
from test_gpu_sensors import _assert_reads
from test_gpu_sensors import _downloads as _sensor_downloads

pytestmark = pytest.mark.gpu

WHITE, YOLK = 0, 1
H60 = 1 / 60
INF = float("inf")
COLLIDERS = [("container", 1050.0, 800.0, 1500.0), ("disc", 560.0, 300.0, 30.0)]
FORCE = [("uniform", 0.0, 300.0)]


@pytest.fixture(scope="module")
def egg():
    import egg_fluid_simulation_amd as e
    return e


def _equal(a, b):
    """two answers of one helper"""
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.shape == b.shape and a.dtype.kind == b.dtype.kind and np.array_equal(a, b)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_equal(p, q) for p, q in zip(a, b))
    return a == b


def _plain(res):
    return [tuple(None if t is None else tuple(t) for t in pair) for pair in res]


class Session:
    """one script on one handle, optionally with the oracle beside it"""

    def __init__(self, egg, name, oracle_mod=None):
        self.egg, self.name, self.events = egg, name, osn.script(name)
        self.plan = osn.plan(self.events, osn.ROTATION_START[name])
        self.h = egg.SimulationHandler()
        self.o = oracle_mod.Oracle() if oracle_mod is not None else None
        self.oracle_mod = oracle_mod
        self.layout = osn.Layout()
        self.order = "exact"
        self.exports, self.sensors, self.steps, self.at = {}, [], 0, 0
        self.comparisons = self.second_answers = self.empty_checks = self.checkpoints = 0
        self.first_calls = []  # (event index, who) of the calls that were a handle's first behind a population change
        self.before_config = None

    def relaxed(self):
        self.h.set_solver_order("relaxed")
        self.h.set_colliders(COLLIDERS)
        self.h.set_forces(FORCE)
        self.order = "relaxed"
        return self

    # ---- the events
    def _spot(self, label):
        return osn.SPOTS[label % len(osn.SPOTS)]

    def _new_batch(self, e):
        label = self.layout.labels
        x, y = self._spot(label)
        if e[0] == "add":
            radius = 50.0 if e[1] < 1000 else 120.0
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", self.egg.EggWarning)
                i = self.h.add(x, y, radius, 15.0, None, None, e[1], osn.N_YOLK)
            if self.o is not None:
                assert self.o.add(x, y, radius, 15.0, e[1], osn.N_YOLK) == i
        else:
            info, ws, ys = _template(self.egg, e[1], osn.N_YOLK_FRONT)
            ws, ys = ws.copy(), ys.copy()
            for state in (ws, ys):
                state[0] += x
                state[4] += x
                state[1] += y
                state[5] += y
            i = self.h.import_batch(dict(info, key=self.layout.front_key(), target_x=x, target_y=y), ws, ys)
        return i

    def _targets(self):
        for b in self.layout.batches:
            x, y = self._spot(b["label"])
            t = 0.7 * self.steps + b["label"]
            for s in (self.h, self.o):
                if s is not None:
                    s.set_target_position(b["id"], x + 40.0 * float(np.cos(t)), y + 40.0 * float(np.sin(t)))

    def run_event(self):
        k, e = self.at, self.events[self.at]
        self.at += 1
        kind, h = e[0], self.h
        if kind in ("add", "import_front"):
            got = self._new_batch(e)
            pos = osn.apply(self.layout, e)
            assert got == self.layout.batches[pos]["id"], (self.name, k, e)
        elif kind in ("remove", "export_remove"):
            i = self.layout.id_of(e[1])
            if kind == "export_remove":
                self.exports[e[1]] = h.export_batch(i)
            h.remove(i)
            if self.o is not None:
                self.o.remove(i)
            osn.apply(self.layout, e)
        elif kind == "import_back":
            info, ws, ys = self.exports.pop(e[1])
            got = h.import_batch(info, ws, ys)
            pos = osn.apply(self.layout, e)
            assert got == self.layout.batches[pos]["id"] and info["key"] == self.layout.batches[pos]["key"], (self.name, k, e)
        elif kind == "config":
            from egg_fluid_simulation_amd.default_config import default_configs
            which = (WHITE, YOLK)[("white", "yolk").index(e[1])]
            cfg = default_configs()[which]
            cfg.update(osn.TWEAKS[e[2]])
            self.before_config = [h.download(which, f) for f in ("radius", "inv_mass")] + [which]
            (h.set_white_config if which == WHITE else h.set_yolk_config)(cfg)
            if self.o is not None:
                base = self.oracle_mod.DEFAULT_WHITE if which == WHITE else self.oracle_mod.DEFAULT_YOLK
                self.o.set_config(which, dict(base, **osn.TWEAKS[e[2]]))
        elif kind == "order":
            assert self.o is None
            if e[1] == "exact":
                h.set_colliders([])
                h.set_forces([])
                h.set_solver_order("exact")
            else:
                self.relaxed()
            self.order = e[1]
        elif kind == "step":
            self._targets()
            h.step(H60, e[1], e[2])
            if self.o is not None:
                self.o.step(H60, e[1], e[2])
            self.steps += 1
        elif kind == "discarded_step":
            assert self.order == "exact"  # (a relaxed handle refuses egg_step_begin)
            self._targets()
            h.step_begin(H60, 2, 3)
            h.step_end(False)
        elif kind == "sensors":
            self.sensors = osn.SENSORS[e[1]]
            h.set_sensors(self.sensors)
        elif kind == "checkpoint":
            _same_as_oracle(h, self.o, (self.name, k))
            self.checkpoints += 1
        elif kind == "impulse":
            if self.plan[k]["first"]:
                self._checked(k, e, "impulse (the first call behind the change)", e[1], lambda: self._impulse_first(k, e))
            else:
                self._checked(k, e, "impulse", e[1], lambda: _assert_impulse(h, osn.IMPULSES[e[1]], "%s event %d" % (self.name, k)))
            self.comparisons += 1
        elif kind == "observe":
            self._observe(k, e)
        else:
            raise KeyError(kind)
        return kind

    def run(self):
        while self.at < len(self.events):
            self.run_event()
        self.finish()
        return self

    def finish(self):
        planned = osn.planned_comparisons(self.events)
        print("%s: %d events, %d observes, %d model comparisons made, %d planned, %d empty-answer checks, %d second answers, %d checkpoints; "
              "first behind a change: %s" % (self.name, len(self.events), sum(1 for e in self.events if e[0] == "observe"), self.comparisons, planned,
                                             self.empty_checks, self.second_answers, self.checkpoints, self.first_calls))
        assert self.at == len(self.events) and self.comparisons == planned, (self.name, self.comparisons, planned)
        assert self.empty_checks == osn.planned(self.events, "empty_checks") and self.second_answers == osn.planned(self.events, "second_answers")
        want = sorted((k, who) for who, where in osn.first_observers(self.events, osn.ROTATION_START[self.name]).items() for k in where)
        assert sorted(c for c in self.first_calls if c[1] != "impulse") == want, (self.name, self.first_calls, want)

    # ---- an observe
    def _checked(self, k, e, observer, arguments, call):
        try:
            return call()
        except Exception:
            print("MISMATCH in script %r at event %d %r: observer %s with %r (the helper's line above names the first differing word)" % (
                self.name, k, e, observer, arguments))
            raise

    def _raw(self, observer, p, v):
        """one observer's own answer, as plain comparable values; nothing is downloaded"""
        h = self.h
        ids, types, region, reach = p["ids"], v["types"], osn.REGIONS[v["region"]], v["reach"]
        probes, (x0, y0, cell, nx, ny), velocity = osn.PROBES[v["probes"]], osn.GRIDS[v["grid"]], v["grid"] == "a"
        if observer == "sensors":
            return (h.sensor_sums(), h.sensor_batches([i for i, _, _ in p["layout"]] if ids is None else ids))
        if observer == "probes":
            return _plain(h.probe(probes))
        if observer == "field":
            return _as_model(h.field((x0, y0), cell, (nx, ny), types, velocity))
        if observer == "pieces":
            return _plain(h.pieces(ids, reach, types))
        if observer == "labels":
            return [a for a in h.piece_labels(reach, types)]
        return h.measure_table(ids, region, types)

    def _observe(self, k, e):
        """The observers' own calls come first, in the order the plan gives, before anything is downloaded: download(w,
        "batch_id") and export_batch run upload_atoms themselves and would leave the observer nothing to notice.  Then each
        helper holds the observer against its model on the downloads, and the answer kept from the first round has to be the
        model's as well."""
        h, v, p = self.h, e[1], self.plan[k]
        what = "%s event %d" % (self.name, k)
        ids, types, region, reach = p["ids"], v["types"], osn.REGIONS[v["region"]], v["reach"]
        probes, grid, velocity = osn.PROBES[v["probes"]], osn.GRIDS[v["grid"]], v["grid"] == "a"
        if p["empty"]:
            self._observe_empty(k, e, what, region, reach, types, probes, grid)
            self._check_layout(p, what)
            return
        kept = {}
        for observer in p["order"]:
            kept[observer] = self._checked(k, e, observer + " (its own call, before any download)", v, lambda: self._raw(observer, p, v))
            if v["twice"]:  # a cache hit: the same call once more at once, the same answer
                again = self._raw(observer, p, v)
                if not _equal(kept[observer], again):
                    print("MISMATCH in script %r at event %d %r: %s answered differently the second time in a row" % (self.name, k, e, observer))
                assert _equal(kept[observer], again), (what, observer, "the second call in a row answered differently")
                self.second_answers += 1
        self._check_layout(p, what)
        listed = [i for i, _, _ in p["layout"]] if ids is None else ids
        calls = {
            "sensors": ((self.sensors, ids), lambda: (_assert_reads(h, self.sensors, what, ids),
                                                      sm.read_batches(self.sensors, *_sensor_downloads(h), listed))),
            "probes": ((probes,), lambda: _assert_probes(h, probes, what)),
            "field": ((grid, types, velocity), lambda: _as_model(_assert_field(h, grid, what, types, velocity))),
            "pieces": ((ids, reach, types), lambda: [tuple(pcm.summary(r) for r in pair) for pair in _assert_pieces(h, ids, reach, types, what)]),
            "labels": ((reach, types), (lambda: (lambda want: [want[w] for w in (WHITE, YOLK)])(_assert_labels(h, reach, types, what)))),
            "measure": ((ids, region, types), lambda: _assert_measure(h, ids, region, types, what)),
        }
        assert tuple(calls) == osn.OBSERVERS
        for observer in p["order"]:
            arguments, call = calls[observer]
            answer = self._checked(k, e, observer, arguments, call)
            self.comparisons += 1
            # what the helper returns is the model's answer, or the observer's that it has just held against the model
            if not _equal(kept[observer], answer):
                print("MISMATCH in script %r at event %d %r: the call of %s made before any download, with %r, is not the model's answer" % (
                    self.name, k, e, observer, arguments))
            assert _equal(kept[observer], answer), (what, observer, "the call made before any download is not the model's answer")
        if p["fresh"]:
            self.first_calls.append((k, p["order"][0]))
        if self.before_config is not None and self.events[k - 1][0] == "step":
            # f_step) the step after the config re-derived radius and inverse mass: the answers above followed them
            radius, inv_mass, which = self.before_config
            assert not np.array_equal(h.download(which, "radius"), radius) and not np.array_equal(h.download(which, "inv_mass"), inv_mass), what
            self.before_config = None

    def _check_layout(self, p, what):
        """the layout model against the handle (behind the observers' calls: the download rebuilds the atoms)"""
        h = self.h
        assert sorted(h.list_ids()) == sorted(i for i, _, _ in p["layout"]), what
        for w in (WHITE, YOLK):
            got = h.download(w, "batch_id")
            assert got.size == len(p["batch_ids"][w]) and np.array_equal(got, np.array(p["batch_ids"][w], dtype=got.dtype)), (what, "layout", w)
        for i, nw, ny in p["layout"]:
            assert tuple(h.get_n_particles(i)) == (nw, ny), what

    def _impulse_first(self, k, e):
        """an impulse as the handle's FIRST call behind a population change: what _assert_impulse checks, with the columns that
        need no atom table downloaded before the call and batch_id only behind it"""
        h, records, what = self.h, osn.IMPULSES[e[1]], "%s event %d" % (self.name, k)
        names = ("x", "y", "vx", "vy", "inv_mass", "last_x", "last_y")
        before = {(w, f): h.download(w, f) for w in (WHITE, YOLK) for f in names}
        got = h.impulse(records)
        bid = [h.download(w, "batch_id").astype(np.int64) for w in (WHITE, YOLK)]
        want_vx, want_vy, want = im.apply(records, *[[before[w, f] for w in (WHITE, YOLK)] for f in names[:5]], bid, known_ids=set(h.list_ids()))
        print("%s: the first call behind the change: %s" % (what, got[:3]))
        assert got == _impulse_results(want), what
        for w in (WHITE, YOLK):
            assert np.array_equal(h.download(w, "vx").view(np.uint64), want_vx[w].view(np.uint64)), (what, w, "vx")
            assert np.array_equal(h.download(w, "vy").view(np.uint64), want_vy[w].view(np.uint64)), (what, w, "vy")
            for f in ("x", "y", "last_x", "last_y", "inv_mass"):
                assert np.array_equal(h.download(w, f).view(np.uint64), before[w, f].view(np.uint64)), (what, w, f)
        assert sum(sum(r.count) for r in got) > 0, what
        self.first_calls.append((k, "impulse"))

    def _observe_empty(self, k, e, what, region, reach, types, probes, grid):
        """a handle without batches: every call returns its empty answer and launches nothing"""
        h, v = self.h, e[1]
        x0, y0, cell, nx, ny = grid
        assert list(h.get_n_particles()) == [0, 0], what
        launches = h.stats()["kernel_launches"]
        for _ in range(2 if v["twice"] else 1):
            sums, dropped = h.sensor_sums()
            assert sums == [((0, 0, 0), (0, 0, 0))] * len(self.sensors) and dropped == [0, 0] and len(self.sensors) > 0, what
            assert h.sensor_batches([]).shape == (0, len(self.sensors), 2), what
            assert h.probe(probes) == [(None, None)] * len(probes), what
            f = h.field((x0, y0), cell, (nx, ny), types, True)
            assert not f.count.any() and not f.svx.any() and not f.svy.any() and f.inside == f.outside == f.dropped == (0, 0), what
            assert h.pieces(None, reach, types) == [] and h.pieces([], reach, types) == [], what
            labels = h.piece_labels(reach, types)
            assert len(labels) == 2 and all(a.dtype == np.int32 and a.size == 0 for a in labels), what
            assert h.measure_table(None, region, types).shape == (0, 2, 24) and h.measure(None, region, types) == [], what
        self.empty_checks += len(osn.OBSERVERS)  # (no model is evaluated here: counted apart from the comparisons)
        with pytest.raises(self.egg.EggError, match="no batch with id"):
            h.measure_table([1])
        assert h.stats()["kernel_launches"] == launches, (what, "a call on the empty handle launched a kernel")


# ------------------------------------------------------------------------------------------------ one handle
def test_exact_session_beside_the_oracle(egg, oracle_mod):
    """the exact-order script on a handle and on the oracle side by side: at every observe the five read-only calls equal
    their models on the handle's downloads, at every checkpoint the particles and pair_solves equal the oracle's bit for bit
    -- the observers only observed"""
    s = Session(egg, "exact", oracle_mod).run()
    assert s.checkpoints == sum(1 for e in s.events if e[0] == "checkpoint") >= 5
    assert s.second_answers == len(osn.OBSERVERS) * sum(1 for e in s.events if e[0] == "observe" and e[1]["twice"]) > 0
    assert {who for _, who in s.first_calls} == set(osn.OBSERVERS)  # (each observer was the first call behind some change)
    assert s.h.stats()["pair_solves"] == s.o.total_visited > 0


def test_relaxed_session_with_impulses(egg):
    """the relaxed script under colliders and a force: imports by key into the middle and in front, order switches, and an
    impulse right behind a population change"""
    s = Session(egg, "relaxed").relaxed().run()
    assert {who for _, who in s.first_calls} == set(osn.OBSERVERS) | {"impulse"}
    assert s.h.get_solver_order() == "relaxed" and s.h.stats()["relaxed_steps"] > 0


def test_two_handles_interleaved(egg):
    """two handles alive in one process, their events alternated: the first one's largest atom is above the one-wave class
    of pieces, the second one's below it (the LDS grant is a per-process attribute of the kernel, remembered per handle)"""
    a, b = Session(egg, "block"), Session(egg, "wave")
    while a.at < len(a.events) or b.at < len(b.events):
        for s in (a, b):
            if s.at < len(s.events):
                s.run_event()
    a.finish()
    b.finish()
    assert {who for s in (a, b) for _, who in s.first_calls} == set(osn.OBSERVERS)
    assert max(n for _, n, _ in a.plan[4]["layout"]) > 512 > max(n for p in b.plan.values() for _, n, _ in p.get("layout", []))


# ------------------------------------------------------------------------------------------------ a device group
EGGS = ((300.0, 300.0), (360.0, 310.0), (330.0, 250.0), (420.0, 330.0))
CUT = 335.0
EGG_SENSORS = [("disc", 330.0, 300.0, 60.0), ("disc", 360.0, 310.0, 25.0, "yolk"), ("box", 380.0, 320.0, 70.0, 30.0, 0.4), ("half_plane", 1.0, 0.0, 345.0),
               ("capsule", 250.0, 380.0, 750.0, 380.0, 90.0, "white")]
EGG_PROBES = [("point", 330.0, 300.0), ("point", 0.0, 0.0), ("point", 700.0, 300.0, 80.0), ("ray", 100.0, 300.0, 800.0, 310.0), ("ray", 700.0, 100.0, 690.0, 500.0, 2.0, "white")]
EGG_GRID = (200.0, 180.0, 9.0, 72, 32)  # [200, 848) x [180, 468)
EGG_REGION = ("box", 345.0, 300.0, 60.0, 25.0, 0.4)
EGG_RECORDS = [("kick", ("disc", 330.0, 300.0, 60.0), 30.0, -10.0, dict(by_inv_mass=True)), ("swirl", ("disc", 360.0, 310.0, 40.0, "yolk"), 360.0, 310.0, 1.5),
               ("brake", ("half_plane", 0.0, 1.0, 300.0), 5.0, 0.0, 0.25)]


def _listed(ids):
    return [ids[-1], ids[0], ids[-1], ids[1]]


def _answers(s, ids, turn=0):
    """every read-only call a group or a sharded handler offers, as plain comparable values; `turn` says which of them is
    called first (the first call behind a hand-over is the one whose tables have to notice it)"""
    origin, cell, shape = EGG_GRID[:2], EGG_GRID[2], EGG_GRID[3:]
    calls = [("sums", lambda: s.sensor_sums()), ("hits", lambda: _plain(s.probe(EGG_PROBES))),
             ("field", lambda: [np.asarray(a).tolist() if isinstance(a, np.ndarray) else a for a in _as_model(s.field(origin, cell, shape, velocity=True))]),
             ("pieces", lambda: _plain(s.pieces())), ("every", lambda: s.measure_table().tolist()),
             ("batches", lambda: s.sensor_batches(_listed(ids)).tolist()), ("white_field", lambda: s.field(origin, cell, shape, "white").count.tolist()),
             ("tight", lambda: _plain(s.pieces(_listed(ids), 1.0, "white"))), ("listed", lambda: s.measure_table(_listed(ids), EGG_REGION, "yolk").tolist())]
    turn %= len(calls)
    return {key: call() for key, call in calls[turn:] + calls[:turn]}


def _one_handle_answers(h, ids, what):
    """the same of ONE handle, each first held against its model on the handle's downloads"""
    _assert_reads(h, EGG_SENSORS, what, _listed(ids))
    _assert_probes(h, EGG_PROBES, what)
    _assert_field(h, EGG_GRID, what, "both", True)
    _assert_field(h, EGG_GRID, what, "white", False)
    _assert_pieces(h, None, None, "both", what)
    _assert_pieces(h, _listed(ids), 1.0, "white", what)
    _assert_measure(h, None, None, "both", what)
    _assert_measure(h, _listed(ids), EGG_REGION, "yolk", what)
    return _answers(h, ids)


def _assert_same_answers(got, want, what):
    for key in want:
        assert got[key] == want[key], "%s: %s differs from one handle's" % (what, key)


def test_group_hand_over(egg):
    """two handles of a group on GPU 0 and one plain handle with the same eggs: every call of the group equals the one
    handle's (itself held against the models) before a hand-over, at the first call after it, and after a remove and an add"""
    g, h = egg.SimulationGroup([0, 0], cuts=[-INF, CUT, INF]), egg.SimulationHandler()
    for s in (g, h):
        s.set_solver_order("relaxed")
    ids = [g.add(x, y) for x, y in EGGS]
    assert [h.add(x, y) for x, y in EGGS] == ids
    for s in (g, h):
        s.set_sensors(EGG_SENSORS)

    def step():
        g.step(H60, 2, 3)
        h.step(H60, 2, 3)

    def same(what, ids, turn):
        _assert_same_answers(_answers(g, ids, turn), _one_handle_answers(h, ids, what), what)
        want = _assert_impulse(h, EGG_RECORDS, what)  # (with results)
        assert g.impulse(EGG_RECORDS) == want and min(want[0].count) > 0, what
        for w in (WHITE, YOLK):
            for f in ("x", "y", "vx", "vy", "last_x", "last_y", "batch_id"):
                assert np.array_equal(g.download(w, f).view(np.uint64), h.download(w, f).view(np.uint64)), (what, w, f)

    for _ in range(2):
        step()
    a = ids[0]
    assert g.owner(a)[0] == 0 and g.owner(ids[1])[0] == 1
    same("before the hand-over", ids, 0)
    before = g.counters()["migrations"]
    for k in range(60):  # the first egg is driven across the cut until it has been handed over
        for s in (g, h):
            s.set_target_position(a, min(300.0 + 12.0 * k, 700.0), 300.0)
        step()
        if g.counters()["migrations"] > before and g.owner(a)[0] == 1:
            break
    assert g.counters()["migrations"] > before and g.owner(a)[0] == 1, "no hand-over within 60 steps"
    same("the first call after the hand-over", ids, 1)  # (a probe is the group's first call behind it)
    g.remove(ids[1])
    h.remove(ids[1])
    new = g.add(350.0, 290.0, 40, 12)
    assert h.add(350.0, 290.0, 40, 12) == new == 5
    same("after a remove and an add", [ids[0], ids[2], ids[3], new], 3)  # (pieces first)


# ------------------------------------------------------------------------------------------------ sharded
SHARDED_CUTS = [-2000.0, CUT, 2.0 ** 41]
MOVED, DEST = 3, 1  # the egg at (330, 250) starts on rank 0 and is handed to rank 1, between that rank's two


def _worker(rank, world, port, q):
    import os
    import sys
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from egg_fluid_simulation_amd import SimulationHandler
    from egg_fluid_simulation_amd.sharding import ShardedSimulationHandler, SlabLayout
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sh = ShardedSimulationHandler(SlabLayout(SHARDED_CUTS), rank, dist, lambda: SimulationHandler(device=0), device="cpu")
        sh.set_solver_order("relaxed")
        ids = [sh.add(x, y, 50, 15) for x, y in EGGS]
        sh.set_sensors(EGG_SENSORS)

        def point(turn):
            return dict(answers=_answers(sh, ids, turn), owner=dict(sh.owner), local=[sh.global_id[i] for i in sh.local.list_ids()],
                        layout=[sh.global_id[int(i)] for i in sh.local.download(WHITE, "batch_id")])

        points = [point(0)]
        src = sh.owner[MOVED]  # (the hand-over of test_gpu_sharded_relaxed.py: a batch placed on another rank between two steps)
        if rank == src:
            sh._send_batches([MOVED], DEST)
        elif rank == DEST:
            sh._recv_batches(1, src)
        sh.owner[MOVED] = DEST
        sh._keys_stale = True
        points.append(point(2))  # the first call after the hand-over, a field: no step in between
        sh.step(H60, 2, 3)
        points.append(point(4))
        results = [tuple(r) for r in sh.impulse(EGG_RECORDS)]
        points.append(point(3))
        q.put((rank, "ok", dict(points=points, results=results, src=src)))
    except Exception:
        import traceback
        q.put((rank, "error: " + traceback.format_exc(), None))
    finally:
        dist.destroy_process_group()


def _spawn(world):
    import queue
    import time

    import torch.multiprocessing as mp
    from test_gpu_sharded_relaxed import _free_port
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    deadline = time.time() + 180
    while len(res) < world and time.time() < deadline:
        try:
            rank, outcome, results = q.get(timeout=2)
            assert outcome == "ok", outcome
            res[rank] = results
        except queue.Empty:
            if any(p.exitcode not in (None, 0) for p in procs):
                break
    for p in procs:
        p.join(20)
        if p.is_alive():
            p.kill()  # the exact child started above
    assert len(res) == world and all(p.exitcode == 0 for p in procs), "a rank failed: see its traceback above"
    return res


def test_sharded_hand_over(egg):
    """two ranks on GPU 0 over gloo; one egg is handed from rank 0 to rank 1, where it gets a new local id and lands BETWEEN
    that rank's two batches: the ranks' answers before, right after (no step in between), a step later and after an impulse
    are one handle's"""
    res = _spawn(2)
    h = egg.SimulationHandler()
    h.set_solver_order("relaxed")
    ids = [h.add(x, y, 50, 15) for x, y in EGGS]
    h.set_sensors(EGG_SENSORS)
    wants = [_one_handle_answers(h, ids, "one handle, before")]
    wants.append(_one_handle_answers(h, ids, "one handle, at the hand-over"))  # (one handle hands nothing over)
    h.step(H60, 2, 3)
    wants.append(_one_handle_answers(h, ids, "one handle, a step later"))
    results = [tuple(r) for r in _assert_impulse(h, EGG_RECORDS, "one handle, the impulse")]
    wants.append(_one_handle_answers(h, ids, "one handle, after the impulse"))
    for r in (0, 1):
        for k, want in enumerate(wants):
            _assert_same_answers(res[r]["points"][k]["answers"], want, "rank %d, point %d" % (r, k))
        assert res[r]["results"] == results, r
    # the hand-over happened, and on the far rank the batch lies between the two that were there
    assert res[0]["src"] == 0 and res[0]["points"][0]["owner"][MOVED] == 0 and res[0]["points"][1]["owner"][MOVED] == DEST
    assert sorted(res[0]["points"][0]["local"]) == [1, 3] and sorted(res[0]["points"][1]["local"]) == [1]
    assert sorted(res[1]["points"][0]["local"]) == [2, 4] and sorted(res[1]["points"][1]["local"]) == [2, 3, 4]
    layout = res[1]["points"][1]["layout"]
    assert [g for k, g in enumerate(layout) if k == 0 or layout[k - 1] != g] == [2, 3, 4]
