"""Host-side mirror of the reference's `SimulationHandler` class.

Same method names, argument meaning, defaults, warnings and errors as
/root/reference/simulation_handler.lua:9-459 ("L:" below), with the particle
state and the whole `_step` on the MI355X behind libeggsim.so (include/eggsim.h).
The LuaJIT twin of this file is lua/egg_fluid_simulation/simulation_handler.lua.

Error conventions (log.lua:9-88): where the reference calls `log.error` /
`log.assert` this raises `EggError`; where it calls `log.warning` this issues an
`EggWarning` through the `warnings` module and carries on.
"""
import copy
import ctypes as C
import collections
import functools
import math
import warnings

import numpy as np

from . import _ffi
from .default_config import default_configs


class EggError(RuntimeError):
    """The reference's `log.error` (a thrown Lua error)."""


# a probe's winner (egg_probe_hit without `found` and `key`): the batch's id, the particle's 0-based index in the batch's run
# of its type, the score (POINT: squared distance, RAY: t) and the particle's committed x, y, radius
ProbeHit = collections.namedtuple("ProbeHit", "id index score x y radius")


class Field(collections.namedtuple("Field", "count svx svy inside outside dropped units_tiled units_direct")):
    """The particles binned into a grid (egg_field): `count` an int32 and `svx`, `svy` int64 numpy planes of shape (2, ny, nx),
    [0] white and [1] yolk, the sums of the velocities scaled by 2^16 and rounded (None without velocity=True); `inside`,
    `outside`, `dropped` the (white, yolk) particles by fate; `units_tiled`, `units_direct` how the device did the work."""
    __slots__ = ()

    def velocity(self):
        """the mean velocity per cell as (2, ny, nx, 2) doubles: `((double)svx / 2^16) / (double)count` and likewise for y,
        NaN where the count is 0"""
        if self.svx is None or self.svy is None:
            raise EggError("Field.velocity: the field was taken without velocity=True")
        out = np.full(self.count.shape + (2,), np.nan, dtype=np.float64)
        some = self.count != 0
        n = self.count[some].astype(np.float64)
        out[..., 0][some] = (self.svx[some].astype(np.float64) / _ffi.FIELD_VELOCITY_SCALE) / n
        out[..., 1][some] = (self.svy[some].astype(np.float64) / _ffi.FIELD_VELOCITY_SCALE) / n
        return out


# what egg_field_to reports beside the planes it fills on the device: Field without its planes
FieldTotals = collections.namedtuple("FieldTotals", "inside outside dropped units_tiled units_direct")


class PieceSummary(collections.namedtuple("PieceSummary", "n pieces largest first singles dropped x y")):
    """The pieces of one atom -- the particles of one type of one batch -- (egg_pieces): `n` particles in `pieces` connected
    pieces, `singles` of them of one particle; the body (the largest piece, the lower label among equals) has `largest`
    particles and the label `first`, its lowest particle index in the batch; `x`, `y` is the body's centroid from the int64
    sums, `(sx / 2^16) / (largest - dropped)`, None while every body particle was dropped."""
    __slots__ = ()


class Touch(collections.namedtuple("Touch", "other pairs particles dropped x y")):
    """One batch that touches a query (egg_touch_record): `other` its id, `pairs` the touching (query particle, other particle)
    pairs, `particles` the distinct particles of the other batch among them, `dropped` the pairs whose scaled coordinates were
    not finite or reached 2^53; `x`, `y` the contact point from the int64 sums, `sx / (2 * (pairs - dropped)) / 2^16`, None
    while every pair was dropped."""
    __slots__ = ()


# egg_touch_record as a numpy record (40 bytes)
_TOUCH_RECORD = np.dtype([("slot", "<i4"), ("pairs", "<i4"), ("particles", "<i4"), ("dropped", "<i4"), ("other", "<i8"), ("sx", "<i8"),
                          ("sy", "<i8")])


# egg_piece_summary as a numpy record (40 bytes)
_PIECE_RECORD = np.dtype([("n", "<i4"), ("pieces", "<i4"), ("largest", "<i4"), ("first", "<i4"), ("singles", "<i4"), ("dropped", "<i4"),
                          ("sx", "<i8"), ("sy", "<i8")])


class Impulse(collections.namedtuple("Impulse", "action region a id linear by_inv_mass", defaults=(None, False, False))):
    """One record of impulse() (egg_impulse_record): `action` = "kick" | "blast" | "swirl" | "brake", `region` a region in the
    tuple form of set_sensors, `a` the action's parameters -- (ax, ay), (cx, cy, s), (cx, cy, omega), (ux, uy, k) --, `id` a
    batch id or None for every batch, `linear` the weight 1 - d / R of a disc or capsule, `by_inv_mass` the weight times the
    particle's inverse mass (kick and blast)."""
    __slots__ = ()


class ImpulseResult(collections.namedtuple("ImpulseResult", "count sdvx sdvy skipped")):
    """What one record of impulse() did, each field a `(white, yolk)` pair of Python ints: `count` the particles whose
    velocity it edited, `sdvx`, `sdvy` the int64 sums of their changes of velocity scaled by 2^16 and rounded, `skipped` the
    particles inside it whose edit was refused because a scaled change was not finite or reached 2^53."""
    __slots__ = ()

    def dv(self):
        """the summed change of velocity per type in px/s: `((double)sdvx / 2^16, (double)sdvy / 2^16)` for (white, yolk)"""
        return tuple((float(sx) / _ffi.IMPULSE_SCALE, float(sy) / _ffi.IMPULSE_SCALE) for sx, sy in zip(self.sdvx, self.sdvy))


class Measure(collections.namedtuple("Measure", _ffi.MEASURE_FIELDS)):
    """One atom -- the particles of one type of one batch -- as a body (egg_measure_record): 24 Python ints, and what the host
    derives from them.  S = 2^16, SM = 2^32.  `atom` particles, `n` of them measured (all without a region), `dropped` of
    those left out because a scaled term was not finite or reached 2^53; the sums run over the `kept = n - dropped` others:
    `sx, sy` of x S, `sm` of m SM, `smx, smy` of m x S, `spx, spy` of m v S, `se` of m v^2 S; `lo_x, lo_y, hi_x, hi_y` the
    box of the discs and `max_v2` the highest squared speed, times S; `ox_q, oy_q` the centroid truncated to 1 / S, about which
    `sxx, sxy, syy` sum d d S, `sl` sums m (d x v) S and `max_reach` is the farthest disc edge times S, over the kept
    particles less `dropped_central`."""
    __slots__ = ()

    @property
    def kept(self):
        return self.n - self.dropped

    @property
    def mass(self):
        """sm / SM"""
        return float(self.sm) / _ffi.MEASURE_MASS_SCALE

    @property
    def centroid(self):
        """((sx / S) / kept, (sy / S) / kept): the mean of the centres; None while every particle was dropped"""
        k = self.kept
        return ((float(self.sx) / _ffi.MEASURE_SCALE) / k, (float(self.sy) / _ffi.MEASURE_SCALE) / k) if k else None

    @property
    def center_of_mass(self):
        """((smx / S) / mass, (smy / S) / mass); None without mass"""
        m = self.mass
        return ((float(self.smx) / _ffi.MEASURE_SCALE) / m, (float(self.smy) / _ffi.MEASURE_SCALE) / m) if m > 0.0 else None

    @property
    def momentum(self):
        """(spx / S, spy / S)"""
        return (float(self.spx) / _ffi.MEASURE_SCALE, float(self.spy) / _ffi.MEASURE_SCALE)

    @property
    def velocity(self):
        """momentum / mass: the velocity of the centre of mass; None without mass"""
        m, p = self.mass, self.momentum
        return (p[0] / m, p[1] / m) if m > 0.0 else None

    @property
    def kinetic_energy(self):
        """0.5 * se / S"""
        return 0.5 * float(self.se) / _ffi.MEASURE_SCALE

    @property
    def bounds(self):
        """(lo_x, lo_y, hi_x, hi_y) / S: the rectangle that holds every kept disc; None while every particle was dropped"""
        s = _ffi.MEASURE_SCALE
        return (float(self.lo_x) / s, float(self.lo_y) / s, float(self.hi_x) / s, float(self.hi_y) / s) if self.kept else None

    @property
    def max_speed(self):
        """sqrt(max_v2 / S)"""
        return math.sqrt(float(self.max_v2) / _ffi.MEASURE_SCALE)

    @property
    def origin(self):
        """(ox_q / S, oy_q / S): the point the second moments, the spin and the reach are about"""
        return (float(self.ox_q) / _ffi.MEASURE_SCALE, float(self.oy_q) / _ffi.MEASURE_SCALE)

    @property
    def reach(self):
        """max_reach / S: the radius of the circle about `origin` that holds every disc"""
        return float(self.max_reach) / _ffi.MEASURE_SCALE

    @property
    def spin(self):
        """sl / S: the angular momentum about `origin`, counter-clockwise positive"""
        return float(self.sl) / _ffi.MEASURE_SCALE

    def axes(self):
        """`(major, minor, angle)`: the two principal standard deviations of the centres about `origin` and the angle of the
        major axis in radians, from the covariance `(sxx, sxy, syy) / S / k` over the k = kept - dropped_central particles;
        None when k is 0"""
        k = self.kept - self.dropped_central
        if k <= 0:
            return None
        s = _ffi.MEASURE_SCALE
        cxx, cxy, cyy = (float(self.sxx) / s) / k, (float(self.sxy) / s) / k, (float(self.syy) / s) / k
        half, diff = 0.5 * (cxx + cyy), 0.5 * (cxx - cyy)
        root = math.sqrt(diff * diff + cxy * cxy)
        return (math.sqrt(max(half + root, 0.0)), math.sqrt(max(half - root, 0.0)), 0.5 * math.atan2(2.0 * cxy, cxx - cyy))


class Cover(collections.namedtuple("Cover", "cover owner cell inside outside dropped hits covered covered_both covered_any "
                                   "units_lanes units_wave units_direct")):
    """The particles' discs rastered into a grid (egg_cover): `cover` an int32 numpy plane of shape (2, ny, nx), [0] white and
    [1] yolk, the number of discs over each cell's centre; `owner` the smallest batch id among them, -1 where there is none
    (None without owner=True); `cell` the side of a cell; `inside`, `outside`, `dropped`, `hits`, `covered` the (white, yolk)
    particles by fate, covered (disc, cell) pairs and covered cells; `covered_both`, `covered_any` the cells under both types
    and under either; `units_lanes`, `units_wave`, `units_direct` how the device did the work."""
    __slots__ = ()

    def area(self):
        """the covered area in px^2 as (white, yolk, both, any): cells * cell * cell"""
        a = self.cell * self.cell
        return (self.covered[0] * a, self.covered[1] * a, self.covered_both * a, self.covered_any * a)

    def depth(self):
        """the mean number of discs over a covered cell as (white, yolk): hits / covered, NaN where nothing is covered"""
        return tuple(h / c if c else float("nan") for h, c in zip(self.hits, self.covered))


# what egg_cover_to reports beside the planes it fills on the device: Cover without its planes
CoverTotals = collections.namedtuple("CoverTotals", "cell inside outside dropped hits covered covered_both covered_any "
                                                    "units_lanes units_wave units_direct")


class EggWarning(UserWarning):
    """The reference's `log.warning` (a line on stderr)."""


def _type_name(v):
    if isinstance(v, bool):
        return "boolean"
    if isinstance(v, (int, float, np.integer, np.floating)):
        return "number"
    if v is None:
        return "nil"
    if isinstance(v, (dict, list, tuple)):
        return "table"
    if isinstance(v, str):
        return "string"
    return type(v).__name__


def _assert_types(*pairs):  # log.assert, log.lua:65-88
    for k in range(0, len(pairs), 2):
        value, expected = pairs[k], pairs[k + 1]
        if _type_name(value) != expected:
            raise EggError("[ERROR] for argument #%d: expected `%s`, got `%s`"
                           % (k // 2 + 1, expected, _type_name(value)))


def _is_nan(x):
    return x != x


# L:1152-1249: key -> (type, min, max)
_VALID_CONFIG_KEYS = {
    "damping": ("number", 0, 1),
    "color": ("color", None, None),
    "outline_color": ("color", None, None),
    "outline_thickness": ("number", 0, None),
    "collision_strength": ("number", 0, 1),
    "collision_overlap_factor": ("number", 0, None),
    "cohesion_strength": ("number", 0, 1),
    "cohesion_interaction_distance_factor": ("number", 0, None),
    "follow_strength": ("number", 0, 1),
    "min_radius": ("number", 0, None),
    "max_radius": ("number", 0, None),
    "min_mass": ("number", 0, None),
    "max_mass": ("number", 0, None),
    "motion_blur": ("number", 0, 1),
    "texture_scale": ("number", 1, None),
    "highlight_strength": ("number", 0, None),
    "shadow_strength": ("number", 0, None),
}

_SOLVER_KEYS = ["damping", "follow_strength", "cohesion_strength", "cohesion_interaction_distance_factor",
                "collision_strength", "collision_overlap_factor", "min_mass", "max_mass", "min_radius",
                "max_radius"]

# What differs between the three tagged kind lists (set_colliders, set_sensors, set_forces), as data for _c_kind_list and
# _kind_tuples.  `word` names a record in the messages; `codes` kind -> code, `names` code -> kind, `params` code -> parameter
# names and `types` name -> type_mask are the tables of _ffi; `limit` the most records a list holds, where the host checks it;
# `loose_types`: the last string of a tuple is its types whatever the tuple's length (else only where the tuple is one value
# too long for its kind); `alt` code -> (other parameter names, their conversion to the stored ones).
_KindList = collections.namedtuple("_KindList", "word struct codes names params types limit loose_types alt")
_COLLIDER_LIST = _KindList("collider", _ffi.EggCollider, _ffi.COLLIDER_CODES, _ffi.COLLIDER_NAMES, _ffi.COLLIDER_PARAM_NAMES,
                           _ffi.COLLIDER_TYPES, None, False, {})
_SENSOR_LIST = _KindList("sensor", _ffi.EggSensor, _ffi.SENSOR_CODES, _ffi.SENSOR_KINDS, _ffi.SENSOR_PARAMS, _ffi.SENSOR_TYPES,
                         _ffi.MAX_SENSORS, True,
                         {_ffi.SENSOR_BOX: (("cx", "cy", "hx", "hy", "angle"), lambda v: v[:4] + [math.cos(v[4]), math.sin(v[4])])})
_FORCE_LIST = _KindList("field", _ffi.EggForce, {n: i for i, n in enumerate(_ffi.FORCE_KINDS)}, _ffi.FORCE_KINDS, _ffi.FORCE_PARAMS,
                        _ffi.FORCE_TYPES, None, False, {})

# A record of fixed shape per collider, as data for _c_records and _get_records.  `what` names it in the messages and `form` is
# what they say was expected; `lengths` the accepted lengths, a shorter one padded with zeros (None is the first length of
# zeros); `number`: a bare number is the first field; `checks`, in order, (field indices, the text where one of them is not
# finite, the text where one is negative or None where that is allowed), each text formatted with the fields' values.
_Record = collections.namedtuple("_Record", "what form struct fields lengths number checks")
_SURFACE = _Record("collider surface", "None, a number mu or (mu, vx, vy)", _ffi.EggColliderSurface, ("friction", "vx", "vy"), (3,), True, ())
_MOTION = _Record("collider motion", "None or (vx, vy)", _ffi.EggColliderMotion, ("vx", "vy"), (2,), False,
                  (((0, 1), "the velocity (%r, %r) is not finite", None),))
_SPIN = _Record("collider spin", "None or (px, py, omega)", _ffi.EggColliderSpin, ("px", "py", "omega"), (3,), False,
                (((0, 1), "the pivot (%r, %r) is not finite", None), ((2,), "omega %r is not finite", None)))
_BODY = _Record("collider body", "None or (inv_mass, inv_inertia[, ax, ay[, drag, spin_drag]])", _ffi.EggColliderBody,
                ("inv_mass", "inv_inertia", "ax", "ay", "drag", "spin_drag"), (2, 4, 6), False,
                tuple(((q,), name + " %r is not finite", None if name in ("ax", "ay") else name + " %r is negative")
                      for q, name in enumerate(("inv_mass", "inv_inertia", "ax", "ay", "drag", "spin_drag"))))


class _HandlerSurface:
    """The part of the reference's class that SimulationHandler (one device handle, `egg_*`) and SimulationGroup (a device
    group, `egg_group_*`) share: argument checks, warnings, error texts and the calls, which differ only in the prefix of the
    C entry point and the pointer they pass (`_PREFIX`, `_ptr`)."""

    _PREFIX = "egg_"

    def _ptr(self):
        return self._h

    def _c(self, name):
        """the C entry point `name` of this object's kind, bound to its handle"""
        return functools.partial(getattr(self._lib, self._PREFIX + name), self._ptr())

    # ------------------------------------------------ what the setters and getters below share
    @staticmethod
    def _c_kind_list(kl, items):
        """a list of tuples `(kind, parameters...[, types])` or dicts `{"kind": ..., <parameter names>, "types": ...}` as an array
        of `kl.struct` (kind, type_mask, p[]); what only the host can check (shape, names) is checked here, the values by the
        library"""
        items = list(items)
        if kl.limit is not None and len(items) > kl.limit:
            raise EggError("%ss: a list holds 0 .. %d %ss, not %d" % (kl.word, kl.limit, kl.word, len(items)))
        arr = (kl.struct * max(len(items), 1))()
        word, codes, params, masks, alt, loose = kl.word, kl.codes, kl.params, kl.types, kl.alt, kl.loose_types
        for k, c in enumerate(items):
            if isinstance(c, dict):
                kind, types = c.get("kind"), c.get("types", "both")
            else:
                c = tuple(c)
                kind = c[0] if c else None
                types = "both"
            if not isinstance(kind, str) or kind not in codes:
                raise EggError("%s %d: kind must be one of %s, not %r" % (word, k, ", ".join(codes), kind))
            code = codes[kind]
            names, other = params[code], alt.get(code)
            if isinstance(c, dict):
                given = set(c) - {"kind", "types"}
                if other is not None and given == set(other[0]):
                    names = other[0]
                if given != set(names):
                    raise EggError("%s %d (%s): expected the keys %s" % (word, k, kind, ", ".join(names)))
                values = [c[n] for n in names]
            else:
                values = list(c[1:])
                if values and isinstance(values[-1], str) and (loose or len(values) == len(names) + 1):
                    types = values.pop()
                if other is not None and len(values) == len(other[0]):
                    names = other[0]
                if len(values) != len(names):
                    raise EggError("%s %d (%s): expected (%r, %s[, types])" % (word, k, kind, kind, ", ".join(names)))
            if not isinstance(types, str) or types not in masks:
                raise EggError("%s %d: types must be 'both', 'white' or 'yolk', not %r" % (word, k, types))
            try:
                values = [float(v) for v in values]
            except (TypeError, ValueError):
                raise EggError("%s %d (%s): the parameters must be numbers" % (word, k, kind)) from None
            if other is not None and names is other[0]:
                values = other[1](values)
            arr[k].kind, arr[k].type_mask = code, masks[types]
            for q, v in enumerate(values):
                arr[k].p[q] = v
        return len(items), arr

    @staticmethod
    def _kind_tuples(kl, records):
        """_c_kind_list backwards: the records as tuples `(kind, parameters..., types)`"""
        types = {v: k for k, v in kl.types.items()}
        return [(kl.names[c.kind],) + tuple(c.p[:len(kl.params[c.kind])]) + (types[c.type_mask],) for c in records]

    @staticmethod
    def _c_records(rec, items):
        """a list with one element per collider -- None, a tuple of one of `rec.lengths` or, with `rec.number`, a number -- as
        an array of `rec.struct`; shape, finiteness and signs are checked here, before any call into the library"""
        items = list(items)
        arr = (rec.struct * max(len(items), 1))()
        for k, v in enumerate(items):
            if v is None:
                v = (0.0,) * rec.lengths[0]
            elif rec.number and isinstance(v, (int, float)):
                v = (v,) + (0.0,) * (len(rec.fields) - 1)
            try:
                v = tuple(float(x) for x in v)
            except (TypeError, ValueError):
                raise EggError("%s %d: expected %s, not %r" % (rec.what, k, rec.form, v)) from None
            if len(v) not in rec.lengths:
                raise EggError("%s %d: expected %s, not %r" % (rec.what, k, rec.form, v))
            v += (0.0,) * (len(rec.fields) - len(v))
            for at, not_finite, negative in rec.checks:
                part = tuple(v[q] for q in at)
                if not all(math.isfinite(x) for x in part):
                    raise EggError("%s %d: %s" % (rec.what, k, not_finite % part))
                if negative is not None and any(x < 0.0 for x in part):
                    raise EggError("%s %d: %s" % (rec.what, k, negative % part))
            for name, x in zip(rec.fields, v):
                setattr(arr[k], name, x)
        return len(items), arr

    def _get_array(self, call, struct, cap):
        """the records an entry point `call(cap, array, &n)` of this object stores"""
        arr = (struct * cap)()
        n = C.c_int32()
        self._check(call(cap, arr, C.byref(n)))
        return arr[:n.value]

    def _get_records(self, call, struct, fields):
        """one tuple of `fields` per collider from `call`"""
        return [tuple(getattr(r, f) for f in fields) for r in self._get_array(call, struct, _ffi.MAX_COLLIDERS)]

    @staticmethod
    def _c_range_pair(what, first, a, strength):
        """(factor | reach, strength) as the two doubles a setter of `what` takes; the ranges are checked here as the library
        checks them"""
        out = []
        for name, v in ((first, a), ("strength", strength)):
            try:
                out.append(float(v))
            except (TypeError, ValueError):
                raise EggError("%s: the %s must be a number, not %r" % (what, name, v)) from None
        if not (0.0 <= out[0] < float("inf")):  # (false for a NaN)
            raise EggError("%s: the %s %r is not a finite number >= 0" % (what, first, out[0]))
        if not (0.0 <= out[1] <= 1.0):
            raise EggError("%s: the strength %r lies outside [0, 1]" % (what, out[1]))
        return out[0], out[1]

    def _get_pair(self, call):
        """the two doubles `call(&a, &b)` stores"""
        a, b = C.c_double(), C.c_double()
        self._check(call(C.byref(a), C.byref(b)))
        return (a.value, b.value)

    def _get_count(self, call):
        """the int64 counter `call(&n)` stores"""
        n = C.c_int64()
        self._check(call(C.byref(n)))
        return int(n.value)

    def _get_counts(self, call):
        """the int64[2] counters, [white, yolk], that `call(v)` fills"""
        v = (C.c_int64 * 2)()
        self._check(call(v))
        return list(v)

    # ------------------------------------------------ static colliders (egg_set_colliders)
    @staticmethod
    def _c_colliders(colliders):
        """a list of tuples `(kind, a, b, c[, d][, types])` or dicts `{"kind": ..., <parameter names>, "types": ...}` as an
        egg_collider array; what only the host can check (shape, names) is checked here, the values by the library"""
        return _HandlerSurface._c_kind_list(_COLLIDER_LIST, colliders)

    def set_colliders(self, colliders):
        """The ordered list of static colliders, at most 64 ("Colliders"; relaxed order only):
        `("half_plane", nx, ny, off)` keeps n . pos - off >= radius, `("disc", cx, cy, R)` is an obstacle,
        `("container", cx, cy, R)` keeps particles inside, `("segment", x0, y0, x1, y1)` is a wall of zero thickness that looks only
        at where a pass has put a particle -- what moves more than its radius past it in one sub-step gets through --,
        `("wall", x0, y0, x1, y1)` is the same wall swept: a particle that starts a sub-step on one side cannot end a pass
        on the other; each
        takes an optional last element (or dict key) types = "both" | "white" | "yolk", and each may be a dict with "kind"
        and the parameter names.  In a relaxed pass every particle's new position is projected collider after collider,
        in list order.  `[]` clears the list.  Raises EggError for a bad list (nothing changes) and for a non-empty list on
        a handle in exact order; set_solver_order("exact") raises while the list is not empty."""
        n, arr = self._c_colliders(colliders)
        self._check(self._c("set_colliders")(n, arr))

    def get_colliders(self):
        """the list as stored, as tuples `(kind, parameters..., types)`: a half-plane's normal comes back normalised"""
        return self._kind_tuples(_COLLIDER_LIST, self._get_array(self._c("get_colliders"), _ffi.EggCollider, _ffi.MAX_COLLIDERS))

    def collider_hits(self):
        """[white, yolk]: how often a collider moved a particle in a pass of a committed step, since creation"""
        return self._get_counts(self._c("get_collider_hits"))

    # ------------------------------------------------ collider surfaces (egg_set_collider_surfaces)
    @staticmethod
    def _c_surfaces(surfaces):
        """a list with one element per collider -- None (the default surface), a number mu, or (mu, vx, vy) -- as an
        egg_collider_surface array; the shape is checked here, the values by the library"""
        return _HandlerSurface._c_records(_SURFACE, surfaces)

    def set_collider_surfaces(self, surfaces):
        """One surface per collider of the current list ("Collider surfaces"): `None` for the default,
        a number `mu` (Coulomb friction, >= 0), or `(mu, vx, vy)` with the surface's velocity in px/s.  Right after a collider
        with mu > 0 has projected a particle, the tangential part of the particle's displacement over the sub-step, relative
        to the surface, is removed up to mu times the depth just corrected: a floor holds what lies on it, a moving surface
        drags it.  `[]` resets every surface to the default, and so does set_colliders.  Raises EggError (nothing changes)
        for a length that is not the collider count, a friction that is negative or not finite, a velocity that is not
        finite."""
        n, arr = self._c_surfaces(surfaces)
        self._check(self._c("set_collider_surfaces")(n, arr))

    def get_collider_surfaces(self):
        """the surfaces as stored, one `(mu, vx, vy)` per collider (defaults included)"""
        return self._get_records(self._c("get_collider_surfaces"), _SURFACE.struct, _SURFACE.fields)

    def collider_grips(self):
        """[white, yolk]: friction applications (stick or slide) in the passes of committed steps, since creation"""
        return self._get_counts(self._c("get_collider_grips"))

    # ------------------------------------------------ collider motion (egg_set_collider_motion)
    @staticmethod
    def _c_motions(motions):
        """a list with one element per collider -- None (at rest) or (vx, vy) -- as an egg_collider_motion array; shape and
        finiteness are checked here, before any call into the library"""
        return _HandlerSurface._c_records(_MOTION, motions)

    def set_collider_motion(self, motions):
        """One motion per collider of the current list ("Collider motion"): `None` for a collider at
        rest or `(vx, vy)`, a rigid velocity in px/s.  The step integrates it on the device: every sub-step uses the geometry
        at its end, a moving wall sweeps in its own frame -- it catches what it passes over and carries it on its front
        side -- and friction is taken relative to the moving surface, so a collider with mu > 0 drags what it touches.  A
        committed step advances the list get_colliders returns.  `[]` resets every motion to zero, and so does
        set_colliders; geometry and surfaces stay.  Raises EggError (nothing changes) for a length that is not the collider
        count or a velocity that is not finite."""
        n, arr = self._c_motions(motions)
        self._check(self._c("set_collider_motion")(n, arr))

    def get_collider_motion(self):
        """the motions as stored, one `(vx, vy)` per collider (zeros included)"""
        return self._get_records(self._c("get_collider_motion"), _MOTION.struct, _MOTION.fields)

    # ------------------------------------------------ collider spin (egg_set_collider_spin)
    @staticmethod
    def _c_spins(spins):
        """a list with one element per collider -- None (no spin) or (px, py, omega) -- as an egg_collider_spin array; shape
        and finiteness are checked here, before any call into the library"""
        return _HandlerSurface._c_records(_SPIN, spins)

    def set_collider_spin(self, spins):
        """One spin per collider of the current list ("Collider spin"): `None` for a collider that
        does not turn or `(px, py, omega)`, a rigid angular velocity in rad/s, counter-clockwise positive, about the pivot
        (px, py), which rides on the collider's motion.  The step integrates it on the device: every sub-step uses the
        geometry at its end, a turning wall sweeps in its own frame -- it catches what it passes over -- and friction takes
        the surface's velocity at the contact point, so a disc spinning about its centre with mu > 0 drags what it touches.
        A committed step advances the list get_colliders returns and the pivots get_collider_spin returns.  `[]` resets
        every spin to zero, and so does set_colliders; geometry, surfaces and motions stay.  Raises EggError (nothing
        changes) for a length that is not the collider count or a component that is not finite."""
        n, arr = self._c_spins(spins)
        self._check(self._c("set_collider_spin")(n, arr))

    def get_collider_spin(self):
        """the spins as stored, one `(px, py, omega)` per collider (zeros included)"""
        return self._get_records(self._c("get_collider_spin"), _SPIN.struct, _SPIN.fields)

    # ------------------------------------------------ collider styles and pose (egg_set_collider_styles)
    _STYLE_DEFAULTS = {"fill": (0.0, 0.0, 0.0, 0.0), "line": (0.0, 0.0, 0.0, 0.0), "line_width": 0.0, "layer": "under"}

    @staticmethod
    def _c_styles(styles):
        """a list with one element per collider -- None (undrawn) or a dict {"fill": rgba, "line": rgba, "line_width": w,
        "layer": "under" | "over"}, missing keys taking the defaults (no fill, no line, under) -- as an egg_collider_style
        array; shape, names and ranges are checked here, before any call into the library"""
        styles = list(styles)
        arr = (_ffi.EggColliderStyle * max(len(styles), 1))()
        for k, st in enumerate(styles):
            if st is None:
                continue  # (all zero: undrawn)
            if not isinstance(st, dict) or set(st) - set(_HandlerSurface._STYLE_DEFAULTS):
                raise EggError("collider style %d: expected None or a dict with the keys fill, line, line_width, layer, not %r" % (k, st))
            st = dict(_HandlerSurface._STYLE_DEFAULTS, **st)
            for name in ("fill", "line"):
                try:
                    rgba = tuple(float(v) for v in st[name])
                except (TypeError, ValueError):
                    raise EggError("collider style %d: %s must be (r, g, b, a), not %r" % (k, name, st[name])) from None
                if len(rgba) != 4 or not all(0.0 <= v <= 1.0 for v in rgba):  # (false for a NaN)
                    raise EggError("collider style %d: %s must be (r, g, b, a) with every component in [0, 1], not %r" % (k, name, st[name]))
                getattr(arr[k], name)[:] = rgba
            try:
                width = float(st["line_width"])
            except (TypeError, ValueError):
                raise EggError("collider style %d: line_width must be a number, not %r" % (k, st["line_width"])) from None
            if not 0.0 <= width <= 64.0:
                raise EggError("collider style %d: line_width %r is not in [0, 64]" % (k, st["line_width"]))
            if not isinstance(st["layer"], str) or st["layer"] not in _ffi.COLLIDER_LAYERS:
                raise EggError("collider style %d: layer must be 'under' or 'over', not %r" % (k, st["layer"]))
            arr[k].line_width, arr[k].layer = width, _ffi.COLLIDER_LAYERS[st["layer"]]
        return len(styles), arr

    def set_collider_styles(self, styles):
        """One style per collider of the current list ("Collider styles"): `None` for a collider
        draw() leaves out, or a dict `{"fill": rgba, "line": rgba, "line_width": px, "layer": "under" | "over"}` with
        defaults for missing keys (no fill, no line, "under").  `fill` colours the solid side (a segment or wall has none),
        `line` the outline or the segment itself, `line_width` pixels wide (0 .. 64); "under" draws after the clear and
        before the eggs, "over" after them.  draw() places every collider at the pose get_collider_pose returns for the
        frame's interpolation alpha.  `[]` draws nothing, and so does set_colliders; with nothing visible draw() launches
        what it launches without styles.  Raises EggError (nothing changes) for a length that is not the collider count,
        a component outside [0, 1], a width outside [0, 64] or an unknown layer."""
        n, arr = self._c_styles(styles)
        self._check(self._c("set_collider_styles")(n, arr))

    def get_collider_styles(self):
        """the styles as stored, one dict per collider -- `None` for one that is not visible"""
        arr = self._get_array(self._c("get_collider_styles"), _ffi.EggColliderStyle, _ffi.MAX_COLLIDERS)
        kinds = self._get_array(self._c("get_colliders"), _ffi.EggCollider, _ffi.MAX_COLLIDERS)
        layers = {v: name for name, v in _ffi.COLLIDER_LAYERS.items()}
        out = []
        for st, c in zip(arr, kinds):
            inside = c.kind not in (_ffi.COLLIDER_SEGMENT, _ffi.COLLIDER_WALL)
            visible = (st.fill[3] > 0 and inside) or (st.line[3] > 0 and st.line_width > 0)
            out.append({"fill": tuple(st.fill), "line": tuple(st.line), "line_width": st.line_width,
                        "layer": layers[st.layer]} if visible else None)
        return out

    def get_collider_pose(self, alpha=None):
        """The list draw() places the colliders at ("Collider styles"), as get_colliders returns
        it: every parameter is `last * (1 - t) + current * t`, `last` the list at the start of the last committed step,
        t = `alpha` clamped to [0, 1] or, with None, this object's interpolation_alpha -- the rule draw() places the
        particles by.  A host that draws the colliders itself reads this once per frame.  set_colliders sets both lists:
        a teleport is not interpolated."""
        call = functools.partial(self._c("get_collider_pose"), float("nan") if alpha is None else float(alpha))
        return self._kind_tuples(_COLLIDER_LIST, self._get_array(call, _ffi.EggCollider, _ffi.MAX_COLLIDERS))

    # ------------------------------------------------ collider loads (egg_set_collider_loads)
    def set_collider_loads(self, on):
        """Switch collider loads on or off ("Collider loads"; off by default).  While on, a relaxed
        step with a non-empty list records per collider the impulse and the torque about its pivot that it received from
        the particles it moved.  It only observes: positions and counters are those of the step with loads off.  Accepted
        in either solver order and with an empty list; the stored loads start again at zero."""
        self._check(self._c("set_collider_loads")(1 if on else 0))
        self._collider_loads = bool(on)

    def get_collider_loads_enabled(self):
        return getattr(self, "_collider_loads", False)

    def collider_load_sums(self):
        """`(sums, dropped, sub_delta)` of the last committed step that recorded loads: `sums` one `(sx, sy, sz)` of Python
        ints per collider -- the int64 sums of the quantised contributions, impulse scaled by 2^20 and torque by 2^10 --,
        the contributions dropped, and the sub-step h of that step (0.0 while no step has recorded any)"""
        arr = (C.c_int64 * (3 * _ffi.MAX_COLLIDERS))()
        dropped, h, n = C.c_int64(), C.c_double(), C.c_int32()
        self._check(self._c("get_collider_load_sums")(_ffi.MAX_COLLIDERS, arr, C.byref(dropped), C.byref(h), C.byref(n)))
        return [(arr[3 * k], arr[3 * k + 1], arr[3 * k + 2]) for k in range(n.value)], dropped.value, h.value

    def collider_loads(self):
        """one `(jx, jy, torque)` per collider: the impulse in mass px/s and the angular impulse about the collider's pivot in
        mass px^2/s that it received over the last committed step that recorded loads; the mean force over a step of
        length delta is j / delta.  All zeros while no step has recorded any."""
        return self._get_records(self._c("get_collider_loads"), _ffi.EggColliderLoad, ("jx", "jy", "torque"))

    # ------------------------------------------------ sensors (egg_set_sensors)
    @staticmethod
    def _c_sensors(sensors):
        """a list of tuples `(kind, parameters...[, types])` or dicts `{"kind": ..., <parameter names>, "types": ...}` as an
        egg_sensor array.  A box takes its first axis `ux, uy` or, one value shorter, an `angle` in radians that the host's
        cos / sin convert.  What only the host can check (shape, names) is checked here, the values by the library."""
        return _HandlerSurface._c_kind_list(_SENSOR_LIST, sensors)

    def set_sensors(self, sensors):
        """The ordered list of sensor regions, at most 64 (either solver order):
        `("half_plane", nx, ny, off)` is the side the normal points to, `("disc", cx, cy, R)`, `("box", cx, cy, hx, hy, angle)`
        (or `..., ux, uy` for the first axis), `("capsule", x0, y0, x1, y1, R)` a band around a segment; each takes an optional
        last element (or dict key) types = "both" | "white" | "yolk".  A particle is inside when its centre is.  Sensors only
        observe: a step launches what it launches without them.  `[]` clears the list.  Raises EggError for a bad list
        (nothing changes)."""
        n, arr = self._c_sensors(sensors)
        self._check(self._c("set_sensors")(n, arr))

    def get_sensors(self):
        """the list as stored, as tuples `(kind, parameters..., types)`: normals and box axes come back normalised, a box
        with its axis `ux, uy`"""
        return self._kind_tuples(_SENSOR_LIST, self._get_array(self._c("get_sensors"), _ffi.EggSensor, _ffi.MAX_SENSORS))

    def sensor_sums(self):
        """`(sums, dropped)` of the positions as committed now: `sums` holds per sensor `((count, sx, sy), (count, sx, sy))`
        for (white, yolk) as Python ints -- sx, sy the int64 sums of the coordinates scaled by 2^16 and rounded --, `dropped`
        the `[white, yolk]` (particle, sensor) incidences left out because a scaled coordinate was not finite or reached 2^53.
        Every call measures."""
        arr = (_ffi.EggSensorReading * _ffi.MAX_SENSORS)()
        dropped, n = (C.c_int64 * 2)(), C.c_int32()
        self._check(self._c("read_sensors")(_ffi.MAX_SENSORS, arr, dropped, C.byref(n)))
        return [tuple((r.count[w], r.sx[w], r.sy[w]) for w in (0, 1)) for r in arr[:n.value]], list(dropped)

    @staticmethod
    def _sensor_readings(sums):
        """per sensor `{"count": (white, yolk), "centroid": (white, yolk)}` from sensor_sums' integers: a centroid is
        `(((double)sx / 2^16) / count, ((double)sy / 2^16) / count)`, or None while the count is 0"""
        scale = _ffi.SENSOR_POSITION_SCALE
        return [{"count": tuple(c for c, _, _ in per_type),
                 "centroid": tuple(((float(sx) / scale) / float(c), (float(sy) / scale) / float(c)) if c else None
                                   for c, sx, sy in per_type)} for per_type in sums]

    def sensors(self):
        """per sensor `{"count": (white, yolk), "centroid": (white, yolk)}`: how many particles of each type lie inside and
        where their centroid is (an `(x, y)`, or None while there is none)"""
        return self._sensor_readings(self.sensor_sums()[0])

    def sensor_batches(self, ids):
        """an int32 array `[len(ids), n_sensors, 2]`: the particles (white, yolk) of each listed batch inside each sensor, in
        the order of `ids`; an id may repeat.  Raises EggError for an unknown id."""
        ids = np.ascontiguousarray([int(i) for i in ids], dtype=np.int64)
        n = C.c_int32()
        self._check(self._c("get_sensors")(0, None, C.byref(n)))
        out = np.zeros((ids.size, n.value, 2), dtype=np.int32)
        self._check(self._c("read_sensor_batches")(ids.size, ids.ctypes.data, out.ctypes.data))
        return out

    # ------------------------------------------------ probes (egg_probe)
    @staticmethod
    def _probe_mask(types, what):
        """`types` as a type_mask: "both" | "white" | "yolk", or the mask itself (1 white, 2 yolk, 3 both)"""
        if isinstance(types, str) and types in _ffi.PROBE_TYPES:
            return _ffi.PROBE_TYPES[types]
        if isinstance(types, int) and not isinstance(types, bool) and 1 <= types <= 3:
            return types
        raise EggError("%s: types must be 'both', 'white', 'yolk' or a mask 1 .. 3, not %r" % (what, types))

    @staticmethod
    def _c_probes(probes):
        """a list of tuples `("point", x, y[, reach[, types]])` / `("ray", x0, y0, x1, y1[, pad[, types]])` as an
        egg_probe_query array; reach defaults to inf, pad to 0, types to both.  What only the host can check (shape, names)
        is checked here, the values by the library."""
        probes = list(probes)
        if len(probes) > _ffi.MAX_PROBES:
            raise EggError("probes: a call takes 0 .. %d probes, not %d" % (_ffi.MAX_PROBES, len(probes)))
        arr = (_ffi.EggProbeQuery * max(len(probes), 1))()
        for k, q in enumerate(probes):
            q = tuple(q) if isinstance(q, (tuple, list)) else ()
            kind = q[0] if q else None
            if not isinstance(kind, str) or kind not in _ffi.PROBE_CODES:
                raise EggError("probe %d: kind must be one of %s, not %r" % (k, ", ".join(_ffi.PROBE_KINDS), kind))
            code = _ffi.PROBE_CODES[kind]
            names, defaults = _ffi.PROBE_PARAMS[code], _ffi.PROBE_DEFAULTS[code]
            values, types = list(q[1:]), "both"
            if len(values) == len(names) + 1 or (values and isinstance(values[-1], str)):  # (types may follow x, y directly)
                types = values.pop()
            if not len(names) - len(defaults) <= len(values) <= len(names):
                raise EggError("probe %d (%s): expected (%r, %s[, %s[, types]])"
                               % (k, kind, kind, ", ".join(names[:-1]), names[-1]))
            values += defaults[len(defaults) - (len(names) - len(values)):]
            mask = _HandlerSurface._probe_mask(types, "probe %d" % k)
            try:
                values = [float(v) for v in values]
            except (TypeError, ValueError):
                raise EggError("probe %d (%s): the parameters must be numbers" % (k, kind)) from None
            arr[k].kind, arr[k].type_mask = code, mask
            for i, v in enumerate(values):
                arr[k].p[i] = v
        return len(probes), arr

    def _probe_table(self, n, arr):
        """the raw answer of one call: per probe `(white, yolk)`, each None or `(score, key, index, id, x, y, radius)`"""
        hits = (_ffi.EggProbeHit * max(2 * n, 1))()
        self._check(self._c("probe")(n, arr, hits))
        return [tuple((t.score, t.key, t.index, t.id, t.x, t.y, t.radius) if t.found else None for t in hits[2 * k:2 * k + 2])
                for k in range(n)]

    @staticmethod
    def _probe_hits(table):
        return [tuple(None if t is None else ProbeHit(t[3], t[2], t[0], t[4], t[5], t[6]) for t in pair) for pair in table]

    def probe(self, probes):
        """What is here (either solver order): per probe `(white_hit_or_None, yolk_hit_or_None)`, a hit
        being the ONE winning particle of that type as a `ProbeHit(id, index, score, x, y, radius)`.
        `("point", x, y[, reach[, types]])` names the particle whose centre is nearest (x, y) within `reach` (default inf;
        score = squared distance); `("ray", x0, y0, x1, y1[, pad[, types]])` the first disc of radius `radius + pad` the segment
        enters (score = t in [0, 1]).  types = "both" | "white" | "yolk".  Equal scores go to the older batch, then to the
        lower index.  Reads the committed state; stores nothing; at most 64 probes.  Raises EggError for a bad list."""
        n, arr = self._c_probes(probes)
        return self._probe_hits(self._probe_table(n, arr))

    @staticmethod
    def _probe_first(pair):
        """`(type_name, hit)` of the lower score of a probe's two hits, an exact tie to white; None without a hit"""
        white, yolk = pair
        if white is None and yolk is None:
            return None
        if yolk is None or (white is not None and not yolk.score < white.score):
            return ("white", white)
        return ("yolk", yolk)

    def pick(self, x, y, reach=float("inf"), types=3):
        """the particle nearest (x, y) within `reach`: None or `(type_name, hit)`, the lower score of the two types, an exact
        tie to white.  `hit.score <= hit.radius ** 2` tells whether the point is ON the particle."""
        return self._probe_first(self.probe([("point", x, y, reach, types)])[0])

    def raycast(self, x0, y0, x1, y1, pad=0.0, types=3):
        """the first particle disc (radius + pad) the segment from (x0, y0) to (x1, y1) enters: None or
        `(type_name, hit, (x, y))` with the point of impact `(x0 + t ex, y0 + t ey)`, t = hit.score"""
        first = self._probe_first(self.probe([("ray", x0, y0, x1, y1, pad, types)])[0])
        if first is None:
            return None
        x0, y0, x1, y1 = float(x0), float(y0), float(x1), float(y1)
        t = first[1].score
        return first + ((x0 + t * (x1 - x0), y0 + t * (y1 - y0)),)

    # ------------------------------------------------ fields (egg_field)
    @staticmethod
    def _c_field_spec(origin, cell, shape, types, path):
        """the grid of a call as an egg_field_spec; what only the host can check (shapes, names, types) is checked here,
        before any call into the library, the values by the library as well"""
        def pair(v, what, names):
            v = tuple(v) if isinstance(v, (tuple, list, np.ndarray)) else ()
            if len(v) != 2:
                raise EggError("field: %s must be (%s), not %r" % (what, names, v if v else None))
            return v
        x0, y0 = pair(origin, "origin", "x0, y0")
        nx, ny = pair(shape, "shape", "nx, ny")
        try:
            x0, y0, cell = float(x0), float(y0), float(cell)
        except (TypeError, ValueError):
            raise EggError("field: origin and cell must be numbers") from None
        for v in (nx, ny):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise EggError("field: shape must be two integers (nx, ny), not %r" % ((nx, ny),))
        nx, ny = int(nx), int(ny)
        if nx < 1 or ny < 1 or nx * ny > _ffi.FIELD_MAX_CELLS:
            raise EggError("field: shape (%d, %d): nx and ny are at least 1 and nx * ny at most %d" % (nx, ny, _ffi.FIELD_MAX_CELLS))
        if not (math.isfinite(cell) and cell > 0.0 and math.isfinite(1.0 / cell)):
            raise EggError("field: cell must be finite and above 0, with a finite inverse, not %r" % cell)
        if not (math.isfinite(x0) and math.isfinite(y0)):
            raise EggError("field: origin (%r, %r) is not finite" % (x0, y0))
        mask = _HandlerSurface._probe_mask(types, "field")
        if not isinstance(path, str) or path not in _ffi.FIELD_PATHS:
            raise EggError("field: path must be 'auto' or 'direct', not %r" % (path,))
        return _ffi.EggFieldSpec(x0, y0, cell, nx, ny, mask, _ffi.FIELD_PATHS[path])

    def _field_planes(self, spec, velocity):
        """one call of this object's entry point into fresh numpy planes: (count, svx, svy, totals)"""
        count = np.zeros((2, spec.ny, spec.nx), dtype=np.int32)
        svx = np.zeros((2, spec.ny, spec.nx), dtype=np.int64) if velocity else None
        svy = np.zeros((2, spec.ny, spec.nx), dtype=np.int64) if velocity else None
        planes = _ffi.EggFieldPlanes(count.ctypes.data, svx.ctypes.data if velocity else None, svy.ctypes.data if velocity else None)
        totals = _ffi.EggFieldTotals()
        self._check(self._c("field")(C.byref(spec), C.byref(planes), C.byref(totals)))
        return count, svx, svy, totals

    def field(self, origin, cell, shape, types="both", velocity=False, path="auto"):
        """The egg as a map (either solver order): the committed particles binned into the grid of
        `shape = (nx, ny)` square cells of side `cell` whose cell (0, 0) has its lower corner at `origin = (x0, y0)`.  Returns a
        `Field(count, svx, svy, inside, outside, dropped, units_tiled, units_direct)`: numpy planes of shape (2, ny, nx), [0]
        white and [1] yolk; with `velocity=True` also the int64 sums of the velocities scaled by 2^16, from which
        `Field.velocity()` derives the mean velocity per cell.  A particle is binned by its centre: cell
        `(int)((x - x0) * (1 / cell))`, inside iff that value is in [0, nx) -- and likewise for y.  types = "both" | "white" |
        "yolk"; path = "direct" is a test hook with the same answer.  Reads the committed state; stores nothing.  Raises
        EggError for a bad grid."""
        spec = self._c_field_spec(origin, cell, shape, types, path)
        count, svx, svy, t = self._field_planes(spec, bool(velocity))
        return Field(count, svx, svy, tuple(t.inside), tuple(t.outside), tuple(t.dropped), t.units_tiled, t.units_direct)

    # ------------------------------------------------ cover (egg_cover)
    @staticmethod
    def _c_cover_spec(origin, cell, shape, scale, types, path, what="cover"):
        """the grid of a call as an egg_cover_spec; what only the host can check (shapes, names, types) is checked here,
        before any call into the library, the values by the library as well"""
        def pair(v, name, names):
            v = tuple(v) if isinstance(v, (tuple, list, np.ndarray)) else ()
            if len(v) != 2:
                raise EggError("%s: %s must be (%s), not %r" % (what, name, names, v if v else None))
            return v
        x0, y0 = pair(origin, "origin", "x0, y0")
        nx, ny = pair(shape, "shape", "nx, ny")
        try:
            x0, y0, cell, scale = float(x0), float(y0), float(cell), float(scale)
        except (TypeError, ValueError):
            raise EggError("%s: origin, cell and scale must be numbers" % what) from None
        for v in (nx, ny):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise EggError("%s: shape must be two integers (nx, ny), not %r" % (what, (nx, ny)))
        nx, ny = int(nx), int(ny)
        if nx < 1 or ny < 1 or nx * ny > _ffi.COVER_MAX_CELLS:
            raise EggError("%s: shape (%d, %d): nx and ny are at least 1 and nx * ny at most %d" % (what, nx, ny, _ffi.COVER_MAX_CELLS))
        if not (math.isfinite(cell) and cell > 0.0 and math.isfinite(1.0 / cell)):
            raise EggError("%s: cell must be finite and above 0, with a finite inverse, not %r" % (what, cell))
        if not (math.isfinite(x0) and math.isfinite(y0)):
            raise EggError("%s: origin (%r, %r) is not finite" % (what, x0, y0))
        if not (math.isfinite(scale) and scale > 0.0):
            raise EggError("%s: scale must be finite and above 0, not %r" % (what, scale))
        mask = _HandlerSurface._probe_mask(types, what)
        if not isinstance(path, str) or path not in _ffi.COVER_PATHS:
            raise EggError("%s: path must be 'auto', 'direct', 'lanes' or 'wave', not %r" % (what, path))
        return _ffi.EggCoverSpec(x0, y0, cell, scale, nx, ny, mask, _ffi.COVER_PATHS[path])

    def _cover_planes(self, spec, owner):
        """one call of this object's entry point into fresh numpy planes: (cover, owner, totals)"""
        cover = np.zeros((2, spec.ny, spec.nx), dtype=np.int32)
        own = np.zeros((2, spec.ny, spec.nx), dtype=np.int32) if owner else None
        planes = _ffi.EggCoverPlanes(cover.ctypes.data, own.ctypes.data if owner else None)
        totals = _ffi.EggCoverTotals()
        self._check(self._c("cover")(C.byref(spec), C.byref(planes), C.byref(totals)))
        return cover, own, totals

    @staticmethod
    def _cover_totals(spec, t):
        return (spec.cell, tuple(t.inside), tuple(t.outside), tuple(t.dropped), tuple(t.hits), tuple(t.covered), t.covered_both, t.covered_any,
                t.units_lanes, t.units_wave, t.units_direct)

    def cover(self, origin, cell, shape, scale=1.0, types="both", owner=False, path="auto"):
        """The floor under the egg (either solver order): every committed particle's disc of radius
        `scale * radius` rastered into the grid of `shape = (nx, ny)` square cells of side `cell` whose cell (0, 0) has its
        lower corner at `origin = (x0, y0)`.  Returns a `Cover`: `cover` an int32 plane of shape (2, ny, nx), [0] white and [1]
        yolk, counting the discs over each cell's CENTRE; with `owner=True` also the smallest batch id among them (-1: none);
        the totals, and `Cover.area()` in px^2.  scale = 1 is the simulated disc, 12 the disc as it is drawn; a disc of more
        than 64 cells in radius is dropped.  types = "both" | "white" | "yolk"; path = "direct" | "lanes" | "wave" are test
        hooks with the same planes.  Reads the committed state; stores nothing.  Raises EggError for a bad grid."""
        spec = self._c_cover_spec(origin, cell, shape, scale, types, path)
        cover, own, t = self._cover_planes(spec, bool(owner))
        return Cover(cover, own, *self._cover_totals(spec, t))

    # ------------------------------------------------ pieces (egg_pieces)
    def _c_pieces_spec(self, reach, types, what="pieces"):
        """the reach per type and the mask of a call as an egg_pieces_spec.  reach=None is, per type,
        max(collision_overlap_factor, cohesion_interaction_distance_factor) of this object's config: the factor the solver
        sizes its spatial hash by.  A number holds for both types, a pair is (white, yolk)."""
        mask = _HandlerSurface._probe_mask(types, what)
        if reach is None:
            reach = tuple(max(float(cfg["collision_overlap_factor"]), float(cfg["cohesion_interaction_distance_factor"]))
                          for cfg in (self._white_config, self._yolk_config))
        elif isinstance(reach, (tuple, list, np.ndarray)):
            reach = tuple(reach)
        else:
            reach = (reach, reach)
        if len(reach) != 2:
            raise EggError("%s: reach must be None, a number or (white, yolk), not %r" % (what, reach))
        try:
            reach = tuple(float(v) for v in reach)
        except (TypeError, ValueError):
            raise EggError("%s: reach must be None, a number or (white, yolk) numbers" % what) from None
        for v in reach:
            if not (math.isfinite(v) and v > 0.0):
                raise EggError("%s: reach must be finite and above 0, not %r" % (what, v))
        return _ffi.EggPiecesSpec((C.c_double * 2)(*reach), mask, 0)

    @staticmethod
    def _piece_ids(ids, what="pieces"):
        """None (every live batch) or the listed ids as a contiguous int64 array"""
        if ids is None:
            return None
        try:
            return np.ascontiguousarray([int(i) for i in ids], dtype=np.int64)
        except (TypeError, ValueError):
            raise EggError("%s: ids must be None or a list of batch ids" % what) from None

    def _piece_table(self, spec, ids):
        """the raw records of one call of this object's entry point: an int64 array [n, 2, 8] of (n, pieces, largest, first,
        singles, dropped, sx, sy), `ids` an int64 array (it may be empty: no batch is asked for) or None for every live batch"""
        n = len(self.list_ids()) if ids is None else ids.size
        if ids is not None and n == 0:
            return np.zeros((0, 2, 8), dtype=np.int64)
        out = np.zeros(max(2 * n, 1), dtype=_PIECE_RECORD)  # (egg_piece_summary, field for field)
        args = (C.byref(spec), 0, None, out.ctypes.data) if ids is None else (C.byref(spec), n, ids.ctypes.data, out.ctypes.data)
        if self._PREFIX == "egg_":
            args += (None, None)
        self._check(self._c("pieces")(*args))
        return np.stack([out[name][:2 * n].astype(np.int64) for name in _PIECE_RECORD.names], axis=1).reshape(n, 2, 8)

    @staticmethod
    def _piece_summaries(table):
        """per batch `(white, yolk)` of PieceSummary, or None where n == 0: the centroid by the library's two divisions"""
        scale = _ffi.SENSOR_POSITION_SCALE
        res = []
        for pair in np.asarray(table, dtype=np.int64).reshape(-1, 2, 8).tolist():
            row = []
            for n, pieces, largest, first, singles, dropped, sx, sy in pair:
                kept = largest - dropped
                row.append(None if n == 0 else PieceSummary(n, pieces, largest, first, singles, dropped,
                                                            (float(sx) / scale) / float(kept) if kept else None,
                                                            (float(sy) / scale) / float(kept) if kept else None))
            res.append(tuple(row))
        return res

    def pieces(self, ids=None, reach=None, types="both"):
        """Is the egg still one egg (either solver order): per id (None: every batch of list_ids(), in
        that order) `(white, yolk)`, each a `PieceSummary(n, pieces, largest, first, singles, dropped, x, y)` or None where the
        batch has no particle of the type or `types` leaves it out.  Two particles of one type of one batch are linked iff
        `d2 <= (reach * (ra + rb)) ** 2`; a piece is a connected component, the body the largest piece.  reach=None takes, per
        type, max(collision_overlap_factor, cohesion_interaction_distance_factor) of the config; a number holds for both
        types, a pair is (white, yolk).  Reads the committed state; stores nothing.  Raises EggError for an unknown id, a bad
        reach, or a batch with more than 4,096 particles of a covered type."""
        return self._piece_summaries(self._piece_table(self._c_pieces_spec(reach, types), self._piece_ids(ids)))

    def is_whole(self, id, reach=None, types="both"):
        """True iff every covered atom of the batch -- its white, its yolk, by `types` -- is ONE piece"""
        return all(a is None or a.pieces == 1 for a in self.pieces([id], reach, types)[0])

    # ------------------------------------------------ touches (egg_touches)
    def _c_touch_spec(self, reach, types, what="touches", flags=0):
        """the reach per type, the mask and the flags of a call as an egg_touch_spec.  reach=None is, per type, the
        collision_overlap_factor of this object's config: a touch is then exactly a pair the solver's collision branch acts
        on.  A number holds for both types, a pair is (white, yolk)."""
        if reach is None:
            reach = tuple(float(cfg["collision_overlap_factor"]) for cfg in (self._white_config, self._yolk_config))
        spec = self._c_pieces_spec(reach, types, what)  # (the same checks: a reach finite and above 0, a known mask)
        return _ffi.EggTouchSpec((C.c_double * 2)(*spec.reach), spec.type_mask, int(flags))

    def _touch_records(self, call):
        """the records of one answer as an int64 array [n, 8] of (entry, type, other, pairs, particles, dropped, sx, sy):
        `call(cap, out, n_out)` is the entry point with everything before its buffer bound.  *n_out is always the size of the
        answer: a call whose buffer was short is made once more with that size."""
        cap, n = 256, C.c_int64(0)
        while True:
            out = np.zeros(max(cap, 1), dtype=_TOUCH_RECORD)
            rc = call(cap, out.ctypes.data, C.byref(n))
            if rc < 0 and n.value > cap:
                cap = n.value
                continue
            self._check(rc)
            rec = out[:n.value]
            return np.stack([rec["slot"].astype(np.int64) >> 1, rec["slot"].astype(np.int64) & 1] +
                            [rec[name].astype(np.int64) for name in ("other", "pairs", "particles", "dropped", "sx", "sy")], axis=1).reshape(-1, 8)

    def _touch_table(self, spec, ids):
        """one call of this object's egg_touches: `ids` an int64 array (it may be empty: no batch is asked for) or None for every
        live batch"""
        if ids is not None and ids.size == 0:
            return np.zeros((0, 8), dtype=np.int64)
        head = (C.byref(spec), 0, None) if ids is None else (C.byref(spec), ids.size, ids.ctypes.data)
        return self._touch_records(functools.partial(self._c("touches"), *head))

    @staticmethod
    def _merge_touch_tables(tables):
        """tables of several handles or ranks as one: the rows of one (entry, type, other) added -- every field is additive over
        any split of the other batch's particles -- and sorted"""
        rows = np.concatenate([np.asarray(t, dtype=np.int64).reshape(-1, 8) for t in tables] + [np.zeros((0, 8), dtype=np.int64)])
        if rows.shape[0] == 0:
            return rows
        keys, inverse = np.unique(rows[:, :3], axis=0, return_inverse=True)
        out = np.zeros((keys.shape[0], 8), dtype=np.int64)
        out[:, :3] = keys
        np.add.at(out[:, 3:], np.asarray(inverse).reshape(-1), rows[:, 3:])  # (int64 wraps as the library's sums do)
        return out

    @staticmethod
    def _touch_lists(table, n):
        """per entry 0 .. n - 1 `(white, yolk)`, each the list of Touch of that query in ascending `other`"""
        scale = _ffi.SENSOR_POSITION_SCALE
        res = [([], []) for _ in range(n)]
        for entry, w, other, pairs, particles, dropped, sx, sy in np.asarray(table, dtype=np.int64).reshape(-1, 8).tolist():
            kept = pairs - dropped
            res[entry][w].append(Touch(other, pairs, particles, dropped, (float(sx) / (2.0 * kept)) / scale if kept > 0 else None,
                                       (float(sy) / (2.0 * kept)) / scale if kept > 0 else None))
        return res

    def touch_table(self, ids=None, reach=None, types="both"):
        """touches() as its raw records: an int64 array [n, 8] of (entry, type, other, pairs, particles, dropped, sx, sy), ordered
        by (entry, type, other); `entry` is the index into `ids` (None: list_ids()), `type` 0 white and 1 yolk."""
        return self._touch_table(self._c_touch_spec(reach, types, "touch_table"), self._piece_ids(ids, "touch_table"))

    def touches(self, ids=None, reach=None, types="both"):
        """Which eggs touch which, how much and where (either solver order): per id (None: every batch
        of list_ids(), in that order; ids may repeat) `(white, yolk)`, each the list of `Touch(other, pairs, particles, dropped,
        x, y)` of the OTHER batches with a particle of that type touching one of this batch's, in ascending id.  Particles a and
        b of one type touch iff `d2 <= (reach * (ra + rb)) ** 2`; reach=None takes the type's collision_overlap_factor, so that
        a touch is a pair the solver's collision branch acts on; a number holds for both types, a pair is (white, yolk).  Never
        across types, never inside a batch (pieces() covers that).  Reads the committed state; stores nothing.  Raises EggError
        for an unknown id or a bad reach."""
        ids = self._piece_ids(ids, "touches")
        n = len(self.list_ids()) if ids is None else ids.size
        return self._touch_lists(self._touch_table(self._c_touch_spec(reach, types), ids), n)

    def touching(self, a, b=None, reach=None, types="both"):
        """True iff batch `a` touches batch `b` in a covered type; with b=None the sorted ids of the batches that touch `a`"""
        others = sorted(set(self.touch_table([a], reach, types)[:, 2].tolist()))
        if b is None:
            return others
        if int(b) not in self.list_ids():
            raise EggError("[ERROR] In SimulationHandler.touching: no batch with id `%s`" % (b,))
        return int(b) in others

    @staticmethod
    def _c_touch_discs(discs, types, key, what="touches_of"):
        """a caller's discs as the arguments of egg_touches_of: `discs` an array [n, 3] of (x, y, r), or a pair (white discs,
        yolk discs) of such arrays when types is "both"; returns (queries, n_queries, x, y, r)"""
        mask = _HandlerSurface._probe_mask(types, what)
        try:
            if mask == 3:
                white, yolk = discs
                parts = [np.asarray(white, dtype=np.float64).reshape(-1, 3), np.asarray(yolk, dtype=np.float64).reshape(-1, 3)]
            else:
                parts = [np.asarray(discs, dtype=np.float64).reshape(-1, 3)]
            key = int(key)
        except (TypeError, ValueError):
            raise EggError("%s: discs must be an array [n, 3] of (x, y, r), or (white, yolk) of them for both types; key an id" % what) from None
        kinds = (0, 1) if mask == 3 else (mask - 1,)
        queries = (_ffi.EggTouchQuery * len(parts))(*[_ffi.EggTouchQuery(key, w, p.shape[0]) for w, p in zip(kinds, parts)])
        xyr = np.concatenate(parts)
        if not np.isfinite(xyr[:, 2]).all():
            raise EggError("%s: a radius is not finite" % what)
        return queries, len(parts), np.ascontiguousarray(xyr[:, 0]), np.ascontiguousarray(xyr[:, 1]), np.ascontiguousarray(xyr[:, 2])

    def _touch_of_table(self, spec, queries, n_queries, x, y, r):
        """one call of egg_touches_of on this handle"""
        return self._touch_records(functools.partial(self._lib.egg_touches_of, self._h, C.byref(spec), n_queries, C.cast(queries, C.c_void_p),
                                                     x.ctypes.data, y.ctypes.data, r.ctypes.data))

    def _touch_of_tables(self, spec, queries, n_queries, x, y, r):
        """the tables of egg_touches_of of every handle behind this object (one here)"""
        return [self._touch_of_table(spec, queries, n_queries, x, y, r)]

    def touches_of(self, discs, reach=None, types="white", key=-1):
        """What a caller-set list of discs touches: `discs` an array [n, 3] of (x, y, r) of the type `types` -- or, with
        types="both", a pair (white discs, yolk discs) --; returns `(white, yolk)` lists of Touch as touches() does for one id.
        A batch whose id equals `key` is left out (the discs are that batch's own, say); -1 leaves none out."""
        spec = self._c_touch_spec(reach, types, "touches_of", self._TOUCH_OF_FLAGS)
        queries, n, x, y, r = self._c_touch_discs(discs, types, key)
        table = self._merge_touch_tables(self._touch_of_tables(spec, queries, n, x, y, r))
        table[:, 0] = 0  # (the one query per type: entry 0)
        return self._touch_lists(table, 1)[0]

    _TOUCH_OF_FLAGS = 0

    # ------------------------------------------------ impulses (egg_impulse)
    @staticmethod
    def _c_impulses(records):
        """a list of Impulse records, or tuples `(action, region, params...[, options])` with options a dict of `id`, `linear`,
        `by_inv_mass`, as an egg_impulse_record array.  What only the host can check (shape, names) is checked here, the values
        by the library."""
        records = list(records)
        if len(records) > _ffi.MAX_IMPULSES:
            raise EggError("impulse: a call takes 0 .. %d records, not %d" % (_ffi.MAX_IMPULSES, len(records)))
        arr = (_ffi.EggImpulse * max(len(records), 1))()
        for k, r in enumerate(records):
            if not isinstance(r, Impulse):
                r = tuple(r) if isinstance(r, (tuple, list)) else ()
                opts = {}
                if r and isinstance(r[-1], dict):
                    opts, r = dict(r[-1]), r[:-1]
                if len(r) < 2 or set(opts) - {"id", "linear", "by_inv_mass"}:
                    raise EggError("impulse: record %d: expected (action, region, params...[, {id, linear, by_inv_mass}])" % k)
                r = Impulse(r[0], r[1], tuple(r[2:]), opts.get("id"), opts.get("linear", False), opts.get("by_inv_mass", False))
            if not isinstance(r.action, str) or r.action not in _ffi.IMPULSE_CODES:
                raise EggError("impulse: record %d: action must be one of %s, not %r" % (k, ", ".join(_ffi.IMPULSE_ACTIONS), r.action))
            code = _ffi.IMPULSE_CODES[r.action]
            names = _ffi.IMPULSE_PARAMS[code]
            values = tuple(r.a) if isinstance(r.a, (tuple, list, np.ndarray)) else ()
            if len(values) != len(names):
                raise EggError("impulse: record %d (%s): expected the parameters (%s)" % (k, r.action, ", ".join(names)))
            try:
                values = [float(v) for v in values]
            except (TypeError, ValueError):
                raise EggError("impulse: record %d (%s): the parameters must be numbers" % (k, r.action)) from None
            try:
                _, region = _HandlerSurface._c_sensors([r.region])
            except EggError as e:
                raise EggError("impulse: record %d: region: %s" % (k, e)) from None
            if r.id is not None and (isinstance(r.id, bool) or not isinstance(r.id, (int, np.integer))):
                raise EggError("impulse: record %d: id must be None or a batch id, not %r" % (k, r.id))
            arr[k].region = region[0]
            arr[k].action = code
            arr[k].flags = (_ffi.IMPULSE_LINEAR if r.linear else 0) | (_ffi.IMPULSE_BY_INV_MASS if r.by_inv_mass else 0)
            arr[k].id = _ffi.IMPULSE_ALL_BATCHES if r.id is None else int(r.id)
            for q, v in enumerate(values):
                arr[k].a[q] = v
        return len(records), arr

    def _impulse_table(self, n, arr, results=True):
        """one call of this object's entry point: an int64 array [n, 8] of (count, sdvx, sdvy, skipped) x (white, yolk), or
        None with results=False (the totals are then neither finished nor copied)"""
        out = (_ffi.EggImpulseResult * max(n, 1))() if results else None
        self._check(self._c("impulse")(n, arr, out))
        if not results:
            return None
        return np.array([list(r.count) + list(r.sdvx) + list(r.sdvy) + list(r.skipped) for r in out[:n]], dtype=np.int64).reshape(n, 8)

    @staticmethod
    def _impulse_results(table):
        return [ImpulseResult(*(tuple(int(v) for v in row[2 * q:2 * q + 2]) for q in range(4))) for row in np.asarray(table).reshape(-1, 8)]

    def impulse(self, records, results=True):
        """Act on the particles (either solver order): the committed velocities of the particles inside
        each record's region are edited on the device, record after record, and per record an `ImpulseResult(count, sdvx, sdvy,
        skipped)` comes back (None with results=False).  A record is an `Impulse(action, region, a, id=None, linear=False,
        by_inv_mass=False)` or a tuple `(action, region, params...[, {"id": .., "linear": .., "by_inv_mass": ..}])`: "kick" adds
        w (ax, ay); "blast" adds w s along the unit vector from (cx, cy); "swirl" adds w omega times the arm from (cx, cy) turned
        a quarter; "brake" moves the velocity the fraction w k towards (ux, uy).  The region takes the tuple form of
        set_sensors; w is 1, with `linear` 1 - d / R of a disc or capsule, with `by_inv_mass` times the inverse mass.  Only vx, vy
        change; stores nothing; at most 64 records; refused while a step is in flight.  Raises EggError for a bad list or an
        unknown id (nothing changes)."""
        n, arr = self._c_impulses(records)
        table = self._impulse_table(n, arr, bool(results))
        return None if table is None else self._impulse_results(table)

    def kick(self, region, ax, ay, id=None, linear=False, by_inv_mass=False):
        """the particles inside `region` get (ax, ay) added to their velocity: the one ImpulseResult"""
        return self.impulse([Impulse("kick", region, (ax, ay), id, linear, by_inv_mass)])[0]

    def blast(self, cx, cy, R, s, id=None, by_inv_mass=False, types="both"):
        """a blast of strength s px/s at (cx, cy) that falls off linearly to 0 at the distance R (s < 0 sucks): the one
        ImpulseResult"""
        return self.impulse([Impulse("blast", ("disc", cx, cy, R, types), (cx, cy, s), id, True, by_inv_mass)])[0]

    def stir(self, cx, cy, R, omega, id=None, linear=False, types="both"):
        """the particles within R of (cx, cy) get the velocity of a turn at omega rad/s about it added: the one ImpulseResult"""
        return self.impulse([Impulse("swirl", ("disc", cx, cy, R, types), (cx, cy, omega), id, linear, False)])[0]

    def brake(self, region, k=1.0, ux=0.0, uy=0.0, id=None, linear=False):
        """the particles inside `region` move their velocity the fraction k towards (ux, uy); k = 1 stops them at it: the one
        ImpulseResult"""
        return self.impulse([Impulse("brake", region, (ux, uy, k), id, linear, False)])[0]

    # ------------------------------------------------ measures (egg_measure)
    @staticmethod
    def _c_measure_spec(region, types, what="measure"):
        """the region (None: every particle of the atom) and the mask of a call as an egg_measure_spec.  The region takes the
        tuple form of set_sensors; what only the host can check (shape, names) is checked here, the values by the library."""
        spec = _ffi.EggMeasureSpec()
        spec.type_mask = _HandlerSurface._probe_mask(types, what)
        if region is not None:
            try:
                _, arr = _HandlerSurface._c_sensors([region])
            except EggError as e:
                raise EggError("%s: region: %s" % (what, e)) from None
            spec.region = arr[0]
            spec.flags = _ffi.MEASURE_REGION
        return spec

    def _measure_check(self, spec):
        """the library's checks of a spec alone: a call with an empty list, which launches and writes nothing"""
        none = np.zeros(1, dtype=np.int64)
        self._check(self._c("measure")(C.byref(spec), 0, none.ctypes.data, none.ctypes.data))

    def _measure_table(self, spec, ids):
        """the raw records of one call of this object's entry point: an int64 array [n, 2, 24], `ids` an int64 array (it may
        be empty: no batch is asked for) or None for every live batch"""
        n = len(self.list_ids()) if ids is None else ids.size
        out = np.zeros((n, 2, len(_ffi.MEASURE_FIELDS)), dtype=np.int64)
        if ids is not None and n == 0:
            self._measure_check(spec)
            return out
        spare = out if n else np.zeros(1, dtype=np.int64)  # (out is never NULL)
        self._check(self._c("measure")(C.byref(spec), 0 if ids is None else n, None if ids is None else ids.ctypes.data, spare.ctypes.data))
        return out

    @staticmethod
    def _measures(table):
        """per batch `(white, yolk)` of Measure, or None where n == 0"""
        return [tuple(None if rec[1] == 0 else Measure(*rec) for rec in pair)
                for pair in np.asarray(table, dtype=np.int64).reshape(-1, 2, len(_ffi.MEASURE_FIELDS)).tolist()]

    def measure_table(self, ids=None, region=None, types="both"):
        """measure() as the library's integers: an int64 array [n, 2, 24], [i][0] the white of ids[i] and [i][1] its yolk, the
        fields in the order of `Measure._fields` (egg_measure_record).  A type `types` leaves out or the batch lacks is all 0."""
        return self._measure_table(self._c_measure_spec(region, types, "measure_table"), self._piece_ids(ids, "measure_table"))

    def measure(self, ids=None, region=None, types="both"):
        """What is this egg doing, as a body (either solver order): per id (None: every batch of
        list_ids(), in that order) `(white, yolk)`, each a `Measure` or None where no particle of the type is measured.  A
        Measure holds the 24 integers the device sums over the particles of one type of one batch -- counts, position, mass,
        momentum, twice the kinetic energy, the bounding box, the highest squared speed, second moments, angular momentum and
        reach about the quantised centroid -- and derives `mass`, `centroid`, `center_of_mass`, `momentum`, `velocity`,
        `kinetic_energy`, `bounds`, `max_speed`, `reach`, `spin` and `axes()` from them on the host.  With `region` (the tuple form
        of set_sensors) only the particles inside it are measured.  Reads the committed state; stores nothing; refused while a
        step is in flight.  Raises EggError for an unknown id or a bad region."""
        return self._measures(self.measure_table(ids, region, types))

    def at_rest(self, id, speed, types="both"):
        """True iff every covered atom of the batch -- its white, its yolk, by `types` -- has `max_speed <= speed`"""
        speed = float(speed)
        return all(a is None or a.max_speed <= speed for a in self.measure([id], None, types)[0])

    # ------------------------------------------------ collider bodies (egg_set_collider_bodies)
    _BODIES_LIMIT =("collider bodies: the device integrates a body from the loads of one handle, so bodies run on a single "
                     "SimulationHandler only; only lists without a body are accepted here")

    @staticmethod
    def _c_bodies(bodies):
        """a list with one element per collider -- None (no body), (inv_mass, inv_inertia), (inv_mass, inv_inertia, ax, ay) or
        (inv_mass, inv_inertia, ax, ay, drag, spin_drag) -- as an egg_collider_body array; shape, finiteness and signs are
        checked here, before any call into the library"""
        return _HandlerSurface._c_records(_BODY, bodies)

    def set_collider_bodies(self, bodies):
        """SimulationHandler.set_collider_bodies where several handles share a step (SimulationGroup,
        ShardedSimulationHandler): a list without a body is accepted and changes nothing, anything else raises EggError naming
        the limit (after the checks of the records)."""
        n, arr = self._c_bodies(bodies)
        if any(arr[k].inv_mass > 0.0 or arr[k].inv_inertia > 0.0 for k in range(n)):
            raise EggError(self._BODIES_LIMIT)

    def get_collider_bodies(self):
        """one all-zero record per collider here, see set_collider_bodies"""
        return [(0.0, 0.0, 0.0, 0.0, 0.0, 0.0)] * len(self.get_colliders())

    # ------------------------------------------------ collider contacts (egg_set_collider_contacts)
    _CONTACTS_LIMIT = ("collider contacts: a contact changes a collider body, and bodies run on a single SimulationHandler only; "
                       "only lists with every contact off are accepted here")

    @staticmethod
    def _c_contacts(contacts, iterations=4):
        """a list with one element per collider -- None (off), a restitution in [0, 1], or True (on, restitution 0) -- as an
        egg_collider_contact array, and the iterations (1 .. 16, or 0 for the default); shape and range are checked here,
        before any call into the library"""
        contacts = list(contacts)
        arr = (_ffi.EggColliderContact * max(len(contacts), 1))()
        for k, c in enumerate(contacts):
            if c is None:
                continue
            if c is True:
                c = 0.0
            if isinstance(c, bool) or not isinstance(c, (int, float)):
                raise EggError("collider contact %d: expected None, True or a restitution in [0, 1], not %r" % (k, c))
            c = float(c)
            if not (math.isfinite(c) and 0.0 <= c <= 1.0):
                raise EggError("collider contact %d: the restitution %r lies outside [0, 1]" % (k, c))
            arr[k].restitution, arr[k].on = c, 1
        if isinstance(iterations, bool) or not isinstance(iterations, int) or not 0 <= iterations <= 16:
            raise EggError("collider contacts: iterations %r is not an integer in 1 .. 16 (or 0 for the default of 4)" % (iterations,))
        return len(contacts), arr, iterations

    def set_collider_contacts(self, contacts, iterations=4):
        """SimulationHandler.set_collider_contacts where several handles share a step (SimulationGroup,
        ShardedSimulationHandler): a list with every contact off is accepted and changes nothing, anything else raises EggError
        naming the limit (after the checks of the records)."""
        n, arr, _ = self._c_contacts(contacts, iterations)
        if any(arr[k].on for k in range(n)):
            raise EggError(self._CONTACTS_LIMIT)

    def get_collider_contacts(self):
        """every contact off here, see set_collider_contacts: `([None, ...], 4)`"""
        return [None] * len(self.get_colliders()), 4

    def collider_contact_solves(self):
        """0 here, see set_collider_contacts"""
        return 0

    # ------------------------------------------------ force fields (egg_set_forces)
    @staticmethod
    def _c_forces(forces):
        """a list of tuples `(kind, parameters...[, types])` or dicts `{"kind": ..., <parameter names>, "types": ...}` as an
        egg_force array; what only the host can check (shape, names) is checked here, the values by the library"""
        return _HandlerSurface._c_kind_list(_FORCE_LIST, forces)

    def set_forces(self, forces):
        """The ordered list of force fields, at most 16 ("Forces"; relaxed order only), as
        accelerations in px/s^2: `("uniform", gx, gy)` is gravity or wind, `("radial", cx, cy, strength, R)` pulls towards
        (cx, cy) (pushes away for a negative strength) within R with a linear falloff, `("vortex", cx, cy, strength, R)`
        stirs around (cx, cy); each takes an optional last element (or dict key) types = "both" | "white" | "yolk", and
        each may be a dict with "kind" and the parameter names.  In every sub-step of a relaxed step the fields' sum
        accelerates a particle's velocity before the pre-solve damps it.  `[]` clears the list.  Raises EggError for a bad
        list (nothing changes) and for a non-empty list on a handle in exact order; set_solver_order("exact") raises while
        the list is not empty."""
        n, arr = self._c_forces(forces)
        self._check(self._c("set_forces")(n, arr))

    def get_forces(self):
        """the list as stored, as tuples `(kind, parameters..., types)`"""
        return self._kind_tuples(_FORCE_LIST, self._get_array(self._c("get_forces"), _ffi.EggForce, _ffi.MAX_FORCES))

    # ------------------------------------------------ viscosity (egg_set_viscosity)
    @staticmethod
    def _c_viscosity(white, yolk):
        """the two coefficients as the double[2] egg_set_viscosity takes; the range is checked here as the library checks it"""
        arr = (C.c_double * 2)()
        for w, (name, v) in enumerate((("white", white), ("yolk", yolk))):
            try:
                v = float(v)
            except (TypeError, ValueError):
                raise EggError("viscosity: the %s coefficient must be a number, not %r" % (name, v)) from None
            if not (0.0 <= v <= 1.0):  # (false for a NaN)
                raise EggError("viscosity: the %s coefficient %r lies outside [0, 1]" % (name, v))
            arr[w] = v
        return arr

    def set_viscosity(self, white=0.0, yolk=0.0):
        """XSPH viscosity per particle type, each coefficient in [0, 1], 0 = off ("Viscosity"; relaxed
        order only).  In every sub-step of a relaxed step, after its last collision pass, a particle's displacement of the
        sub-step is blended with the weighted mean of its neighbours' within one spatial-hash cell size: relative motion
        inside an egg dies out, common motion stays (which `damping` cannot tell apart).  Positions are not touched; the
        committed velocity is the smoothed one.  Raises EggError for a value outside [0, 1] (nothing changes) and for a
        non-zero coefficient on a handle in exact order; set_solver_order("exact") raises while a coefficient is not 0."""
        arr = self._c_viscosity(white, yolk)  # (refused here before any device call)
        self._check(self._c("set_viscosity")(arr))

    def viscosity(self):
        """(white, yolk): the coefficients as stored"""
        c = (C.c_double * 2)()
        self._check(self._c("get_viscosity")(c))
        return (c[0], c[1])

    def viscosity_pairs(self):
        """[white, yolk]: distinct pairs within the cell size, over the viscosity passes of committed steps, since creation"""
        return self._get_counts(self._c("get_viscosity_pairs"))

    # ------------------------------------------------ white-yolk coupling (egg_set_coupling)
    _COUPLING_LIMIT = ("coupling: white-yolk coupling runs on a single SimulationHandler only -- the halo of a device group "
                       "or of sharded ranks carries no ghosts of the other type; only factor 0 (off) is accepted here")

    @staticmethod
    def _c_coupling(factor, strength):
        """(factor, strength) as the doubles egg_set_coupling takes; the ranges are checked here as the library checks them"""
        return _HandlerSurface._c_range_pair("coupling", "factor", factor, strength)

    def set_coupling(self, factor=0.0, strength=1.0):
        """SimulationHandler.set_coupling where several handles share a step (SimulationGroup, ShardedSimulationHandler):
        factor 0 is accepted and changes nothing, anything else raises EggError naming the limit (after the range check)."""
        factor, strength = self._c_coupling(factor, strength)
        if factor != 0.0:
            raise EggError(self._COUPLING_LIMIT)

    def coupling(self):
        """(factor, strength): always (0.0, 1.0) here, see set_coupling"""
        return (0.0, 1.0)

    def coupling_solves(self):
        return 0

    # ------------------------------------------------ white-yolk adhesion (egg_set_adhesion)
    _ADHESION_LIMIT = ("adhesion: white-yolk adhesion is a band in the coupling pass, which runs on a single "
                       "SimulationHandler only; only reach 0 (off) is accepted here")

    @staticmethod
    def _c_adhesion(reach, strength):
        """(reach, strength) as the doubles egg_set_adhesion takes; the ranges are checked here as the library checks them"""
        return _HandlerSurface._c_range_pair("adhesion", "reach", reach, strength)

    def set_adhesion(self, reach=0.0, strength=1.0):
        """SimulationHandler.set_adhesion where several handles share a step (SimulationGroup, ShardedSimulationHandler):
        reach 0 is accepted and changes nothing, anything else raises EggError naming the limit (after the range check)."""
        reach, strength = self._c_adhesion(reach, strength)
        if reach != 0.0:
            raise EggError(self._ADHESION_LIMIT)

    def adhesion(self):
        """(reach, strength): always (0.0, 1.0) here, see set_adhesion"""
        return (0.0, 1.0)

    def adhesion_solves(self):
        return 0

    # ------------------------------------------------ yolk containment (egg_set_containment)
    @staticmethod
    def _c_containment(factor, strength):
        """(factor, strength) as the doubles egg_set_containment takes; the ranges are checked here as the library checks them"""
        return _HandlerSurface._c_range_pair("containment", "factor", factor, strength)

    def set_containment(self, factor=0.0, strength=1.0):
        """Yolk containment: a disc around the centroid of each batch's white that no yolk particle of that batch may leave
        ("Containment"; relaxed order only).  In every sub-step of a relaxed step, after the coupling
        pass and before the collision passes, the disc's radius is L = factor * (RMS distance of the batch's white from
        its centroid), and a yolk particle farther out than L is moved back along its ray to
        L + (1 - strength) * (d - L); factor 0 = off, and 2 and more suit a default egg.  One-way: the white is never
        moved.  It needs neither coupling nor adhesion, and works on device groups and sharded ranks alike: a batch lives
        wholly on one handle.  Raises EggError for a NaN, negative or infinite factor or a strength outside [0, 1]
        (nothing changes) and for factor > 0 in exact order; set_solver_order("exact") raises while factor > 0."""
        factor, strength = self._c_containment(factor, strength)  # (refused here before any device call)
        self._check(self._c("set_containment")(factor, strength))

    def containment(self):
        """(factor, strength) as stored"""
        return self._get_pair(self._c("get_containment"))

    def containment_hits(self):
        """projections, one per (yolk particle, sub-step), over committed steps, since creation"""
        return self._get_count(self._c("get_containment_hits"))

    def _init_host_state(self, white_config, yolk_config):
        """config tables (validated like the reference, L:1253-1320), hidden constants and render switches; no device"""
        if white_config is None and yolk_config is None:
            white_config, yolk_config = default_configs()
        if yolk_config is None:  # L:426
            yolk_config = white_config
        _assert_types(white_config, "table", yolk_config, "table")
        self._white_config = {}
        self._yolk_config = {}
        self._load_config(copy.deepcopy(white_config), True)
        self._load_config(copy.deepcopy(yolk_config), False)
        # hidden constants (L:447-448, math.lua:2)
        self._mass_distribution_variance = 4
        self._max_collision_fraction = 0.05
        self._batch_colors = {}
        # render constants (L:444-449)
        self._thresholding_threshold = 0.3
        self._thresholding_smoothness = 0.01
        self._use_particle_color_flag = False
        self._use_lighting_flag = True

    # ------------------------------------------------------------------ config
    def _load_config(self, config, white_or_yolk):  # L:1253-1320
        scope = "In SimulationHandler.set_white_config: " if white_or_yolk else "In SimulationHandler.set_yolk_config: "
        target = self._white_config if white_or_yolk else self._yolk_config
        for key, value in config.items():
            entry = _VALID_CONFIG_KEYS.get(key)
            if entry is None:
                warnings.warn(scope + "unrecognized config key `%s`, it will be ignored" % key, EggWarning)
                continue
            typ, lo, hi = entry
            if typ == "color":
                value = list(value)
                if len(value) != 4:
                    raise EggError("[ERROR] " + scope + "color `%s` does not have 4 components" % key)
                for i in range(4):
                    component = value[i]
                    if _type_name(component) != "number" or _is_nan(component):
                        raise EggError("[ERROR] " + scope + "color `%s` has a component that is not a number" % key)
                    if component < 0 or component > 1:
                        warnings.warn(scope + "color `%s` has a component that is outside of [0, 1]" % key, EggWarning)
                    value[i] = min(max(component, 0), 1)
            else:
                if _type_name(value) != typ:
                    raise EggError("[ERROR] " + scope + "wrong type for config key `%s`, expected `%s`, got `%s`"
                                   % (key, typ, _type_name(value)))
                if _is_nan(value):
                    warnings.warn(scope + "config key `%s` is NaN, it will be ignored" % key, EggWarning)
                    continue
                if lo is not None and value < lo:
                    warnings.warn(scope + "config key `%s`'s value is `%s`, expected a value larger than `%s`"
                                  % (key, value, lo), EggWarning)
                    value = max(value, lo)
                elif hi is not None and value > hi:
                    warnings.warn(scope + "config key `%s`'s value is `%s`, expected a value smaller than `%s`"
                                  % (key, value, hi), EggWarning)
                    value = min(value, hi)
            target[key] = value

    def _c_config(self, white_or_yolk):
        cfg = self._white_config if white_or_yolk else self._yolk_config
        c = _ffi.EggConfig()
        for k in _SOLVER_KEYS:
            if k not in cfg:
                raise EggError("[ERROR] In SimulationHandler.new: config key `%s` is missing" % k)
            setattr(c, k, float(cfg[k]))
        c.max_collision_fraction = getattr(self, "_max_collision_fraction", 0.05)
        c.mass_distribution_variance = getattr(self, "_mass_distribution_variance", 4)
        c.eps = 1e-8
        return c

    _RENDER_DEFAULTS = dict(outline_thickness=1.0, highlight_strength=0.0, shadow_strength=0.0, texture_scale=12.0,
                            motion_blur=0.0003)

    def _send_render_config(self):
        # this object's config tables are the authority for the render keys (colour tables may be shared with batches,
        # L:49-50); the library gets a copy whenever they may have changed
        for which in range(2):
            self._check(self._c("set_render_config")(which, C.byref(self._c_render_config(which == 0))))

    def _c_render_config(self, white_or_yolk):
        """the render keys of a config table (simulation_handler_default_config.lua:22-36) as egg_render_config"""
        cfg = self._white_config if white_or_yolk else self._yolk_config
        c = _ffi.EggRenderConfig()
        c.color[:] = [float(v) for v in cfg.get("color", [1, 1, 1, 1])]
        c.outline_color[:] = [float(v) for v in cfg.get("outline_color", [1, 1, 1, 1])]
        for k, d in self._RENDER_DEFAULTS.items():
            setattr(c, k, float(cfg.get(k, d)))
        return c

    # the handler's private render switches (L:448-449): particles take their batch's colour at `add` only while
    # _use_particle_color is set (L:978-990)
    @property
    def _use_particle_color(self):
        return self._use_particle_color_flag

    def _apply_render_flags(self):
        self._check(self._c("set_render_flags")(int(self._use_particle_color_flag), int(self._use_lighting_flag)))

    @_use_particle_color.setter
    def _use_particle_color(self, flag):
        self._use_particle_color_flag = bool(flag)
        self._apply_render_flags()

    @property
    def _use_lighting(self):
        return self._use_lighting_flag

    @_use_lighting.setter
    def _use_lighting(self, flag):
        self._use_lighting_flag = bool(flag)
        self._apply_render_flags()

    def _apply_config(self, white_or_yolk):
        """the validated config table of one type to the device (ShardedSimulationHandler has its own)"""
        self._check(self._c("set_config")(_ffi.WHITE if white_or_yolk else _ffi.YOLK, C.byref(self._c_config(white_or_yolk))))
        self._send_render_config()

    def set_white_config(self, config):  # L:226-229
        _assert_types(config, "table")
        self._load_config(copy.deepcopy(config), True)
        self._apply_config(True)

    def set_yolk_config(self, config):  # L:233-236
        _assert_types(config, "table")
        self._load_config(copy.deepcopy(config), False)
        self._apply_config(False)

    def get_white_config(self):  # L:240-242
        return copy.deepcopy(self._white_config)

    def get_yolk_config(self):  # L:246-248
        return copy.deepcopy(self._yolk_config)

    # ------------------------------------------------------------ error mapping
    def _message(self):
        return self._c("last_error")().decode()

    def _check(self, rc):
        if rc == _ffi.EGG_OK:
            return rc
        if rc > 0:  # warning class: the reference prints and carries on
            warnings.warn(self._message(), EggWarning)
            return rc
        raise EggError("[ERROR] " + self._message())

    # --------------------------------------------------------------------- add
    def add(self, x, y, white_radius=None, yolk_radius=None, white_color=None, yolk_color=None,
            white_n_particles=None, yolk_n_particles=None):  # L:27-135
        white_color, yolk_color, given = self._check_add(x, y, white_radius, yolk_radius, white_color, yolk_color,
                                                         white_n_particles, yolk_n_particles)
        out = C.c_int64()
        rc = self._c("add")(float(x), float(y),
                               float("nan") if white_radius is None else float(white_radius),
                               float("nan") if yolk_radius is None else float(yolk_radius),
                               _ffi.DEFAULT_COUNT if white_n_particles is None else int(math.ceil(white_n_particles)),
                               _ffi.DEFAULT_COUNT if yolk_n_particles is None else int(math.ceil(yolk_n_particles)),
                               C.byref(out))
        self._check(rc)
        # L:49-50, L:124-129: a batch created without a colour shares the CONFIG's colour table (set_*_color on it then
        # changes config.color too); the device library is told which tables are the batch's own
        self._batch_colors[out.value] = [white_color, yolk_color]
        for which, color in enumerate((white_color, yolk_color)):
            if given[which]:
                self._c("set_add_color")(out.value, which, *[float(c) for c in color[:4]])
        return out.value

    def _check_add(self, x, y, white_radius, yolk_radius, white_color, yolk_color, white_n_particles, yolk_n_particles):
        """the argument checks of add (L:27-108), in the reference's order; returns the two colour tables (the config's
        where none was given) and which of them were given"""
        _assert_types(x, "number", y, "number")
        given = (white_color is not None, yolk_color is not None)
        white_color = white_color if white_color is not None else self._white_config.get("color", [1, 1, 1, 1])
        yolk_color = yolk_color if yolk_color is not None else self._yolk_config.get("color", [1, 1, 1, 1])
        for v in (white_radius, yolk_radius, white_n_particles, yolk_n_particles):
            if v is not None:
                _assert_types(v, "number")
        _assert_types(white_color, "table", yolk_color, "table")
        # L:71-85 come before the colour checks in the reference; nothing may be created when they fail, so they
        # are made here before the C call (the library repeats them: only EGG_DEFAULT_COUNT means "not given")
        if white_radius is not None and white_radius <= 0:
            raise EggError("[ERROR] In SimulationHandler.add: white radius cannot be 0 or negative")
        if yolk_radius is not None and yolk_radius <= 0:
            raise EggError("[ERROR] In SimulationHandler.add: yolk radius cannot be 0 or negative")
        if white_n_particles is not None and white_n_particles <= 1:
            raise EggError("[ERROR] In SimulationHandler.add: white particle count cannot be 1 or negative")
        if yolk_n_particles is not None and yolk_n_particles <= 1:
            raise EggError("[ERROR] In SimulationHandler.add: yolk particle count cannot be 1 or negative")
        for name, color in (("white", white_color), ("yolk", yolk_color)):  # L:87-108
            for i, cname in enumerate("rgba"):
                if i >= len(color) or _type_name(color[i]) != "number" or _is_nan(color[i]):
                    raise EggError("[ERROR] In SimulationHandler.add: %s color component `%s` is not a number"
                                   % (name, cname))
                if color[i] < 0 or color[i] > 1:
                    warnings.warn("In SimulationHandler.add: %s color component `%s` is outside of [0, 1]"
                                  % (name, cname), EggWarning)
        return white_color, yolk_color, given

    def remove(self, batch_id):  # L:140-155
        _assert_types(batch_id, "number")
        rc = self._check(self._c("remove")(int(batch_id)))
        if rc == _ffi.EGG_OK:
            self._batch_colors.pop(int(batch_id), None)

    def draw(self, screen_size=(800, 600), origin=(0.0, 0.0), interpolation_alpha=None, clear=(0.0, 0.0, 0.0, 0.0),
             canvas_sizes=None, use_instancing=True):  # L:159-162
        """`draw()` without a window: _update_canvases + _draw_canvases (L:1995-2175) as HIP kernels into a float32
        RGBA image of screen_size = (width, height); world px = screen px + origin.  Returns an (H, W, 4) array.
        canvas_sizes = [(w, h) white, (w, h) yolk] overrides the sizes resize_canvas_maybe would pick (L:1935-1975)."""
        p = self._render_params(screen_size, origin, interpolation_alpha, clear, canvas_sizes, use_instancing)
        # (the render config is NOT re-sent here: egg_set_render_config means "set_*_config was called" -- a new colour
        # table, L:1307-1311 -- and would end the sharing of the old one between the config and its colourless batches)
        image = np.empty((p.screen_h, p.screen_w, 4), dtype=np.float32)
        self._check(self._c("render")(C.byref(p), image.ctypes.data_as(C.c_void_p)))
        return image

    def _render_params(self, screen_size, origin, interpolation_alpha, clear, canvas_sizes, use_instancing):
        """draw()'s arguments as egg_render_params"""
        p = _ffi.EggRenderParams()
        self._check(self._lib.egg_default_render_params(C.byref(p)))
        p.screen_w, p.screen_h = int(screen_size[0]), int(screen_size[1])
        p.origin_x, p.origin_y = float(origin[0]), float(origin[1])
        if interpolation_alpha is not None:
            p.interpolation_alpha = float(interpolation_alpha)
        p.threshold = float(self._thresholding_threshold)
        p.smoothness = float(self._thresholding_smoothness)
        p.use_instancing = int(bool(use_instancing))
        if canvas_sizes is not None:
            for which in range(2):
                p.canvas_w[which], p.canvas_h[which] = int(canvas_sizes[which][0]), int(canvas_sizes[which][1])
        p.clear[:] = [float(c) for c in clear]
        return p

    def render_canvas(self, which):
        """the density canvas of `which` as the last draw() left it: ((h, w, 4) float32 array, (x0, y0) in world px)"""
        w, h, x0, y0 = C.c_int32(), C.c_int32(), C.c_double(), C.c_double()
        self._check(self._c("render_canvas")(int(which), None, 0, C.byref(w), C.byref(h), C.byref(x0), C.byref(y0)))
        canvas = np.empty((h.value, w.value, 4), dtype=np.float32)
        self._check(self._c("render_canvas")(int(which), canvas.ctypes.data_as(C.c_void_p), w.value * h.value,
                                                None, None, None, None))
        return canvas, (x0.value, y0.value)

    # ------------------------------------------------------------------ update
    def update(self, delta, step_delta=None, n_substeps=None, n_collision_steps=None):  # L:168-222
        step_delta, n_substeps, n_collision_steps = self._check_update(delta, step_delta, n_substeps, n_collision_steps)
        n = C.c_int32()
        self._check(self._c("update")(float(delta), float(step_delta), int(n_substeps),
                                         int(n_collision_steps), C.byref(n)))
        return n.value

    @staticmethod
    def _check_update(delta, step_delta, n_substeps, n_collision_steps):
        """defaults, type checks and rounding of update's arguments (L:168-182)"""
        if step_delta is None:
            step_delta = 1 / 60
        if n_substeps is None:
            n_substeps = 2
        if n_collision_steps is None:
            n_collision_steps = 3
        _assert_types(delta, "number", step_delta, "number", n_substeps, "number", n_collision_steps, "number")
        if _is_nan(n_substeps) or _is_nan(n_collision_steps):
            raise EggError("[ERROR] In SimulationHandler.update: `n_substeps` is not a number > 0")
        n_substeps = math.ceil(n_substeps)  # L:181-182
        n_collision_steps = math.ceil(n_collision_steps)
        return step_delta, n_substeps, n_collision_steps

    def step(self, delta=1 / 60, n_substeps=2, n_collision_steps=3):
        """`_step` directly (L:1722); not part of the reference's public surface."""
        self._check(self._c("step")(float(delta), int(n_substeps), int(n_collision_steps)))

    # ---------------------------------------------------------------- targets
    def set_target_position(self, batch_id, x, y):  # L:254-264
        _assert_types(batch_id, "number", x, "number", y, "number")
        self._check(self._c("set_target")(int(batch_id), float(x), float(y)))

    def get_target_position(self, batch_id):  # L:268-278
        _assert_types(batch_id, "number")
        x, y = C.c_double(), C.c_double()
        self._check(self._c("get_target")(int(batch_id), C.byref(x), C.byref(y)))
        return x.value, y.value

    def get_position(self, batch_id):  # L:281-295
        _assert_types(batch_id, "number")
        x, y = C.c_double(), C.c_double()
        self._check(self._c("get_position")(int(batch_id), C.byref(x), C.byref(y)))
        return x.value, y.value

    # ----------------------------------------------------------------- colors
    # render attributes: kept on the host, never read by the solver (L:297-395)
    def _set_color(self, scope, which, batch_id, r, g, b, a):
        if a is None:
            a = 1
        _assert_types(batch_id, "number")
        _assert_types(r, "number", g, "number", b, "number", a, "number")
        if any(c > 1 or c < 0 for c in (r, g, b, a)):
            warnings.warn("In SimulationHandler.%s: color component is outside of [0, 1]" % scope, EggWarning)
        rgba = [min(max(c, 0), 1) for c in (r, g, b, a)]
        if int(batch_id) not in self._batch_colors:
            warnings.warn("In SimulationHandler.%s: no batch with id `%s`" % (scope, batch_id), EggWarning)
            return
        # in place (L:349-350, L:386-387): a batch created without a colour shares the config's table
        table = self._batch_colors[int(batch_id)][which]
        if isinstance(table, list):
            table[:] = rgba
        else:
            self._batch_colors[int(batch_id)][which] = rgba
        self._apply_color(int(batch_id), int(which), rgba)

    def _apply_color(self, batch_id, which, rgba):
        # its particles (L:1110-1129) and, when the batch shares the config's table, the config's colour: the library
        # applies the same aliasing as the tables above
        self._c("set_color")(batch_id, which, *[float(c) for c in rgba])

    def set_white_color(self, batch_id, r, g, b, a=None, *outline):  # L:365-394
        self._set_color("set_white_color", 0, batch_id, r, g, b, a)

    def set_yolk_color(self, batch_id, r, g, b, a=None, *outline):  # L:328-357
        self._set_color("set_egg_yolk_color", 1, batch_id, r, g, b, a)

    # ------------------------------------------------------------ bookkeeping
    def list_ids(self):  # L:399-405
        n = C.c_int64()
        self._check(self._c("list_ids")(0, None, C.byref(n)))
        ids = np.empty(n.value, dtype=np.int64)
        self._check(self._c("list_ids")(n.value, ids.ctypes.data, C.byref(n)))
        return [int(i) for i in ids]

    def get_n_particles(self, batch_or_nil=None):  # L:409-419
        w, y = C.c_int64(), C.c_int64()
        self._check(self._c("get_n_particles")(-1 if batch_or_nil is None else int(batch_or_nil),
                                                  C.byref(w), C.byref(y)))
        return w.value, y.value

    @property
    def elapsed(self):
        e, a = C.c_double(), C.c_double()
        self._c("get_elapsed")(C.byref(e), C.byref(a))
        return e.value

    @property
    def interpolation_alpha(self):
        e, a = C.c_double(), C.c_double()
        self._c("get_elapsed")(C.byref(e), C.byref(a))
        return a.value

    def download(self, which, field):
        """One particle field (name from _ffi.FIELDS) of every particle, particle-index order."""
        w, y = self.get_n_particles()
        n = w if which == _ffi.WHITE else y
        out = np.empty(n, dtype=np.float64)
        self._check(self._c("download_particles")(which, _ffi.FIELD_ID[field], out.ctypes.data, n))
        return out

    def download_instance_data(self, which):
        """The reference's instanced-draw record per particle (L:513-517, L:744-813):
        columns x, y, last_x, last_y, vx, vy, radius."""
        cols = [self.download(which, f) for f in ("x", "y", "last_x", "last_y", "vx", "vy", "radius")]
        return np.stack(cols, axis=1) if cols[0].size else np.zeros((0, 7))

    def instances(self, which, color=True):
        """The reference's two per-particle meshes of type `which`, packed on the device (egg_get_instances, L:513-523):
        (data, color, color_version) -- data (n, 7) float32 with the columns of download_instance_data, each value its
        double rounded to nearest even; color (n, 4) float32 rgba, the colour the splat of draw() reads for the particle
        (None with color=False); color_version an int that goes up whenever a call that can change a colour or the
        particle count succeeds and stands still over update(): skip the colour upload while it stands."""
        w, y = self.get_n_particles()
        n = w if which == _ffi.WHITE else y
        data = np.empty((n, 7), dtype=np.float32)
        col = np.empty((n, 4), dtype=np.float32) if color else None
        got, version = C.c_int64(), C.c_uint64()
        self._check(self._c("get_instances")(int(which), data.ctypes.data_as(C.c_void_p),
                                              col.ctypes.data_as(C.c_void_p) if color else None, n, C.byref(got), C.byref(version)))
        return data, col, int(version.value)

    def get_environment(self, which):
        """the reductions the reference keeps per particle type for :draw() -- AABB incl. radius, centroid, largest
        radius and speed, centroid at the start of the last step (simulation_handler.lua:1669-1718, 1795-1815)"""
        e = _ffi.EggEnvironment()
        self._check(self._c("get_environment")(int(which), C.byref(e)))
        return {k: getattr(e, k) for k in _ffi.ENVIRONMENT_FIELDS}


class SimulationHandler(_HandlerSurface):
    """`SimulationHandler(white_config, yolk_config)` (L:11-15, L:425-459)."""

    def __init__(self, white_config=None, yolk_config=None, device=0):
        self._lib = _ffi.load()
        self._h = None
        self._init_host_state(white_config, yolk_config)
        h = C.c_void_p()
        rc = self._lib.egg_create(C.byref(self._c_config(True)), C.byref(self._c_config(False)), int(device),
                                  C.byref(h))
        if rc != _ffi.EGG_OK:
            raise EggError("[ERROR] In SimulationHandler.new: " + self._lib.egg_last_error(None).decode())
        self._h = h
        self._send_render_config()

    def __del__(self):
        self.close()

    def close(self):
        if getattr(self, "_h", None):
            self._lib.egg_destroy(self._h)
            self._h = None

    def set_collider_bodies(self, bodies):
        """One body per collider of the current list ("Collider bodies"): `None` for a collider that
        stays kinematic, or `(inv_mass, inv_inertia[, ax, ay[, drag, spin_drag]])`.  inv_mass > 0 frees the translation,
        inv_inertia > 0 the rotation about the collider's spin pivot: a plate is `(1 / M, 0)`, a hinge `(0, 1 / I)`, a free
        ball both.  ax, ay (px/s^2) act on a freed translation; drag and spin_drag are in 1/s.  In a relaxed step with
        collider loads on, the device integrates every body from the loads it receives, once per sub-step, and a committed
        step advances what get_colliders, get_collider_motion and get_collider_spin return.  A step with a body and loads
        off raises EggError (set_collider_loads(True) first).  `[]` resets, and so does set_colliders; geometry, surfaces,
        motions and spins stay.  Raises EggError (nothing changes) for a length that is not the collider count, a component
        that is not finite or a negative inv_mass, inv_inertia, drag or spin_drag."""
        n, arr = self._c_bodies(bodies)  # (refused here before any device call)
        self._check(self._c("set_collider_bodies")(n, arr))

    def get_collider_bodies(self):
        """the bodies as stored, one `(inv_mass, inv_inertia, ax, ay, drag, spin_drag)` per collider (zeros included)"""
        return self._get_records(self._c("get_collider_bodies"), _BODY.struct, _BODY.fields)

    def set_collider_contacts(self, contacts, iterations=4):
        """One contact record per collider of the current list ("Collider contacts"): `None` for a
        collider that meets no other, a restitution in [0, 1], or `True` (restitution 0).  Where collider bodies act and some
        record is on, every sub-step ends with `iterations` (1 .. 16; 0 = the default, 4) rounds in which every pair of
        contact-enabled colliders of which one is a disc -- against a half-plane, disc, container, segment or wall -- and one
        a body takes the impulse that keeps the next sub-step's pose from overlapping; a pair bounces with the larger of its
        two restitutions.  A free ball lands on a plate, two balls collide, a ball tips a hinged wall.  No friction between
        bodies.  `[]` resets, and so does set_colliders; the bodies stay.  Raises EggError (nothing changes) for a length
        that is not the collider count, a restitution outside [0, 1], iterations outside 0 .. 16, or a contact in exact
        order."""
        n, arr, iterations = self._c_contacts(contacts, iterations)  # (refused here before any device call)
        self._check(self._c("set_collider_contacts")(n, arr, iterations))

    def get_collider_contacts(self):
        """`(contacts, iterations)`: the contacts as stored, one per collider -- `None` where off, else the restitution"""
        arr = (_ffi.EggColliderContact * _ffi.MAX_COLLIDERS)()
        n, iterations = C.c_int32(), C.c_int32()
        self._check(self._c("get_collider_contacts")(_ffi.MAX_COLLIDERS, arr, C.byref(n), C.byref(iterations)))
        return [c.restitution if c.on else None for c in arr[:n.value]], iterations.value

    def collider_contact_solves(self):
        """the fires of collider contacts, one per (pair, sub-step, iteration), over committed steps"""
        return self._get_count(self._c("get_collider_contact_solves"))

    def set_coupling(self, factor=0.0, strength=1.0):
        """White-yolk coupling: one cross-type collision pass per sub-step of a relaxed step, before the sub-step's first
        collision pass ("Coupling"; relaxed order only).  A white and a yolk particle closer than
        factor * (ra + rb) are pushed apart to that distance with the collision correction's arithmetic and the
        compliance of `strength` in [0, 1]; factor 0 = off.  All pairs of both types couple, whatever their batch, and
        nothing pulls a yolk back to its white.  Raises EggError for a NaN, negative or infinite factor or a strength
        outside [0, 1] (nothing changes) and for factor > 0 on a handle in exact order; set_solver_order("exact") raises
        while factor > 0."""
        factor, strength = self._c_coupling(factor, strength)  # (refused here before any device call)
        self._check(self._c("set_coupling")(factor, strength))

    def coupling(self):
        """(factor, strength) as stored"""
        return self._get_pair(self._c("get_coupling"))

    def coupling_solves(self):
        """distinct white-yolk pairs that fired over the coupling passes of committed steps, since creation"""
        return self._get_count(self._c("get_coupling_solves"))

    def set_adhesion(self, reach=0.0, strength=1.0):
        """White-yolk adhesion: a same-batch band in the coupling pass ("Adhesion"; relaxed order
        only).  It acts while coupling acts and reach > the coupling factor: a white and a yolk particle of one batch
        farther apart than factor * (ra + rb) but within reach * (ra + rb) are pulled back to the coupling distance,
        never closer, with the coupling correction's arithmetic and the compliance of `strength` in [0, 1]; reach 0 = off.
        reach > 0 while coupling is off is accepted and does nothing.  Raises EggError for a NaN, negative or infinite
        reach or a strength outside [0, 1] (nothing changes) and for reach > 0 on a handle in exact order;
        set_solver_order("exact") raises while reach > 0."""
        reach, strength = self._c_adhesion(reach, strength)  # (refused here before any device call)
        self._check(self._c("set_adhesion")(reach, strength))

    def adhesion(self):
        """(reach, strength) as stored"""
        return self._get_pair(self._c("get_adhesion"))

    def adhesion_solves(self):
        """distinct white-yolk pairs whose adhesion branch fired over the coupling passes of committed steps"""
        return self._get_count(self._c("get_adhesion_solves"))

    def add_many(self, xs, ys, white_radius=None, yolk_radius=None, white_n_particles=None,
                 yolk_n_particles=None):
        """Bulk form of `add` for 10^4..10^5 batches (one C call); returns the ids."""
        xs = np.ascontiguousarray(xs, dtype=np.float64)
        ys = np.ascontiguousarray(ys, dtype=np.float64)
        if xs.shape != ys.shape or xs.ndim != 1:
            raise EggError("[ERROR] In SimulationHandler.add_many: xs and ys must be 1-d arrays of equal length")
        ids = np.empty(xs.shape[0], dtype=np.int64)
        self._check(self._lib.egg_add_many(
            self._h, xs.shape[0], xs.ctypes.data, ys.ctypes.data,
            float("nan") if white_radius is None else float(white_radius),
            float("nan") if yolk_radius is None else float(yolk_radius),
            _ffi.DEFAULT_COUNT if white_n_particles is None else int(white_n_particles),
            _ffi.DEFAULT_COUNT if yolk_n_particles is None else int(yolk_n_particles), ids.ctypes.data))
        return ids

    def add_many_keyed(self, xs, ys, keys, white_radius=None, yolk_radius=None, white_n_particles=None,
                       yolk_n_particles=None):
        """`add_many` with explicit global-order keys (multi-GPU sharding, see include/eggsim.h)"""
        xs = np.ascontiguousarray(xs, dtype=np.float64)
        ys = np.ascontiguousarray(ys, dtype=np.float64)
        keys = np.ascontiguousarray(keys, dtype=np.int64)
        ids = np.empty(xs.shape[0], dtype=np.int64)
        self._check(self._lib.egg_add_many_keyed(
            self._h, xs.shape[0], xs.ctypes.data, ys.ctypes.data,
            float("nan") if white_radius is None else float(white_radius),
            float("nan") if yolk_radius is None else float(yolk_radius),
            _ffi.DEFAULT_COUNT if white_n_particles is None else int(white_n_particles),
            _ffi.DEFAULT_COUNT if yolk_n_particles is None else int(yolk_n_particles),
            keys.ctypes.data, ids.ctypes.data))
        return ids

    def set_solver_config(self, which, c_config):
        """egg_set_config with an _ffi.EggConfig somebody else validated (ShardedSimulationHandler owns the tables)"""
        self._check(self._lib.egg_set_config(self._h, int(which), C.byref(c_config)))

    def export_batch(self, batch_id):
        """(info dict, white_state[9, n_w], yolk_state[9, n_y]) of a batch: everything another handler
        needs to continue it bit for bit"""
        nw, ny = self.get_n_particles(batch_id)
        info = _ffi.EggBatchInfo()
        ws, ys = np.empty((9, nw)), np.empty((9, ny))
        self._check(self._lib.egg_export_batch(self._h, int(batch_id), C.byref(info), ws.ctypes.data, ys.ctypes.data))
        return {k: getattr(info, k) for k, _ in _ffi.EggBatchInfo._fields_}, ws, ys

    def export_batch_to(self, batch_id, white_ptr, yolk_ptr):
        """export_batch into caller-owned buffers given by ADDRESS (host memory or memory of this handle's device, e.g.
        torch.Tensor.data_ptr() of a CUDA tensor: a device-to-device hand-over, nothing touches the host); returns info"""
        info = _ffi.EggBatchInfo()
        self._check(self._lib.egg_export_batch(self._h, int(batch_id), C.byref(info), C.c_void_p(int(white_ptr)), C.c_void_p(int(yolk_ptr))))
        return {k: getattr(info, k) for k, _ in _ffi.EggBatchInfo._fields_}

    def import_batch_from(self, info, white_ptr, yolk_ptr):
        """import_batch from buffers given by address (host or this handle's device memory, field-major [9, n])"""
        c = _ffi.EggBatchInfo(**{k: info[k] for k, _ in _ffi.EggBatchInfo._fields_})
        out = C.c_int64()
        self._check(self._lib.egg_import_batch(self._h, C.byref(c), C.c_void_p(int(white_ptr)), C.c_void_p(int(yolk_ptr)), C.byref(out)))
        return out.value

    def import_batch(self, info, white_state, yolk_state):
        c = _ffi.EggBatchInfo(**{k: info[k] for k, _ in _ffi.EggBatchInfo._fields_})
        ws = np.ascontiguousarray(white_state, dtype=np.float64)
        ys = np.ascontiguousarray(yolk_state, dtype=np.float64)
        out = C.c_int64()
        self._check(self._lib.egg_import_batch(self._h, C.byref(c), ws.ctypes.data, ys.ctypes.data, C.byref(out)))
        return out.value

    def particle_texture(self):
        """alpha of the particle density texture (L:620-682) the splat pass samples"""
        n = C.c_int32()
        self._check(self._lib.egg_render_particle_texture(self._h, None, 0, C.byref(n)))
        tex = np.empty((n.value, n.value), dtype=np.float32)
        self._check(self._lib.egg_render_particle_texture(self._h, tex.ctypes.data_as(C.c_void_p), tex.size, None))
        return tex

    def step_begin(self, delta=1 / 60, n_substeps=2, n_collision_steps=3):
        """launch a `_step` without waiting for it (see egg_step_begin)"""
        self._check(self._lib.egg_step_begin(self._h, float(delta), int(n_substeps), int(n_collision_steps)))

    def step_end(self, commit=True):
        self._check(self._lib.egg_step_end(self._h, 1 if commit else 0))

    def step_peek_visits(self):
        """(max visits in one pass per type, budget per type) of the step launched with step_begin, before it is
        committed (see egg_step_peek_visits)"""
        v, b = (C.c_int64 * 2)(), (C.c_double * 2)()
        self._check(self._lib.egg_step_peek_visits(self._h, C.byref(v), C.byref(b)))
        return list(v), list(b)

    def prepare_step(self, step_delta=1 / 60, n_substeps=2, n_collision_steps=3):
        """form the tiles/claims of the next step without running it (multi-GPU exchange)"""
        self._check(self._lib.egg_prepare_step(self._h, float(step_delta), int(n_substeps), int(n_collision_steps)))

    def set_target_positions(self, ids, xs, ys):
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        xs = np.ascontiguousarray(xs, dtype=np.float64)
        ys = np.ascontiguousarray(ys, dtype=np.float64)
        self._check(self._lib.egg_set_targets_many(self._h, ids.shape[0], ids.ctypes.data, xs.ctypes.data,
                                                   ys.ctypes.data))

    def get_positions(self, ids):
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        xs = np.empty(ids.shape[0], dtype=np.float64)
        ys = np.empty(ids.shape[0], dtype=np.float64)
        self._check(self._lib.egg_get_positions_many(self._h, ids.shape[0], ids.ctypes.data, xs.ctypes.data,
                                                     ys.ctypes.data))
        return xs, ys

    def get_bounds(self, ids):
        """[n, 4] array (lo_x, lo_y, hi_x, hi_y) in px: the cells each batch's particles occupy."""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        out = np.empty((4, ids.shape[0]), dtype=np.float64)
        self._check(self._lib.egg_get_bounds_many(self._h, ids.shape[0], ids.ctypes.data, out[0].ctypes.data,
                                                  out[1].ctypes.data, out[2].ctypes.data, out[3].ctypes.data))
        return out.T.copy()

    def get_claims(self, ids):
        """([n, 8] array: white box then yolk box, lo_x lo_y hi_x hi_y in px; (white cell, yolk cell))"""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        out = np.empty((ids.shape[0], 8), dtype=np.float64)
        cells = np.empty(2, dtype=np.float64)
        self._check(self._lib.egg_get_claims_many(self._h, ids.shape[0], ids.ctypes.data, out.ctypes.data, cells.ctypes.data))
        return out, (float(cells[0]), float(cells[1]))

    # ------------------------------------------- draw of a scene sharded over processes (egg_draw_*, include/eggsim.h)
    # A message is double[7][n] (_ffi.DRAW_FIELDS), given by ADDRESS: host memory or memory of this handle's device.
    def draw_pack(self, which, pointer, cap_particles):
        """this handle's particles of `which` as one message at `pointer` (complete when this returns)"""
        self._check(self._lib.egg_draw_pack(self._h, int(which), C.c_void_p(int(pointer)), int(cap_particles)))

    def draw_source_layout(self, which, total, atom_offset, atom_color):
        """the layout of `which` over all ranks: atom_offset [atoms] int64 ascending from 0, atom_color [atoms, 4]"""
        off = np.ascontiguousarray(atom_offset, dtype=np.int64)
        col = np.ascontiguousarray(atom_color, dtype=np.float32).reshape(-1, 4)
        self._check(self._lib.egg_draw_source_layout(self._h, int(which), int(total), off.shape[0], off.ctypes.data, col.ctypes.data))

    def draw_source_place(self, which, pointer, n, run_src, run_dst):
        """one message (pointer 0: this handle's own particles) into its places; the message must be complete"""
        rs = np.ascontiguousarray(run_src, dtype=np.int64)
        rd = np.ascontiguousarray(run_dst, dtype=np.int64)
        self._check(self._lib.egg_draw_source_place(self._h, int(which), C.c_void_p(int(pointer)) if pointer else None, int(n),
                                                    rs.shape[0], rs.ctypes.data, rd.ctypes.data))

    def draw_source_render(self, params, render_configs, use_particle_color, use_lighting, stepped, interpolation_alpha):
        """egg_render over the placed particles; render_configs = (white, yolk) _ffi.EggRenderConfig"""
        cfg = (_ffi.EggRenderConfig * 2)(*render_configs)
        image = np.empty((params.screen_h, params.screen_w, 4), dtype=np.float32)
        self._check(self._lib.egg_draw_source_render(self._h, C.byref(params), cfg, int(bool(use_particle_color)), int(bool(use_lighting)),
                                                     int(bool(stepped)), float(interpolation_alpha), image.ctypes.data_as(C.c_void_p)))
        return image

    def draw_source_render_canvas(self, which):
        w, h, x0, y0 = C.c_int32(), C.c_int32(), C.c_double(), C.c_double()
        self._check(self._lib.egg_draw_source_render_canvas(self._h, int(which), None, 0, C.byref(w), C.byref(h), C.byref(x0), C.byref(y0)))
        canvas = np.empty((h.value, w.value, 4), dtype=np.float32)
        self._check(self._lib.egg_draw_source_render_canvas(self._h, int(which), canvas.ctypes.data_as(C.c_void_p), w.value * h.value,
                                                            None, None, None, None))
        return canvas, (x0.value, y0.value)

    def draw_source_environment(self, which, stepped):
        e = _ffi.EggEnvironment()
        self._check(self._lib.egg_draw_source_environment(self._h, int(which), int(bool(stepped)), C.byref(e)))
        return {k: getattr(e, k) for k in _ffi.ENVIRONMENT_FIELDS}

    def draw_source_download(self, which, field, n):
        out = np.empty(int(n), dtype=np.float64)
        self._check(self._lib.egg_draw_source_download(self._h, int(which), _ffi.FIELD_ID[field], out.ctypes.data, int(n)))
        return out

    def draw_source_instances(self, which, n, color=True):
        """the two meshes of instances() over the placed particles: ((n, 7) float32, (n, 4) float32 or None)"""
        data = np.empty((int(n), 7), dtype=np.float32)
        col = np.empty((int(n), 4), dtype=np.float32) if color else None
        got = C.c_int64()
        self._check(self._lib.egg_draw_source_instances(self._h, int(which), data.ctypes.data_as(C.c_void_p),
                                                        col.ctypes.data_as(C.c_void_p) if color else None, int(n), C.byref(got)))
        return data, col

    # ------------------------------------------- the instanced-draw record in two halves (egg_instances_begin / _end)
    def instances_to(self, which, data_ptr, color_ptr, cap):
        """instances() into caller-owned buffers given by ADDRESS (host memory or memory of this handle's device, e.g.
        torch.Tensor.data_ptr(); 0 skips a mesh); returns (n, color_version).  Complete when this returns."""
        got, version = C.c_int64(), C.c_uint64()
        self._check(self._lib.egg_get_instances(self._h, int(which), C.c_void_p(int(data_ptr)) if data_ptr else None,
                                                C.c_void_p(int(color_ptr)) if color_ptr else None, int(cap), C.byref(got),
                                                C.byref(version)))
        return got.value, int(version.value)

    # ------------------------------------------- fields into planes on the device (egg_field_to)
    def field_to(self, origin, cell, shape, count, svx=None, svy=None, types="both", path="auto"):
        """field() into caller-owned planes on this handle's device: `count` an int32 and `svx`, `svy` (both or neither) int64
        planes of shape (2, ny, nx), contiguous, given as objects with `data_ptr()` (a torch tensor) or as addresses.  The
        call zeroes them itself and they are complete when it returns; nothing is copied to the host.  Returns
        `FieldTotals(inside, outside, dropped, units_tiled, units_direct)`.  (A process that uses torch tensors imports torch
        before this package loads its library: torch brings its own HIP runtime.)"""
        spec = self._c_field_spec(origin, cell, shape, types, path)
        if count is None:
            raise EggError("field_to: count is required")
        if (svx is None) != (svy is None):
            raise EggError("field_to: svx and svy are given together or not at all")
        words = 2 * spec.nx * spec.ny

        def address(plane, what, word, dtype):
            if plane is None:
                return None
            if hasattr(plane, "data_ptr"):
                if str(getattr(plane, "dtype", dtype)).split(".")[-1] != dtype:
                    raise EggError("field_to: %s must hold %s, not %s" % (what, dtype, plane.dtype))
                if hasattr(plane, "numel") and plane.numel() != words:
                    raise EggError("field_to: %s must hold 2 x %d x %d elements, not %d" % (what, spec.ny, spec.nx, plane.numel()))
                if hasattr(plane, "is_contiguous") and not plane.is_contiguous():
                    raise EggError("field_to: %s must be contiguous" % what)
                plane = plane.data_ptr()
            if isinstance(plane, bool) or not isinstance(plane, (int, np.integer)) or int(plane) <= 0:
                raise EggError("field_to: %s must be an object with data_ptr() or an address, not %r" % (what, plane))
            if int(plane) % word:
                raise EggError("field_to: %s is not aligned to %d bytes" % (what, word))
            return int(plane)
        planes = _ffi.EggFieldPlanes(address(count, "count", 4, "int32"), address(svx, "svx", 8, "int64"), address(svy, "svy", 8, "int64"))
        t = _ffi.EggFieldTotals()
        self._check(self._lib.egg_field_to(self._h, C.byref(spec), C.byref(planes), C.byref(t)))
        return FieldTotals(tuple(t.inside), tuple(t.outside), tuple(t.dropped), t.units_tiled, t.units_direct)

    # ------------------------------------------- cover into planes on the device (egg_cover_to)
    def cover_to(self, origin, cell, shape, cover, owner=None, scale=1.0, types="both", path="auto"):
        """cover() into caller-owned planes on this handle's device: `cover` and, if wanted, `owner` int32 planes of shape
        (2, ny, nx), contiguous, given as objects with `data_ptr()` (a torch tensor) or as addresses.  The call zeroes and
        presets them itself and they are complete when it returns; nothing but the totals is copied to the host.  Returns
        `CoverTotals`.  (A process that uses torch tensors imports torch before this package loads its library.)"""
        spec = self._c_cover_spec(origin, cell, shape, scale, types, path, "cover_to")
        if cover is None:
            raise EggError("cover_to: cover is required")
        words = 2 * spec.nx * spec.ny

        def address(plane, what):
            if plane is None:
                return None
            if hasattr(plane, "data_ptr"):
                if str(getattr(plane, "dtype", "int32")).split(".")[-1] != "int32":
                    raise EggError("cover_to: %s must hold int32, not %s" % (what, plane.dtype))
                if hasattr(plane, "numel") and plane.numel() != words:
                    raise EggError("cover_to: %s must hold 2 x %d x %d elements, not %d" % (what, spec.ny, spec.nx, plane.numel()))
                if hasattr(plane, "is_contiguous") and not plane.is_contiguous():
                    raise EggError("cover_to: %s must be contiguous" % what)
                plane = plane.data_ptr()
            if isinstance(plane, bool) or not isinstance(plane, (int, np.integer)) or int(plane) <= 0:
                raise EggError("cover_to: %s must be an object with data_ptr() or an address, not %r" % (what, plane))
            return int(plane)
        planes = _ffi.EggCoverPlanes(address(cover, "cover"), address(owner, "owner"))
        t = _ffi.EggCoverTotals()
        self._check(self._lib.egg_cover_to(self._h, C.byref(spec), C.byref(planes), C.byref(t)))
        return CoverTotals(*self._cover_totals(spec, t))

    # ------------------------------------------- measures into a table on the device (egg_measure_to)
    def measure_to(self, out, ids=None, region=None, types="both"):
        """measure_table() into caller-owned memory on this handle's device: `out` an int64 tensor of at least n x 2 x 24
        elements, contiguous, given as an object with `data_ptr()` (a torch tensor) or as a `(address, capacity_bytes)` pair.
        The first n x 2 x 24 words are complete when the call returns; nothing is copied to the host.  Returns n, the number
        of batches measured.  (A process that uses torch tensors imports torch before this package loads its library.)"""
        spec = self._c_measure_spec(region, types, "measure_to")
        ids = self._piece_ids(ids, "measure_to")
        if hasattr(out, "data_ptr"):
            if str(getattr(out, "dtype", "int64")).split(".")[-1] != "int64":
                raise EggError("measure_to: out must hold int64, not %s" % out.dtype)
            if hasattr(out, "is_contiguous") and not out.is_contiguous():
                raise EggError("measure_to: out must be contiguous")
            address, capacity = out.data_ptr(), 8 * int(out.numel())
        else:
            try:
                address, capacity = out
            except (TypeError, ValueError):
                raise EggError("measure_to: out must be an object with data_ptr() or (address, capacity_bytes), not %r" % (out,)) from None
        for v in (address, capacity):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise EggError("measure_to: out must be an object with data_ptr() or (address, capacity_bytes), not %r" % (out,))
        n = len(self.list_ids()) if ids is None else ids.size
        if ids is not None and n == 0:
            return 0
        self._check(self._lib.egg_measure_to(self._h, C.byref(spec), 0 if ids is None else n, None if ids is None else ids.ctypes.data,
                                             C.c_void_p(int(address)), int(capacity)))
        return n

    # ------------------------------------------- pieces: the label of every particle (egg_pieces with label arrays)
    def piece_labels(self, reach=None, types="both"):
        """`(white, yolk)` int32 arrays in download() order: the label of every particle -- the lowest index in the batch among
        the particles of its piece, under pieces()' rule, every batch asked for -- and -1 throughout for a type that `types`
        leaves out.  One handle only: a group's and sharded ranks' particles live in several arrays."""
        spec = self._c_pieces_spec(reach, types, "piece_labels")
        labels = [np.full(int(n), -1, dtype=np.int32) for n in self.get_n_particles()]
        out = (_ffi.EggPieceSummary * max(2 * len(self.list_ids()), 1))()
        self._check(self._lib.egg_pieces(self._h, C.byref(spec), 0, None, out, labels[0].ctypes.data, labels[1].ctypes.data))
        return labels[0], labels[1]

    def instances_begin(self, types=(0, 1)):
        """Launch the pack of instances() for `types` and the copy into pinned buffers the handle owns; returns at once.
        The host draws, or starts the next update(), meanwhile: later work of the handle runs behind the pack on the
        device.  Every type of `types` is fetched with instances_end before the next instances_begin."""
        mask = 0
        for w in types:
            mask |= 1 << int(w)
        self._check(self._lib.egg_instances_begin(self._h, mask))

    def instances_end(self, which):
        """Wait for instances_begin's copy of `which`: (data, color, color_version) as instances() returns them, but as
        numpy VIEWS of the handle's pinned buffers (read-only, nothing is copied).  Lifetime: two buffers alternate, so
        a view stays valid until the SECOND following instances_begin, and no longer than the handler itself; copy what
        must live longer.  While color_version stands the colour mesh is not packed again and `color` is a view of the
        last one."""
        d, c, n, version = C.c_void_p(), C.c_void_p(), C.c_int64(), C.c_uint64()
        self._check(self._lib.egg_instances_end(self._h, int(which), C.byref(d), C.byref(c), C.byref(n), C.byref(version)))

        def view(ptr, cols):
            if n.value == 0 or not ptr.value:
                return np.zeros((0, cols), dtype=np.float32)
            a = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_float)), shape=(n.value, cols))
            a.flags.writeable = False
            return a
        return view(d, 7), view(c, 4), int(version.value)

    # ---------------------------------------------------------- device access
    def synchronize(self):
        self._check(self._lib.egg_synchronize(self._h))

    def stats(self):
        s = _ffi.EggStats()
        self._check(self._lib.egg_get_stats(self._h, C.byref(s)))
        return dict(steps=s.steps, pair_solves=s.pair_solves, follow_solves=s.follow_solves,
                    kernel_launches=s.kernel_launches, retiles=s.retiles, redo_steps=s.redo_steps,
                    n_tiles=list(s.n_tiles), max_tile_particles=list(s.max_tile_particles),
                    last_step_kernel_ms=s.last_step_kernel_ms, single_tile=list(s.single_tile),
                    kernel_ms=list(s.kernel_ms), kernel_ms_sum=list(s.kernel_ms_sum), timed_steps=s.timed_steps,
                    max_pass_visits=list(s.max_pass_visits), budget=list(s.budget), fused_launch=int(s.fused_launch),
                    packed=list(s.packed), pk_kernel_ms=[list(r) for r in s.pk_kernel_ms],
                    pk_kernel_launches=[list(r) for r in s.pk_kernel_launches], host_ms=list(s.host_ms), max_levels=list(s.max_levels),
                    pk_variants=list(s.pk_variants), relaxed_steps=s.relaxed_steps, cohesion_solves=s.cohesion_solves,
                    cell_hash=list(s.cell_hash))

    def selftest_arith(self, n=1 << 24, seed=1):
        """mismatches of the kernel's hand-expanded f64 division against `/` on n random operand pairs"""
        bad = C.c_int64()
        self._check(self._lib.egg_selftest_arith(self._h, int(n), int(seed), C.byref(bad)))
        return bad.value

    def selftest_arith_operands(self, n, d, x):
        """the kernel's hand-expanded division and square roots on the caller's operand triples, raw: an array [count, 8]
        with the columns of _ffi.ARITH_COLUMNS (see egg_selftest_arith_operands); nothing is judged on the device"""
        n, d, x = (np.ascontiguousarray(v, dtype=np.float64) for v in (n, d, x))
        if not (n.ndim == 1 and n.shape == d.shape == x.shape):
            raise EggError("selftest_arith_operands takes three one-dimensional arrays of one length")
        out = np.empty((n.size, 8), dtype=np.float64)
        self._check(self._lib.egg_selftest_arith_operands(self._h, n.size, n.ctypes.data, d.ctypes.data, x.ctypes.data, out.ctypes.data))
        return out

    def set_option(self, option, value):
        self._check(self._lib.egg_set_option(self._h, int(option), float(value)))

    _SOLVER_ORDERS = {"exact": _ffi.SOLVER_EXACT, "relaxed": _ffi.SOLVER_RELAXED}

    def set_solver_order(self, order, relaxation=None):
        """"exact" (default): the reference's sequential pair order, bit for bit.  "relaxed": every collision pass a
        Jacobi pass with constraint averaging, scaled by `relaxation` in (0, 2] (None keeps the current value) --
        plausible and deterministic, several times faster on large scenes, but not the reference's numbers
        (DESIGN.md section 2.7).  A relaxed handle steps alone, inside a SimulationGroup
        (SimulationGroup.set_solver_order) or pass by pass under a ShardedSimulationHandler (the rx_* methods):
        step_begin / step_end / get_claims raise EggError."""
        if order not in self._SOLVER_ORDERS:
            raise EggError("solver order must be 'exact' or 'relaxed', not %r" % (order,))
        if relaxation is not None:
            self.set_option(_ffi.OPT_RELAXATION, relaxation)
        self.set_option(_ffi.OPT_SOLVER_ORDER, self._SOLVER_ORDERS[order])
        self._solver_order = order

    def get_solver_order(self):
        return getattr(self, "_solver_order", "exact")

    _COHESION_MODES = {"reference": _ffi.COHESION_REFERENCE, "effective": _ffi.COHESION_EFFECTIVE}

    def set_cohesion(self, mode):
        """"reference" (default): `cohesion_strength` and `cohesion_interaction_distance_factor` move no particle, as in
        the reference.  "effective": in a relaxed pass a same-batch pair beyond the collision distance but within
        cohesion_interaction_distance_factor * (ra + rb) is pulled back to the collision distance with the cohesion
        compliance ("Cohesion"); stats()["cohesion_solves"] counts those pairs.  Relaxed order
        only: raises EggError on a handle in exact order, and set_solver_order("exact") raises while cohesion is
        effective."""
        if mode not in self._COHESION_MODES:
            raise EggError("cohesion must be 'reference' or 'effective', not %r" % (mode,))
        self.set_option(_ffi.OPT_COHESION, self._COHESION_MODES[mode])
        self._cohesion = mode

    def get_cohesion(self):
        return getattr(self, "_cohesion", "reference")

    # ------------------------------------------------- relaxed order between processes (egg_rx_*, include/eggsim.h)
    # One relaxed _step driven pass by pass; ShardedSimulationHandler carries boxes and ghost messages between the ranks.
    # Boxes are int32 arrays [..., 5]: lo_x, lo_y, hi_x, hi_y (cells), empty flag.  Messages are given by ADDRESS (host
    # memory or memory of this handle's device, e.g. torch.Tensor.data_ptr()); 0 means none.
    def rx_set_keys(self, which, keys, bases, total):
        """global key bases of the batches with keys `keys` (this handle's at least) and the type's total over all ranks"""
        keys = np.ascontiguousarray(keys, dtype=np.int64)
        bases = np.ascontiguousarray(bases, dtype=np.int64)
        self._check(self._lib.egg_rx_set_keys(self._h, int(which), keys.shape[0], keys.ctypes.data, bases.ctypes.data, int(total)))

    def rx_begin(self, delta=1 / 60, n_substeps=2, n_collision_steps=3):
        self._check(self._lib.egg_rx_begin(self._h, float(delta), int(n_substeps), int(n_collision_steps)))

    def rx_substep(self, sub):
        self._check(self._lib.egg_rx_substep(self._h, int(sub)))

    def rx_get_boxes(self, pass_index):
        """[2, 5] int32: this handle's cell box per type at the start of the pass (waits for the device)"""
        out = np.zeros((2, _ffi.RX_BOX_INTS), dtype=np.int32)
        self._check(self._lib.egg_rx_get_boxes(self._h, int(pass_index), out.ctypes.data))
        return out

    def rx_pack(self, pass_index, boxes):
        """boxes [n_dest, 2, 5] int32 -> counts [n_dest, 2]: records packed for every destination and type"""
        boxes = np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 2, _ffi.RX_BOX_INTS)
        counts = np.zeros((boxes.shape[0], 2), dtype=np.int64)
        self._check(self._lib.egg_rx_pack(self._h, int(pass_index), boxes.shape[0], boxes.ctypes.data, counts.ctypes.data))
        return counts

    def rx_fetch(self, pointers):
        """pointers [n_dest, 2]: where the messages of the last rx_pack go (8 * (1 + 5 * count) bytes each; 0 skips);
        they are complete when this returns"""
        ptrs = np.ascontiguousarray(pointers, dtype=np.uint64).reshape(-1, 2)
        self._check(self._lib.egg_rx_fetch(self._h, ptrs.shape[0], ptrs.ctypes.data))

    def rx_run_pass(self, pass_index, pointers, counts):
        """the pass over the local particles + the ghosts of the received messages (pointers / counts [n_src, 2]).  The
        messages must be complete, and host buffers must live until the next rx_get_boxes / rx_check / rx_end returns."""
        ptrs = np.ascontiguousarray(pointers, dtype=np.uint64).reshape(-1, 2)
        counts = np.ascontiguousarray(counts, dtype=np.int64).reshape(-1, 2)
        self._check(self._lib.egg_rx_run_pass(self._h, int(pass_index), ptrs.shape[0], ptrs.ctypes.data, counts.ctypes.data))

    def rx_check(self):
        """(bad, [pairs white, pairs yolk], ghost records received) of the step in flight, before anything is committed"""
        bad, pairs, rec = C.c_int32(), (C.c_int64 * 2)(), C.c_int64()
        self._check(self._lib.egg_rx_check(self._h, C.byref(bad), C.byref(pairs), C.byref(rec)))
        return bool(bad.value), list(pairs), rec.value

    def rx_end(self, commit=True):
        self._check(self._lib.egg_rx_end(self._h, 1 if commit else 0))
