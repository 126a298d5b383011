"""SimulationGroup -- several GPUs of ONE process behind the SimulationHandler surface (ctypes twin of the egg_group_*
entry points of include/eggsim.h; csrc/eggsim_group.cpp).  One device handle per x-slab, global batch ids, batches
handed between devices when their claims meet across a cut; results equal a single handler's bit for bit, draw()
included: its particles are gathered to the device of handle 0 in one global order and drawn there.
(Between processes -- one per GPU, RCCL -- the same protocol is sharding.ShardedSimulationHandler.)"""
import ctypes as C

from . import _ffi
from .simulation_handler import EggError, SimulationHandler, _HandlerSurface


class _Borrowed(SimulationHandler):
    """a device handle owned by the group: downloads and statistics only, never destroyed from here"""

    def __init__(self, lib, ptr):  # (no egg_create)
        self._lib, self._h = lib, C.c_void_p(ptr)

    def close(self):
        self._h = None


class SimulationGroup(_HandlerSurface):
    """The reference's `SimulationHandler` class over a device group: every public method of the class, with the
    signatures, argument checks, warnings and error texts of SimulationHandler (shared code: _HandlerSurface).  Whatever
    it returns or draws equals, bit for bit, what one SimulationHandler holding the same batches returns or draws."""

    _PREFIX = "egg_group_"

    def _ptr(self):
        return self._g

    def __init__(self, devices, cuts=None, white_config=None, yolk_config=None):
        self._lib = _ffi.load()
        self._g = None
        self._init_host_state(white_config, yolk_config)
        devs = (C.c_int32 * len(devices))(*[int(d) for d in devices])
        cut = None
        if cuts is not None:
            if len(cuts) != len(devices) + 1:
                raise EggError("[ERROR] In SimulationGroup.new: need len(devices) + 1 cuts")
            cut = (C.c_double * len(cuts))(*[float(c) for c in cuts])
        g = C.c_void_p()
        rc = self._lib.egg_group_create(C.byref(self._c_config(True)), C.byref(self._c_config(False)), len(devices), devs, cut, C.byref(g))
        if rc != _ffi.EGG_OK:
            raise EggError("[ERROR] In SimulationGroup.new: " + self._lib.egg_last_error(None).decode())
        self._g = g
        self._n_issued = 0  # ids issued so far (1 .. _n_issued; never reused)
        self.handles = [_Borrowed(self._lib, self._lib.egg_group_handle(self._g, k)) for k in range(len(devices))]
        self._send_render_config()

    def __del__(self):
        self.close()

    def close(self):
        if getattr(self, "_g", None):
            for h in self.handles:
                h.close()
            self._lib.egg_group_destroy(self._g)
            self._g = None

    def add(self, x, y, white_radius=None, yolk_radius=None, white_color=None, yolk_color=None,
            white_n_particles=None, yolk_n_particles=None, white_n=None, yolk_n=None):  # L:27-135
        """SimulationHandler.add; `white_n` / `yolk_n` are older names of the two counts"""
        if white_n_particles is None:
            white_n_particles = white_n
        if yolk_n_particles is None:
            yolk_n_particles = yolk_n
        gid = _HandlerSurface.add(self, x, y, white_radius, yolk_radius, white_color, yolk_color, white_n_particles,
                                  yolk_n_particles)
        self._n_issued = max(self._n_issued, gid)
        return gid

    def owner(self, batch_id):
        k, lid = C.c_int32(), C.c_int64()
        if self._lib.egg_group_owner(self._g, int(batch_id), C.byref(k), C.byref(lid)) != _ffi.EGG_OK:
            raise EggError("[ERROR] In SimulationGroup.owner: no batch with id `%s`" % batch_id)
        return k.value, lid.value

    def counters(self):
        m, d = C.c_int64(), C.c_int64()
        self._check(self._lib.egg_group_get_counters(self._g, C.byref(m), C.byref(d)))
        return dict(migrations=m.value, discarded_steps=d.value)

    _SOLVER_ORDERS = SimulationHandler._SOLVER_ORDERS

    def set_solver_order(self, order, relaxation=None):
        """SimulationHandler.set_solver_order for every device handle.  In relaxed order a step runs every collision
        pass on all devices at once, each over its own particles plus ghost copies of its neighbours' particles near
        it: no batch is handed over before a step, and the results equal one relaxed handle's bit for bit (DESIGN.md
        section 2.7).  `relaxation` None keeps the current value."""
        if order not in self._SOLVER_ORDERS:
            raise EggError("solver order must be 'exact' or 'relaxed', not %r" % (order,))
        if relaxation is None:
            omega = -1.0
        else:
            omega = float(relaxation)
            if not (0.0 < omega <= 2.0):  # (the C entry point reads <= 0 as "keep": refuse it here, as a handle does)
                raise EggError("relaxation must be in (0, 2], not %r" % (relaxation,))
        self._check(self._lib.egg_group_set_solver_order(self._g, self._SOLVER_ORDERS[order], omega))
        self._solver_order = order

    def get_solver_order(self):
        return getattr(self, "_solver_order", "exact")

    _COHESION_MODES = SimulationHandler._COHESION_MODES

    def set_cohesion(self, mode):
        """SimulationHandler.set_cohesion for every device handle (relaxed order only).  A same-batch pair across a cut
        coheres too: a ghost carries its batch tag, in a record that stays 40 bytes."""
        if mode not in self._COHESION_MODES:
            raise EggError("cohesion must be 'reference' or 'effective', not %r" % (mode,))
        self._check(self._lib.egg_group_set_cohesion(self._g, self._COHESION_MODES[mode]))
        self._cohesion = mode

    def get_cohesion(self):
        return getattr(self, "_cohesion", "reference")

    def halo_counters(self):
        """cumulative over relaxed group steps: collision passes, ghost records received, their bytes"""
        p, r, b = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self._lib.egg_group_get_halo_counters(self._g, C.byref(p), C.byref(r), C.byref(b)))
        return dict(passes=p.value, records=r.value, bytes=b.value)

    # touches_of: there is no group entry point -- the discs go to every handle, by keys (a batch's key on its handle is the
    # group's id), and the tables are added
    _TOUCH_OF_FLAGS = _ffi.TOUCH_BY_KEYS

    def _touch_of_tables(self, spec, queries, n_queries, x, y, r):
        return [h._touch_of_table(spec, queries, n_queries, x, y, r) for h in self.handles]

    def particles(self, which, fields=("x", "y")):
        """{global id: (x[n], y[n])} over all devices (the batches of a handle are laid out in ascending global id);
        `fields` picks other per-particle fields (SimulationHandler.download names)"""
        out = {}
        owners = {}
        for gid in range(1, self._n_issued + 1):  # removed ids are skipped, not the end
            try:
                owners[gid] = self.owner(gid)
            except EggError:
                continue
        for k, h in enumerate(self.handles):
            mine = sorted(g for g, (dev, _l) in owners.items() if dev == k)
            if not mine:
                continue
            cols = [h.download(which, f) for f in fields]
            off = 0
            for g in mine:
                nw, ny = h.get_n_particles(owners[g][1])
                n = nw if which == _ffi.WHITE else ny
                out[g] = tuple(c[off:off + n] for c in cols)
                off += n
        return out
