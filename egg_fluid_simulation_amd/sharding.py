"""Multi-GPU sharding of the particle step: one process per GPU, 1-D slabs along x.

The reference is single-process (no distributed backend exists), so this is new
design.  The step only couples particles in adjacent spatial-hash cells
(simulation_handler.lua:1568-1578), and the device path already isolates work in *tiles* of
batches that provably cannot interact.  Sharding therefore works on whole batches:

  * every rank owns the batches whose target lies in its x-slab and steps them with its own
    SimulationHandler -- no particle data crosses ranks while no batch comes near a cut;
  * once per step neighbouring ranks exchange the boxes of their batches that lie within
    `halo_px` of the shared cut (point-to-point isend/irecv, RCCL over xGMI with the "nccl"
    backend: a 1-D chain uses one link per neighbour pair).  These are the ghost records of
    the halo exchange SURVEY.md 8e asks for; at batch granularity they are 4 doubles + an id
    per boundary batch instead of per-particle records;
  * a ghost box within interaction range of a local batch means the two batches could meet in
    this step.  Exact Gauss-Seidel order across a cut cannot be kept in parallel (8e, exactness
    caveat), so that pair must be stepped by ONE rank: ShardedSimulationHandler hands the batch of
    the higher rank over to the lower rank (complete particle state, egg_export_batch /
    egg_import_batch; two messages per neighbour and round, device to device over RCCL) before the step, and hands batches that have strayed deep into another slab
    to that slab's rank.  Every handler lays its particles out in ascending global batch id, so the
    result is bit-identical to one handler holding everything.  BoundaryExchange alone (bench.py)
    raises SlabConflict instead of migrating.

Not covered: the collision budget's exact-mode (a type with so few particles that 0.05 N^2 visits
can bind) needs all particles in one tile and therefore on one rank.  ShardedSimulationHandler.step
watches for it (per-pass visits of the step in flight, summed over ranks against the global budget,
BEFORE the step is committed) and raises EggError instead of stepping on.

Collectives: ONE small all_reduce per step (4 flags: conflict seen / budget suspect / batch strayed out of its
slab's halo / a claim reaches past a whole neighbouring slab) tells every rank whether the launched step may be
committed; everything else on the data path is neighbour point-to-point.  The rare hand-over round exchanges its
plan with two all_gathers of fixed-shape integer tensors (no pickling).

Relaxed order (ShardedSimulationHandler.set_solver_order("relaxed"), DESIGN.md section 2.7 "Several processes") needs none of
this: a Jacobi pass reads only the positions at the start of the pass, so every rank runs every collision pass over its
own particles plus read-only ghost copies of the other ranks' particles near its cell box.  HaloExchange carries the
boxes (one all_gather per pass) and the 40-byte ghost records (point to point, only between ranks whose boxes are
within one cell of each other); nothing is handed over before a step, no step is re-run, and the results equal ONE
relaxed handler holding every batch, bit for bit.

draw(), the environment and the particle download depend on particle ORDER (the screen blend and the serial centroid
sums), so they gather to one render rank ("Several processes"): per type every other rank sends
ONE message -- the seven draw fields of its particles, packed by egg_draw_pack -- and the render rank places the
messages in global-key order (egg_draw_source_*) and runs the single handle's renderer over them, unchanged.
"""
import copy
import math
import time
import warnings

import numpy as np

from . import _ffi
from .simulation_handler import Cover, EggError, EggWarning, Field, _HandlerSurface, _assert_types, _is_nan

_COVER_NO_OWNER = 1 << 62  # "no disc here" in an owner plane while the ranks merge it: above every id


class SlabConflict(RuntimeError):
    """A local batch and a neighbour rank's batch are close enough to interact."""


class SlabLayout:
    """x-slabs [cuts[r], cuts[r+1]) for r in range(world)."""

    def __init__(self, cuts):
        self.cuts = [float(c) for c in cuts]
        if any(b <= a for a, b in zip(self.cuts, self.cuts[1:])):
            raise ValueError("slab cuts must ascend")
        self.world = len(self.cuts) - 1

    @classmethod
    def uniform(cls, x_lo, x_hi, world, align=1.0):
        """equal slabs with cuts on multiples of `align` (use the spatial-hash cell size)"""
        cuts = [x_lo + (x_hi - x_lo) * r / world for r in range(world + 1)]
        return cls([np.floor(c / align) * align for c in cuts[:-1]] + [np.ceil(cuts[-1] / align) * align])

    def owner_of(self, x):
        x = np.asarray(x, dtype=np.float64)
        r = np.searchsorted(np.array(self.cuts[1:-1]), x, side="right")
        return r.astype(np.int64)

    def bounds(self, rank):
        return self.cuts[rank], self.cuts[rank + 1]


class BoundaryExchange:
    """Per-step exchange of slab-boundary batch boxes with the left and right neighbour rank.

    The exchanged boxes are the batches' CLAIMS for the upcoming step (SimulationHandler.prepare_step +
    get_bounds): two batches on different ranks are independent iff their claims stay at least one
    spatial-hash cell apart -- the same criterion that separates tiles inside one handler.
    Boxes are [n, 8]: the white claim then the yolk claim; interact_px = (white cell, yolk cell).

    handler      SimulationHandler of this rank, or None when `bounds_fn` is given
    bounds_fn    () -> (ids[n] int64, boxes[n, 4] float64 px) of the local batches (tests inject this)
    group        a torch.distributed module/process group handle (None: world must be 1)
    """

    RECORD = 9  # id, white box (lo_x, lo_y, hi_x, hi_y), yolk box

    def __init__(self, handler, rank, world, slab_lo, slab_hi, group=None, halo_px=64.0, interact_px=(8.0, 12.0),
                 capacity=4096, bounds_fn=None, device=None):
        self.handler, self.rank, self.world = handler, int(rank), int(world)
        self.slab_lo, self.slab_hi = float(slab_lo), float(slab_hi)
        if np.isscalar(interact_px):
            interact_px = (interact_px, interact_px)
        self.halo_px, self.interact_px, self.capacity = float(halo_px), tuple(float(v) for v in interact_px), int(capacity)
        self.dist = group
        self.bounds_fn = bounds_fn or self._handler_bounds
        self.claims_fixed = False
        self.ghosts = {}          # neighbour rank -> (ids, boxes) received in the last exchange
        self.sent = {}            # neighbour rank -> number of boxes sent
        self.bytes_exchanged = 0
        if self.world > 1:
            import torch
            self.torch = torch
            if device is None:
                device = "cuda" if group.get_backend() == "nccl" else "cpu"
            self.device = device
            n = 1 + self.RECORD * self.capacity
            self._send = {r: torch.zeros(n, dtype=torch.float64, device=device) for r in self._neighbours()}
            self._recv = {r: torch.zeros(n, dtype=torch.float64, device=device) for r in self._neighbours()}
            # host images of the messages (pinned when the wire tensors live on the GPU): no per-step
            # allocation, one async copy each way
            pin = str(device).startswith("cuda")
            self._send_host = {r: torch.zeros(n, dtype=torch.float64, pin_memory=pin) for r in self._neighbours()}
            self._recv_host = {r: torch.zeros(n, dtype=torch.float64, pin_memory=pin) for r in self._neighbours()}

    def _neighbours(self):
        return [r for r in (self.rank - 1, self.rank + 1) if 0 <= r < self.world]

    def _handler_bounds(self):
        if not self.claims_fixed:  # a step already launched (step_begin) has fixed this step's claims
            self.handler.prepare_step()
        ids = np.asarray(self.handler.list_ids(), dtype=np.int64)
        boxes, cells = self.handler.get_claims(ids)
        self.interact_px = cells
        return ids, boxes

    def select_boundary(self, ids, boxes, towards):
        """local batches within halo_px of the cut shared with rank `towards`"""
        if towards < self.rank:
            m = np.minimum(boxes[:, 0], boxes[:, 4]) < self.slab_lo + self.halo_px
        else:
            m = np.maximum(boxes[:, 2], boxes[:, 6]) > self.slab_hi - self.halo_px
        return ids[m], boxes[m]

    @staticmethod
    def conflicts(ids, boxes, ghost_ids, ghost_boxes, reach):
        """pairs (local id, ghost id) whose claims are LESS than one hash cell apart in both x and y, for
        the white boxes (columns 0-3, cell reach[0]) or the yolk boxes (columns 4-7, cell reach[1])"""
        if np.isscalar(reach):
            reach = (reach, reach)
        if len(ids) == 0 or len(ghost_ids) == 0:
            return []
        boxes = np.asarray(boxes, dtype=np.float64).reshape(len(ids), -1)
        ghost_boxes = np.asarray(ghost_boxes, dtype=np.float64).reshape(len(ghost_ids), -1)
        if boxes.shape[1] == 4:  # one box per batch: use it for both types
            boxes = np.concatenate([boxes, boxes], axis=1)
        if ghost_boxes.shape[1] == 4:
            ghost_boxes = np.concatenate([ghost_boxes, ghost_boxes], axis=1)
        ids = np.asarray(ids)
        ghost_ids = np.asarray(ghost_ids)
        near = np.zeros((len(ids), len(ghost_ids)), dtype=bool)
        for t in (0, 1):
            b, g, c = boxes[:, None, 4 * t:4 * t + 4], ghost_boxes[None, :, 4 * t:4 * t + 4], reach[t]
            near |= ((b[..., 0] - g[..., 2] < c) & (g[..., 0] - b[..., 2] < c) &
                     (b[..., 1] - g[..., 3] < c) & (g[..., 1] - b[..., 3] < c))
        li, gi = np.nonzero(near.T)[::-1]
        return [(int(ids[a]), int(ghost_ids[b_])) for a, b_ in zip(li, gi)]

    def post(self, claims_fixed=False):
        """First half of the exchange: collect this rank's claims and start the sends / receives.
        claims_fixed: the step was already launched with step_begin (its tiling fixed the claims), so the
        host work of the exchange runs while the kernels do."""
        if self.world == 1:
            return
        self.claims_fixed = claims_fixed
        torch, dist = self.torch, self.dist
        ids, boxes = self.bounds_fn()
        ids = np.asarray(ids, dtype=np.int64)
        boxes = np.asarray(boxes, dtype=np.float64).reshape(len(ids), -1) if len(ids) else np.zeros((0, 8))
        if boxes.shape[1] == 4:
            boxes = np.concatenate([boxes, boxes], axis=1)
        ops = []
        for r in self._neighbours():
            bi, bb = self.select_boundary(ids, boxes, r)
            if len(bi) > self.capacity:
                raise RuntimeError("more than %d boundary batches; raise BoundaryExchange(capacity=...)" % self.capacity)
            rec = self._send_host[r].numpy()
            rec[0] = len(bi)
            body = rec[1:1 + self.RECORD * len(bi)].reshape(len(bi), self.RECORD)
            body[:, 0] = bi
            body[:, 1:] = bb
            if self._send[r].data_ptr() != self._send_host[r].data_ptr():
                self._send[r].copy_(self._send_host[r], non_blocking=True)
            self.sent[r] = len(bi)
            ops.append(dist.P2POp(dist.isend, self._send[r], r))
            ops.append(dist.P2POp(dist.irecv, self._recv[r], r))
        self._pending = dist.batch_isend_irecv(ops)
        self.last_ids, self.last_boxes = ids, boxes

    def finish(self, raise_on_conflict=True):
        """Second half: wait for the neighbours' claims and test them against the local ones.  Returns
        the conflicts as (local id, ghost id, ghost rank); raises SlabConflict for them unless told
        otherwise."""
        if self.world == 1:
            return []
        for req in self._pending:
            req.wait()
        self._pending = []
        ids, boxes = self.last_ids, self.last_boxes
        found = []
        for r in self._neighbours():
            self._recv_host[r].copy_(self._recv[r])
            rec = self._recv_host[r].numpy()
            n = int(rec[0])
            body = rec[1:1 + self.RECORD * n].reshape(n, self.RECORD)
            gids, gboxes = body[:, 0].astype(np.int64), body[:, 1:].copy()
            self.ghosts[r] = (gids, gboxes)
            self.bytes_exchanged += 8 * (2 + self.RECORD * (n + self.sent[r]))
            if n:
                # only local batches that reach as far towards that cut as the ghosts reach into this slab
                # (at least the halo) can meet them
                c = max(self.interact_px)
                if r < self.rank:
                    depth = max(self.halo_px, float(np.max(gboxes[:, [2, 6]])) - self.slab_lo + c)
                    m = np.minimum(boxes[:, 0], boxes[:, 4]) < self.slab_lo + depth
                else:
                    depth = max(self.halo_px, self.slab_hi - float(np.min(gboxes[:, [0, 4]])) + c)
                    m = np.maximum(boxes[:, 2], boxes[:, 6]) > self.slab_hi - depth
                found += [(i, g, r) for i, g in self.conflicts(ids[m], boxes[m], gids, gboxes, self.interact_px)]
        if raise_on_conflict and found:
            raise SlabConflict(
                "rank %d: %d local/ghost batch pairs less than one hash cell apart across a slab cut (first: %s); "
                "use ShardedSimulationHandler to hand such batches over" % (self.rank, len(found), found[:1]))
        return found

    def exchange(self, raise_on_conflict=True):
        """post() + finish()"""
        self.post()
        return self.finish(raise_on_conflict)


class HaloExchange:
    """Per-pass exchange of the relaxed-order ghost halo between the ranks ("Several processes").

    Per collision pass p, on every rank:
      1. source.rx_get_boxes(p): this rank's cell box per type (lo_x, lo_y, hi_x, hi_y, empty; int32);
      2. ONE all_gather of the [2, 5] int32 boxes: every rank knows every box of the pass;
      3. the PARTNERS of a rank are the ranks whose box of some type lies within one cell of its own box of that type
         (a symmetric relation both sides compute from the same gathered boxes -- nothing else decides who talks);
      4. source.rx_pack(p, partners' boxes) -> record counts; a fixed-shape count message (2 int64) goes to every
         partner and one comes back; then, where a count is not zero, ONE payload message of the announced size:
         the white message followed by the yolk message, each `count, records...` in 64-bit words (5 per record);
      5. the caller runs the pass over its particles + the received messages (received()).
    Nothing is pickled and every message size is fixed or announced.  `source` is a SimulationHandler or anything with
    its rx_get_boxes / rx_pack / rx_fetch (tests inject a numpy model)."""

    BOX = 5            # int32 per box
    RECORD_WORDS = 5   # 64-bit words per ghost record
    RECORD_BYTES = 40

    def __init__(self, source, rank, world, group=None, device=None):
        self.source, self.rank, self.world = source, int(rank), int(world)
        self.dist = group
        self.passes = self.records = 0          # passes exchanged; ghost records received
        self.collectives = self.messages = 0    # all_gathers; point-to-point messages sent
        self.host_seconds = 0.0                 # wall time spent in exchange()
        self.host_syncs = 0                     # source calls that wait for the device (boxes; pack and fetch with partners)
        self.partners, self.boxes = [], None    # of the last exchange
        self._recv, self._send, self._counts_in = [], [], np.zeros((0, 2), dtype=np.int64)
        if self.world > 1:
            import torch
            self.torch = torch
            if device is None:
                device = "cuda" if group.get_backend() == "nccl" else "cpu"
            self.device = device
            self._on_gpu = str(device).startswith("cuda")

    @property
    def bytes(self):
        return self.RECORD_BYTES * self.records

    @staticmethod
    def near(a, b):
        """two boxes (lo_x, lo_y, hi_x, hi_y, empty) are within one cell of each other: a particle of the one can lie in
        the other grown by one cell"""
        return bool(not a[4] and not b[4] and a[0] - 1 <= b[2] and b[0] - 1 <= a[2] and a[1] - 1 <= b[3] and b[1] - 1 <= a[3])

    def _wait(self, ops):
        if not ops:
            return
        for req in self.dist.batch_isend_irecv(ops):
            req.wait()
        if self._on_gpu:  # the receives ran on torch's stream: complete before anyone else reads the tensors
            self.torch.cuda.current_stream().synchronize()

    def exchange(self, p):
        """the halo of pass p; returns (pointers [n, 2], counts [n, 2]) of the received messages for rx_run_pass.  The
        tensors behind the pointers live until the next exchange()."""
        t0 = time.perf_counter()
        torch, dist = self.torch, self.dist
        mine = np.ascontiguousarray(self.source.rx_get_boxes(p), dtype=np.int32).reshape(2, self.BOX)
        box = torch.from_numpy(mine.reshape(-1).copy()).to(self.device)
        parts = [torch.zeros(2 * self.BOX, dtype=torch.int32, device=self.device) for _ in range(self.world)]
        dist.all_gather(parts, box)
        self.collectives += 1
        boxes = np.stack([q.cpu().numpy() for q in parts]).reshape(self.world, 2, self.BOX)
        partners = [k for k in range(self.world)
                    if k != self.rank and any(self.near(boxes[self.rank, w], boxes[k, w]) for w in (0, 1))]
        self.partners, self.boxes = partners, boxes
        n = len(partners)
        out_counts = np.asarray(self.source.rx_pack(p, boxes[partners]), dtype=np.int64).reshape(n, 2)
        # counts: fixed shape, both ways
        cs = [torch.from_numpy(out_counts[i].copy()).to(self.device) for i in range(n)]
        cr = [torch.zeros(2, dtype=torch.int64, device=self.device) for _ in range(n)]
        ops = []
        for i, k in enumerate(partners):
            ops.append(dist.P2POp(dist.isend, cs[i], k))
            ops.append(dist.P2POp(dist.irecv, cr[i], k))
        self._wait(ops)
        self.messages += n
        in_counts = np.array([c.cpu().numpy() for c in cr], dtype=np.int64).reshape(n, 2)
        # payloads: [white message | yolk message], only where something travels
        W = self.RECORD_WORDS
        send = [torch.empty(2 + W * int(c.sum()), dtype=torch.int64, device=self.device) if c.sum() else None for c in out_counts]
        recv = [torch.empty(2 + W * int(c.sum()), dtype=torch.int64, device=self.device) if c.sum() else None for c in in_counts]
        ptr = np.zeros((n, 2), dtype=np.uint64)
        for i, t in enumerate(send):
            if t is not None:
                ptr[i] = (t.data_ptr(), t.data_ptr() + 8 * (1 + W * int(out_counts[i, 0])))
        if n:
            self.source.rx_fetch(ptr)  # (complete when it returns: the sends may start)
        self.host_syncs += 3 if n else 1
        ops = []
        for i, k in enumerate(partners):
            if send[i] is not None:
                ops.append(dist.P2POp(dist.isend, send[i], k))
                self.messages += 1
            if recv[i] is not None:
                ops.append(dist.P2POp(dist.irecv, recv[i], k))
        self._wait(ops)
        rptr = np.zeros((n, 2), dtype=np.uint64)
        for i, t in enumerate(recv):
            if t is not None:
                rptr[i] = (t.data_ptr(), t.data_ptr() + 8 * (1 + W * int(in_counts[i, 0])))
        self._send, self._recv, self._counts_in = send, recv, in_counts
        self.passes += 1
        self.records += int(in_counts.sum())
        self.host_seconds += time.perf_counter() - t0
        return rptr, in_counts

    def received(self, which):
        """the ghost records of type `which` received in the last exchange: int64 words [m, 5] (view the first four columns
        as float64 for x, y, inverse mass, radius; the fifth is the global key)"""
        W, rows = self.RECORD_WORDS, []
        for t, c in zip(self._recv, self._counts_in):
            if t is None or c[which] == 0:
                continue
            words = t.cpu().numpy()
            off = 0 if which == 0 else 1 + W * int(c[0])
            assert int(words[off]) == int(c[which]), "message header and announced count differ"
            rows.append(words[off + 1:off + 1 + W * int(c[which])].reshape(-1, W))
        return np.concatenate(rows) if rows else np.zeros((0, W), dtype=np.int64)


class ShardedSimulationHandler(_HandlerSurface):
    """The reference's `SimulationHandler` class spread over the ranks of a process group, one x-slab per rank: every
    public method of the class with the signatures, argument checks, warnings and error texts of SimulationHandler
    (shared code: _HandlerSurface).

    SPMD: every rank makes the same calls with the same arguments; batch ids are global.  `make_handler` builds the
    local device handler (tests inject their own).  Whatever it returns or draws equals, bit for bit, what ONE
    SimulationHandler holding every batch, added in the same order, returns or draws (tests/test_gpu_sharded.py,
    tests/test_gpu_sharded_draw.py) -- in exact and in relaxed order, before and after hand-overs and removes.

    State that is a function of the call sequence lives on EVERY rank, keyed by global id: configs, render configs and
    switches, per-batch colours with the reference's aliasing (a batch added without a colour shares the config's
    colour table, L:49-50, L:349), targets, radii, particle counts, the id list.  add / remove / set_* / get_n_particles /
    list_ids / get_target_position need no communication beyond the count table; get_position is one broadcast from
    the owner.

    add, remove and set_target_position reach the device on the OWNER only.  If its handle refuses the call (a step left
    open on that rank by hand: nothing in this class does that), the owner raises with its tables unchanged while the
    other ranks have applied the call: the ranks then disagree, and the object is to be discarded.  Argument errors are
    raised on every rank before anything changes.

    draw(), get_environment(), download(), download_instance_data(), instances() are COLLECTIVE (every rank calls them) and ANSWER
    ON THE RENDER RANK (`root`, rank 0 by default): the image / dict / array there, None on the other ranks;
    render_canvas() answers on the render rank without communication.  A refusal on any rank (a step in flight, a limit
    of DESIGN.md section 7 on the render rank) raises EggError on EVERY rank.

    set_solver_order("relaxed") switches every rank to relaxed order (the same call on every rank): step() then runs
    every collision pass with a ghost halo between the ranks (HaloExchange) instead of handing batches over, and the
    results equal ONE relaxed handler holding every batch, bit for bit (tests/test_gpu_sharded_relaxed.py).
    """

    STATE_FIELDS = 9

    def __init__(self, layout, rank, group, make_handler, halo_px=64.0, interact_px=(8.0, 12.0), device=None, root=0):
        import torch
        self.torch, self.dist = torch, group
        # instances(): counts the calls that can change a particle's colour or the particle count, as the library does per
        # handle (egg_get_instances); replicated, since every rank makes the same calls
        self._color_version = 1
        self.layout, self.rank, self.world = layout, int(rank), layout.world
        self.root = int(root)     # the render rank
        if not 0 <= self.root < self.world:
            raise ValueError("root must be a rank of the layout")
        self.local = make_handler()
        self._lib = getattr(self.local, "_lib", None)
        self.owner = {}       # global id -> rank
        self.local_id = {}    # global id -> id in self.local (batches this rank owns)
        self.global_id = {}   # local id -> global id
        self.radii = {}       # global id -> (white_radius, yolk_radius)
        self.next_gid = 1
        self.migrations = 0
        self.bytes_handed_over = 0
        self._committed_visits = [0, 0]  # most pairs one pass of the last committed step visited, per type
        self._elapsed = 0.0
        self._alpha = 0.0
        self._n_steps = 0         # committed _steps: nothing is drawn before the first (L:1997-1999)
        self._budget_stale = True
        self._step_args = (1 / 60, 2, 3)
        lo, hi = layout.bounds(rank)
        self.exchange = BoundaryExchange(None, rank, self.world, lo, hi, group=group, halo_px=halo_px,
                                         interact_px=interact_px, bounds_fn=self._bounds, device=device)
        self.device = self.exchange.device if self.world > 1 else "cpu"
        self._on_gpu = str(self.device).startswith("cuda")
        self._order = "exact"
        self._keys_stale = True   # the global keys of relaxed order: rebuilt after adds, removes and hand-overs
        self.halo = HaloExchange(self.local, rank, self.world, group=group, device=self.device) if self.world > 1 else None
        self._halo_passes = 0     # (world == 1 counts its passes here: there is no exchange)
        # replicated host state: the config tables start as the local handler's (every rank builds the same)
        self._init_host_state(copy.deepcopy(getattr(self.local, "_white_config", None)),
                              copy.deepcopy(getattr(self.local, "_yolk_config", None)))
        self._targets = {}        # global id -> (x, y)
        self._counts = {}         # global id -> (white particles, yolk particles): gathered from the owners
        # what the device library keeps per handle for its own draw, kept here per GLOBAL id so that a hand-over cannot
        # lose it: the render keys as last sent, the rgba a batch's particles carry (L:978-990, L:1110-1129) and whether
        # its colour table is its own (L:49-50)
        self._rcfg = [self._c_render_config(True), self._c_render_config(False)]
        self._pcolor = {}
        self._own_color = {}
        self._draw = dict(draws=0, messages=0, bytes=0, host_seconds=0.0)

    # ------------------------------------------------------------------ API
    def add(self, x, y, white_radius=50.0, yolk_radius=15.0, white_color=None, yolk_color=None, white_n_particles=None,
            yolk_n_particles=None, white_n=None, yolk_n=None):  # L:27-135
        """SimulationHandler.add (the radii keep this class's defaults; None takes the reference's); `white_n` / `yolk_n`
        are other names of the two counts"""
        for long, short, name in ((white_n_particles, white_n, "white"), (yolk_n_particles, yolk_n, "yolk")):
            if long is not None and short is not None and long != short:
                raise EggError("[ERROR] In SimulationHandler.add: %s_n_particles and %s_n are two names of one count and "
                               "differ (%r, %r)" % (name, name, long, short))
        if white_n_particles is None:
            white_n_particles = white_n
        if yolk_n_particles is None:
            yolk_n_particles = yolk_n
        white_color, yolk_color, given = self._check_add(x, y, white_radius, yolk_radius, white_color, yolk_color,
                                                         white_n_particles, yolk_n_particles)
        if not (math.isfinite(x) and math.isfinite(y)):  # (refused on every rank, not by the owner's handle alone)
            raise EggError("[ERROR] In SimulationHandler.add: position is not a finite number")
        gid = self.next_gid
        r = int(self.layout.owner_of([x])[0])
        if r == self.rank:
            counts = {}  # (the overrides travel only when given: add_many_keyed keeps its positional form)
            if white_n_particles is not None:
                counts["white_n_particles"] = int(math.ceil(white_n_particles))
            if yolk_n_particles is not None:
                counts["yolk_n_particles"] = int(math.ceil(yolk_n_particles))
            lid = int(self.local.add_many_keyed([x], [y], [gid], white_radius, yolk_radius, **counts)[0])
            self.local_id[gid] = lid
            self.global_id[lid] = gid
        self.next_gid += 1
        self.owner[gid] = r
        self.radii[gid] = (white_radius, yolk_radius)
        self._targets[gid] = (float(x), float(y))
        # colours: L:978-990 (the particles take the batch colour only while _use_particle_color is set; add does not
        # clamp), L:49-50 (no colour argument: the batch shares the config's table)
        self._batch_colors[gid] = [white_color, yolk_color]
        self._own_color[gid] = [bool(given[0]), bool(given[1])]
        pc = np.ones((2, 4), dtype=np.float32)
        if self._use_particle_color_flag:
            for which, color in enumerate((white_color, yolk_color)):
                pc[which] = list(color[:4]) if given[which] else list(self._rcfg[which].color)
        self._pcolor[gid] = pc
        self._budget_stale = True  # summed over the ranks before the next step
        self._keys_stale = True
        self._color_version += 1
        return gid

    def remove(self, batch_id):  # L:140-155
        _assert_types(batch_id, "number")
        gid = int(batch_id)
        if gid not in self.owner:
            warnings.warn("In SimulationHandler.remove: no batch with id `%d`" % gid, EggWarning)
            return
        if self.owner[gid] == self.rank:
            lid = self.local_id[gid]
            self.local.remove(lid)
            del self.local_id[gid], self.global_id[lid]
        for table in (self.owner, self.radii, self._targets, self._counts, self._batch_colors, self._own_color, self._pcolor):
            table.pop(gid, None)
        self._budget_stale = True
        self._keys_stale = True
        self._color_version += 1

    def list_ids(self):  # L:399-405
        return sorted(self.owner)

    def get_n_particles(self, batch_or_nil=None):  # L:409-419
        if batch_or_nil is not None and int(batch_or_nil) not in self.owner:
            raise EggError("[ERROR] In SimulationHandler:get_n_particles: no batch with id `%d`" % int(batch_or_nil))
        self._sync_counts()
        if batch_or_nil is not None:
            return self._counts[int(batch_or_nil)]
        return (sum(c[0] for c in self._counts.values()), sum(c[1] for c in self._counts.values()))

    def get_target_position(self, batch_id):  # L:268-278
        _assert_types(batch_id, "number")
        if int(batch_id) not in self.owner:
            raise EggError("[ERROR] In SimulationHandler.get_target_position: no batch with id `%d`" % int(batch_id))
        return self._targets[int(batch_id)]

    def get_position(self, batch_id):  # L:281-295
        """the owner's egg_get_position (the reference's serial centroid), the same value on every rank: one
        fixed-shape broadcast from the owner"""
        _assert_types(batch_id, "number")
        gid = int(batch_id)
        if gid not in self.owner:
            raise EggError("[ERROR] In SimulationHandler.get_position: no batch with id `%d`" % gid)
        src, err, rec = self.owner[gid], None, [0.0, 0.0, 0.0]
        if src == self.rank:
            try:
                rec[0], rec[1] = self.local.get_position(self.local_id[gid])
            except EggError as e:
                err, rec[2] = e, 1.0
        if self.world > 1:
            t = self.torch.tensor(rec, dtype=self.torch.float64).to(self.device)
            self.dist.broadcast(t, src)
            rec = t.tolist()
        if err is not None:
            raise err
        if rec[2] != 0.0:
            raise EggError("[ERROR] In SimulationHandler.get_position: refused on rank %d, which owns batch `%d`" % (src, gid))
        return rec[0], rec[1]

    # configs: validated on every rank by _HandlerSurface, then applied to the local handle; the re-derivation of mass
    # and radius is per particle (L:1731-1744) and lands on the same bits wherever the particle lives
    def _apply_config(self, white_or_yolk):
        self.local.set_solver_config(_ffi.WHITE if white_or_yolk else _ffi.YOLK, self._c_config(white_or_yolk))
        self._send_render_config()
        self._budget_stale = True

    def _send_render_config(self):  # egg_set_render_config, per global id
        for which in range(2):
            c = self._c_render_config(which == 0)
            ok = (0 <= c.outline_thickness <= 256 and c.texture_scale > 0 and
                  all(math.isfinite(v) for v in (c.motion_blur, c.highlight_strength, c.shadow_strength)))
            if not ok:
                raise EggError("[ERROR] egg_set_render_config: value out of range")
            self._rcfg[which] = c
            for own in self._own_color.values():  # config.color is a new table now (L:1307-1311)
                own[which] = True
        self._color_version += 1

    def _apply_render_flags(self):
        self._color_version += 1  # (the switches themselves are read at add and at draw)

    def _message(self):  # (_check of a library call that takes no handle)
        return self._lib.egg_last_error(None).decode()

    def _apply_color(self, gid, which, rgba):  # egg_set_color, per global id
        if any(_is_nan(c) for c in rgba):
            return
        c = np.array([float(v) for v in rgba], dtype=np.float32)
        self._pcolor[gid][which] = c
        if not self._own_color[gid][which]:  # the shared table (L:49-50, L:349-350)
            self._rcfg[which].color[:] = [float(v) for v in c]
        self._color_version += 1

    @property
    def elapsed(self):
        return self._elapsed

    @property
    def interpolation_alpha(self):
        return self._alpha

    def set_solver_order(self, order, relaxation=None):
        """"exact" (default) or "relaxed" with omega `relaxation` (None keeps the current value), on every rank alike.
        Back in "exact" the handlers re-tile and the exact protocol hands islands over again."""
        self.local.set_solver_order(order, relaxation)
        self._order = order
        self._budget_stale = True

    def get_solver_order(self):
        return self._order

    def set_cohesion(self, mode):
        """SimulationHandler.set_cohesion on every rank alike (the same call on every rank; relaxed order only).  A ghost
        carries its batch tag in the upper half of its key word: a record stays 40 bytes."""
        self.local.set_cohesion(mode)
        self._cohesion = mode

    def get_cohesion(self):
        return getattr(self, "_cohesion", "reference")

    # ------------------------------------------------ what the reads below share
    def _all_reduce_sum(self, values):
        """`values`, a list or numpy array of integers, added over the ranks: the same shape as int64 after ONE all_reduce(SUM)
        of an int64 tensor on self.device (a collective: every rank calls it with the same shape).  Integer addition has no
        order, so the sum equals one handle's bit for bit.  A one-rank object gets its own values back and needs no process
        group; nothing travels for an empty table either."""
        values = np.ascontiguousarray(values, dtype=np.int64)
        if self.world == 1 or values.size == 0:
            return values
        tot = self.torch.from_numpy(values).to(self.device)
        self.dist.all_reduce(tot, op=self.dist.ReduceOp.SUM)
        return tot.cpu().numpy()

    def _owner_table(self, ids, unknown, shape, rows):
        """an int64 table [len(ids)] + shape over all ranks: every global id of `ids` is checked against the owners (the
        EggError text is `unknown` % the id, raised on every rank before anything travels), the rows of the batches this rank
        holds come from `rows(their local ids)` -- called on every rank, with an empty list where it holds none --, the others
        stay zero, and _all_reduce_sum adds the ranks"""
        for gid in ids:
            if gid not in self.owner:
                raise EggError(unknown % gid)
        table = np.zeros((len(ids),) + tuple(shape), dtype=np.int64)
        mine = [k for k, gid in enumerate(ids) if gid in self.local_id]
        table[mine] = rows([self.local_id[ids[k]] for k in mine])
        return self._all_reduce_sum(table)

    def set_colliders(self, colliders):
        """SimulationHandler.set_colliders on every rank alike (the same call on every rank; relaxed order only).  Nothing
        new travels: every rank projects the particles it owns, before their positions go out as ghosts."""
        self.local.set_colliders(colliders)

    def get_colliders(self):
        return self.local.get_colliders()

    def collider_hits(self):
        """SimulationHandler.collider_hits summed over the ranks (a collective: every rank calls it)"""
        return self._all_reduce_sum(self.local.collider_hits()).tolist()

    def set_collider_surfaces(self, surfaces):
        """SimulationHandler.set_collider_surfaces on every rank alike (the same call on every rank).  Nothing new travels:
        every rank applies friction to the particles it owns, from their own start-of-sub-step positions."""
        self.local.set_collider_surfaces(surfaces)

    def get_collider_surfaces(self):
        return self.local.get_collider_surfaces()

    def collider_grips(self):
        """SimulationHandler.collider_grips summed over the ranks (a collective: every rank calls it)"""
        return self._all_reduce_sum(self.local.collider_grips()).tolist()

    def set_collider_motion(self, motions):
        """SimulationHandler.set_collider_motion on every rank alike (the same call on every rank).  Nothing new travels:
        every rank moves its own copy of the list, in every pass and at every commit, by the same arithmetic."""
        self.local.set_collider_motion(motions)

    def get_collider_motion(self):
        return self.local.get_collider_motion()

    def set_collider_spin(self, spins):
        """SimulationHandler.set_collider_spin on every rank alike (the same call on every rank).  Nothing new travels:
        every rank turns its own copy of the list, in every pass and at every commit, by the same arithmetic."""
        self.local.set_collider_spin(spins)

    def get_collider_spin(self):
        return self.local.get_collider_spin()

    def set_collider_styles(self, styles):
        """SimulationHandler.set_collider_styles on every rank alike (the same call on every rank).  Nothing new travels:
        the render rank draws its own copy of the list, which every rank holds and advances by the same arithmetic."""
        self.local.set_collider_styles(styles)

    def get_collider_styles(self):
        return self.local.get_collider_styles()

    def get_collider_pose(self, alpha=None):
        """SimulationHandler.get_collider_pose on this rank's copy of the list (no communication: every rank holds the
        same two lists); `alpha` None takes this object's interpolation_alpha, as draw() does."""
        return self.local.get_collider_pose(self._alpha if alpha is None else alpha)

    def set_collider_loads(self, on):
        """SimulationHandler.set_collider_loads on every rank alike (the same call on every rank).  Nothing new travels:
        every rank projects only the particles it owns, so only they contribute to its sums."""
        self.local.set_collider_loads(on)

    def get_collider_loads_enabled(self):
        return self.local.get_collider_loads_enabled()

    def collider_load_sums(self):
        """SimulationHandler.collider_load_sums with the int64 sums and the dropped count added over the ranks (a collective:
        every rank calls it).  Integer addition has no order, so the result equals one handle's bit for bit."""
        sums, dropped, h = self.local.collider_load_sums()
        flat = self._all_reduce_sum([v for t in sums for v in t] + [dropped]).tolist()
        return [tuple(flat[3 * k:3 * k + 3]) for k in range(len(sums))], flat[-1], h

    def collider_loads(self):
        """SimulationHandler.collider_loads over all ranks (a collective): the summed integers, converted here with the
        library's two divisions"""
        sums, _dropped, h = self.collider_load_sums()
        if not h > 0.0:
            return [(0.0, 0.0, 0.0)] * len(sums)
        si, st = _ffi.COLLIDER_LOAD_IMPULSE_SCALE, _ffi.COLLIDER_LOAD_TORQUE_SCALE
        return [((float(sx) / si) / h, (float(sy) / si) / h, (float(sz) / st) / h) for sx, sy, sz in sums]

    def set_sensors(self, sensors):
        """SimulationHandler.set_sensors on every rank alike (the same call on every rank; either solver order).  Nothing
        travels in a step: every rank measures the particles it owns, when a read asks."""
        self.local.set_sensors(sensors)

    def get_sensors(self):
        return self.local.get_sensors()

    def sensor_sums(self):
        """SimulationHandler.sensor_sums with the integers and the dropped pair added over the ranks (a collective: every
        rank calls it; one all_reduce of an int64 tensor).  Integer addition has no order, so the result equals one
        handle's bit for bit."""
        sums, dropped = self.local.sensor_sums()
        flat = self._all_reduce_sum([v for per_type in sums for rec in per_type for v in rec] + list(dropped)).tolist()
        return [(tuple(flat[6 * k:6 * k + 3]), tuple(flat[6 * k + 3:6 * k + 6])) for k in range(len(sums))], flat[-2:]

    def sensors(self):
        """SimulationHandler.sensors over all ranks (a collective): the summed integers, converted here with the library's
        two divisions"""
        return self._sensor_readings(self.sensor_sums()[0])

    def sensor_batches(self, ids):
        """SimulationHandler.sensor_batches over all ranks (a collective: every rank calls it with the same ids): every rank
        fills in the batches it holds and zeros elsewhere, one all_reduce of an int64 tensor adds them"""
        n_sensors = len(self.local.get_sensors())
        table = self._owner_table([int(i) for i in ids], "[ERROR] In SimulationHandler.sensor_batches: no batch with id `%d`", (n_sensors, 2),
                                  lambda lids: self.local.sensor_batches(lids) if lids and n_sensors else 0)
        return table.astype(np.int32)

    def probe(self, probes):
        """SimulationHandler.probe over all ranks (a collective: every rank calls it with the same list).  Every rank asks its
        own handle, the ranks all_gather their hit tables (one int64 tensor, the doubles as their bit patterns) and each rank
        keeps per (probe, type) the best by (score, key, index): one handle's answer bit for bit, with the global id.  Nothing
        travels in a step."""
        n, arr = self._c_probes(probes)
        table = self.local._probe_table(n, arr)
        mine = np.zeros((n, 2, 7), dtype=np.int64)  # found, key, index, then the bits of score, x, y, radius
        for k, pair in enumerate(table):
            for w, t in enumerate(pair):
                if t is not None:
                    mine[k, w, :3] = (1, t[1], t[2])
                    mine[k, w, 3:] = np.array([t[0], t[4], t[5], t[6]], dtype=np.float64).view(np.int64)
        parts = [mine]
        if self.world > 1 and n:
            own = self.torch.from_numpy(mine).to(self.device)
            got = [self.torch.zeros_like(own) for _ in range(self.world)]
            self.dist.all_gather(got, own)
            parts = [q.cpu().numpy() for q in got]
        best = []
        for k in range(n):
            pair = []
            for w in (0, 1):
                found = None
                for part in parts:
                    rec = part[k, w]
                    if not rec[0]:
                        continue
                    score, x, y, radius = (float(v) for v in rec[3:].view(np.float64))
                    key, index = int(rec[1]), int(rec[2])  # (the global id of a batch is the key its rank's handle holds)
                    if found is None or score < found[0] or (score == found[0] and (key, index) < found[1:3]):
                        found = (score, key, index, key, x, y, radius)
                pair.append(found)
            best.append(tuple(pair))
        return self._probe_hits(best)

    def field(self, origin, cell, shape, types="both", velocity=False, path="auto"):
        """SimulationHandler.field over all ranks (a collective: every rank calls it with the same grid).  Every rank bins the
        particles it owns; one all_reduce(SUM) per plane and one for the totals add them.  The planes are integers, so the
        result equals one handle's bit for bit (units_tiled / units_direct count the ranks' units).  Nothing travels in a
        step.  There is no field_to here: the planes of the ranks live on different devices."""
        spec = self._c_field_spec(origin, cell, shape, types, path)
        count, svx, svy, t = self.local._field_planes(spec, bool(velocity))
        flat = np.array(list(t.inside) + list(t.outside) + list(t.dropped) + [t.units_tiled, t.units_direct], dtype=np.int64)
        planes = []
        for plane in (count, svx, svy, flat):
            planes.append(None if plane is None else self._all_reduce_sum(plane))
        count, svx, svy, flat = planes
        flat = flat.tolist()
        return Field(count.astype(np.int32), svx, svy, tuple(flat[0:2]), tuple(flat[2:4]), tuple(flat[4:6]), flat[6], flat[7])

    def cover(self, origin, cell, shape, scale=1.0, types="both", owner=False, path="auto"):
        """SimulationHandler.cover over all ranks (a collective: every rank calls it with the same grid).  Every rank rasters
        the particles it owns; one all_reduce(SUM) adds the cover plane and the additive totals, one all_reduce(MIN) merges
        the owner plane -- taken as keys (the global id of a batch is the key its rank's handle holds), "none" mapped to the
        largest value -- and covered, covered_both and
        covered_any are recounted locally from the merged plane: one handle's answer, bit for bit (units_* count the ranks'
        units).  Nothing travels in a step.  There is no cover_to here: the planes of the ranks live on different devices."""
        spec = self._c_cover_spec(origin, cell, shape, scale, types, path)
        spec.path |= _ffi.COVER_OWNER_KEYS
        plane, own, t = self.local._cover_planes(spec, bool(owner))
        flat = list(t.inside) + list(t.outside) + list(t.dropped) + list(t.hits) + [t.units_lanes, t.units_wave, t.units_direct]
        both = self._all_reduce_sum(np.concatenate([plane.ravel().astype(np.int64), np.array(flat, dtype=np.int64)]))
        plane, flat = both[:plane.size].reshape(plane.shape).astype(np.int32), both[plane.size:].tolist()
        if own is not None:
            own = self._all_reduce_min(np.where(own < 0, _COVER_NO_OWNER, own.astype(np.int64)))
            own = np.where(own == _COVER_NO_OWNER, -1, own).astype(np.int32)
        a, b = plane[0] > 0, plane[1] > 0
        return Cover(plane, own, spec.cell, tuple(flat[0:2]), tuple(flat[2:4]), tuple(flat[4:6]), tuple(flat[6:8]), (int(a.sum()), int(b.sum())),
                     int((a & b).sum()), int((a | b).sum()), flat[8], flat[9], flat[10])

    def _all_reduce_min(self, values):
        """`values`, an int64 numpy array, merged over the ranks by minimum: ONE all_reduce(MIN) of an int64 tensor on
        self.device (a collective).  A one-rank object gets its own values back and needs no process group."""
        values = np.ascontiguousarray(values, dtype=np.int64)
        if self.world == 1 or values.size == 0:
            return values
        low = self.torch.from_numpy(values).to(self.device)
        self.dist.all_reduce(low, op=self.dist.ReduceOp.MIN)
        return low.cpu().numpy()

    def pieces(self, ids=None, reach=None, types="both"):
        """SimulationHandler.pieces over all ranks (a collective: every rank calls it with the same arguments).  A batch lives
        wholly on one rank: every rank fills the records of the batches it owns and zeros elsewhere, one all_reduce(SUM) of an
        int64 table adds them, so the records equal one handle's bit for bit.  Nothing travels in a step.  There is no
        piece_labels here: the particles of the ranks live in different arrays."""
        spec = self._c_pieces_spec(reach, types)
        ids = self.list_ids() if ids is None else [int(i) for i in ids]
        table = self._owner_table(ids, "[ERROR] In SimulationHandler.pieces: no batch with id `%d`", (2, 8),
                                  lambda lids: self.local._piece_table(spec, np.ascontiguousarray(lids, dtype=np.int64)))
        return self._piece_summaries(table)

    # ------------------------------------------------ touches (egg_touches / egg_touches_of)
    def _touch_gather(self, table):
        """the ranks' tables of touch records as one (a collective): all_gather of the rows -- every int64 as its two 32-bit
        halves, which a float64 holds exactly --, the rows of one (entry, type, other) added and sorted"""
        t = np.asarray(table, dtype=np.int64).reshape(-1, 8)
        if self.world == 1:
            return self._merge_touch_tables([t])
        parts = self._all_gather_rows(np.concatenate([t >> 32, t & 0xFFFFFFFF], axis=1).astype(np.float64))
        return self._merge_touch_tables([(p[:, :8].astype(np.int64) << 32) | p[:, 8:].astype(np.int64) for p in parts])

    def _touch_table(self, spec, ids):
        """SimulationHandler._touch_table over all ranks (a collective: every rank calls it with the same arguments).  A
        query's batch lives wholly on one rank, its partners on any: the owners publish their queries' discs -- rows 0, 1 and 7
        of export_batch: x, y, radius -- in one all_gather, every rank scans its own particles (egg_touches for the batches it
        owns, egg_touches_of with the others' discs and their keys), and the record tables are gathered and added: one
        handle's table, bit for bit.  Ids are global ids, which are the keys.  Nothing travels in a step."""
        spec = _ffi.EggTouchSpec(spec.reach, spec.type_mask, spec.flags | _ffi.TOUCH_BY_KEYS)
        ids = self.list_ids() if ids is None else [int(i) for i in ids]
        for gid in ids:
            if gid not in self.owner:
                raise EggError("[ERROR] In SimulationHandler.touches: no batch with id `%d`" % gid)
        rows = [np.zeros((0, 5))]
        if self.world > 1:
            for gid in sorted(set(ids) & set(self.local_id)):
                _info, ws, ys = self.local.export_batch(self.local_id[gid])
                for w, st in ((0, ws), (1, ys)):
                    rows.append(np.stack([np.full(st.shape[1], float(gid)), np.full(st.shape[1], float(w)), st[0], st[1], st[7]], axis=1))
        parts = self._all_gather_rows(np.concatenate(rows)) if self.world > 1 else []
        discs = {}
        for p in parts:
            for w in (0, 1):
                sel = p[p[:, 1] == w]
                for gid in np.unique(sel[:, 0]).tolist():
                    discs[(int(gid), w)] = sel[sel[:, 0] == gid][:, 2:]
        tables = []
        mine = [k for k, gid in enumerate(ids) if gid in self.local_id]
        if mine:
            t = self.local._touch_table(spec, np.ascontiguousarray([self.local_id[ids[k]] for k in mine], dtype=np.int64))
            t[:, 0] = np.asarray(mine, dtype=np.int64)[t[:, 0]]
            tables.append(t)
        others = [k for k, gid in enumerate(ids) if gid not in self.local_id]
        if others:  # two queries per entry, white then yolk: a record's slot >> 1 is 2 j + w
            got = [discs.get((ids[k], w), np.zeros((0, 3))) for k in others for w in (0, 1)]
            queries = (_ffi.EggTouchQuery * len(got))(*[_ffi.EggTouchQuery(ids[others[q // 2]], q % 2, d.shape[0]) for q, d in enumerate(got)])
            xyr = np.concatenate(got)
            t = self.local._touch_of_table(spec, queries, len(got), *(np.ascontiguousarray(xyr[:, c]) for c in range(3)))
            t[:, 0] = np.asarray(others, dtype=np.int64)[t[:, 0] // 2]
            tables.append(t)
        return self._touch_gather(self._merge_touch_tables(tables))

    _TOUCH_OF_FLAGS = _ffi.TOUCH_BY_KEYS

    def _touch_of_tables(self, spec, queries, n_queries, x, y, r):
        """SimulationHandler.touches_of over all ranks (a collective): every rank scans its own particles, by keys"""
        return [self._touch_gather(self.local._touch_of_table(spec, queries, n_queries, x, y, r))]

    def impulse(self, records, results=True):
        """SimulationHandler.impulse over all ranks (a collective: every rank calls it with the same list).  The ranks agree
        first: an id no rank owns raises on every rank alike, and every rank has its handle check the list with every record
        inert, which launches nothing.  Then each rank applies the list to the particles it owns -- a record for a batch of
        another rank stays in its place, inert -- and one all_reduce(SUM) of an int64 table adds the totals: one handle's,
        bit for bit.  Nothing travels in a step."""
        n, arr = self._c_impulses(records)
        gids = [int(arr[k].id) for k in range(n)]
        for k, gid in enumerate(gids):
            if gid not in (_ffi.IMPULSE_ALL_BATCHES, _ffi.IMPULSE_NO_BATCH) and gid not in self.owner:
                raise EggError("[ERROR] In SimulationHandler.impulse: record %d: no batch with id `%d`" % (k, gid))
        for k in range(n):
            arr[k].id = _ffi.IMPULSE_NO_BATCH
        self.local._impulse_table(n, arr, False)  # (the checks alone; the same verdict on every rank)
        for k, gid in enumerate(gids):
            arr[k].id = gid if gid in (_ffi.IMPULSE_ALL_BATCHES, _ffi.IMPULSE_NO_BATCH) else self.local_id.get(gid, _ffi.IMPULSE_NO_BATCH)
        table = self.local._impulse_table(n, arr, bool(results))
        return None if table is None else self._impulse_results(self._all_reduce_sum(table))

    def measure_table(self, ids=None, region=None, types="both"):
        """SimulationHandler.measure_table over all ranks (a collective: every rank calls it with the same arguments).  A
        batch lives wholly on one rank: every rank fills the rows of the batches it owns and zeros elsewhere, one
        all_reduce(SUM) of the int64 table adds them, so the table equals one handle's bit for bit.  Nothing travels in a
        step.  There is no measure_to here: the tables of the ranks live on different devices."""
        spec = self._c_measure_spec(region, types, "measure_table")

        def rows(lids):
            self.local._measure_check(spec)  # (the same verdict on every rank, whatever it owns)
            return self.local._measure_table(spec, np.ascontiguousarray(lids, dtype=np.int64)) if lids else 0
        ids = self.list_ids() if ids is None else [int(i) for i in ids]
        return self._owner_table(ids, "[ERROR] In SimulationHandler.measure: no batch with id `%d`", (2, len(_ffi.MEASURE_FIELDS)), rows)

    def set_forces(self, forces):
        """SimulationHandler.set_forces on every rank alike (the same call on every rank; relaxed order only).  Nothing
        new travels: every rank accelerates the particles it owns."""
        self.local.set_forces(forces)

    def get_forces(self):
        return self.local.get_forces()

    def set_viscosity(self, white=0.0, yolk=0.0):
        """SimulationHandler.set_viscosity on every rank alike (the same call on every rank; relaxed order only).  A type
        whose coefficient is not 0 exchanges one more halo per sub-step, after its last collision pass: the ghost records
        of that pass carry the sender's displacement of the sub-step where a collision pass's carry inverse mass and
        radius, so a record stays 40 bytes."""
        self.local.set_viscosity(white, yolk)

    def viscosity(self):
        return self.local.viscosity()

    def viscosity_pairs(self):
        """SimulationHandler.viscosity_pairs summed over the ranks (a collective: every rank calls it)"""
        return self._all_reduce_sum(self.local.viscosity_pairs()).tolist()

    def set_containment(self, factor=0.0, strength=1.0):
        """SimulationHandler.set_containment on every rank alike (the same call on every rank; relaxed order only).
        Nothing new travels: a batch lives wholly on one rank, which summarises its white and projects its yolk."""
        self.local.set_containment(factor, strength)

    def containment(self):
        return self.local.containment()

    def containment_hits(self):
        """SimulationHandler.containment_hits summed over the ranks (a collective: every rank calls it)"""
        return int(self._all_reduce_sum([self.local.containment_hits()])[0])

    def _viscous(self):
        """the coefficients the local handle holds: what the library decides a step's pass sequence from"""
        return self.local.viscosity()

    def halo_counters(self):
        """relaxed steps of this rank, summed over the run: passes with a halo (the collision passes and, while a viscosity
        coefficient is not 0, one viscosity pass per sub-step), ghost records received, their bytes"""
        if self.halo is None:
            return dict(passes=self._halo_passes, records=0, bytes=0)
        return dict(passes=self.halo.passes, records=self.halo.records, bytes=self.halo.bytes)

    def set_target_position(self, batch_id, x, y):  # L:254-264
        _assert_types(batch_id, "number", x, "number", y, "number")
        gid = int(batch_id)
        if gid not in self.owner:
            warnings.warn("In SimulationHandler.set_target_position: no batch with id `%d`" % gid, EggWarning)
            return
        if self.owner[gid] == self.rank:
            self.local.set_target_position(self.local_id[gid], x, y)
        self._targets[gid] = (float(x), float(y))

    def update(self, delta, step_delta=None, n_substeps=None, n_collision_steps=None):
        """The reference's fixed-step accumulator (simulation_handler.lua:199-216) around the exchanging step():
        every `_step` gets its own claim exchange (the claims of one exchange cover one step only)."""
        step_delta, n_substeps, n_collision_steps = self._check_update(delta, step_delta, n_substeps, n_collision_steps)
        for bad, text in ((_is_nan(delta), "`delta` is not a number"),  # egg_update's refusals
                          (step_delta < 0 or _is_nan(step_delta), "`step_delta` is not a number > 0"),
                          (step_delta == 0, "`step_delta` is 0"),
                          (n_substeps < 1, "`n_substeps` is not a number > 0"),
                          (n_collision_steps < 1, "`n_collision_steps` is not a number > 0")):
            if bad:
                raise EggError("[ERROR] In SimulationHandler.update: " + text)
        n_substeps, n_collision_steps = int(n_substeps), int(n_collision_steps)
        self._elapsed = self._elapsed + delta
        n_steps = 0
        max_n_steps = max(4.0, 4 * math.ceil((1 / 60) / step_delta))
        while self._elapsed >= step_delta:
            self.step(step_delta, n_substeps, n_collision_steps)
            self._elapsed = self._elapsed - step_delta
            n_steps += 1
            if n_steps > max_n_steps:  # death-spiral guard, L:208-213
                self._elapsed = 0
                break
        self._alpha = min(max(self._elapsed / step_delta, 0.0), 1.0)
        return n_steps

    def step(self, delta=1 / 60, n_substeps=2, n_collision_steps=3):
        """`_step` directly (L:1722); returns the batches handed over"""
        moved = self._step(delta, n_substeps, n_collision_steps)
        self._n_steps += 1  # (a refused step raised)
        return moved

    def _step(self, delta, n_substeps, n_collision_steps):
        """One `_step` on every rank with the neighbour exchange hidden behind the kernels: post the
        claims, launch the local step, then look at the neighbours' claims; only if some pair of batches
        on different ranks could interact is the launched step discarded, the batches handed over and
        the step run again."""
        self._step_args = (delta, n_substeps, n_collision_steps)
        if self.world == 1:
            self.local.step(delta, n_substeps, n_collision_steps)
            if self._order == "relaxed":
                self._halo_passes += n_substeps * n_collision_steps + (n_substeps if any(self._viscous()) else 0)
            return 0
        if self._order == "relaxed":
            return self._step_relaxed(delta, n_substeps, n_collision_steps)
        self._sync_budget()
        self.local.step_begin(delta, n_substeps, n_collision_steps)  # fixes this step's claims, launches the kernels
        self.exchange.post(claims_fixed=True)
        conflicts = self.exchange.finish(raise_on_conflict=False)
        ids, boxes = self.exchange.last_ids, self.exchange.last_boxes
        lo, hi = self.exchange.slab_lo, self.exchange.slab_hi
        halo = self.exchange.halo_px
        stray = wide = False
        if len(ids):
            bl, bh = np.minimum(boxes[:, 0], boxes[:, 4]), np.maximum(boxes[:, 2], boxes[:, 6])
            # strayed: wholly beyond the halo of this slab (it belongs to the neighbour now)
            stray = bool(np.any((bh < lo - halo) & (self.rank > 0)) or np.any((bl > hi + halo) & (self.rank + 1 < self.world)))
            # wide: a claim reaches past the whole neighbouring slab, where only the rank after next could see it
            left_far = self.layout.cuts[self.rank - 1] if self.rank > 0 else -np.inf
            right_far = self.layout.cuts[self.rank + 2] if self.rank + 2 <= self.world else np.inf
            wide = bool(np.any(bl < left_far + halo) and self.rank > 1) or bool(np.any(bh > right_far - halo) and self.rank + 2 < self.world)
        # The budget guard (simulation_handler.lua:1657-1658): the reference counts the visits of ALL particles
        # against 0.05 N^2, a rank only sees its own.  While every rank stays below budget / world the global count
        # cannot bind; a rank above it triggers the exact sum -- of THIS step, which is still uncommitted.
        visits, budget = self.local.step_peek_visits()
        # (the peek sees the FIRST attempt of the step in flight; step_end may re-run it after a failed claim check, and
        # the step after a hand-over is not peeked at all: what those COMMITTED steps visited is folded into the next
        # step's test -- a binding budget is then refused one step late instead of never)
        visits = [max(int(v), int(c)) for v, c in zip(visits, self._committed_visits)]
        suspect = any(v * self.world > max(1.0, math.ceil(b)) for v, b in zip(visits, budget))
        flag = self.torch.tensor([1.0 if conflicts else 0.0, 1.0 if suspect else 0.0, 1.0 if stray else 0.0,
                                  1.0 if wide else 0.0], dtype=self.torch.float64, device=self.device)
        self.dist.all_reduce(flag, op=self.dist.ReduceOp.MAX)
        flags = flag.tolist()
        if flags[1] != 0.0:
            tot = self.torch.tensor([float(v) for v in visits], dtype=self.torch.float64, device=self.device)
            self.dist.all_reduce(tot, op=self.dist.ReduceOp.SUM)
            for which, (v, b) in enumerate(zip(tot.tolist(), budget)):
                if v > max(1.0, math.ceil(b)):
                    self.local.step_end(False)  # nothing of the suspect step is kept
                    raise EggError("collision budget may bind across ranks (type %d: up to %d visits in a pass, "
                                   "budget %.2f): exact-budget mode needs all particles of the type on one rank"
                                   % (which, int(v), b))
        if flags[3] != 0.0:
            self.local.step_end(False)
            raise EggError("a batch's claim for this step reaches past a whole neighbouring slab; slabs must be wider "
                           "than the distance a batch travels in one step plus the halo")
        if flags[0] == 0.0:
            self.local.step_end(True)
            self._note_committed()
            # a batch that left its slab's halo without meeting anything is handed to the slab it is in before the
            # next step, so that every batch is always known to the ranks on both sides of it
            return self.rebalance() if flags[2] != 0.0 else 0
        self.local.step_end(False)
        moved = self.rebalance()
        self.local.step(delta, n_substeps, n_collision_steps)
        self._note_committed()
        return moved

    # ------------------------------------------------------------ relaxed order
    def _step_relaxed(self, delta, n_substeps, n_collision_steps):
        """One relaxed `_step` on every rank: no budget sync, no claims, nothing handed over before it and nothing
        re-run.  Every pass exchanges its halo; ONE all_reduce after the passes decides on all ranks together whether
        the step is committed (a NaN or out-of-range cell anywhere fails it everywhere, nothing committed)."""
        loc, torch, dist = self.local, self.torch, self.dist
        self._sync_keys()
        viscous = any(self._viscous())
        loc.rx_begin(delta, n_substeps, n_collision_steps)
        try:
            for sub in range(n_substeps):
                loc.rx_substep(sub)
                for c in range(n_collision_steps):
                    p = sub * n_collision_steps + c
                    pointers, counts = self.halo.exchange(p)
                    loc.rx_run_pass(p, pointers, counts)
                if viscous:  # the viscosity pass of the sub-step: the same exchange, the records carry displacements
                    p = _ffi.RX_VISCOSITY_PASS + sub
                    pointers, counts = self.halo.exchange(p)
                    loc.rx_run_pass(p, pointers, counts)
            bad, _pairs, _records = loc.rx_check()
        except BaseException:
            loc.rx_end(False)
            raise
        flag = torch.tensor([1.0 if bad else 0.0], dtype=torch.float64, device=self.device)
        dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        if flag.item() != 0.0:
            loc.rx_end(False)
            raise EggError("[ERROR] relaxed order: a position is NaN or its spatial-hash cell lies outside +-2^30 "
                           "(on this rank or another): nothing was committed on any rank")
        loc.rx_end(True)
        return self._rebalance_relaxed()

    def _sync_counts(self):
        """(white, yolk) particle counts of every live batch on every rank: the owners of the batches nobody has counted
        yet report them in one all_gather of (gid, n_white, n_yolk) rows; nothing travels while no batch was added"""
        if all(g in self._counts for g in self.owner):  # (the same on every rank: both tables are replicated)
            return
        rows = [[g] + list(self.local.get_n_particles(l)) for g, l in sorted(self.local_id.items()) if g not in self._counts]
        rows = np.array(rows, dtype=np.float64).reshape(-1, 3)
        for part in (self._all_gather_rows(rows) if self.world > 1 else [rows]):
            for g, nw, ny in part:
                self._counts[int(g)] = (int(nw), int(ny))

    def _key_table(self):
        """int64 [live batches, 3]: (gid, n_white, n_yolk) in ascending global id -- the particle order of ONE handle
        holding every batch: a batch's particles start at the sum of the counts before it"""
        self._sync_counts()
        return np.array([[g, self._counts[g][0], self._counts[g][1]] for g in sorted(self.owner)], dtype=np.int64).reshape(-1, 3)

    def _sync_keys(self):
        """global keys: a batch's particles start at the sum of the type's particle counts over
        the batches OF ALL RANKS with a smaller id.  Rebuilt only after a batch was added, removed or handed over."""
        if not self._keys_stale:
            return
        table = self._key_table()
        for which in (0, 1):
            n = table[:, 1 + which]
            self.local.rx_set_keys(which, table[:, 0], np.cumsum(n) - n, int(n.sum()))
        self._keys_stale = False

    def _rebalance_relaxed(self):
        """After a committed relaxed step: a batch whose position lies more than halo_px outside its slab moves to the
        slab that holds it (the device group's rule).  It only balances load: the halo makes every rank see what one
        handler would, wherever a batch sits."""
        torch, dist = self.torch, self.dist
        lo, hi, halo = self.exchange.slab_lo, self.exchange.slab_hi, self.exchange.halo_px
        rows = []
        gids = sorted(self.local_id)
        if gids:
            xs, _ys = self.local.get_positions([self.local_id[g] for g in gids])
            for g, x in zip(gids, xs):
                if x < lo - halo or x >= hi + halo:
                    dest = int(self.layout.owner_of([x])[0])
                    if dest != self.rank:
                        rows.append([self.rank, dest, g])
        n = torch.tensor([float(len(rows))], dtype=torch.float64, device=self.device)
        dist.all_reduce(n, op=dist.ReduceOp.SUM)
        if n.item() == 0.0:
            return 0
        parts = self._all_gather_rows(np.array(rows, dtype=np.float64).reshape(-1, 3))
        moves = {}
        for part in parts:
            for src, dest, g in part:
                moves.setdefault((int(src), int(dest)), []).append(int(g))
        # every rank walks the same ordered list of (source, destination) pairs: the earliest unfinished transfer never
        # waits for a later one
        for (src, dest), gs in sorted(moves.items()):
            if self.rank == src:
                self._send_batches(sorted(gs), dest)
            elif self.rank == dest:
                self._recv_batches(len(gs), src)
            for g in gs:
                self.owner[g] = dest
        moved = sum(len(gs) for gs in moves.values())
        self.migrations += moved
        self._keys_stale = True
        return moved

    def _note_committed(self):
        st = self.local.stats()
        self._committed_visits = [int(v) for v in st["max_pass_visits"]]

    def positions(self):
        """{global id: (x, y)} of every batch, gathered on all ranks"""
        mine = {g: self.local.get_position(l) for g, l in self.local_id.items()}
        if self.world == 1:
            return mine
        rec = np.array([[g, p[0], p[1]] for g, p in sorted(mine.items())], dtype=np.float64).reshape(-1, 3)
        merged = {}
        for part in self._all_gather_rows(rec):
            for g, x, y in part:
                merged[int(g)] = (float(x), float(y))
        return merged

    def _all_gather_rows(self, rows):
        """all_gather of a [n, k] float64 array with a different n on every rank: counts first, then the rows padded to
        the largest count (two fixed-shape tensor collectives, nothing is pickled)"""
        torch, dist = self.torch, self.dist
        rows = np.asarray(rows, dtype=np.float64)
        k = rows.shape[1]
        cnt = torch.tensor([float(rows.shape[0])], dtype=torch.float64, device=self.device)
        counts = [torch.zeros(1, dtype=torch.float64, device=self.device) for _ in range(self.world)]
        dist.all_gather(counts, cnt)
        counts = [int(c.item()) for c in counts]
        m = max(1, max(counts))
        buf = torch.zeros(m * k, dtype=torch.float64, device=self.device)
        if rows.shape[0]:
            buf[:rows.size] = torch.from_numpy(rows.reshape(-1)).to(self.device)
        parts = [torch.zeros(m * k, dtype=torch.float64, device=self.device) for _ in range(self.world)]
        dist.all_gather(parts, buf)
        return [p.cpu().numpy()[:c * k].reshape(c, k) for p, c in zip(parts, counts)]

    def particles(self, which):
        """{global id: (x[n], y[n])} of this rank's batches"""
        x, y, b = self.local.download(which, "x"), self.local.download(which, "y"), self.local.download(which, "batch_id")
        return {self.global_id[int(l)]: (x[b == l], y[b == l]) for l in np.unique(b)}

    # ------------------------------------------------------------ draw: gather to the render rank
    def draw_counters(self):
        """this rank's share of the draws so far (draw, get_environment and download each count as one): messages and bytes
        it sent or received, wall time it spent in them.  A message is 56 B per particle + one 8 B status word."""
        return dict(self._draw)

    @staticmethod
    def _runs(counts, bases):
        """run tables of one message: its batches in the sender's order (ascending global id) with `counts` particles each go
        to `bases`; batches whose destinations follow each other share a run"""
        src, dst, at, nxt = [], [], 0, None
        for n, b in zip(counts, bases):
            if b != nxt:
                src.append(at)
                dst.append(int(b))
            at += int(n)
            nxt = int(b) + int(n)
        return src, dst

    def _gather(self, which):
        """Type `which` of every rank into the render rank's external draw source, in global-key order.  Per non-render
        rank ONE message: double[7][n] packed by the library straight into the tensor that is sent (device memory with
        "nccl", host memory with gloo), then one status word (1.0: the pack was refused).  Its size and the place of every
        batch in it follow from the replicated tables: a rank's particles lie in ascending global id.  Returns the error
        of this rank (or, on the render rank, of a sender), None when the type is placed."""
        table = self._key_table()
        gids, n = table[:, 0], table[:, 1 + which]
        base, total = np.cumsum(n) - n, int(n.sum())
        owners = np.array([self.owner[int(g)] for g in gids], dtype=np.int64)
        held = [int(n[owners == r].sum()) for r in range(self.world)]
        F, err, recv = len(_ffi.DRAW_FIELDS), None, {}
        if self.world > 1:
            torch, dist = self.torch, self.dist
            ops = []
            if self.rank != self.root:
                msg = torch.empty(F * held[self.rank] + 1, dtype=torch.float64, device=self.device)
                try:
                    self.local.draw_pack(which, msg.data_ptr(), held[self.rank])  # (complete when it returns)
                except EggError as e:
                    err = e
                msg[-1:].fill_(0.0 if err is None else 1.0)
                ops.append(dist.P2POp(dist.isend, msg, self.root))
                sizes = [msg.numel()]
            else:
                for r in range(self.world):
                    if r != self.root:
                        recv[r] = torch.empty(F * held[r] + 1, dtype=torch.float64, device=self.device)
                        ops.append(dist.P2POp(dist.irecv, recv[r], r))
                sizes = [t.numel() for t in recv.values()]
            for req in dist.batch_isend_irecv(ops):
                req.wait()
            if self._on_gpu:  # the receives ran on torch's stream: complete before the library reads the tensors
                torch.cuda.current_stream().synchronize()
            self._draw["messages"] += len(sizes)
            self._draw["bytes"] += 8 * sum(sizes)
        if self.rank != self.root:
            return err
        refused = [r for r, t in recv.items() if float(t[-1]) != 0.0]
        if refused:
            return EggError("[ERROR] In ShardedSimulationHandler.draw: rank %d could not pack its particles" % refused[0])
        try:
            colors = np.array([self._pcolor[int(g)][which] for g in gids], dtype=np.float32).reshape(-1, 4)
            self.local.draw_source_layout(which, total, base, colors)
            for r in range(self.world):
                m = owners == r
                if r != self.rank and not m.any():
                    continue  # a rank that owns nothing of the type is normal
                src, dst = self._runs(n[m], base[m])
                self.local.draw_source_place(which, 0 if r == self.rank else recv[r].data_ptr(), held[r], src, dst)
        except EggError as e:
            err = e
        return err

    def _agree(self, err):
        """ONE flag all-reduce: a refusal on any rank raises on every rank, never on one while the others wait"""
        flag = 0.0 if err is None else 1.0
        if self.world > 1:
            t = self.torch.tensor([flag], dtype=self.torch.float64).to(self.device)
            self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
            flag = t.item()
        if err is not None:
            raise err
        if flag != 0.0:
            raise EggError("[ERROR] In ShardedSimulationHandler.draw: refused on another rank (its error says why); "
                           "nothing was drawn on any rank")

    def _collective(self, types, on_root):
        t0 = time.perf_counter()
        err = None
        for which in types:
            e = self._gather(which)
            err = err or e
        out = None
        if self.rank == self.root and err is None:
            try:
                out = on_root()
            except EggError as e:
                err = e
        self._draw["draws"] += 1
        self._draw["host_seconds"] += time.perf_counter() - t0
        self._agree(err)
        return out

    def draw(self, screen_size=(800, 600), origin=(0.0, 0.0), interpolation_alpha=None, clear=(0.0, 0.0, 0.0, 0.0),
             canvas_sizes=None, use_instancing=True):  # L:159-162
        """SimulationHandler.draw over the sharded scene.  Collective; returns the (H, W, 4) image on the render rank and
        None on the other ranks.  Nothing is drawn before the first `_step` or while the SCENE has no particles of a type
        (a rank that owns nothing is normal); interpolation_alpha None takes this object's; the canvases grow only, over
        this object's draws."""
        p = self._render_params(screen_size, origin, interpolation_alpha, clear, canvas_sizes, use_instancing)
        return self._collective((0, 1), lambda: self.local.draw_source_render(
            p, self._rcfg, self._use_particle_color_flag, self._use_lighting_flag, self._n_steps > 0, self._alpha))

    def render_canvas(self, which):
        """the density canvas of `which` as the last draw() left it, on the render rank (None elsewhere; no communication)"""
        return self.local.draw_source_render_canvas(which) if self.rank == self.root else None

    def get_environment(self, which):
        """SimulationHandler.get_environment over the sharded scene.  Collective; the dict on the render rank, None elsewhere."""
        return self._collective((which,), lambda: self.local.draw_source_environment(which, self._n_steps > 0))

    def download(self, which, field):
        """One of the seven draw fields (_ffi.DRAW_FIELDS) or "batch_id" (global ids) of every particle of the scene in
        global-key order.  Collective; the array on the render rank, None elsewhere."""
        if field != "batch_id" and field not in _ffi.DRAW_FIELDS:
            raise EggError("[ERROR] In ShardedSimulationHandler.download: only %s and batch_id travel to the render rank, "
                           "not `%s` (particles() reads the local handler)" % (", ".join(_ffi.DRAW_FIELDS), field))
        table = self._key_table()
        if field == "batch_id":
            out = np.repeat(table[:, 0], table[:, 1 + which]).astype(np.float64)
            return out if self.rank == self.root else None
        total = int(table[:, 1 + which].sum())
        return self._collective((which,), lambda: self.local.draw_source_download(which, field, total))

    def download_instance_data(self, which):
        """SimulationHandler.download_instance_data over the sharded scene: one gather.  Collective; render rank only."""
        total = int(self._key_table()[:, 1 + which].sum())

        def on_root():
            cols = [self.local.draw_source_download(which, f, total) for f in _ffi.DRAW_FIELDS]
            return np.stack(cols, axis=1) if total else np.zeros((0, 7))
        return self._collective((which,), on_root)

    def instances(self, which, color=True):
        """SimulationHandler.instances over the sharded scene: ONE gather, then the pack on the render rank's device
        (egg_draw_source_instances).  Collective; (data, color, color_version) on the render rank, None elsewhere."""
        total = int(self._key_table()[:, 1 + which].sum())
        out = self._collective((which,), lambda: self.local.draw_source_instances(which, total, color))
        return None if out is None else (out[0], out[1], self._color_version)

    # ------------------------------------------------------------ internals
    def _bounds(self):
        if not self.exchange.claims_fixed:
            self.local.prepare_step(*self._step_args)
        gids = np.array(sorted(self.local_id), dtype=np.int64)
        if len(gids) == 0:
            return gids, np.zeros((0, 8))
        boxes, cells = self.local.get_claims([self.local_id[int(g)] for g in gids])
        self.exchange.interact_px = cells
        return gids, boxes

    def _sync_budget(self):
        """the budget 0.05 N^2 counts the particles of ALL ranks (simulation_handler.lua:1752-1753): the sum of what the
        handlers actually hold (hand-overs do not change it; adds and removes mark it stale)"""
        if self.world == 1 or not self._budget_stale:
            return
        from . import _ffi
        nw, ny = self.local.get_n_particles()
        tot = self.torch.tensor([float(nw), float(ny)], dtype=self.torch.float64, device=self.device)
        self.dist.all_reduce(tot, op=self.dist.ReduceOp.SUM)
        nw, ny = (int(v) for v in tot.tolist())
        self.local.set_option(_ffi.OPT_BUDGET_PARTICLES_WHITE, nw)
        self.local.set_option(_ffi.OPT_BUDGET_PARTICLES_YOLK, ny)
        self._budget_stale = False

    HEAD = 7  # gid, target x, y, white radius, yolk radius, white particles, yolk particles

    def _send_batches(self, gids, to):
        """hands the batches `gids` to rank `to`: ONE header message and ONE payload message for all of them.  With the
        wire tensors on the GPU ("nccl" = RCCL) the particle state goes device to device: egg_export_batch writes it
        straight into the tensor RCCL sends, nothing passes through host memory."""
        torch, dist = self.torch, self.dist
        gids = list(gids)
        if not gids:
            return
        on_gpu = str(self.device).startswith("cuda") and hasattr(self.local, "export_batch_to")
        counts = [self.local.get_n_particles(self.local_id[g]) for g in gids] if on_gpu else None
        heads, parts = [], []
        if on_gpu:
            total = sum(self.STATE_FIELDS * (nw + ny) for nw, ny in counts)
            payload = torch.empty(total, dtype=torch.float64, device=self.device)
            off = 0
            for g, (nw, ny) in zip(gids, counts):
                w0, y0 = off, off + self.STATE_FIELDS * nw
                info = self.local.export_batch_to(self.local_id[g], payload.data_ptr() + 8 * w0, payload.data_ptr() + 8 * y0)
                heads += [g, info["target_x"], info["target_y"], info["white_radius"], info["yolk_radius"], nw, ny]
                off = y0 + self.STATE_FIELDS * ny
        else:
            for g in gids:
                info, ws, ys = self.local.export_batch(self.local_id[g])
                heads += [g, info["target_x"], info["target_y"], info["white_radius"], info["yolk_radius"], info["n_white"], info["n_yolk"]]
                parts += [np.asarray(ws, dtype=np.float64).reshape(-1), np.asarray(ys, dtype=np.float64).reshape(-1)]
            payload = torch.from_numpy(np.concatenate(parts)).to(self.device)
        head = torch.tensor(heads, dtype=torch.float64).to(self.device)
        dist.send(head, to)
        dist.send(payload, to)
        self.bytes_handed_over += 8 * (head.numel() + payload.numel())
        for g in gids:
            lid = self.local_id.pop(g)
            del self.global_id[lid]
            self.local.remove(lid)

    def _recv_batches(self, n, frm):
        """receives the `n` batches rank `frm` hands over in this round (the plan told every rank how many)"""
        torch, dist = self.torch, self.dist
        if n == 0:
            return []
        head = torch.zeros(self.HEAD * n, dtype=torch.float64, device=self.device)
        dist.recv(head, frm)
        rows = head.cpu().numpy().reshape(n, self.HEAD)
        total = int(sum(self.STATE_FIELDS * (int(r[5]) + int(r[6])) for r in rows))
        payload = torch.zeros(total, dtype=torch.float64, device=self.device)
        dist.recv(payload, frm)
        on_gpu = str(self.device).startswith("cuda") and hasattr(self.local, "import_batch_from")
        host = None if on_gpu else payload.cpu().numpy()
        got, off = [], 0
        for r in rows:
            gid, nw, ny = int(r[0]), int(r[5]), int(r[6])
            info = dict(key=gid, target_x=float(r[1]), target_y=float(r[2]), white_radius=float(r[3]), yolk_radius=float(r[4]),
                        n_white=nw, n_yolk=ny)
            w0, y0 = off, off + self.STATE_FIELDS * nw
            if on_gpu:
                lid = self.local.import_batch_from(info, payload.data_ptr() + 8 * w0, payload.data_ptr() + 8 * y0)
            else:
                lid = self.local.import_batch(info, host[w0:y0].reshape(self.STATE_FIELDS, nw),
                                              host[y0:y0 + self.STATE_FIELDS * ny].reshape(self.STATE_FIELDS, ny))
            off = y0 + self.STATE_FIELDS * ny
            self.local_id[gid] = lid
            self.global_id[lid] = gid
            got.append(gid)
        return got

    def rebalance(self, max_rounds=None):
        """Before a step: exchange boundary boxes and hand batches over until no local batch is within
        interaction range of another rank's batch.  Conflicts move the higher rank's batch down;
        batches that strayed past the halo of their slab move to the slab they are in."""
        if self.world == 1:
            return 0
        torch, dist = self.torch, self.dist
        moved_total = 0
        for _ in range(max_rounds or 2 * self.world + 2):
            conflicts = self.exchange.exchange(raise_on_conflict=False)
            ids, boxes = self.exchange.last_ids, self.exchange.last_boxes
            lo, hi = self.exchange.slab_lo, self.exchange.slab_hi
            to_left, to_right, want_right = set(), set(), set()
            # batches move as whole ISLANDS (local batches chained by claims less than a cell apart): one member going
            # alone would meet its island-mates across the cut in the next round and come straight back
            island = {int(g): int(g) for g in ids}

            def find(g):
                while island[g] != g:
                    island[g] = island[island[g]]
                    g = island[g]
                return g

            for a, b in self.exchange.conflicts(ids, boxes, ids, boxes, self.exchange.interact_px):
                if a != b:
                    ra, rb = find(int(a)), find(int(b))
                    if ra != rb:
                        island[max(ra, rb)] = min(ra, rb)
            members = {}
            for g in island:
                members.setdefault(find(g), []).append(g)
            for lid_g, ghost, ghost_rank in conflicts:
                if ghost_rank < self.rank:
                    to_left.update(members[find(int(lid_g))])   # the lower rank steps the pair
                else:
                    want_right.add(int(ghost))  # its owner may not see my batch: ask for it
            in_conflict = {find(int(c[0])) for c in conflicts}
            box_of = {int(g): b for g, b in zip(ids, boxes)}
            for root, gs in members.items():
                if root in in_conflict:
                    continue
                # strayed: the whole island lies beyond the halo of this slab -> it belongs to the slab it is in
                if self.rank > 0 and all(max(box_of[g][2], box_of[g][6]) < lo - self.exchange.halo_px for g in gs):
                    to_left.update(gs)
                elif self.rank + 1 < self.world and all(min(box_of[g][0], box_of[g][4]) > hi + self.exchange.halo_px for g in gs):
                    to_right.update(gs)
            # everyone learns every plan: how many batches arrive from whom, and the new owner table
            rows = [[0.0, g] for g in sorted(to_left)] + [[1.0, g] for g in sorted(to_right)] + [[2.0, g] for g in sorted(want_right)]
            parts = self._all_gather_rows(np.array(rows, dtype=np.float64).reshape(-1, 2))
            gathered = [([int(g) for k, g in part if k == 0.0], [int(g) for k, g in part if k == 1.0],
                         [int(g) for k, g in part if k == 2.0]) for part in parts]
            plan = []
            for r, (l, rr, _w) in enumerate(gathered):
                wanted = set(gathered[r - 1][2]) if r > 0 else set()
                l = sorted(set(l) | {g for g in wanted if self.owner.get(g) == r})
                plan.append((l, [g for g in rr if g not in l]))
            to_left, to_right = set(plan[self.rank][0]), set(plan[self.rank][1])
            n_moves = sum(len(l) + len(r) for l, r in plan)
            if n_moves == 0:
                # nothing left to move anywhere: every rank decides TOGETHER whether that is a clean end (a rank that
                # raised alone would leave the others hanging in their next collective)
                bad = torch.tensor([1.0 if conflicts else 0.0], dtype=torch.float64, device=self.device)
                dist.all_reduce(bad, op=dist.ReduceOp.MAX)
                if bad.item() != 0.0:
                    raise SlabConflict("rank %d: unresolved cross-slab pairs %s" % (self.rank, conflicts[:3]))
                return moved_total
            # even ranks send first, odd ranks receive first: neighbour pairs never both block in send
            for phase in (0, 1):
                if self.rank % 2 == phase:
                    self._send_batches(sorted(to_left), self.rank - 1)
                    self._send_batches(sorted(to_right), self.rank + 1)
                else:
                    if self.rank + 1 < self.world:
                        self._recv_batches(len(plan[self.rank + 1][0]), self.rank + 1)
                    if self.rank > 0:
                        self._recv_batches(len(plan[self.rank - 1][1]), self.rank - 1)
            for r, (l, rr) in enumerate(plan):
                for g in l:
                    self.owner[g] = r - 1
                for g in rr:
                    self.owner[g] = r + 1
            moved_total += n_moves
            self.migrations += n_moves
            self._keys_stale = True
        raise SlabConflict("rank %d: batch hand-over did not settle" % self.rank)
