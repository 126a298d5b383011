"""ctypes binding of libeggsim.so (include/eggsim.h).

This is the Python twin of the LuaJIT `ffi.cdef` block in
lua/egg_fluid_simulation/simulation_handler.lua: every call the Lua wrapper makes
goes through the same C entry point here.  There is no fallback: if the shared
library is missing or no HIP device is usable, construction raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# EGGSIM_LIB lets a developer load a diagnostic build (e.g. libeggsim_prof.so); default is the product library
LIB_PATH = os.environ.get("EGGSIM_LIB") or os.path.join(_HERE, "libeggsim.so")

EGG_OK = 0
EGG_WARN_UNKNOWN_ID = 1
EGG_WARN_FEW_PARTICLES = 2
EGG_ERR_UNKNOWN_ID = -1
EGG_ERR_INVALID_ARGUMENT = -2
EGG_ERR_NO_DEVICE = -3
EGG_ERR_DEVICE = -4
EGG_ERR_UNSUPPORTED = -5
EGG_ERR_INTERNAL = -6

WHITE, YOLK = 0, 1
DEFAULT_COUNT = -1  # EGG_DEFAULT_COUNT: the caller gave nil for a particle count

FIELDS = ["x", "y", "vx", "vy", "last_x", "last_y", "radius", "inv_mass", "mass_t", "batch_id"]
FIELD_ID = {n: i for i, n in enumerate(FIELDS)}

OPT_CLAIM_MARGIN_CELLS = 0
OPT_TILE_TARGET_PARTICLES = 1
OPT_TIMING = 2
OPT_FORCE_SINGLE_TILE = 3
OPT_THREADS_PER_PARTICLE = 4
OPT_SPIN_SLEEP = 5
OPT_BUDGET_PARTICLES_WHITE = 6
OPT_BUDGET_PARTICLES_YOLK = 7
OPT_FORCE_GLOBAL_STATE = 8
OPT_FUSE_TYPES = 9
OPT_PACKED = 10
OPT_GROUP_PARTICLES = 11
OPT_LEVEL_WALK = 12
OPT_SOLVER_ORDER = 13  # 0 exact (default), 1 relaxed
OPT_RELAXATION = 14    # omega of the relaxed pass, in (0, 2]
OPT_COHESION = 15      # 0 as the reference: cohesion moves nothing (default), 1 effective (relaxed order only)
OPT_FORCE_CELL_HASH = 16  # test hook: 1 = the LDS hash table keys every tile's cells (exact order only)
SOLVER_EXACT, SOLVER_RELAXED = 0, 1
COHESION_REFERENCE, COHESION_EFFECTIVE = 0, 1
RELAXATION_DEFAULT = 1.8  # EGG_RELAXATION_DEFAULT
PK_VARIANT_LEVELS_INORDER, PK_VARIANT_LEVELS_OOO, PK_VARIANT_EXEC, PK_VARIANT_EXEC_CHAIN, PK_VARIANT_SORT_LDS, PK_VARIANT_SORT_DIRECT = 1, 2, 4, 8, 16, 32
PK_VARIANT_PASS_FUSED = 64
# the eight results egg_selftest_arith_operands returns per operand triple (n, d, x)
ARITH_COLUMNS = ("div", "sqrt", "root", "rroot", "div_root", "op_div", "op_sqrt", "op_div_sqrt")

CONFIG_FIELDS = ["damping", "follow_strength", "cohesion_strength",
                 "cohesion_interaction_distance_factor", "collision_strength",
                 "collision_overlap_factor", "min_mass", "max_mass", "min_radius", "max_radius",
                 "max_collision_fraction", "mass_distribution_variance", "eps"]


class EggConfig(C.Structure):
    _fields_ = [(k, C.c_double) for k in CONFIG_FIELDS]


class EggBatchInfo(C.Structure):
    _fields_ = [("key", C.c_int64), ("target_x", C.c_double), ("target_y", C.c_double), ("white_radius", C.c_double),
                ("yolk_radius", C.c_double), ("n_white", C.c_int64), ("n_yolk", C.c_int64)]


ENVIRONMENT_FIELDS = ("min_x", "min_y", "max_x", "max_y", "centroid_x", "centroid_y", "max_radius", "max_velocity",
                      "last_centroid_x", "last_centroid_y")


class EggEnvironment(C.Structure):  # egg_environment
    _fields_ = [(k, C.c_double) for k in ENVIRONMENT_FIELDS]


class EggStats(C.Structure):
    _fields_ = [("steps", C.c_int64), ("pair_solves", C.c_int64), ("follow_solves", C.c_int64),
                ("kernel_launches", C.c_int64), ("retiles", C.c_int64), ("redo_steps", C.c_int64),
                ("n_tiles", C.c_int64 * 2), ("max_tile_particles", C.c_int64 * 2),
                ("last_step_kernel_ms", C.c_double), ("single_tile", C.c_int64 * 2),
                ("kernel_ms", C.c_double * 2), ("kernel_ms_sum", C.c_double * 2), ("timed_steps", C.c_int64),
                ("max_pass_visits", C.c_int64 * 2), ("budget", C.c_double * 2), ("fused_launch", C.c_int64),
                ("packed", C.c_int64 * 2), ("pk_kernel_ms", (C.c_double * 10) * 2), ("pk_kernel_launches", (C.c_int64 * 10) * 2),
                ("host_ms", C.c_double * 3), ("max_levels", C.c_int64 * 2), ("pk_variants", C.c_int64 * 2),
                ("relaxed_steps", C.c_int64), ("cohesion_solves", C.c_int64),
                ("cell_hash", C.c_int64 * 2)]


class EggRenderConfig(C.Structure):  # egg_render_config
    _fields_ = [("color", C.c_float * 4), ("outline_color", C.c_float * 4), ("outline_thickness", C.c_double),
                ("highlight_strength", C.c_double), ("shadow_strength", C.c_double), ("texture_scale", C.c_double),
                ("motion_blur", C.c_double)]


class EggRenderParams(C.Structure):  # egg_render_params
    _fields_ = [("screen_w", C.c_int32), ("screen_h", C.c_int32), ("origin_x", C.c_double), ("origin_y", C.c_double),
                ("interpolation_alpha", C.c_double), ("threshold", C.c_double), ("smoothness", C.c_double),
                ("use_instancing", C.c_int32), ("canvas_w", C.c_int32 * 2), ("canvas_h", C.c_int32 * 2),
                ("clear", C.c_float * 4)]


class EggCollider(C.Structure):  # egg_collider: a static collider of the relaxed pass (40 bytes)
    _fields_ = [("kind", C.c_int32), ("type_mask", C.c_int32), ("p", C.c_double * 4)]


class EggColliderSurface(C.Structure):  # egg_collider_surface: friction and surface velocity of a collider (24 bytes)
    _fields_ = [("friction", C.c_double), ("vx", C.c_double), ("vy", C.c_double)]


class EggColliderMotion(C.Structure):  # egg_collider_motion: the rigid velocity of a collider (16 bytes)
    _fields_ = [("vx", C.c_double), ("vy", C.c_double)]


class EggColliderSpin(C.Structure):  # egg_collider_spin: the pivot and angular velocity of a collider (24 bytes)
    _fields_ = [("px", C.c_double), ("py", C.c_double), ("omega", C.c_double)]


class EggColliderLoad(C.Structure):  # egg_collider_load: the impulse and torque a collider received in a step (24 bytes)
    _fields_ = [("jx", C.c_double), ("jy", C.c_double), ("torque", C.c_double)]


class EggColliderBody(C.Structure):  # egg_collider_body: a collider the device integrates from its own loads (48 bytes)
    _fields_ = [("inv_mass", C.c_double), ("inv_inertia", C.c_double), ("ax", C.c_double), ("ay", C.c_double),
                ("drag", C.c_double), ("spin_drag", C.c_double)]


class EggColliderStyle(C.Structure):  # egg_collider_style: how the headless renderer draws a collider (40 bytes)
    _fields_ = [("fill", C.c_float * 4), ("line", C.c_float * 4), ("line_width", C.c_float), ("layer", C.c_int32)]


COLLIDER_LAYERS = {"under": 0, "over": 1}  # egg_collider_style.layer
class EggColliderContact(C.Structure):  # egg_collider_contact: a collider that meets the other colliders (16 bytes)
    _fields_ = [("restitution", C.c_double), ("on", C.c_int32), ("reserved", C.c_int32)]


COLLIDER_LOAD_IMPULSE_SCALE = 1048576.0  # EGG_COLLIDER_LOAD_IMPULSE_SCALE, 2^20
COLLIDER_LOAD_TORQUE_SCALE = 1024.0      # EGG_COLLIDER_LOAD_TORQUE_SCALE, 2^10
MAX_COLLIDERS = 64  # EGG_MAX_COLLIDERS
COLLIDER_HALF_PLANE, COLLIDER_DISC, COLLIDER_CONTAINER, COLLIDER_SEGMENT = 0, 1, 2, 3
COLLIDER_KINDS = ("half_plane", "disc", "container", "segment")  # by EGG_COLLIDER_* value: the kinds 0 .. 3
COLLIDER_PARAMS = (("nx", "ny", "off"), ("cx", "cy", "R"), ("cx", "cy", "R"), ("x0", "y0", "x1", "y1"))
COLLIDER_WALL = 5  # EGG_COLLIDER_WALL: a segment that sweeps the sub-step's path (4 is not a kind and stays refused)
# every kind, the wall included: name -> EGG_COLLIDER_* value, value -> name, value -> parameter names
COLLIDER_CODES = dict({n: i for i, n in enumerate(COLLIDER_KINDS)}, wall=COLLIDER_WALL)
COLLIDER_NAMES = {v: n for n, v in COLLIDER_CODES.items()}
COLLIDER_PARAM_NAMES = dict(enumerate(COLLIDER_PARAMS))
COLLIDER_PARAM_NAMES[COLLIDER_WALL] = COLLIDER_PARAMS[COLLIDER_SEGMENT]
COLLIDER_TYPES = {"white": 1, "yolk": 2, "both": 3}  # type_mask


class EggForce(C.Structure):  # egg_force: a force field of the relaxed step (40 bytes)
    _fields_ = [("kind", C.c_int32), ("type_mask", C.c_int32), ("p", C.c_double * 4)]


MAX_FORCES = 16  # EGG_MAX_FORCES
FORCE_UNIFORM, FORCE_RADIAL, FORCE_VORTEX = 0, 1, 2
FORCE_KINDS = ("uniform", "radial", "vortex")  # by EGG_FORCE_* value
FORCE_PARAMS = (("gx", "gy"), ("cx", "cy", "strength", "R"), ("cx", "cy", "strength", "R"))
FORCE_TYPES = COLLIDER_TYPES  # type_mask


class EggSensor(C.Structure):  # egg_sensor: a region whose particles a read counts and locates (56 bytes)
    _fields_ = [("kind", C.c_int32), ("type_mask", C.c_int32), ("p", C.c_double * 6)]


class EggSensorReading(C.Structure):  # egg_sensor_reading: int64 count and quantised position sums, [0] white, [1] yolk (48 bytes)
    _fields_ = [("count", C.c_int64 * 2), ("sx", C.c_int64 * 2), ("sy", C.c_int64 * 2)]


MAX_SENSORS = 64  # EGG_MAX_SENSORS
SENSOR_POSITION_SCALE = 65536.0  # EGG_SENSOR_POSITION_SCALE, 2^16
SENSOR_HALF_PLANE, SENSOR_DISC, SENSOR_BOX, SENSOR_CAPSULE = 0, 1, 2, 3
SENSOR_KINDS = ("half_plane", "disc", "box", "capsule")  # by EGG_SENSOR_* value
# the parameters as stored; the wrappers also take a box as (cx, cy, hx, hy, angle) and convert with the host's cos / sin
SENSOR_PARAMS = (("nx", "ny", "off"), ("cx", "cy", "R"), ("cx", "cy", "hx", "hy", "ux", "uy"), ("x0", "y0", "x1", "y1", "R"))
SENSOR_CODES = {n: i for i, n in enumerate(SENSOR_KINDS)}
SENSOR_TYPES = COLLIDER_TYPES  # type_mask


class EggProbeQuery(C.Structure):  # egg_probe_query: a point or a ray whose one winning particle per type a call reports (48 bytes)
    _fields_ = [("kind", C.c_int32), ("type_mask", C.c_int32), ("p", C.c_double * 5)]


class EggProbeHit(C.Structure):  # egg_probe_hit: the winner of one (probe, type), all zeros while found == 0 (56 bytes)
    _fields_ = [("id", C.c_int64), ("key", C.c_int64), ("index", C.c_int32), ("found", C.c_int32), ("score", C.c_double),
                ("x", C.c_double), ("y", C.c_double), ("radius", C.c_double)]


MAX_PROBES = 64  # EGG_MAX_PROBES
PROBE_POINT, PROBE_RAY = 0, 1
PROBE_KINDS = ("point", "ray")  # by EGG_PROBE_* value
PROBE_PARAMS = (("x", "y", "reach"), ("x0", "y0", "x1", "y1", "pad"))
PROBE_DEFAULTS = ((float("inf"),), (0.0,))  # reach, pad: the trailing parameters a tuple may leave out
PROBE_CODES = {n: i for i, n in enumerate(PROBE_KINDS)}
PROBE_TYPES = dict(COLLIDER_TYPES)  # type_mask by name; the wrappers take the mask itself (1, 2, 3) as well


class EggFieldSpec(C.Structure):  # egg_field_spec: the grid of one call, nx x ny square cells from (x0, y0) (40 bytes)
    _fields_ = [("x0", C.c_double), ("y0", C.c_double), ("cell", C.c_double), ("nx", C.c_int32), ("ny", C.c_int32),
                ("type_mask", C.c_int32), ("path", C.c_int32)]


class EggFieldPlanes(C.Structure):  # egg_field_planes: int32 count and int64 svx / svy, each [2][ny][nx]; svx / svy both or neither
    _fields_ = [("count", C.c_void_p), ("svx", C.c_void_p), ("svy", C.c_void_p)]


class EggFieldTotals(C.Structure):  # egg_field_totals: particles per type by fate, and the units of each path (56 bytes)
    _fields_ = [("inside", C.c_int64 * 2), ("outside", C.c_int64 * 2), ("dropped", C.c_int64 * 2), ("units_tiled", C.c_int32),
                ("units_direct", C.c_int32)]


FIELD_MAX_CELLS = 1 << 20  # EGG_FIELD_MAX_CELLS: nx * ny
FIELD_VELOCITY_SCALE = 65536.0  # EGG_FIELD_VELOCITY_SCALE, 2^16
FIELD_PATH_AUTO, FIELD_PATH_DIRECT = 0, 1
FIELD_PATHS = {"auto": FIELD_PATH_AUTO, "direct": FIELD_PATH_DIRECT}  # direct: test hook, every unit adds particle by particle
FIELD_TYPES = dict(COLLIDER_TYPES)  # type_mask by name; the wrappers take the mask itself (1, 2, 3) as well


class EggPiecesSpec(C.Structure):  # egg_pieces_spec: the reach per type in units of (radius[i] + radius[j]) and the type mask (24 bytes)
    _fields_ = [("reach", C.c_double * 2), ("type_mask", C.c_int32), ("reserved", C.c_int32)]


class EggPieceSummary(C.Structure):  # egg_piece_summary: the pieces of one atom and its body's position sums (40 bytes)
    _fields_ = [("n", C.c_int32), ("pieces", C.c_int32), ("largest", C.c_int32), ("first", C.c_int32), ("singles", C.c_int32),
                ("dropped", C.c_int32), ("sx", C.c_int64), ("sy", C.c_int64)]


PIECES_MAX_ATOM = 4096  # EGG_PIECES_MAX_ATOM: particles of one type of one batch
PIECES_TYPES = dict(COLLIDER_TYPES)  # type_mask by name; the wrappers take the mask itself (1, 2, 3) as well


class EggImpulse(C.Structure):  # egg_impulse_record: a region, what happens to the velocities inside it, and the batch it is for (96 bytes)
    _fields_ = [("region", EggSensor), ("action", C.c_int32), ("flags", C.c_int32), ("id", C.c_int64), ("a", C.c_double * 3)]


class EggImpulseResult(C.Structure):  # egg_impulse_result: per type the accepted edits, their int64 sums and the skipped ones (64 bytes)
    _fields_ = [("count", C.c_int64 * 2), ("sdvx", C.c_int64 * 2), ("sdvy", C.c_int64 * 2), ("skipped", C.c_int64 * 2)]


MAX_IMPULSES = 64  # EGG_MAX_IMPULSES
IMPULSE_SCALE = 65536.0  # EGG_IMPULSE_SCALE, 2^16
IMPULSE_ALL_BATCHES, IMPULSE_NO_BATCH = -1, -2  # EGG_IMPULSE_ALL_BATCHES, EGG_IMPULSE_NO_BATCH
IMPULSE_KICK, IMPULSE_BLAST, IMPULSE_SWIRL, IMPULSE_BRAKE = 0, 1, 2, 3
IMPULSE_ACTIONS = ("kick", "blast", "swirl", "brake")  # by EGG_IMPULSE_* value
IMPULSE_PARAMS = (("ax", "ay"), ("cx", "cy", "s"), ("cx", "cy", "omega"), ("ux", "uy", "k"))
IMPULSE_CODES = {n: i for i, n in enumerate(IMPULSE_ACTIONS)}
IMPULSE_LINEAR, IMPULSE_BY_INV_MASS = 1, 2  # flag bits


class EggMeasureSpec(C.Structure):  # egg_measure_spec: the region (read with EGG_MEASURE_REGION only), the flags and the type mask (64 bytes)
    _fields_ = [("region", EggSensor), ("flags", C.c_int32), ("type_mask", C.c_int32)]


# egg_measure_record, field for field: 24 int64 (192 bytes)
MEASURE_FIELDS = ("atom", "n", "dropped", "sx", "sy", "sm", "smx", "smy", "spx", "spy", "se", "lo_x", "lo_y", "hi_x", "hi_y", "max_v2",
                  "ox_q", "oy_q", "dropped_central", "sxx", "sxy", "syy", "sl", "max_reach")


class EggMeasureRecord(C.Structure):
    _fields_ = [(name, C.c_int64) for name in MEASURE_FIELDS]


MEASURE_SCALE = 65536.0  # EGG_MEASURE_SCALE, 2^16
MEASURE_MASS_SCALE = 4294967296.0  # EGG_MEASURE_MASS_SCALE, 2^32
MEASURE_REGION = 1  # EGG_MEASURE_REGION: flag bit


class EggCoverSpec(C.Structure):  # egg_cover_spec: the grid of one call, the factor on the radii, the types and the path (48 bytes)
    _fields_ = [("x0", C.c_double), ("y0", C.c_double), ("cell", C.c_double), ("scale", C.c_double), ("nx", C.c_int32), ("ny", C.c_int32),
                ("type_mask", C.c_int32), ("path", C.c_int32)]


class EggCoverPlanes(C.Structure):  # egg_cover_planes: int32 cover and int32 owner (or NULL), each [2][ny][nx] (16 bytes)
    _fields_ = [("cover", C.c_void_p), ("owner", C.c_void_p)]


class EggCoverTotals(C.Structure):  # egg_cover_totals: particles per type by fate, covered cells, and the units of each path (112 bytes)
    _fields_ = [("inside", C.c_int64 * 2), ("outside", C.c_int64 * 2), ("dropped", C.c_int64 * 2), ("hits", C.c_int64 * 2),
                ("covered", C.c_int64 * 2), ("covered_both", C.c_int64), ("covered_any", C.c_int64), ("units_lanes", C.c_int32),
                ("units_wave", C.c_int32), ("units_direct", C.c_int32), ("reserved", C.c_int32)]


COVER_MAX_CELLS = 1 << 20  # EGG_COVER_MAX_CELLS: nx * ny
COVER_MAX_SPAN = 64.0  # EGG_COVER_MAX_SPAN: scale * radius / cell
COVER_OWNER_KEYS = 0x100  # EGG_COVER_OWNER_KEYS: flag bit of spec.path, the owner plane holds keys in place of ids
COVER_PATHS = {"auto": 0, "direct": 1, "lanes": 2, "wave": 3}  # EGG_COVER_PATH_*; all but auto are test hooks


class EggTouchSpec(C.Structure):  # egg_touch_spec: the reach per type in units of (ra + rb), the type mask and the flags (24 bytes)
    _fields_ = [("reach", C.c_double * 2), ("type_mask", C.c_int32), ("flags", C.c_int32)]


class EggTouchQuery(C.Structure):  # egg_touch_query: the key a query leaves out (-1: none), its type and its number of discs (16 bytes)
    _fields_ = [("key", C.c_int64), ("type", C.c_int32), ("count", C.c_int32)]


class EggTouchRecord(C.Structure):  # egg_touch_record: one (slot, other batch) with a touching pair (40 bytes)
    _fields_ = [("slot", C.c_int32), ("pairs", C.c_int32), ("particles", C.c_int32), ("dropped", C.c_int32), ("other", C.c_int64),
                ("sx", C.c_int64), ("sy", C.c_int64)]


TOUCH_BY_KEYS = 1  # EGG_TOUCH_BY_KEYS: flag bit of spec.flags, `other` and the queries' keys are batch keys in place of ids
TOUCH_MAX_QUERY = 1 << 20  # EGG_TOUCH_MAX_QUERY: discs of one query


class EggRxBox(C.Structure):  # egg_rx_box: a cell box of the relaxed halo between processes
    _fields_ = [("lo_x", C.c_int32), ("lo_y", C.c_int32), ("hi_x", C.c_int32), ("hi_y", C.c_int32), ("empty", C.c_int32)]


RX_BOX_INTS = 5        # int32 fields of egg_rx_box
RX_VISCOSITY_PASS = 0x40000000  # EGG_RX_VISCOSITY_PASS: + sub addresses the viscosity pass of sub-step sub
RX_RECORD_WORDS = 5    # 64-bit words of a ghost record: x, y, inverse mass, radius (doubles), global key (int64; with
                       # effective cohesion the batch tag in its upper 32 bits)
RX_RECORD_BYTES = 40

# the draw record of a particle (egg_draw_pack, egg_draw_source_*): a message is double[7][n] in this field order
DRAW_FIELDS = ("x", "y", "last_x", "last_y", "vx", "vy", "radius")
DRAW_RECORD_BYTES = 56

PK_KINDS = ["egg_pk_begin_kernel", "egg_pk_mid_kernel", "egg_pk_lists_fresh_kernel", "egg_pk_lists_stale_kernel",
            "egg_pk_levels_kernel", "egg_pk_sort_kernel", "egg_pk_exec_kernel", "egg_pk_end_kernel", "egg_pk_reduce_kernel",
            "egg_pk_pass_kernel"]


# every symbol include/eggsim.h declares, with its signature
_SIGNATURES = {
    "egg_default_config": (C.c_int, [C.c_int, C.POINTER(EggConfig)]),
    "egg_create": (C.c_int, [C.POINTER(EggConfig), C.POINTER(EggConfig), C.c_int, C.POINTER(C.c_void_p)]),
    "egg_destroy": (None, [C.c_void_p]),
    "egg_last_error": (C.c_char_p, [C.c_void_p]),
    "egg_set_config": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(EggConfig)]),
    "egg_get_config": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(EggConfig)]),
    "egg_add": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int64, C.c_int64,
                          C.POINTER(C.c_int64)]),
    "egg_add_many": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_double, C.c_double,
                               C.c_int64, C.c_int64, C.c_void_p]),
    "egg_add_many_keyed": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_double, C.c_double,
                                     C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "egg_export_batch": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(EggBatchInfo), C.c_void_p, C.c_void_p]),
    "egg_import_batch": (C.c_int, [C.c_void_p, C.POINTER(EggBatchInfo), C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]),
    "egg_group_create": (C.c_int, [C.POINTER(EggConfig), C.POINTER(EggConfig), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_void_p)]),
    "egg_group_destroy": (None, [C.c_void_p]),
    "egg_group_last_error": (C.c_char_p, [C.c_void_p]),
    "egg_group_n_devices": (C.c_int32, [C.c_void_p]),
    "egg_group_handle": (C.c_void_p, [C.c_void_p, C.c_int32]),
    "egg_group_set_halo": (C.c_int, [C.c_void_p, C.c_double]),
    "egg_group_add": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int64, C.c_int64, C.POINTER(C.c_int64)]),
    "egg_group_remove": (C.c_int, [C.c_void_p, C.c_int64]),
    "egg_group_set_target": (C.c_int, [C.c_void_p, C.c_int64, C.c_double, C.c_double]),
    "egg_group_get_position": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "egg_group_update": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "egg_group_step": (C.c_int, [C.c_void_p, C.c_double, C.c_int32, C.c_int32]),
    "egg_group_owner": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "egg_group_get_counters": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "egg_group_set_solver_order": (C.c_int, [C.c_void_p, C.c_int32, C.c_double]),
    "egg_group_set_cohesion": (C.c_int, [C.c_void_p, C.c_int32]),
    "egg_set_colliders": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggCollider)]),
    "egg_get_colliders": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggCollider), C.POINTER(C.c_int32)]),
    "egg_get_collider_hits": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "egg_set_collider_surfaces": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggColliderSurface)]),
    "egg_get_collider_surfaces": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggColliderSurface), C.POINTER(C.c_int32)]),
    "egg_get_collider_grips": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "egg_set_collider_motion": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggColliderMotion)]),
    "egg_get_collider_motion": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggColliderMotion), C.POINTER(C.c_int32)]),
    "egg_group_set_collider_motion": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggColliderMotion)]),
    "egg_group_get_collider_motion": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggColliderMotion), C.POINTER(C.c_int32)]),
    "egg_set_collider_spin": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggColliderSpin)]),
    "egg_get_collider_spin": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggColliderSpin), C.POINTER(C.c_int32)]),
    "egg_group_set_collider_spin": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggColliderSpin)]),
    "egg_group_get_collider_spin": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggColliderSpin), C.POINTER(C.c_int32)]),
    "egg_set_collider_styles": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggColliderStyle)]),
    "egg_get_collider_styles": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggColliderStyle), C.POINTER(C.c_int32)]),
    "egg_get_collider_pose": (C.c_int, [C.c_void_p, C.c_double, C.c_int32, C.POINTER(EggCollider), C.POINTER(C.c_int32)]),
    "egg_group_set_collider_styles": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggColliderStyle)]),
    "egg_group_get_collider_styles": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggColliderStyle), C.POINTER(C.c_int32)]),
    "egg_group_get_collider_pose": (C.c_int, [C.c_void_p, C.c_double, C.c_int32, C.POINTER(EggCollider), C.POINTER(C.c_int32)]),
    "egg_set_collider_loads": (C.c_int, [C.c_void_p, C.c_int]),
    "egg_get_collider_loads_enabled": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "egg_get_collider_load_sums": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double),
                                             C.POINTER(C.c_int32)]),
    "egg_get_collider_loads": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggColliderLoad), C.POINTER(C.c_int32)]),
    "egg_set_collider_bodies": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggColliderBody)]),
    "egg_get_collider_bodies": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggColliderBody), C.POINTER(C.c_int32)]),
    "egg_set_collider_contacts": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggColliderContact), C.c_int32]),
    "egg_get_collider_contacts": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggColliderContact), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "egg_get_collider_contact_solves": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "egg_group_set_collider_loads": (C.c_int, [C.c_void_p, C.c_int]),
    "egg_group_get_collider_load_sums": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double),
                                                   C.POINTER(C.c_int32)]),
    "egg_group_get_collider_loads": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggColliderLoad), C.POINTER(C.c_int32)]),
    "egg_set_sensors": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggSensor)]),
    "egg_get_sensors": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggSensor), C.POINTER(C.c_int32)]),
    "egg_read_sensors": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggSensorReading), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "egg_read_sensor_batches": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "egg_probe": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggProbeQuery), C.POINTER(EggProbeHit)]),
    "egg_group_probe": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggProbeQuery), C.POINTER(EggProbeHit)]),
    "egg_field": (C.c_int, [C.c_void_p, C.POINTER(EggFieldSpec), C.POINTER(EggFieldPlanes), C.POINTER(EggFieldTotals)]),
    "egg_field_to": (C.c_int, [C.c_void_p, C.POINTER(EggFieldSpec), C.POINTER(EggFieldPlanes), C.POINTER(EggFieldTotals)]),
    "egg_group_field": (C.c_int, [C.c_void_p, C.POINTER(EggFieldSpec), C.POINTER(EggFieldPlanes), C.POINTER(EggFieldTotals)]),
    "egg_pieces": (C.c_int, [C.c_void_p, C.POINTER(EggPiecesSpec), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "egg_group_pieces": (C.c_int, [C.c_void_p, C.POINTER(EggPiecesSpec), C.c_int64, C.c_void_p, C.c_void_p]),
    "egg_group_set_sensors": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggSensor)]),
    "egg_group_get_sensors": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggSensor), C.POINTER(C.c_int32)]),
    "egg_group_read_sensors": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggSensorReading), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "egg_group_read_sensor_batches": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "egg_group_set_collider_surfaces": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggColliderSurface)]),
    "egg_group_get_collider_surfaces": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggColliderSurface), C.POINTER(C.c_int32)]),
    "egg_group_get_collider_grips": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "egg_group_set_colliders": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggCollider)]),
    "egg_group_get_colliders": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggCollider), C.POINTER(C.c_int32)]),
    "egg_group_get_collider_hits": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "egg_set_forces": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggForce)]),
    "egg_get_forces": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggForce), C.POINTER(C.c_int32)]),
    "egg_group_set_forces": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggForce)]),
    "egg_group_get_forces": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggForce), C.POINTER(C.c_int32)]),
    "egg_set_viscosity": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "egg_get_viscosity": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "egg_get_viscosity_pairs": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "egg_set_coupling": (C.c_int, [C.c_void_p, C.c_double, C.c_double]),
    "egg_get_coupling": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "egg_get_coupling_solves": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "egg_set_adhesion": (C.c_int, [C.c_void_p, C.c_double, C.c_double]),
    "egg_get_adhesion": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "egg_get_adhesion_solves": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "egg_set_containment": (C.c_int, [C.c_void_p, C.c_double, C.c_double]),
    "egg_get_containment": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "egg_get_containment_hits": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "egg_group_set_containment": (C.c_int, [C.c_void_p, C.c_double, C.c_double]),
    "egg_group_get_containment": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "egg_group_get_containment_hits": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "egg_group_set_viscosity": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "egg_group_get_viscosity": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "egg_group_get_viscosity_pairs": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "egg_group_get_halo_counters": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "egg_group_set_config": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(EggConfig)]),
    "egg_group_get_config": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(EggConfig)]),
    "egg_group_get_target": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "egg_group_list_ids": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_int64)]),
    "egg_group_get_n_particles": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "egg_group_get_elapsed": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "egg_group_download_particles": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64]),
    "egg_group_get_environment": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(EggEnvironment)]),
    "egg_group_set_render_config": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(EggRenderConfig)]),
    "egg_group_get_render_config": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(EggRenderConfig)]),
    "egg_group_set_render_flags": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "egg_group_set_add_color": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double]),
    "egg_group_set_color": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double]),
    "egg_group_render": (C.c_int, [C.c_void_p, C.POINTER(EggRenderParams), C.c_void_p]),
    "egg_group_render_canvas": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                          C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "egg_remove": (C.c_int, [C.c_void_p, C.c_int64]),
    "egg_set_target": (C.c_int, [C.c_void_p, C.c_int64, C.c_double, C.c_double]),
    "egg_set_targets_many": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "egg_get_target": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "egg_update": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "egg_step": (C.c_int, [C.c_void_p, C.c_double, C.c_int32, C.c_int32]),
    "egg_prepare_step": (C.c_int, [C.c_void_p, C.c_double, C.c_int32, C.c_int32]),
    "egg_step_begin": (C.c_int, [C.c_void_p, C.c_double, C.c_int32, C.c_int32]),
    "egg_step_end": (C.c_int, [C.c_void_p, C.c_int32]),
    "egg_step_peek_visits": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64 * 2), C.POINTER(C.c_double * 2)]),
    "egg_synchronize": (C.c_int, [C.c_void_p]),
    "egg_get_position": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "egg_get_positions_many": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "egg_get_bounds_many": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "egg_get_claims_many": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "egg_get_n_particles": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "egg_list_ids": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_int64)]),
    "egg_get_elapsed": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "egg_download_particles": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64]),
    "egg_selftest_arith": (C.c_int, [C.c_void_p, C.c_int64, C.c_uint64, C.POINTER(C.c_int64)]),
    "egg_selftest_arith_operands": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "egg_get_stats": (C.c_int, [C.c_void_p, C.POINTER(EggStats)]),
    "egg_get_environment": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(EggEnvironment)]),
    "egg_set_option": (C.c_int, [C.c_void_p, C.c_int, C.c_double]),
    "egg_default_render_config": (C.c_int, [C.c_int, C.POINTER(EggRenderConfig)]),
    "egg_set_render_config": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(EggRenderConfig)]),
    "egg_get_render_config": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(EggRenderConfig)]),
    "egg_set_render_flags": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "egg_set_add_color": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double]),
    "egg_set_color": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double]),
    "egg_default_render_params": (C.c_int, [C.POINTER(EggRenderParams)]),
    "egg_render": (C.c_int, [C.c_void_p, C.POINTER(EggRenderParams), C.c_void_p]),
    "egg_render_canvas": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                    C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "egg_render_particle_texture": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int32)]),
    "egg_rx_set_keys": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64]),
    "egg_rx_begin": (C.c_int, [C.c_void_p, C.c_double, C.c_int32, C.c_int32]),
    "egg_rx_substep": (C.c_int, [C.c_void_p, C.c_int32]),
    "egg_rx_get_boxes": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "egg_rx_pack": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "egg_rx_fetch": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "egg_rx_run_pass": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "egg_rx_check": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64 * 2), C.POINTER(C.c_int64)]),
    "egg_rx_end": (C.c_int, [C.c_void_p, C.c_int32]),
    "egg_draw_pack": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]),
    "egg_draw_source_layout": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "egg_draw_source_place": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "egg_draw_source_render": (C.c_int, [C.c_void_p, C.POINTER(EggRenderParams), C.POINTER(EggRenderConfig), C.c_int32, C.c_int32,
                                         C.c_int32, C.c_double, C.c_void_p]),
    "egg_draw_source_render_canvas": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                                C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "egg_draw_source_environment": (C.c_int, [C.c_void_p, C.c_int, C.c_int32, C.POINTER(EggEnvironment)]),
    "egg_draw_source_download": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64]),
    "egg_draw_source_instances": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "egg_get_instances": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_uint64)]),
    "egg_instances_begin": (C.c_int, [C.c_void_p, C.c_int32]),
    "egg_instances_end": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                    C.POINTER(C.c_uint64)]),
    "egg_group_get_instances": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64),
                                          C.POINTER(C.c_uint64)]),
}

EXPORTED_SYMBOLS = sorted(_SIGNATURES)
# the entry points of include/eggsim_impulse.h, the header include/eggsim.h brings along: with them the library exports 175
_IMPULSE_SIGNATURES = {
    "egg_impulse": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggImpulse), C.POINTER(EggImpulseResult)]),
    "egg_group_impulse": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(EggImpulse), C.POINTER(EggImpulseResult)]),
}
IMPULSE_SYMBOLS = sorted(_IMPULSE_SIGNATURES)
# the entry points of include/eggsim_measure.h, brought along the same way: with them the library exports 178
_MEASURE_SIGNATURES = {
    "egg_measure": (C.c_int, [C.c_void_p, C.POINTER(EggMeasureSpec), C.c_int64, C.c_void_p, C.c_void_p]),
    "egg_measure_to": (C.c_int, [C.c_void_p, C.POINTER(EggMeasureSpec), C.c_int64, C.c_void_p, C.c_void_p, C.c_int64]),
    "egg_group_measure": (C.c_int, [C.c_void_p, C.POINTER(EggMeasureSpec), C.c_int64, C.c_void_p, C.c_void_p]),
}
MEASURE_SYMBOLS = sorted(_MEASURE_SIGNATURES)
# the entry points of include/eggsim_cover.h, brought along the same way: with them the library exports 181
_COVER_SIGNATURES = {
    "egg_cover": (C.c_int, [C.c_void_p, C.POINTER(EggCoverSpec), C.POINTER(EggCoverPlanes), C.POINTER(EggCoverTotals)]),
    "egg_cover_to": (C.c_int, [C.c_void_p, C.POINTER(EggCoverSpec), C.POINTER(EggCoverPlanes), C.POINTER(EggCoverTotals)]),
    "egg_group_cover": (C.c_int, [C.c_void_p, C.POINTER(EggCoverSpec), C.POINTER(EggCoverPlanes), C.POINTER(EggCoverTotals)]),
}
COVER_SYMBOLS = sorted(_COVER_SIGNATURES)
# the entry points of include/eggsim_touch.h, brought along the same way: with them the library exports 184
_TOUCH_SIGNATURES = {
    "egg_touches": (C.c_int, [C.c_void_p, C.POINTER(EggTouchSpec), C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_int64)]),
    "egg_touches_of": (C.c_int, [C.c_void_p, C.POINTER(EggTouchSpec), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                 C.c_void_p, C.POINTER(C.c_int64)]),
    "egg_group_touches": (C.c_int, [C.c_void_p, C.POINTER(EggTouchSpec), C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_int64)]),
}
TOUCH_SYMBOLS = sorted(_TOUCH_SIGNATURES)

_lib = None


class LibraryMissing(RuntimeError):
    pass


def load():
    """Load libeggsim.so.  Raises LibraryMissing (no CPU fallback exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LibraryMissing(
                "libeggsim.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C egg_fluid_simulation_amd/csrc` (needs hipcc; the solver has no CPU path)")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in list(_SIGNATURES.items()) + list(_IMPULSE_SIGNATURES.items()) + list(_MEASURE_SIGNATURES.items()) + \
                list(_COVER_SIGNATURES.items()) + list(_TOUCH_SIGNATURES.items()):
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib
