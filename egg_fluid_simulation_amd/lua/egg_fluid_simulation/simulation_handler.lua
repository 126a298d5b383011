--- Drop-in replacement for egg_fluid_simulation/simulation_handler.lua whose particle
--- solver runs on an AMD MI355X through libeggsim.so (include/eggsim.h).
---
--- NOT EXECUTED IN THIS PIPELINE: no Lua / LuaJIT interpreter exists in the build or GPU image
--- (SURVEY.md 8c).  The file is kept thin and declarative; every FFI call it makes is mirrored
--- one-to-one by egg_fluid_simulation_amd/simulation_handler.py over ctypes, which IS tested.
---
--- Surface kept from the reference (same names, argument order, defaults, warnings, errors):
---   SimulationHandler(white_config, yolk_config), :add, :remove, :update, :set_target_position,
---   :get_target_position, :get_position, :set_white_config/:set_yolk_config, :get_*_config,
---   :list_ids, :get_n_particles, :set_white_color, :set_yolk_color.  In a LOVE host :draw stays with the reference's
---   own shaders: :instances() returns the data mesh and the colour mesh of a type as the reference's vertex format lays
---   them out (packed on the device, one call per frame; :get_instance_data() is the older per-field form) and
---   :get_environment() what sizes and places the canvases.  Without a window, :render_to_image() runs the same
---   passes as HIP kernels (include/eggsim.h, "headless renderer") into a float32 RGBA buffer.

local prefix = "egg_fluid_simulation"
require(string.gsub(prefix .. "/math", "[/\\]", "."))
local log = require(string.gsub(prefix .. "/log", "[/\\]", "."))
local ffi = require("ffi")

ffi.cdef[[
typedef struct egg_handle egg_handle;
typedef struct {
    double damping, follow_strength, cohesion_strength, cohesion_interaction_distance_factor,
           collision_strength, collision_overlap_factor, min_mass, max_mass, min_radius, max_radius,
           max_collision_fraction, mass_distribution_variance, eps;
} egg_config;
int egg_create(const egg_config *white, const egg_config *yolk, int device, egg_handle **out);
void egg_destroy(egg_handle *h);
const char *egg_last_error(const egg_handle *h);
int egg_set_config(egg_handle *h, int which, const egg_config *cfg);
int egg_add(egg_handle *h, double x, double y, double white_radius, double yolk_radius,
            int64_t white_n, int64_t yolk_n, int64_t *out_id);
int egg_remove(egg_handle *h, int64_t id);
int egg_set_target(egg_handle *h, int64_t id, double x, double y);
int egg_get_target(const egg_handle *h, int64_t id, double *x, double *y);
int egg_update(egg_handle *h, double delta, double step_delta, int32_t n_substeps,
               int32_t n_collision_steps, int32_t *out_n_steps);
int egg_get_position(egg_handle *h, int64_t id, double *x, double *y);
int egg_get_n_particles(const egg_handle *h, int64_t id, int64_t *n_white, int64_t *n_yolk);
int egg_list_ids(const egg_handle *h, int64_t cap, int64_t *ids, int64_t *n);
int egg_download_particles(egg_handle *h, int which, int field, double *dst, int64_t cap);
typedef struct { float x, y, last_x, last_y, vx, vy, radius; } egg_instance;
int egg_get_instances(egg_handle *h, int which, egg_instance *data, float *color, int64_t cap, int64_t *n,
                      uint64_t *color_version);
int egg_instances_begin(egg_handle *h, int32_t type_mask);
int egg_instances_end(egg_handle *h, int which, const egg_instance **data, const float **color, int64_t *n,
                      uint64_t *color_version);
typedef struct { double min_x, min_y, max_x, max_y, centroid_x, centroid_y, max_radius, max_velocity,
                 last_centroid_x, last_centroid_y; } egg_environment;
int egg_get_environment(egg_handle *h, int which, egg_environment *out);
typedef struct {
    float color[4], outline_color[4];
    double outline_thickness;
    double highlight_strength, shadow_strength;
    double texture_scale, motion_blur;
} egg_render_config;
int egg_set_render_config(egg_handle *h, int which, const egg_render_config *cfg);
int egg_set_add_color(egg_handle *h, int64_t id, int which, double r, double g, double b, double a);
int egg_set_color(egg_handle *h, int64_t id, int which, double r, double g, double b, double a);
typedef struct {
    int32_t screen_w, screen_h;
    double origin_x, origin_y;
    double interpolation_alpha;
    double threshold, smoothness;
    int32_t use_instancing;
    int32_t canvas_w[2], canvas_h[2];
    float clear[4];
} egg_render_params;
int egg_default_render_params(egg_render_params *p);
int egg_render(egg_handle *h, const egg_render_params *p, float *rgba);
int egg_set_option(egg_handle *h, int option, double value);
typedef struct { int32_t kind; int32_t type_mask; double p[4]; } egg_collider;
int egg_set_colliders(egg_handle *h, int32_t n, const egg_collider *c);
int egg_get_colliders(const egg_handle *h, int32_t cap, egg_collider *c, int32_t *n);
int egg_get_collider_hits(egg_handle *h, int64_t hits[2]);
typedef struct { int32_t kind; int32_t type_mask; double p[4]; } egg_force;
int egg_set_forces(egg_handle *h, int32_t n, const egg_force *f);
int egg_get_forces(const egg_handle *h, int32_t cap, egg_force *f, int32_t *n);
int egg_set_viscosity(egg_handle *h, const double c[2]);
int egg_get_viscosity(const egg_handle *h, double c[2]);
int egg_get_viscosity_pairs(egg_handle *h, int64_t pairs[2]);
int egg_set_coupling(egg_handle *h, double factor, double strength);
int egg_get_coupling(const egg_handle *h, double *factor, double *strength);
int egg_get_coupling_solves(egg_handle *h, int64_t *solves);
int egg_set_adhesion(egg_handle *h, double reach, double strength);
int egg_get_adhesion(const egg_handle *h, double *reach, double *strength);
int egg_get_adhesion_solves(egg_handle *h, int64_t *solves);
int egg_set_containment(egg_handle *h, double factor, double strength);
int egg_get_containment(const egg_handle *h, double *factor, double *strength);
int egg_get_containment_hits(egg_handle *h, int64_t *hits);
typedef struct { double friction; double vx, vy; } egg_collider_surface;
int egg_set_collider_surfaces(egg_handle *h, int32_t n, const egg_collider_surface *s);
int egg_get_collider_surfaces(const egg_handle *h, int32_t cap, egg_collider_surface *s, int32_t *n);
typedef struct { double vx, vy; } egg_collider_motion;
int egg_set_collider_motion(egg_handle *h, int32_t n, const egg_collider_motion *m);
int egg_get_collider_motion(const egg_handle *h, int32_t cap, egg_collider_motion *m, int32_t *n);
typedef struct { double px, py, omega; } egg_collider_spin;
int egg_set_collider_spin(egg_handle *h, int32_t n, const egg_collider_spin *s);
int egg_get_collider_spin(const egg_handle *h, int32_t cap, egg_collider_spin *s, int32_t *n);
int egg_get_collider_grips(egg_handle *h, int64_t grips[2]);
typedef struct { double jx, jy, torque; } egg_collider_load;
int egg_set_collider_loads(egg_handle *h, int on);
int egg_get_collider_loads_enabled(const egg_handle *h, int *on);
int egg_get_collider_load_sums(egg_handle *h, int32_t cap, int64_t *sums, int64_t *dropped, double *sub_delta, int32_t *n);
int egg_get_collider_loads(egg_handle *h, int32_t cap, egg_collider_load *out, int32_t *n);
typedef struct { double inv_mass, inv_inertia, ax, ay, drag, spin_drag; } egg_collider_body;
int egg_set_collider_bodies(egg_handle *h, int32_t n, const egg_collider_body *b);
int egg_get_collider_bodies(const egg_handle *h, int32_t cap, egg_collider_body *b, int32_t *n);
typedef struct { double restitution; int32_t on; int32_t reserved; } egg_collider_contact;
int egg_set_collider_contacts(egg_handle *h, int32_t n, const egg_collider_contact *c, int32_t iterations);
int egg_get_collider_contacts(const egg_handle *h, int32_t cap, egg_collider_contact *out, int32_t *n, int32_t *iterations);
int egg_get_collider_contact_solves(egg_handle *h, int64_t *solves);
typedef struct { float fill[4]; float line[4]; float line_width; int32_t layer; } egg_collider_style;
int egg_set_collider_styles(egg_handle *h, int32_t n, const egg_collider_style *s);
int egg_get_collider_styles(const egg_handle *h, int32_t cap, egg_collider_style *s, int32_t *n);
int egg_get_collider_pose(egg_handle *h, double alpha, int32_t cap, egg_collider *c, int32_t *n);
typedef struct { int32_t kind; int32_t type_mask; double p[6]; } egg_sensor;
typedef struct { int64_t count[2], sx[2], sy[2]; } egg_sensor_reading;
int egg_set_sensors(egg_handle *h, int32_t n, const egg_sensor *sensors);
int egg_get_sensors(const egg_handle *h, int32_t cap, egg_sensor *out, int32_t *n);
int egg_read_sensors(egg_handle *h, int32_t cap, egg_sensor_reading *readings, int64_t dropped[2], int32_t *n);
int egg_read_sensor_batches(egg_handle *h, int64_t n_ids, const int64_t *ids, int32_t *counts);
typedef struct { int32_t kind; int32_t type_mask; double p[5]; } egg_probe_query;
typedef struct { int64_t id, key; int32_t index, found; double score, x, y, radius; } egg_probe_hit;
int egg_probe(egg_handle *h, int32_t n, const egg_probe_query *probes, egg_probe_hit *hits);
typedef struct { double x0, y0, cell; int32_t nx, ny, type_mask, path; } egg_field_spec;
typedef struct { int32_t *count; int64_t *svx, *svy; } egg_field_planes;
typedef struct { int64_t inside[2], outside[2], dropped[2]; int32_t units_tiled, units_direct; } egg_field_totals;
int egg_field(egg_handle *h, const egg_field_spec *spec, const egg_field_planes *host_out, egg_field_totals *totals);
typedef struct { double reach[2]; int32_t type_mask; int32_t reserved; } egg_pieces_spec;
typedef struct { int32_t n, pieces, largest, first, singles, dropped; int64_t sx, sy; } egg_piece_summary;
int egg_pieces(egg_handle *h, const egg_pieces_spec *spec, int64_t n_ids, const int64_t *ids, egg_piece_summary *out, int32_t *white_labels, int32_t *yolk_labels);
typedef struct egg_group egg_group;
int egg_group_set_solver_order(egg_group *g, int32_t order, double relaxation);
int egg_group_set_cohesion(egg_group *g, int32_t mode);
int egg_group_get_halo_counters(const egg_group *g, int64_t *passes, int64_t *records, int64_t *bytes);
]]

local lib = ffi.load(os.getenv("EGGSIM_LIB") or "eggsim")
local NaN = 0 / 0
local EGG_DEFAULT_COUNT = -1 -- include/eggsim.h

local SimulationHandler = {}
setmetatable(SimulationHandler, { __call = function(_, ...) return SimulationHandler.new(...) end })
local _type_metatable = { __index = SimulationHandler }

-- keys, bounds and messages of the reference's _load_config (simulation_handler.lua:1152-1320)
local _valid_config_keys = {
    damping = { type = "number", min = 0, max = 1 }, color = { type = "color" }, outline_color = { type = "color" },
    outline_thickness = { type = "number", min = 0 }, collision_strength = { type = "number", min = 0, max = 1 },
    collision_overlap_factor = { type = "number", min = 0 }, cohesion_strength = { type = "number", min = 0, max = 1 },
    cohesion_interaction_distance_factor = { type = "number", min = 0 }, follow_strength = { type = "number", min = 0, max = 1 },
    min_radius = { type = "number", min = 0 }, max_radius = { type = "number", min = 0 },
    min_mass = { type = "number", min = 0 }, max_mass = { type = "number", min = 0 },
    motion_blur = { type = "number", min = 0, max = 1 }, texture_scale = { type = "number", min = 1 },
    highlight_strength = { type = "number", min = 0 }, shadow_strength = { type = "number", min = 0 },
}
local _solver_keys = { "damping", "follow_strength", "cohesion_strength", "cohesion_interaction_distance_factor",
    "collision_strength", "collision_overlap_factor", "min_mass", "max_mass", "min_radius", "max_radius" }

local function _deepcopy(v)
    if type(v) ~= "table" then return v end
    local out = {}
    for k, x in pairs(v) do out[k] = _deepcopy(x) end
    return out
end

--- status -> the reference's conventions: > 0 warns and carries on, < 0 throws (log.lua:9-46)
function SimulationHandler:_check(rc)
    if rc == 0 then return rc end
    local message = ffi.string(lib.egg_last_error(self._h))
    if rc > 0 then log.warning(message) else log.error(message) end
    return rc
end

function SimulationHandler:_load_config(config, white_or_yolk)
    local scope = white_or_yolk and "In SimulationHandler.set_white_config: " or "In SimulationHandler.set_yolk_config: "
    local target = white_or_yolk and self._white_config or self._yolk_config
    for key, value in pairs(config) do
        local entry = _valid_config_keys[key]
        if entry == nil then
            log.warning(scope, "unrecognized config key `", key, "`, it will be ignored")
        elseif entry.type == "color" then
            for i = 1, 4 do
                local c = value[i]
                if c == nil or #value > 4 then log.error(scope, "color `", key, "` does not have 4 components") return end
                if type(c) ~= "number" or math.is_nan(c) then log.error(scope, "color `", key, "` has a component that is not a number") return end
                if c < 0 or c > 1 then log.warning(scope, "color `", key, "` has a component that is outside of [0, 1]") end
                value[i] = math.clamp(c, 0, 1)
            end
            target[key] = value
        elseif type(value) ~= entry.type then
            log.error(scope, "wrong type for config key `", key, "`, expected `", entry.type, "`, got `", type(value), "`")
            return
        elseif math.is_nan(value) then
            log.warning(scope, "config key `", key, "` is NaN, it will be ignored")
        else
            if entry.min ~= nil and value < entry.min then
                log.warning(scope, "config key `", key, "`'s value is `", value, "`, expected a value larger than `", entry.min, "`")
                value = math.max(value, entry.min)
            elseif entry.max ~= nil and value > entry.max then
                log.warning(scope, "config key `", key, "`'s value is `", value, "`, expected a value smaller than `", entry.max, "`")
                value = math.min(value, entry.max)
            end
            target[key] = value
        end
    end
end

function SimulationHandler:_c_config(white_or_yolk)
    local cfg = white_or_yolk and self._white_config or self._yolk_config
    local c = ffi.new("egg_config")
    for _, key in ipairs(_solver_keys) do c[key] = cfg[key] end
    c.max_collision_fraction = self._max_collision_fraction
    c.mass_distribution_variance = self._mass_distribution_variance
    c.eps = math.eps
    return c
end

function SimulationHandler.new(white_config, yolk_config, device)
    if yolk_config == nil then yolk_config = white_config end
    log.assert(white_config, "table", yolk_config, "table")
    local self = setmetatable({}, _type_metatable)
    self._white_config, self._yolk_config = {}, {}
    self._mass_distribution_variance = 4
    self._max_collision_fraction = 0.05
    self._batch_colors = {} -- render attribute, host side only (simulation_handler.lua:297-395)
    self:_load_config(_deepcopy(white_config), true)
    self:_load_config(_deepcopy(yolk_config), false)
    local out = ffi.new("egg_handle*[1]")
    local rc = lib.egg_create(self:_c_config(true), self:_c_config(false), device or 0, out)
    if rc ~= 0 then log.error("In SimulationHandler.new: ", ffi.string(lib.egg_last_error(nil))) end
    self._h = ffi.gc(out[0], lib.egg_destroy)
    return self
end

function SimulationHandler:add(x, y, white_radius, yolk_radius, white_color, yolk_color, white_n_particles, yolk_n_particles)
    -- argument handling of the reference's add (simulation_handler.lua:27-120), in its order: defaults, type
    -- assertion, radius / count errors, colour errors and warnings; the particle-count defaults themselves
    -- are computed by the library (EGG_DEFAULT_COUNT = "the caller gave nil"), from the same formula (L:52-58)
    -- (whether the caller gave a colour decides if the batch gets a table of its own or shares the config's, L:49-50)
    local given_white, given_yolk = white_color ~= nil, yolk_color ~= nil
    white_color = white_color or self._white_config.color
    yolk_color = yolk_color or self._yolk_config.color
    log.assert(x, "number", y, "number")
    if white_radius ~= nil then log.assert(white_radius, "number") end
    if yolk_radius ~= nil then log.assert(yolk_radius, "number") end
    log.assert(white_color, "table", yolk_color, "table")
    if white_n_particles ~= nil then log.assert(white_n_particles, "number") end
    if yolk_n_particles ~= nil then log.assert(yolk_n_particles, "number") end

    if white_radius ~= nil and white_radius <= 0 then
        log.error("In SimulationHandler.add: white radius cannot be 0 or negative")
    end
    if yolk_radius ~= nil and yolk_radius <= 0 then
        log.error("In SimulationHandler.add: yolk radius cannot be 0 or negative")
    end
    if white_n_particles ~= nil and white_n_particles <= 1 then
        log.error("In SimulationHandler.add: white particle count cannot be 1 or negative")
    end
    if yolk_n_particles ~= nil and yolk_n_particles <= 1 then
        log.error("In SimulationHandler.add: yolk particle count cannot be 1 or negative")
    end

    local component_names = { "r", "g", "b", "a" }
    for _, entry in ipairs({ { "white", white_color }, { "yolk", yolk_color } }) do
        local name, color = entry[1], entry[2]
        for i, component_name in ipairs(component_names) do
            if type(color[i]) ~= "number" or math.is_nan(color[i]) then
                log.error("In SimulationHandler.add: ", name, " color component `", component_name, "` is not a number")
                return
            end
            if color[i] < 0 or color[i] > 1 then
                log.warning("In SimulationHandler.add: ", name, " color component `", component_name, "` is outside of [0, 1]")
            end
            color[i] = math.clamp(color[i], 0, 1)
        end
    end

    local id = ffi.new("int64_t[1]")
    -- status 2 (EGG_WARN_FEW_PARTICLES) carries the reference's "only `n` particles will be created" warning
    self:_check(lib.egg_add(self._h, x, y, white_radius or NaN, yolk_radius or NaN,
        white_n_particles and math.ceil(white_n_particles) or EGG_DEFAULT_COUNT,
        yolk_n_particles and math.ceil(yolk_n_particles) or EGG_DEFAULT_COUNT, id))
    local batch_id = tonumber(id[0])
    -- a batch created without a colour shares the config's colour table (simulation_handler.lua:49-50)
    self._batch_colors[batch_id] = { white_color, yolk_color }
    if given_white then lib.egg_set_add_color(self._h, batch_id, 0, white_color[1], white_color[2], white_color[3], white_color[4]) end
    if given_yolk then lib.egg_set_add_color(self._h, batch_id, 1, yolk_color[1], yolk_color[2], yolk_color[3], yolk_color[4]) end
    return batch_id
end

--- the render keys of a config table as egg_render_config (simulation_handler_default_config.lua:22-36)
function SimulationHandler:_c_render_config(white_or_yolk)
    local cfg = white_or_yolk and self._white_config or self._yolk_config
    local c = ffi.new("egg_render_config")
    for i = 1, 4 do
        c.color[i - 1] = cfg.color[i]
        c.outline_color[i - 1] = cfg.outline_color[i]
    end
    c.outline_thickness, c.highlight_strength, c.shadow_strength = cfg.outline_thickness, cfg.highlight_strength, cfg.shadow_strength
    c.texture_scale, c.motion_blur = cfg.texture_scale, cfg.motion_blur
    return c
end

--- set_white_color / set_yolk_color (simulation_handler.lua:328-398): in place, like the reference
function SimulationHandler:_set_color(scope, which, batch_id, r, g, b, a)
    if a == nil then a = 1 end
    log.assert(batch_id, "number", r, "number", g, "number", b, "number", a, "number")
    if r > 1 or r < 0 or g > 1 or g < 0 or b > 1 or b < 0 or a > 1 or a < 0 then
        log.warning("In SimulationHandler.", scope, ": color component is outside of [0, 1]")
    end
    local colors = self._batch_colors[batch_id]
    if colors == nil then
        log.warning("In SimulationHandler.", scope, ": no batch with id `", batch_id, "`")
        return
    end
    local color = colors[which + 1]
    color[1], color[2], color[3], color[4] = math.clamp(r, 0, 1), math.clamp(g, 0, 1), math.clamp(b, 0, 1), math.clamp(a, 0, 1)
    lib.egg_set_color(self._h, batch_id, which, color[1], color[2], color[3], color[4])
end
function SimulationHandler:set_white_color(batch_id, r, g, b, a) self:_set_color("set_white_color", 0, batch_id, r, g, b, a) end
function SimulationHandler:set_yolk_color(batch_id, r, g, b, a) self:_set_color("set_egg_yolk_color", 1, batch_id, r, g, b, a) end

--- :draw() without a window: both passes of the reference's draw path as HIP kernels (include/eggsim.h) into a
--- float32 RGBA buffer of width x height; world px = screen px + origin.  Returns the buffer (row-major).
function SimulationHandler:render_to_image(width, height, origin_x, origin_y)
    local p = ffi.new("egg_render_params[1]")
    lib.egg_default_render_params(p)
    p[0].screen_w, p[0].screen_h = width, height
    p[0].origin_x, p[0].origin_y = origin_x or 0, origin_y or 0
    for which = 0, 1 do self:_check(lib.egg_set_render_config(self._h, which, self:_c_render_config(which == 0))) end
    local image = ffi.new("float[?]", width * height * 4)
    self:_check(lib.egg_render(self._h, p, image))
    return image
end

function SimulationHandler:remove(batch_id)
    log.assert(batch_id, "number")
    if self:_check(lib.egg_remove(self._h, batch_id)) == 0 then self._batch_colors[batch_id] = nil end
end

function SimulationHandler:update(delta, step_delta, n_substeps, n_collision_steps)
    if step_delta == nil then step_delta = 1 / 60 end
    if n_substeps == nil then n_substeps = 2 end
    if n_collision_steps == nil then n_collision_steps = 3 end
    log.assert(delta, "number", step_delta, "number", n_substeps, "number", n_collision_steps, "number")
    local n = ffi.new("int32_t[1]")
    self:_check(lib.egg_update(self._h, delta, step_delta, math.ceil(n_substeps), math.ceil(n_collision_steps), n))
    return n[0]
end

function SimulationHandler:set_white_config(config)
    log.assert(config, "table")
    self:_load_config(_deepcopy(config), true)
    self:_check(lib.egg_set_config(self._h, 0, self:_c_config(true)))
end

function SimulationHandler:set_yolk_config(config)
    log.assert(config, "table")
    self:_load_config(_deepcopy(config), false)
    self:_check(lib.egg_set_config(self._h, 1, self:_c_config(false)))
end

function SimulationHandler:get_white_config() return _deepcopy(self._white_config) end
function SimulationHandler:get_yolk_config() return _deepcopy(self._yolk_config) end

function SimulationHandler:set_target_position(batch_id, x, y)
    log.assert(batch_id, "number", x, "number", y, "number")
    self:_check(lib.egg_set_target(self._h, batch_id, x, y))
end

function SimulationHandler:get_target_position(batch_id)
    log.assert(batch_id, "number")
    local x, y = ffi.new("double[1]"), ffi.new("double[1]")
    if self:_check(lib.egg_get_target(self._h, batch_id, x, y)) ~= 0 then return nil, nil end
    return x[0], y[0]
end

function SimulationHandler:get_position(batch_id)
    log.assert(batch_id, "number")
    local x, y = ffi.new("double[1]"), ffi.new("double[1]")
    if self:_check(lib.egg_get_position(self._h, batch_id, x, y)) ~= 0 then return nil, nil end
    return x[0], y[0]
end

function SimulationHandler:list_ids()
    local n = ffi.new("int64_t[1]")
    self:_check(lib.egg_list_ids(self._h, 0, nil, n))
    local buf = ffi.new("int64_t[?]", math.max(1, tonumber(n[0])))
    self:_check(lib.egg_list_ids(self._h, n[0], buf, n))
    local ids = {}
    for i = 0, tonumber(n[0]) - 1 do ids[i + 1] = tonumber(buf[i]) end
    return ids
end

function SimulationHandler:get_n_particles(batch_or_nil)
    local w, y = ffi.new("int64_t[1]"), ffi.new("int64_t[1]")
    self:_check(lib.egg_get_n_particles(self._h, batch_or_nil == nil and -1 or batch_or_nil, w, y))
    return tonumber(w[0]), tonumber(y[0])
end

--- the reference's instanced-draw record per particle (simulation_handler.lua:513-517, 744-813)
function SimulationHandler:get_instance_data(white_or_yolk)
    local which = white_or_yolk and 0 or 1
    local n_white, n_yolk = self:get_n_particles()
    local n = white_or_yolk and n_white or n_yolk
    local fields = { 0, 1, 4, 5, 2, 3, 6 } -- x, y, last_x, last_y, vx, vy, radius
    local out = {}
    for col, field in ipairs(fields) do
        local buf = ffi.new("double[?]", math.max(1, n))
        self:_check(lib.egg_download_particles(self._h, which, field, buf, n))
        out[col] = buf
    end
    return out, n
end

--- The reference's two per-particle meshes (simulation_handler.lua:513-523), packed on the device: returns
--- data (const egg_instance*: x, y, last_x, last_y, vx, vy, radius as float, 28 bytes per particle = the data mesh's
--- vertex format), color (const float*: rgba per particle = the colour mesh's), n and color_version, ready for
--- love.data.newByteData(ffi.string(data, n * 28)) / mesh:setVertices.  The pointers are pinned buffers of the handle:
--- valid until the second following :instances() of the same type.  color_version stands while no call changed a colour
--- or the particle count: skip the colour upload while it does (simulation_handler.lua:519-520).
function SimulationHandler:instances(white_or_yolk)
    local which = white_or_yolk and 0 or 1
    self:_check(lib.egg_instances_begin(self._h, which == 0 and 1 or 2))
    local data, color = ffi.new("const egg_instance*[1]"), ffi.new("const float*[1]")
    local n, version = ffi.new("int64_t[1]"), ffi.new("uint64_t[1]")
    self:_check(lib.egg_instances_end(self._h, which, data, color, n, version))
    return data[0], color[0], tonumber(n[0]), tonumber(version[0])
end

--- the fields the reference's environments hold for :draw(): particle AABB incl. radius, centroid, largest
--- radius / speed, centroid at the start of the last step (simulation_handler.lua:1669-1718, 1795-1815,
--- used at 1946-1950, 2007, 2132 to size and place the canvases)
function SimulationHandler:get_environment(white_or_yolk)
    local e = ffi.new("egg_environment[1]")
    self:_check(lib.egg_get_environment(self._h, white_or_yolk and 0 or 1, e))
    local v = e[0]
    return { min_x = v.min_x, min_y = v.min_y, max_x = v.max_x, max_y = v.max_y, centroid_x = v.centroid_x,
             centroid_y = v.centroid_y, max_radius = v.max_radius, max_velocity = v.max_velocity,
             last_centroid_x = v.last_centroid_x, last_centroid_y = v.last_centroid_y }
end

-- Not in the reference: the opt-in, non-parity modes of include/eggsim.h (EGG_OPT_SOLVER_ORDER = 13, EGG_OPT_RELAXATION = 14,
-- EGG_OPT_COHESION = 15; DESIGN.md section 2.7).
local _solver_orders = { exact = 0, relaxed = 1 }
local _cohesion_modes = { reference = 0, effective = 1 }

--- "exact" (default) or "relaxed", omega `relaxation` in (0, 2] (nil keeps the current value)
function SimulationHandler:set_solver_order(order, relaxation)
    if _solver_orders[order] == nil then log.error("In SimulationHandler.set_solver_order: expected `exact` or `relaxed`") return end
    if relaxation ~= nil and self:_check(lib.egg_set_option(self._h, 14, relaxation)) ~= 0 then return end
    if self:_check(lib.egg_set_option(self._h, 13, _solver_orders[order])) == 0 then self._solver_order = order end
end
function SimulationHandler:get_solver_order() return self._solver_order or "exact" end

--- "reference" (default): cohesion_strength / cohesion_interaction_distance_factor move nothing, as in the reference;
--- "effective": same-batch particles within factor * (ra + rb) are pulled back to the collision distance.  Relaxed
--- order only: refused in exact order, and set_solver_order("exact") is refused while cohesion is effective.
function SimulationHandler:set_cohesion(mode)
    if _cohesion_modes[mode] == nil then log.error("In SimulationHandler.set_cohesion: expected `reference` or `effective`") return end
    if self:_check(lib.egg_set_option(self._h, 15, _cohesion_modes[mode])) == 0 then self._cohesion = mode end
end
function SimulationHandler:get_cohesion() return self._cohesion or "reference" end

-- Not in the reference, which has no boundary of any kind: static colliders of the relaxed pass (egg_set_colliders in
-- include/eggsim.h; DESIGN.md section 2.7, "Colliders").  Relaxed order only.
local _collider_kinds = { half_plane = 0, disc = 1, container = 2, segment = 3, wall = 5 }  -- (4 is not a kind)
local _collider_names = { [0] = "half_plane", "disc", "container", "segment", [5] = "wall" }
local _collider_n_params = { [0] = 3, 3, 3, 4, [5] = 4 }
local _collider_types = { white = 1, yolk = 2, both = 3 }
local _collider_type_names = { "white", "yolk", "both" }

--- the ordered list of at most 64 colliders, each `{ "half_plane", nx, ny, off }`, `{ "disc", cx, cy, R }`,
--- `{ "container", cx, cy, R }`, `{ "segment", x0, y0, x1, y1 }` or `{ "wall", x0, y0, x1, y1 }` (a segment that fast
--- particles cannot cross: it sweeps the sub-step's path) with an optional `types = "both" | "white" | "yolk"`;
--- applied in list order to every particle's new position in a relaxed pass.  `{}` clears the list.
function SimulationHandler:set_colliders(colliders)
    local n = #colliders
    local arr = ffi.new("egg_collider[?]", math.max(n, 1))
    for k, c in ipairs(colliders) do
        local kind = _collider_kinds[c[1]]
        local mask = _collider_types[c.types or "both"]
        if kind == nil or mask == nil or #c ~= 1 + _collider_n_params[kind] then
            log.error("In SimulationHandler.set_colliders: collider " .. k .. ": expected { kind, parameters..., types = ... }")
            return
        end
        arr[k - 1].kind, arr[k - 1].type_mask = kind, mask
        for q = 1, _collider_n_params[kind] do arr[k - 1].p[q - 1] = c[q + 1] end
    end
    self:_check(lib.egg_set_colliders(self._h, n, arr))
end

--- the list as stored (a half-plane's normal normalised), in the shapes set_colliders takes
function SimulationHandler:get_colliders()
    local arr, n = ffi.new("egg_collider[64]"), ffi.new("int32_t[1]")
    if self:_check(lib.egg_get_colliders(self._h, 64, arr, n)) ~= 0 then return {} end
    local out = {}
    for k = 0, n[0] - 1 do
        local c = { _collider_names[arr[k].kind], types = _collider_type_names[arr[k].type_mask] }
        for q = 1, _collider_n_params[arr[k].kind] do c[q + 1] = arr[k].p[q - 1] end
        out[k + 1] = c
    end
    return out
end

--- white, yolk: how often a collider moved a particle in a pass of a committed step
function SimulationHandler:collider_hits()
    local hits = ffi.new("int64_t[2]")
    self:_check(lib.egg_get_collider_hits(self._h, hits))
    return tonumber(hits[0]), tonumber(hits[1])
end

-- Not in the reference: collider surfaces (egg_set_collider_surfaces in include/eggsim.h; DESIGN.md section 2.7,
-- "Collider surfaces").

local _max_colliders = 64  -- EGG_MAX_COLLIDERS

--- one surface per collider of the current list: `false` for the default, a number `mu` (Coulomb friction, >= 0) or
--- `{ mu, vx, vy }` with the surface's velocity in px/s.  `{}` resets every surface to the default, and so does set_colliders.
function SimulationHandler:set_collider_surfaces(surfaces)
    local n = #surfaces
    local arr = ffi.new("egg_collider_surface[?]", math.max(n, 1))
    for k = 1, n do  -- (not ipairs: a nil hole must not end the walk short of n)
        local s = surfaces[k]
        if s == false then s = { 0, 0, 0 } elseif type(s) == "number" then s = { s, 0, 0 } end
        if type(s) ~= "table" or #s ~= 3 then
            log.error("In SimulationHandler.set_collider_surfaces: surface " .. k .. ": expected false, mu or { mu, vx, vy }")
            return
        end
        arr[k - 1].friction, arr[k - 1].vx, arr[k - 1].vy = s[1], s[2], s[3]
    end
    self:_check(lib.egg_set_collider_surfaces(self._h, n, arr))
end

--- the surfaces as stored, one `{ mu, vx, vy }` per collider (defaults included)
function SimulationHandler:get_collider_surfaces()
    local arr, n = ffi.new("egg_collider_surface[?]", _max_colliders), ffi.new("int32_t[1]")
    if self:_check(lib.egg_get_collider_surfaces(self._h, _max_colliders, arr, n)) ~= 0 then return {} end
    local out = {}
    for k = 0, n[0] - 1 do out[k + 1] = { arr[k].friction, arr[k].vx, arr[k].vy } end
    return out
end

--- white, yolk: friction applications (stick or slide) in the passes of committed steps
function SimulationHandler:collider_grips()
    local grips = ffi.new("int64_t[2]")
    self:_check(lib.egg_get_collider_grips(self._h, grips))
    return tonumber(grips[0]), tonumber(grips[1])
end

-- Not in the reference: collider motion (egg_set_collider_motion in include/eggsim.h; DESIGN.md section 2.7,
-- "Collider motion").

--- one motion per collider of the current list: `false` for a collider at rest or `{ vx, vy }`, a rigid velocity in px/s
--- that the step integrates on the device.  `{}` resets every motion to zero, and so does set_colliders.
function SimulationHandler:set_collider_motion(motions)
    local n = #motions
    local arr = ffi.new("egg_collider_motion[?]", math.max(n, 1))
    for k = 1, n do  -- (not ipairs: a nil hole must not end the walk short of n)
        local m = motions[k]
        if m == false then m = { 0, 0 } end
        if type(m) ~= "table" or #m ~= 2 then
            log.error("In SimulationHandler.set_collider_motion: motion " .. k .. ": expected false or { vx, vy }")
            return
        end
        arr[k - 1].vx, arr[k - 1].vy = m[1], m[2]
    end
    self:_check(lib.egg_set_collider_motion(self._h, n, arr))
end

--- the motions as stored, one `{ vx, vy }` per collider (zeros included)
function SimulationHandler:get_collider_motion()
    local arr, n = ffi.new("egg_collider_motion[?]", _max_colliders), ffi.new("int32_t[1]")
    if self:_check(lib.egg_get_collider_motion(self._h, _max_colliders, arr, n)) ~= 0 then return {} end
    local out = {}
    for k = 0, n[0] - 1 do out[k + 1] = { arr[k].vx, arr[k].vy } end
    return out
end

-- Not in the reference: collider spin (egg_set_collider_spin in include/eggsim.h; DESIGN.md section 2.7,
-- "Collider spin").

--- one spin per collider of the current list: `false` for a collider that does not turn or `{ px, py, omega }`, a rigid
--- angular velocity in rad/s (counter-clockwise positive) about the pivot (px, py) that the step integrates on the device.
--- `{}` resets every spin to zero, and so does set_colliders.
function SimulationHandler:set_collider_spin(spins)
    local n = #spins
    local arr = ffi.new("egg_collider_spin[?]", math.max(n, 1))
    for k = 1, n do  -- (not ipairs: a nil hole must not end the walk short of n)
        local s = spins[k]
        if s == false then s = { 0, 0, 0 } end
        if type(s) ~= "table" or #s ~= 3 then
            log.error("In SimulationHandler.set_collider_spin: spin " .. k .. ": expected false or { px, py, omega }")
            return
        end
        arr[k - 1].px, arr[k - 1].py, arr[k - 1].omega = s[1], s[2], s[3]
    end
    self:_check(lib.egg_set_collider_spin(self._h, n, arr))
end

--- the spins as stored, one `{ px, py, omega }` per collider (zeros included); a committed step advances the pivots
function SimulationHandler:get_collider_spin()
    local arr, n = ffi.new("egg_collider_spin[?]", _max_colliders), ffi.new("int32_t[1]")
    if self:_check(lib.egg_get_collider_spin(self._h, _max_colliders, arr, n)) ~= 0 then return {} end
    local out = {}
    for k = 0, n[0] - 1 do out[k + 1] = { arr[k].px, arr[k].py, arr[k].omega } end
    return out
end

-- Not in the reference: collider bodies (egg_set_collider_bodies in include/eggsim.h; DESIGN.md section 2.7,
-- "Collider bodies").

--- one body per collider of the current list: `false` for a collider that stays kinematic or
--- `{ inv_mass, inv_inertia [, ax, ay [, drag, spin_drag ] ] }`.  inv_mass > 0 frees the translation, inv_inertia > 0 the rotation
--- about the collider's spin pivot; in a relaxed step with collider loads on the device integrates every body from the loads
--- it receives.  `{}` resets, and so does set_colliders.
function SimulationHandler:set_collider_bodies(bodies)
    local n = #bodies
    local arr = ffi.new("egg_collider_body[?]", math.max(n, 1))
    for k = 1, n do  -- (not ipairs: a nil hole must not end the walk short of n)
        local b = bodies[k]
        if b == false then b = { 0, 0 } end
        if type(b) ~= "table" or (#b ~= 2 and #b ~= 4 and #b ~= 6) then
            log.error("In SimulationHandler.set_collider_bodies: body " .. k ..
                ": expected false or { inv_mass, inv_inertia [, ax, ay [, drag, spin_drag ] ] }")
            return
        end
        local o = arr[k - 1]
        o.inv_mass, o.inv_inertia, o.ax, o.ay, o.drag, o.spin_drag = b[1], b[2], b[3] or 0, b[4] or 0, b[5] or 0, b[6] or 0
    end
    self:_check(lib.egg_set_collider_bodies(self._h, n, arr))
end

--- the bodies as stored, one `{ inv_mass, inv_inertia, ax, ay, drag, spin_drag }` per collider (zeros included)
function SimulationHandler:get_collider_bodies()
    local arr, n = ffi.new("egg_collider_body[?]", _max_colliders), ffi.new("int32_t[1]")
    if self:_check(lib.egg_get_collider_bodies(self._h, _max_colliders, arr, n)) ~= 0 then return {} end
    local out = {}
    for k = 0, n[0] - 1 do
        out[k + 1] = { arr[k].inv_mass, arr[k].inv_inertia, arr[k].ax, arr[k].ay, arr[k].drag, arr[k].spin_drag }
    end
    return out
end

-- Not in the reference, which has no colliders and draws none: collider styles and the pose a frame draws
-- (egg_set_collider_styles, egg_get_collider_pose in include/eggsim.h; DESIGN.md section 2.7, "Collider styles").

local _collider_layers = { under = 0, over = 1 }
local _collider_layer_names = { [0] = "under", "over" }

--- one style per collider of the current list for the headless renderer: `false` for a collider that is not drawn or
--- `{ fill = { r, g, b, a }, line = { r, g, b, a }, line_width = px, layer = "under" | "over" }`, missing keys meaning no
--- fill, no line, "under".  `{}` draws nothing, and so does set_colliders.  (A LOVE host draws the colliders itself, at
--- get_collider_pose: these styles only reach egg_render.)
function SimulationHandler:set_collider_styles(styles)
    local n = #styles
    local arr = ffi.new("egg_collider_style[?]", math.max(n, 1))
    for k = 1, n do  -- (not ipairs: a nil hole must not end the walk short of n)
        local s = styles[k]
        if s == false then s = {} end
        local layer = type(s) == "table" and _collider_layers[s.layer or "under"]
        if type(s) ~= "table" or layer == nil or (s.fill and #s.fill ~= 4) or (s.line and #s.line ~= 4) then
            log.error("In SimulationHandler.set_collider_styles: style " .. k ..
                ": expected false or { fill = rgba, line = rgba, line_width = px, layer = \"under\" | \"over\" }")
            return
        end
        local o = arr[k - 1]
        for q = 1, 4 do
            o.fill[q - 1] = s.fill and s.fill[q] or 0
            o.line[q - 1] = s.line and s.line[q] or 0
        end
        o.line_width, o.layer = s.line_width or 0, layer
    end
    self:_check(lib.egg_set_collider_styles(self._h, n, arr))
end

--- the styles as stored, one table per collider in the shape set_collider_styles takes (an undrawn one: all zero)
function SimulationHandler:get_collider_styles()
    local arr, n = ffi.new("egg_collider_style[?]", _max_colliders), ffi.new("int32_t[1]")
    if self:_check(lib.egg_get_collider_styles(self._h, _max_colliders, arr, n)) ~= 0 then return {} end
    local out = {}
    for k = 0, n[0] - 1 do
        local s = arr[k]
        out[k + 1] = { fill = { s.fill[0], s.fill[1], s.fill[2], s.fill[3] }, line = { s.line[0], s.line[1], s.line[2], s.line[3] },
                       line_width = s.line_width, layer = _collider_layer_names[s.layer] }
    end
    return out
end

--- the list a frame draws the colliders at, in the shapes set_colliders takes: every parameter is
--- `last * (1 - t) + current * t`, `last` the list at the start of the last committed step, t = `alpha` clamped to [0, 1]
--- or, without one, the handler's interpolation alpha -- the rule :draw() places the particles by.  Call it once per
--- frame and draw with love.graphics (INTEGRATION.md shows how).
function SimulationHandler:get_collider_pose(alpha)
    local arr, n = ffi.new("egg_collider[64]"), ffi.new("int32_t[1]")
    if self:_check(lib.egg_get_collider_pose(self._h, alpha or (0 / 0), 64, arr, n)) ~= 0 then return {} end
    local out = {}
    for k = 0, n[0] - 1 do
        local c = { _collider_names[arr[k].kind], types = _collider_type_names[arr[k].type_mask] }
        for q = 1, _collider_n_params[arr[k].kind] do c[q + 1] = arr[k].p[q - 1] end
        out[k + 1] = c
    end
    return out
end

-- Not in the reference: collider contacts (egg_set_collider_contacts in include/eggsim.h; DESIGN.md section 2.7,
-- "Collider contacts").

--- one contact per collider of the current list: `false` for a collider that meets no other, `true` (restitution 0) or a
--- restitution in [0, 1].  Where collider bodies act and some contact is on, every sub-step ends with `iterations`
--- (1 .. 16, default 4) rounds that keep contact-enabled colliders -- a disc against a half-plane, disc, container, segment or
--- wall -- from overlapping.  `{}` resets, and so does set_colliders.
function SimulationHandler:set_collider_contacts(contacts, iterations)
    local n = #contacts
    local arr = ffi.new("egg_collider_contact[?]", math.max(n, 1))
    for k = 1, n do  -- (not ipairs: a nil hole must not end the walk short of n)
        local c = contacts[k]
        if c == true then c = 0 end
        if c ~= false and type(c) ~= "number" then
            log.error("In SimulationHandler.set_collider_contacts: contact " .. k .. ": expected false, true or a restitution in [0, 1]")
            return
        end
        if c ~= false then
            arr[k - 1].restitution, arr[k - 1].on = c, 1
        end
    end
    self:_check(lib.egg_set_collider_contacts(self._h, n, arr, iterations or 4))
end

--- the contacts as stored, one per collider (`false` where off, else the restitution), and the iterations
function SimulationHandler:get_collider_contacts()
    local arr, n, it = ffi.new("egg_collider_contact[?]", _max_colliders), ffi.new("int32_t[1]"), ffi.new("int32_t[1]")
    if self:_check(lib.egg_get_collider_contacts(self._h, _max_colliders, arr, n, it)) ~= 0 then return {}, 4 end
    local out = {}
    for k = 0, n[0] - 1 do
        if arr[k].on ~= 0 then out[k + 1] = arr[k].restitution else out[k + 1] = false end
    end
    return out, it[0]
end

--- the fires of collider contacts, one per (pair, sub-step, iteration), over committed steps
function SimulationHandler:collider_contact_solves()
    local out = ffi.new("int64_t[1]")
    if self:_check(lib.egg_get_collider_contact_solves(self._h, out)) ~= 0 then return 0 end
    return tonumber(out[0])
end

-- Not in the reference: collider loads (egg_set_collider_loads in include/eggsim.h; DESIGN.md section 2.7,
-- "Collider loads").

--- switch collider loads on or off (off by default): while on, a relaxed step with a non-empty list records per collider the
--- impulse and the torque about its pivot that it received from the particles it moved.  It only observes.
function SimulationHandler:set_collider_loads(on)
    self:_check(lib.egg_set_collider_loads(self._h, on and 1 or 0))
end

function SimulationHandler:get_collider_loads_enabled()
    local on = ffi.new("int[1]")
    if self:_check(lib.egg_get_collider_loads_enabled(self._h, on)) ~= 0 then return false end
    return on[0] ~= 0
end

--- one `{ jx, jy, torque }` per collider: the impulse in mass px/s and the angular impulse about the collider's pivot in
--- mass px^2/s it received over the last committed step that recorded loads; the mean force is j / delta
function SimulationHandler:collider_loads()
    local arr, n = ffi.new("egg_collider_load[?]", _max_colliders), ffi.new("int32_t[1]")
    if self:_check(lib.egg_get_collider_loads(self._h, _max_colliders, arr, n)) ~= 0 then return {} end
    local out = {}
    for k = 0, n[0] - 1 do out[k + 1] = { arr[k].jx, arr[k].jy, arr[k].torque } end
    return out
end

--- the raw sums: `{ { sx, sy, sz }, ... }` as int64 cdata (impulse scaled by 2^20, torque by 2^10), the dropped count and
--- the sub-step h of the step that produced them
function SimulationHandler:collider_load_sums()
    local arr, n = ffi.new("int64_t[?]", 3 * _max_colliders), ffi.new("int32_t[1]")
    local dropped, h = ffi.new("int64_t[1]"), ffi.new("double[1]")
    if self:_check(lib.egg_get_collider_load_sums(self._h, _max_colliders, arr, dropped, h, n)) ~= 0 then return {}, 0, 0 end
    local out = {}
    for k = 0, n[0] - 1 do out[k + 1] = { arr[3 * k], arr[3 * k + 1], arr[3 * k + 2] } end
    return out, dropped[0], h[0]
end

-- Not in the reference: sensors (egg_set_sensors in include/eggsim.h; DESIGN.md section 2.8).  Regions that count and
-- locate the particles whose centres lie inside them, from the committed positions; either solver order.  They only
-- observe: a step launches what it launches without them.
local _sensor_kinds = { half_plane = 0, disc = 1, box = 2, capsule = 3 }
local _sensor_names = { [0] = "half_plane", "disc", "box", "capsule" }
local _sensor_n_params = { [0] = 3, 3, 6, 5 }
local _max_sensors = 64 -- EGG_MAX_SENSORS
local _sensor_scale = 65536 -- EGG_SENSOR_POSITION_SCALE

--- fills one egg_sensor from a region in the shape set_sensors takes (impulse's regions too); false for a malformed one
local function _fill_region(dst, s)
    if type(s) ~= "table" then return false end
    local kind = _sensor_kinds[s[1]]
    local mask = _collider_types[s.types or "both"]
    local by_angle = kind == 2 and #s == 6
    if kind == nil or mask == nil or (#s ~= 1 + _sensor_n_params[kind] and not by_angle) then return false end
    dst.kind, dst.type_mask = kind, mask
    if by_angle then -- the host's cos / sin, as spin does
        for q = 1, 4 do dst.p[q - 1] = s[q + 1] end
        dst.p[4], dst.p[5] = math.cos(s[6]), math.sin(s[6])
    else
        for q = 1, _sensor_n_params[kind] do dst.p[q - 1] = s[q + 1] end
    end
    return true
end

--- the ordered list of at most 64 sensors, each `{ "half_plane", nx, ny, off }` (the side the normal points to),
--- `{ "disc", cx, cy, R }`, `{ "box", cx, cy, hx, hy, angle }` (or `hx, hy, ux, uy` with the first axis),
--- `{ "capsule", x0, y0, x1, y1, R }`, with an optional `types = "both" | "white" | "yolk"`.  `{}` clears the list.
function SimulationHandler:set_sensors(sensors)
    local n = #sensors
    if n > _max_sensors then
        log.error("In SimulationHandler.set_sensors: a list holds 0 .. 64 sensors")
        return
    end
    local arr = ffi.new("egg_sensor[?]", math.max(n, 1))
    for k, s in ipairs(sensors) do
        if not _fill_region(arr[k - 1], s) then
            log.error("In SimulationHandler.set_sensors: sensor " .. k .. ": expected { kind, parameters..., types = ... }")
            return
        end
    end
    self:_check(lib.egg_set_sensors(self._h, n, arr))
end

--- the list as stored, in the shapes set_sensors takes: normals and box axes normalised, a box with its axis
function SimulationHandler:get_sensors()
    local arr, n = ffi.new("egg_sensor[?]", _max_sensors), ffi.new("int32_t[1]")
    if self:_check(lib.egg_get_sensors(self._h, _max_sensors, arr, n)) ~= 0 then return {} end
    local out = {}
    for k = 0, n[0] - 1 do
        local s = { _sensor_names[arr[k].kind], types = _collider_type_names[arr[k].type_mask] }
        for q = 1, _sensor_n_params[arr[k].kind] do s[q + 1] = arr[k].p[q - 1] end
        out[k + 1] = s
    end
    return out
end

--- the raw integers of the positions as committed now: `{ { white = { count, sx, sy }, yolk = { count, sx, sy } }, ... }`
--- as int64 cdata (sx, sy scaled by 2^16), and `{ white, yolk }` dropped.  Every call measures.
function SimulationHandler:sensor_sums()
    local arr, n = ffi.new("egg_sensor_reading[?]", _max_sensors), ffi.new("int32_t[1]")
    local dropped = ffi.new("int64_t[2]")
    if self:_check(lib.egg_read_sensors(self._h, _max_sensors, arr, dropped, n)) ~= 0 then return {}, { 0, 0 } end
    local out = {}
    for k = 0, n[0] - 1 do
        out[k + 1] = { white = { arr[k].count[0], arr[k].sx[0], arr[k].sy[0] }, yolk = { arr[k].count[1], arr[k].sx[1], arr[k].sy[1] } }
    end
    return out, { dropped[0], dropped[1] }
end

--- per sensor `{ white = { count = n, x = cx, y = cy }, yolk = { ... } }`: the particles inside and their centroid,
--- `(sx / 2^16) / count`; x and y are nil while the count is 0
function SimulationHandler:sensors()
    local sums = self:sensor_sums()
    local out = {}
    for k, rec in ipairs(sums) do
        local one = {}
        for _, name in ipairs({ "white", "yolk" }) do
            local count = tonumber(rec[name][1])
            one[name] = { count = count }
            if count > 0 then
                one[name].x = (tonumber(rec[name][2]) / _sensor_scale) / count
                one[name].y = (tonumber(rec[name][3]) / _sensor_scale) / count
            end
        end
        out[k] = one
    end
    return out
end

--- the counts only, per listed batch: `out[i][k] = { white, yolk }` for id i of `ids` and sensor k; an id may repeat
function SimulationHandler:sensor_batches(ids)
    local n_ids = #ids
    local n = ffi.new("int32_t[1]")
    if self:_check(lib.egg_get_sensors(self._h, 0, nil, n)) ~= 0 then return {} end
    local c_ids = ffi.new("int64_t[?]", math.max(n_ids, 1))
    for i, id in ipairs(ids) do c_ids[i - 1] = id end
    local counts = ffi.new("int32_t[?]", math.max(n_ids * n[0] * 2, 1))
    if self:_check(lib.egg_read_sensor_batches(self._h, n_ids, c_ids, counts)) ~= 0 then return {} end
    local out = {}
    for i = 0, n_ids - 1 do
        out[i + 1] = {}
        for k = 0, n[0] - 1 do
            out[i + 1][k + 1] = { counts[(i * n[0] + k) * 2], counts[(i * n[0] + k) * 2 + 1] }
        end
    end
    return out
end

-- Not in the reference: probes (egg_probe in include/eggsim.h; DESIGN.md section 2.9).  What is here: the ONE particle per
-- type nearest a point or first along a ray, from the committed state; either solver order.  A call stores nothing and
-- only observes: a step launches what it launches without it.
local _probe_kinds = { point = 0, ray = 1 }
local _probe_n_params = { [0] = 3, 5 }
local _probe_defaults = { [0] = math.huge, 0 } -- reach, pad: the last parameter may be left out
local _max_probes = 64 -- EGG_MAX_PROBES
local _probe_type_names = { [0] = "white", "yolk" }

--- at most 64 probes, each `{ "point", x, y[, reach] }` (reach defaults to infinity) or `{ "ray", x0, y0, x1, y1[, pad] }`
--- (pad defaults to 0), with an optional `types = "both" | "white" | "yolk"`.  Returns per probe
--- `{ white = hit_or_nil, yolk = hit_or_nil }`, a hit being `{ id, index, score, x, y, radius }` by name: the batch, the
--- particle's 0-based index in the batch's run of that type, squared distance (point) or t (ray), and the particle.
function SimulationHandler:probe(probes)
    local n = #probes
    if n > _max_probes then
        log.error("In SimulationHandler.probe: a call takes 0 .. 64 probes")
        return {}
    end
    local arr = ffi.new("egg_probe_query[?]", math.max(n, 1))
    for k, q in ipairs(probes) do
        local kind = _probe_kinds[q[1]]
        local mask = _collider_types[q.types or "both"]
        if kind == nil or mask == nil or (#q ~= 1 + _probe_n_params[kind] and #q ~= _probe_n_params[kind]) then
            log.error("In SimulationHandler.probe: probe " .. k .. ": expected { kind, parameters..., types = ... }")
            return {}
        end
        arr[k - 1].kind, arr[k - 1].type_mask = kind, mask
        for i = 1, _probe_n_params[kind] do
            local v = q[i + 1]
            if v == nil then v = _probe_defaults[kind] end
            arr[k - 1].p[i - 1] = v
        end
    end
    local hits = ffi.new("egg_probe_hit[?]", math.max(2 * n, 1))
    if self:_check(lib.egg_probe(self._h, n, arr, hits)) ~= 0 then return {} end
    local out = {}
    for k = 0, n - 1 do
        local one = {}
        for w = 0, 1 do
            local t = hits[2 * k + w]
            if t.found ~= 0 then
                one[_probe_type_names[w]] = { id = tonumber(t.id), index = t.index, score = t.score, x = t.x, y = t.y, radius = t.radius }
            end
        end
        out[k + 1] = one
    end
    return out
end

-- the lower score of a probe's two hits, an exact tie to white: type_name, hit; nil without a hit
local function _probe_first(one)
    if one == nil or (one.white == nil and one.yolk == nil) then return nil end
    if one.yolk == nil or (one.white ~= nil and not (one.yolk.score < one.white.score)) then return "white", one.white end
    return "yolk", one.yolk
end

--- the particle nearest (x, y) within `reach` (default: wherever it is): nil, or type_name and the hit; `types` as in probe
function SimulationHandler:pick(x, y, reach, types)
    return _probe_first(self:probe({ { "point", x, y, reach or math.huge, types = types } })[1])
end

--- the first particle disc (radius + pad) the segment enters: nil, or type_name, the hit and the point of impact x, y
function SimulationHandler:raycast(x0, y0, x1, y1, pad, types)
    local name, hit = _probe_first(self:probe({ { "ray", x0, y0, x1, y1, pad or 0, types = types } })[1])
    if name == nil then return nil end
    return name, hit, x0 + hit.score * (x1 - x0), y0 + hit.score * (y1 - y0)
end

-- Not in the reference: fields (egg_field in include/eggsim.h; DESIGN.md section 2.10).  The egg as a map: the committed
-- particles binned by their centres into a caller-set grid; either solver order.  A call stores nothing and only observes.
local _field_paths = { auto = 0, direct = 1 }
local _field_max_cells = 1048576 -- EGG_FIELD_MAX_CELLS
local _field_velocity_scale = 65536 -- EGG_FIELD_VELOCITY_SCALE

--- the grid of `nx` x `ny` square cells of side `cell` whose cell (0, 0) has its lower corner at (x0, y0); `options` may hold
--- `types = "both" | "white" | "yolk"`, `velocity = true` and `path = "auto" | "direct"` (a test hook).  Returns
--- `{ nx, ny, count, svx, svy, inside, outside, dropped, units_tiled, units_direct }` by name: `count` an `int32_t` and
--- `svx`, `svy` (nil without velocity) `int64_t` arrays laid out [2][ny][nx], 0-based, [0] white and [1] yolk -- the word of
--- type w and cell (ix, iy) is `(w * ny + iy) * nx + ix` --; `inside`, `outside`, `dropped` are `{ white, yolk }` counts.  The
--- mean velocity of a cell is `(tonumber(svx[i]) / 65536) / count[i]`, see `field_velocity`.
function SimulationHandler:field(x0, y0, cell, nx, ny, options)
    options = options or {}
    local mask = _collider_types[options.types or "both"]
    local path = _field_paths[options.path or "auto"]
    if mask == nil or path == nil or type(nx) ~= "number" or type(ny) ~= "number" or nx < 1 or ny < 1 or nx * ny > _field_max_cells
        or nx ~= math.floor(nx) or ny ~= math.floor(ny) then
        log.error("In SimulationHandler.field: expected (x0, y0, cell, nx, ny, { types = ..., velocity = ..., path = ... }) with nx * ny in 1 .. 1048576")
        return nil
    end
    local words = 2 * nx * ny
    local spec = ffi.new("egg_field_spec", { x0 = x0, y0 = y0, cell = cell, nx = nx, ny = ny, type_mask = mask, path = path })
    local count = ffi.new("int32_t[?]", words)
    local svx = options.velocity and ffi.new("int64_t[?]", words) or nil
    local svy = options.velocity and ffi.new("int64_t[?]", words) or nil
    local planes = ffi.new("egg_field_planes", { count = count, svx = svx, svy = svy })
    local totals = ffi.new("egg_field_totals")
    if self:_check(lib.egg_field(self._h, spec, planes, totals)) ~= 0 then return nil end
    local function pair(a) return { tonumber(a[0]), tonumber(a[1]) } end
    return { nx = nx, ny = ny, count = count, svx = svx, svy = svy, inside = pair(totals.inside), outside = pair(totals.outside),
             dropped = pair(totals.dropped), units_tiled = totals.units_tiled, units_direct = totals.units_direct }
end

--- the mean velocity vx, vy of type `w` (0 white, 1 yolk) in cell (ix, iy) of a field taken with `velocity = true`; nil while
--- the cell is empty
function SimulationHandler:field_velocity(field, w, ix, iy)
    local i = (w * field.ny + iy) * field.nx + ix
    local n = field.count[i]
    if n == 0 or field.svx == nil then return nil end
    return (tonumber(field.svx[i]) / _field_velocity_scale) / n, (tonumber(field.svy[i]) / _field_velocity_scale) / n
end

-- Not in the reference: pieces (egg_pieces in include/eggsim.h; DESIGN.md section 2.11).  Is the egg still one egg: the
-- connected pieces of each batch's white and yolk under the link rule d2 <= (reach * (ra + rb))^2, from the committed
-- state; either solver order.  A call stores nothing and only observes.
local _pieces_max_atom = 4096 -- EGG_PIECES_MAX_ATOM

--- the egg_pieces_spec of a call, or nil: `reach` nil (per type max(collision_overlap_factor,
--- cohesion_interaction_distance_factor) of the config), a number (both types) or `{ white, yolk }`
function SimulationHandler:_pieces_spec(reach, types, scope)
    local mask = _collider_types[types or "both"]
    local rw, ry
    if reach == nil then
        rw = math.max(self._white_config.collision_overlap_factor, self._white_config.cohesion_interaction_distance_factor)
        ry = math.max(self._yolk_config.collision_overlap_factor, self._yolk_config.cohesion_interaction_distance_factor)
    elseif type(reach) == "table" then
        rw, ry = reach[1], reach[2]
    else
        rw, ry = reach, reach
    end
    local function good(v) return type(v) == "number" and v > 0 and v < math.huge end
    if mask == nil or not good(rw) or not good(ry) then
        log.error("In SimulationHandler." .. scope .. ": expected (..., reach, types) with reach nil, a number above 0 or { white, yolk } and types \"both\" | \"white\" | \"yolk\"")
        return nil
    end
    return ffi.new("egg_pieces_spec", { reach = { rw, ry }, type_mask = mask })
end

local function _piece_summary(rec)
    if rec.n == 0 then return nil end
    local kept = rec.largest - rec.dropped
    local one = { n = rec.n, pieces = rec.pieces, largest = rec.largest, first = rec.first, singles = rec.singles, dropped = rec.dropped }
    if kept > 0 then
        one.x = (tonumber(rec.sx) / _sensor_scale) / kept
        one.y = (tonumber(rec.sy) / _sensor_scale) / kept
    end
    return one
end

--- per id of `ids` (nil: every batch of list_ids(), in that order) `{ white = summary or nil, yolk = summary or nil }`, a
--- summary `{ n, pieces, largest, first, singles, dropped, x, y }` by name: `pieces` connected pieces, `singles` of them of one
--- particle; the body (the largest piece, the lower label among equals) has `largest` particles, the label `first` and the
--- centroid `x, y` (nil while every body particle was dropped).  An id may repeat.
function SimulationHandler:pieces(ids, reach, types)
    local spec = self:_pieces_spec(reach, types, "pieces")
    if spec == nil then return nil end
    local listed = ids or self:list_ids()
    local n = #listed
    if n == 0 then return {} end
    local c_ids = ffi.new("int64_t[?]", n)
    for i, id in ipairs(listed) do c_ids[i - 1] = id end
    local out = ffi.new("egg_piece_summary[?]", 2 * n)
    if self:_check(lib.egg_pieces(self._h, spec, n, c_ids, out, nil, nil)) ~= 0 then return nil end
    local res = {}
    for i = 0, n - 1 do res[i + 1] = { white = _piece_summary(out[2 * i]), yolk = _piece_summary(out[2 * i + 1]) } end
    return res
end

--- true iff every covered atom of the batch -- its white, its yolk, by `types` -- is one piece
function SimulationHandler:is_whole(id, reach, types)
    local res = self:pieces({ id }, reach, types)
    if res == nil then return nil end
    return (res[1].white == nil or res[1].white.pieces == 1) and (res[1].yolk == nil or res[1].yolk.pieces == 1)
end

--- `white, yolk`: 0-based `int32_t` arrays with the label of every particle in particle order -- the lowest index in the
--- batch among the particles of its piece --, -1 throughout for a type that `types` leaves out; and their lengths
function SimulationHandler:piece_labels(reach, types)
    local spec = self:_pieces_spec(reach, types, "piece_labels")
    if spec == nil then return nil end
    local n_white, n_yolk = ffi.new("int64_t[1]"), ffi.new("int64_t[1]")
    if self:_check(lib.egg_get_n_particles(self._h, -1, n_white, n_yolk)) ~= 0 then return nil end
    local nw, ny = tonumber(n_white[0]), tonumber(n_yolk[0])
    local white, yolk = ffi.new("int32_t[?]", math.max(nw, 1)), ffi.new("int32_t[?]", math.max(ny, 1))
    local out = ffi.new("egg_piece_summary[?]", math.max(2 * #self:list_ids(), 1))
    if self:_check(lib.egg_pieces(self._h, spec, 0, nil, out, white, yolk)) ~= 0 then return nil end
    return white, yolk, nw, ny
end

-- Not in the reference: impulses (egg_impulse in include/eggsim_impulse.h; DESIGN.md section 2.12).  Act on the particles: the
-- committed velocities of the particles inside a region are edited on the device, now; either solver order.  Only vx and vy
-- change; nothing is stored.
-- include/eggsim_impulse.h, the header include/eggsim.h brings along
ffi.cdef[[
typedef struct { egg_sensor region; int32_t action, flags; int64_t id; double a[3]; } egg_impulse_record;
typedef struct { int64_t count[2], sdvx[2], sdvy[2], skipped[2]; } egg_impulse_result;
int egg_impulse(egg_handle *h, int32_t n, const egg_impulse_record *list, egg_impulse_result *results);
]]
local _impulse_actions = { kick = 0, blast = 1, swirl = 2, brake = 3 }
local _impulse_n_params = { [0] = 2, 3, 3, 3 }
local _max_impulses = 64 -- EGG_MAX_IMPULSES
local _impulse_scale = 65536 -- EGG_IMPULSE_SCALE
local _impulse_all_batches = -1 -- EGG_IMPULSE_ALL_BATCHES

--- an ordered list of at most 64 records `{ action, region, params..., id = nil, linear = false, by_inv_mass = false }`:
--- `{ "kick", region, ax, ay }`, `{ "blast", region, cx, cy, s }`, `{ "swirl", region, cx, cy, omega }`,
--- `{ "brake", region, ux, uy, k }`, the region in the shape set_sensors takes.  Returns per record
--- `{ white = { count, dvx, dvy, skipped }, yolk = { ... } }` by name, dvx / dvy the summed change of velocity in px/s
--- (`tonumber(sdvx) / 2^16`); with `want_results == false` nothing is finished or copied and the call returns true.
function SimulationHandler:impulse(records, want_results)
    local n = #records
    if n > _max_impulses then
        log.error("In SimulationHandler.impulse: a call takes 0 .. 64 records")
        return nil
    end
    local arr = ffi.new("egg_impulse_record[?]", math.max(n, 1))
    for k, r in ipairs(records) do
        local action = _impulse_actions[r[1]]
        if action == nil or #r ~= 2 + _impulse_n_params[action] or not _fill_region(arr[k - 1].region, r[2]) then
            log.error("In SimulationHandler.impulse: record " .. k .. ": expected { action, region, parameters..., id = ..., linear = ..., by_inv_mass = ... }")
            return nil
        end
        arr[k - 1].action = action
        arr[k - 1].flags = (r.linear and 1 or 0) + (r.by_inv_mass and 2 or 0)
        arr[k - 1].id = r.id or _impulse_all_batches
        for q = 1, _impulse_n_params[action] do arr[k - 1].a[q - 1] = r[q + 2] end
    end
    if want_results == false then
        if self:_check(lib.egg_impulse(self._h, n, arr, nil)) ~= 0 then return nil end
        return true
    end
    local out = ffi.new("egg_impulse_result[?]", math.max(n, 1))
    if self:_check(lib.egg_impulse(self._h, n, arr, out)) ~= 0 then return nil end
    local res = {}
    for k = 0, n - 1 do
        local one = {}
        for w, name in ipairs({ "white", "yolk" }) do
            one[name] = { count = tonumber(out[k].count[w - 1]), skipped = tonumber(out[k].skipped[w - 1]),
                          dvx = tonumber(out[k].sdvx[w - 1]) / _impulse_scale, dvy = tonumber(out[k].sdvy[w - 1]) / _impulse_scale }
        end
        res[k + 1] = one
    end
    return res
end

--- the particles inside `region` get (ax, ay) added to their velocity; `opts = { id, linear, by_inv_mass }`
function SimulationHandler:kick(region, ax, ay, opts)
    opts = opts or {}
    local res = self:impulse({ { "kick", region, ax, ay, id = opts.id, linear = opts.linear, by_inv_mass = opts.by_inv_mass } })
    return res and res[1]
end

--- a blast of strength s px/s at (cx, cy) that falls off linearly to 0 at the distance R (s < 0 sucks)
function SimulationHandler:blast(cx, cy, R, s, opts)
    opts = opts or {}
    local res = self:impulse({ { "blast", { "disc", cx, cy, R, types = opts.types }, cx, cy, s, id = opts.id, linear = true, by_inv_mass = opts.by_inv_mass } })
    return res and res[1]
end

--- the particles within R of (cx, cy) get the velocity of a turn at omega rad/s about it added
function SimulationHandler:stir(cx, cy, R, omega, opts)
    opts = opts or {}
    local res = self:impulse({ { "swirl", { "disc", cx, cy, R, types = opts.types }, cx, cy, omega, id = opts.id, linear = opts.linear } })
    return res and res[1]
end

--- the particles inside `region` move their velocity the fraction k (default 1: a stop) towards (ux, uy) (default 0, 0)
function SimulationHandler:brake(region, k, ux, uy, opts)
    opts = opts or {}
    local res = self:impulse({ { "brake", region, ux or 0, uy or 0, k or 1, id = opts.id, linear = opts.linear } })
    return res and res[1]
end

-- Not in the reference: measures (egg_measure in include/eggsim_measure.h; DESIGN.md section 2.13).  What is this egg doing, as
-- a body: per batch and type 24 int64 summed on the device -- counts, position, mass, momentum, energy, the box, second
-- moments, angular momentum and reach -- from the committed state; either solver order.  A call stores nothing and only
-- observes.
-- include/eggsim_measure.h, the second header include/eggsim.h brings along (a level-1 long bracket: the third cdef block)
ffi.cdef[=[
typedef struct { egg_sensor region; int32_t flags, type_mask; } egg_measure_spec;
typedef struct {
    int64_t atom, n, dropped, sx, sy, sm, smx, smy, spx, spy, se, lo_x, lo_y, hi_x, hi_y, max_v2, ox_q, oy_q, dropped_central,
        sxx, sxy, syy, sl, max_reach;
} egg_measure_record;
int egg_measure(egg_handle *h, const egg_measure_spec *spec, int64_t n_ids, const int64_t *ids, egg_measure_record *out);
]=]
local _measure_scale = 65536 -- EGG_MEASURE_SCALE
local _measure_mass_scale = 4294967296 -- EGG_MEASURE_MASS_SCALE
local _measure_region = 1 -- EGG_MEASURE_REGION
local _measure_fields = { "atom", "n", "dropped", "sx", "sy", "sm", "smx", "smy", "spx", "spy", "se", "lo_x", "lo_y", "hi_x", "hi_y", "max_v2",
                          "ox_q", "oy_q", "dropped_central", "sxx", "sxy", "syy", "sl", "max_reach" }

-- a record as a table: the 24 integers by name (as Lua numbers: exact below 2^53) and what the host derives from them
local function _measure_of(rec)
    if rec.n == 0 then return nil end
    local one = {}
    for _, name in ipairs(_measure_fields) do one[name] = tonumber(rec[name]) end
    local S = _measure_scale
    one.kept = one.n - one.dropped
    one.mass = one.sm / _measure_mass_scale
    if one.kept > 0 then
        one.centroid = { (one.sx / S) / one.kept, (one.sy / S) / one.kept }
        one.bounds = { one.lo_x / S, one.lo_y / S, one.hi_x / S, one.hi_y / S }
    end
    one.momentum = { one.spx / S, one.spy / S }
    if one.mass > 0 then
        one.center_of_mass = { (one.smx / S) / one.mass, (one.smy / S) / one.mass }
        one.velocity = { one.momentum[1] / one.mass, one.momentum[2] / one.mass }
    end
    one.kinetic_energy = 0.5 * one.se / S
    one.max_speed = math.sqrt(one.max_v2 / S)
    one.origin = { one.ox_q / S, one.oy_q / S }
    one.reach = one.max_reach / S
    one.spin = one.sl / S
    local k = one.kept - one.dropped_central
    if k > 0 then -- the principal standard deviations and the angle of the major axis
        local cxx, cxy, cyy = (one.sxx / S) / k, (one.sxy / S) / k, (one.syy / S) / k
        local half, diff = 0.5 * (cxx + cyy), 0.5 * (cxx - cyy)
        local root = math.sqrt(diff * diff + cxy * cxy)
        one.axes = { math.sqrt(math.max(half + root, 0)), math.sqrt(math.max(half - root, 0)), 0.5 * math.atan2(2 * cxy, cxx - cyy) }
    end
    return one
end

--- per id of `ids` (nil: every batch of list_ids(), in that order) `{ white = measure or nil, yolk = measure or nil }`, a
--- measure the 24 integers of egg_measure_record by name plus `kept, mass, centroid, center_of_mass, momentum, velocity,
--- kinetic_energy, bounds, max_speed, origin, reach, spin, axes`; nil where no particle of the type is measured.  `region` (nil:
--- the whole atom) takes the shape set_sensors takes; types = "both" | "white" | "yolk".  An id may repeat.
function SimulationHandler:measure(ids, region, types)
    local spec = ffi.new("egg_measure_spec")
    local mask = _collider_types[types or "both"]
    if mask == nil or (region ~= nil and not _fill_region(spec.region, region)) then
        log.error("In SimulationHandler.measure: expected (ids, region, types) with region nil or a region as set_sensors takes it and types \"both\" | \"white\" | \"yolk\"")
        return nil
    end
    spec.type_mask = mask
    spec.flags = region ~= nil and _measure_region or 0
    local listed = ids or self:list_ids()
    local n = #listed
    local c_ids = ffi.new("int64_t[?]", math.max(n, 1))
    for i, id in ipairs(listed) do c_ids[i - 1] = id end
    local out = ffi.new("egg_measure_record[?]", math.max(2 * n, 1))
    if self:_check(lib.egg_measure(self._h, spec, n, c_ids, out)) ~= 0 then return nil end
    local res = {}
    for i = 0, n - 1 do res[i + 1] = { white = _measure_of(out[2 * i]), yolk = _measure_of(out[2 * i + 1]) } end
    return res
end

--- true iff every covered atom of the batch -- its white, its yolk, by `types` -- has max_speed <= speed
function SimulationHandler:at_rest(id, speed, types)
    local res = self:measure({ id }, nil, types)
    if res == nil then return nil end
    return (res[1].white == nil or res[1].white.max_speed <= speed) and (res[1].yolk == nil or res[1].yolk.max_speed <= speed)
end

-- Not in the reference: cover (egg_cover in include/eggsim_cover.h; DESIGN.md section 2.14).  The floor under the egg: every
-- committed particle's disc of radius scale * radius rastered into a caller-set grid -- per cell and type how many discs lie
-- over the cell's centre and, on request, the oldest batch among them; either solver order.  A call stores nothing and only
-- observes.
-- include/eggsim_cover.h, the third header include/eggsim.h brings along (declared from a string: the blocks above stay three)
local _cover_decls = [==[
typedef struct { double x0, y0, cell, scale; int32_t nx, ny, type_mask, path; } egg_cover_spec;
typedef struct { int32_t *cover; int32_t *owner; } egg_cover_planes;
typedef struct {
    int64_t inside[2], outside[2], dropped[2], hits[2], covered[2], covered_both, covered_any;
    int32_t units_lanes, units_wave, units_direct, reserved;
} egg_cover_totals;
int egg_cover(egg_handle *h, const egg_cover_spec *spec, const egg_cover_planes *host_planes, egg_cover_totals *totals);
]==]
ffi.cdef(_cover_decls)
local _cover_paths = { auto = 0, direct = 1, lanes = 2, wave = 3 }
local _cover_max_cells = 1048576 -- EGG_COVER_MAX_CELLS

--- the grid of `nx` x `ny` square cells of side `cell` whose cell (0, 0) has its lower corner at (x0, y0); `options` may hold
--- `scale` (1: the simulated discs, 12: the discs as they are drawn), `types = "both" | "white" | "yolk"`, `owner = true` and
--- `path = "auto" | "direct" | "lanes" | "wave"` (test hooks).  Returns `{ nx, ny, cell, cover, owner, inside, outside, dropped,
--- hits, covered, covered_both, covered_any, area, units_lanes, units_wave, units_direct }` by name: `cover` and `owner` (nil
--- without owner; -1: no disc) `int32_t` arrays laid out [2][ny][nx], 0-based, [0] white and [1] yolk -- the word of type w and
--- cell (ix, iy) is `(w * ny + iy) * nx + ix` --; `inside` .. `covered` are `{ white, yolk }` counts and `area` is
--- `{ white, yolk, both, any }` in px^2.
function SimulationHandler:cover(x0, y0, cell, nx, ny, options)
    options = options or {}
    local mask = _collider_types[options.types or "both"]
    local path = _cover_paths[options.path or "auto"]
    local scale = options.scale or 1.0
    if mask == nil or path == nil or type(scale) ~= "number" or type(nx) ~= "number" or type(ny) ~= "number" or nx < 1 or ny < 1
        or nx * ny > _cover_max_cells or nx ~= math.floor(nx) or ny ~= math.floor(ny) then
        log.error("In SimulationHandler.cover: expected (x0, y0, cell, nx, ny, { scale = ..., types = ..., owner = ..., path = ... }) with nx * ny in 1 .. 1048576")
        return nil
    end
    local words = 2 * nx * ny
    local spec = ffi.new("egg_cover_spec", { x0 = x0, y0 = y0, cell = cell, scale = scale, nx = nx, ny = ny, type_mask = mask, path = path })
    local cover = ffi.new("int32_t[?]", words)
    local owner = options.owner and ffi.new("int32_t[?]", words) or nil
    local planes = ffi.new("egg_cover_planes", { cover = cover, owner = owner })
    local totals = ffi.new("egg_cover_totals")
    if self:_check(lib.egg_cover(self._h, spec, planes, totals)) ~= 0 then return nil end
    local function pair(a) return { tonumber(a[0]), tonumber(a[1]) } end
    local covered, both, any = pair(totals.covered), tonumber(totals.covered_both), tonumber(totals.covered_any)
    local a = cell * cell
    return { nx = nx, ny = ny, cell = cell, cover = cover, owner = owner, inside = pair(totals.inside), outside = pair(totals.outside),
             dropped = pair(totals.dropped), hits = pair(totals.hits), covered = covered, covered_both = both, covered_any = any,
             area = { covered[1] * a, covered[2] * a, both * a, any * a },
             units_lanes = totals.units_lanes, units_wave = totals.units_wave, units_direct = totals.units_direct }
end

-- Not in the reference as a call: touches (egg_touches in include/eggsim_touch.h; DESIGN.md section 2.15).  Which eggs touch
-- which, how much and where: two particles of one type in different batches touch iff d2 <= (reach * (ra + rb))^2, the
-- predicate of the collision branch (L:1632-1653) when reach is the type's collision_overlap_factor; either solver order.  A
-- call stores nothing and only observes.
-- include/eggsim_touch.h, the fourth header include/eggsim.h brings along (declared from a string: the blocks above stay three)
local _touch_decls = [==[
typedef struct { double reach[2]; int32_t type_mask, flags; } egg_touch_spec;
typedef struct { int64_t key; int32_t type, count; } egg_touch_query;
typedef struct { int32_t slot, pairs, particles, dropped; int64_t other, sx, sy; } egg_touch_record;
int egg_touches(egg_handle *h, const egg_touch_spec *spec, int64_t n_ids, const int64_t *ids, int64_t cap, egg_touch_record *out, int64_t *n_out);
int egg_touches_of(egg_handle *h, const egg_touch_spec *spec, int64_t n_queries, const egg_touch_query *queries, const double *x,
                   const double *y, const double *r, int64_t cap, egg_touch_record *out, int64_t *n_out);
]==]
ffi.cdef(_touch_decls)

--- the egg_touch_spec of a call, or nil: `reach` nil (per type the config's collision_overlap_factor), a number (both types)
--- or `{ white, yolk }`
function SimulationHandler:_touch_spec(reach, types, scope)
    if reach == nil then
        reach = { self._white_config.collision_overlap_factor, self._yolk_config.collision_overlap_factor }
    end
    local pieces = self:_pieces_spec(reach, types, scope) -- (the same checks: a reach above 0 and finite, a known mask)
    if pieces == nil then return nil end
    return ffi.new("egg_touch_spec", { reach = { pieces.reach[0], pieces.reach[1] }, type_mask = pieces.type_mask, flags = 0 })
end

--- the records of one answer as `n` lists `{ white = {}, yolk = {} }` of `{ other, pairs, particles, dropped, x, y }` by name, in
--- ascending `other`; `call(cap, out, n_out)` is the entry point with everything before its buffer bound.  n_out is always the
--- size of the answer: a call whose buffer was short is made once more with that size.
function SimulationHandler:_touch_lists(n, call)
    local cap, n_out = 256, ffi.new("int64_t[1]")
    local out, rc
    while true do
        out = ffi.new("egg_touch_record[?]", math.max(cap, 1))
        n_out[0] = 0
        rc = call(cap, out, n_out)
        if rc < 0 and tonumber(n_out[0]) > cap then cap = tonumber(n_out[0]) else break end
    end
    if self:_check(rc) ~= 0 then return nil end
    local res = {}
    for i = 1, n do res[i] = { white = {}, yolk = {} } end
    for k = 0, tonumber(n_out[0]) - 1 do
        local rec = out[k]
        local kept = rec.pairs - rec.dropped
        local one = { other = tonumber(rec.other), pairs = rec.pairs, particles = rec.particles, dropped = rec.dropped }
        if kept > 0 then
            one.x = (tonumber(rec.sx) / (2 * kept)) / _sensor_scale
            one.y = (tonumber(rec.sy) / (2 * kept)) / _sensor_scale
        end
        local side = res[math.floor(rec.slot / 2) + 1]
        table.insert(rec.slot % 2 == 0 and side.white or side.yolk, one)
    end
    return res
end

--- per id of `ids` (nil: every batch of list_ids(), in that order; an id may repeat) `{ white = {...}, yolk = {...} }`: the OTHER
--- batches with a particle of that type touching one of this batch's, each `{ other, pairs, particles, dropped, x, y }` --
--- `pairs` touching pairs over `particles` distinct particles of the other batch, the contact point `x, y` (nil while every
--- pair was dropped).  Never across types, never inside a batch (pieces() covers that).
function SimulationHandler:touches(ids, reach, types)
    local spec = self:_touch_spec(reach, types, "touches")
    if spec == nil then return nil end
    local listed = ids or self:list_ids()
    local n = #listed
    if n == 0 then return {} end
    local c_ids = ffi.new("int64_t[?]", n)
    for i, id in ipairs(listed) do c_ids[i - 1] = id end
    return self:_touch_lists(n, function(cap, out, n_out) return lib.egg_touches(self._h, spec, n, c_ids, cap, out, n_out) end)
end

--- true iff batch `a` touches batch `b` in a covered type; with b nil the sorted ids of the batches that touch `a`
function SimulationHandler:touching(a, b, reach, types)
    local res = self:touches({ a }, reach, types)
    if res == nil then return nil end
    local seen, others = {}, {}
    for _, side in ipairs({ res[1].white, res[1].yolk }) do
        for _, t in ipairs(side) do
            if not seen[t.other] then
                seen[t.other] = true
                table.insert(others, t.other)
            end
        end
    end
    table.sort(others)
    if b == nil then return others end
    return seen[b] == true
end

--- what a caller-set list of discs `{ { x, y, r }, ... }` of the type `types` ("white" or "yolk"; default "white") touches:
--- `{ white = {...}, yolk = {...} }` as touches() gives for one id.  A batch whose id equals `key` is left out; nil leaves none out.
function SimulationHandler:touches_of(discs, reach, types, key)
    types = types or "white"
    local spec = self:_touch_spec(reach, types, "touches_of")
    if spec == nil then return nil end
    if types ~= "white" and types ~= "yolk" then
        log.error("In SimulationHandler.touches_of: types is \"white\" or \"yolk\"")
        return nil
    end
    local n = #discs
    local x, y, r = ffi.new("double[?]", math.max(n, 1)), ffi.new("double[?]", math.max(n, 1)), ffi.new("double[?]", math.max(n, 1))
    for i, d in ipairs(discs) do x[i - 1], y[i - 1], r[i - 1] = d[1], d[2], d[3] end
    local w = types == "white" and 0 or 1
    local query = ffi.new("egg_touch_query[1]", { { key = key or -1, type = w, count = n } })
    local res = self:_touch_lists(1, function(cap, out, n_out)
        return lib.egg_touches_of(self._h, spec, 1, query, x, y, r, cap, out, n_out)
    end)
    if res == nil then return nil end
    return res[1]
end

-- Not in the reference, which has no forces as it has no boundary: force fields of the relaxed step (egg_set_forces in
-- include/eggsim.h; DESIGN.md section 2.7, "Forces").  Relaxed order only.
local _force_kinds = { uniform = 0, radial = 1, vortex = 2 }
local _force_names = { [0] = "uniform", "radial", "vortex" }
local _force_n_params = { [0] = 2, 4, 4 }

--- the ordered list of at most 16 force fields as accelerations in px/s^2, each `{ "uniform", gx, gy }`,
--- `{ "radial", cx, cy, strength, R }` or `{ "vortex", cx, cy, strength, R }` with an optional
--- `types = "both" | "white" | "yolk"`; their sum accelerates every particle before the pre-solve of every sub-step of a
--- relaxed step.  `{}` clears the list.
function SimulationHandler:set_forces(forces)
    local n = #forces
    local arr = ffi.new("egg_force[?]", math.max(n, 1))
    for k, f in ipairs(forces) do
        local kind = _force_kinds[f[1]]
        local mask = _collider_types[f.types or "both"]
        if kind == nil or mask == nil or #f ~= 1 + _force_n_params[kind] then
            log.error("In SimulationHandler.set_forces: field " .. k .. ": expected { kind, parameters..., types = ... }")
            return
        end
        arr[k - 1].kind, arr[k - 1].type_mask = kind, mask
        for q = 1, _force_n_params[kind] do arr[k - 1].p[q - 1] = f[q + 1] end
    end
    self:_check(lib.egg_set_forces(self._h, n, arr))
end

--- the list as stored, in the shapes set_forces takes
function SimulationHandler:get_forces()
    local arr, n = ffi.new("egg_force[16]"), ffi.new("int32_t[1]")
    if self:_check(lib.egg_get_forces(self._h, 16, arr, n)) ~= 0 then return {} end
    local out = {}
    for k = 0, n[0] - 1 do
        local f = { _force_names[arr[k].kind], types = _collider_type_names[arr[k].type_mask] }
        for q = 1, _force_n_params[arr[k].kind] do f[q + 1] = arr[k].p[q - 1] end
        out[k + 1] = f
    end
    return out
end

-- Not in the reference, whose cohesion_strength moves nothing: XSPH viscosity of the relaxed step (egg_set_viscosity in
-- include/eggsim.h; DESIGN.md section 2.7, "Viscosity").  Relaxed order only.

--- a coefficient in [0, 1] per particle type, 0 (the default) = off: after the last collision pass of every sub-step of a
--- relaxed step a particle's displacement of the sub-step is blended with the weighted mean of its neighbours' within one
--- spatial-hash cell size, so motion relative to the neighbours dies out and common motion stays
function SimulationHandler:set_viscosity(white, yolk)
    local c = ffi.new("double[2]", white or 0, yolk or 0)
    self:_check(lib.egg_set_viscosity(self._h, c))
end

--- white, yolk: the coefficients as stored
function SimulationHandler:viscosity()
    local c = ffi.new("double[2]")
    self:_check(lib.egg_get_viscosity(self._h, c))
    return c[0], c[1]
end

--- white, yolk: distinct pairs within the cell size over the viscosity passes of committed steps
function SimulationHandler:viscosity_pairs()
    local pairs = ffi.new("int64_t[2]")
    self:_check(lib.egg_get_viscosity_pairs(self._h, pairs))
    return tonumber(pairs[0]), tonumber(pairs[1])
end

-- Not in the reference, whose white and yolk never see each other (L:1776-1786): white-yolk coupling of the relaxed step
-- (egg_set_coupling in include/eggsim.h; DESIGN.md section 2.7, "Coupling").  Relaxed order, one handle only.

--- factor >= 0 (0, the default, = off) and strength in [0, 1] (default 1): before the first collision pass of every
--- sub-step of a relaxed step, a white and a yolk particle closer than factor * (ra + rb) are pushed apart to that
--- distance; all pairs of both types couple, whatever their batch
function SimulationHandler:set_coupling(factor, strength)
    self:_check(lib.egg_set_coupling(self._h, factor or 0, strength or 1))
end

--- factor, strength: as stored
function SimulationHandler:coupling()
    local f, s = ffi.new("double[1]"), ffi.new("double[1]")
    self:_check(lib.egg_get_coupling(self._h, f, s))
    return f[0], s[0]
end

--- distinct white-yolk pairs that fired over the coupling passes of committed steps
function SimulationHandler:coupling_solves()
    local n = ffi.new("int64_t[1]")
    self:_check(lib.egg_get_coupling_solves(self._h, n))
    return tonumber(n[0])
end

-- White-yolk adhesion, the same-batch band of the coupling pass (egg_set_adhesion in include/eggsim.h; DESIGN.md section
-- 2.7, "Adhesion").  Relaxed order, one handle only.

--- reach >= 0 (0, the default, = off) and strength in [0, 1] (default 1): while coupling acts and reach > its factor, a
--- white and a yolk particle of one batch farther apart than factor * (ra + rb) but within reach * (ra + rb) are pulled
--- back to the coupling distance, never closer
function SimulationHandler:set_adhesion(reach, strength)
    self:_check(lib.egg_set_adhesion(self._h, reach or 0, strength or 1))
end

--- reach, strength: as stored
function SimulationHandler:adhesion()
    local r, s = ffi.new("double[1]"), ffi.new("double[1]")
    self:_check(lib.egg_get_adhesion(self._h, r, s))
    return r[0], s[0]
end

--- distinct white-yolk pairs whose adhesion branch fired over the coupling passes of committed steps
function SimulationHandler:adhesion_solves()
    local n = ffi.new("int64_t[1]")
    self:_check(lib.egg_get_adhesion_solves(self._h, n))
    return tonumber(n[0])
end

-- Yolk containment, a disc around the centroid of each batch's white (egg_set_containment in include/eggsim.h; DESIGN.md
-- section 2.7, "Containment").  Relaxed order; independent of coupling and adhesion.

--- factor >= 0 (0, the default, = off) and strength in [0, 1] (default 1): in every sub-step a yolk particle farther than
--- L = factor * (RMS radius of its batch's white) from the white's centroid goes back to L + (1 - strength) * (d - L)
function SimulationHandler:set_containment(factor, strength)
    self:_check(lib.egg_set_containment(self._h, factor or 0, strength or 1))
end

--- factor, strength: as stored
function SimulationHandler:containment()
    local f, s = ffi.new("double[1]"), ffi.new("double[1]")
    self:_check(lib.egg_get_containment(self._h, f, s))
    return f[0], s[0]
end

--- projections, one per (yolk particle, sub-step), over committed steps
function SimulationHandler:containment_hits()
    local n = ffi.new("int64_t[1]")
    self:_check(lib.egg_get_containment_hits(self._h, n))
    return tonumber(n[0])
end

function SimulationHandler:draw()
    -- in a LOVE host: feed :instances() and :get_environment() to the reference's shaders and canvas code
    -- (simulation_handler.lua:1995-2175); without a window use :render_to_image()
end

return SimulationHandler
