// eggsim_group_draw.h -- what eggsim_group.cpp (plain C++, a client of include/eggsim.h) and
// eggsim_host_render_group.hip share: the calls behind egg_group_render, egg_group_render_canvas,
// egg_group_get_environment, egg_group_download_particles and egg_group_get_instances.  0 or an EGG_ERR_* code; on failure *error has the reason.
#pragma once
#include <cstdint>
#include <string>

#include "../../include/eggsim.h"

namespace egghost {

struct GroupDraw;  // device side of a group's draws: shadow arrays, run tables, canvases (on the device of handle 0)

// The group's own records, as one call needs them.  Render attributes live in the group, not in its handles.
struct GroupView {
    egg_handle *const *hs = nullptr;
    int n = 0;
    const egg_render_config *cfg = nullptr;  // [2]
    int use_particle_color = 0, use_lighting = 1;
    const float *pcolor = nullptr;           // [ids issued][2][4]: the rgba the particles of batch `id - 1` carry, per type
    int64_t n_ids = 0;
    bool stepped = false;                    // the group has run a _step
    double alpha = 0;                        // its interpolation_alpha (egg_group_update)
};

GroupDraw *group_draw_create();
void group_draw_destroy(GroupDraw *d);
int group_draw_render(GroupDraw *d, const GroupView &v, const egg_render_params *p, float *rgba, std::string *error);
int group_draw_canvas(GroupDraw *d, const GroupView &v, int which, float *rgba, int64_t cap_pixels, int32_t *w, int32_t *hgt, double *x0,
                      double *y0, std::string *error);
int group_draw_environment(GroupDraw *d, const GroupView &v, int which, egg_environment *out, std::string *error);
int group_draw_download(GroupDraw *d, const GroupView &v, int which, int field, double *dst, int64_t cap, std::string *error);
int group_draw_instances(GroupDraw *d, const GroupView &v, int which, egg_instance *data, float *color, int64_t cap, int64_t *n,
                         std::string *error);

}  // namespace egghost
