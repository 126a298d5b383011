/* The instanced-draw record of include/eggsim.h from a plain C99 caller: egg_instance has the layout of the reference's
 * data mesh (simulation_handler.lua:513-517: floatvec4, floatvec2, float = 28 bytes, no padding), and the five entry
 * points link.  Without a handle they return EGG_ERR_INVALID_ARGUMENT and touch nothing. */
#include <stddef.h>
#include <stdio.h>

#include "eggsim.h"

int main(void) {
    egg_instance one[2];
    float color[8];
    const egg_instance *data = NULL;
    const float *col = NULL;
    int64_t n = -1;
    uint64_t version = 0;
    printf("sizeof %d\n", (int)sizeof(egg_instance));
    printf("offsets %d %d %d %d %d %d %d\n", (int)offsetof(egg_instance, x), (int)offsetof(egg_instance, y),
           (int)offsetof(egg_instance, last_x), (int)offsetof(egg_instance, last_y), (int)offsetof(egg_instance, vx),
           (int)offsetof(egg_instance, vy), (int)offsetof(egg_instance, radius));
    printf("stride %d\n", (int)((char *)&one[1] - (char *)&one[0]));
    printf("null %d %d %d %d %d\n", egg_get_instances(NULL, EGG_WHITE, one, color, 2, &n, &version), egg_instances_begin(NULL, 3),
           egg_instances_end(NULL, EGG_WHITE, &data, &col, &n, &version),
           egg_group_get_instances(NULL, EGG_YOLK, one, color, 2, &n, &version),
           egg_draw_source_instances(NULL, EGG_YOLK, one, color, 2, &n));
    return 0;
}
