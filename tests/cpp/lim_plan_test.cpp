// lim_plan_test.cpp -- csrc/lim_plan.h over every geometry, as a stand-alone program: g++ alone compiles it (the header
// includes no HIP), tests/test_lim_host.py runs it plainly and under AddressSanitizer + UBSan.
//   lim_plan_test  ->  "plans ok: N geometries"
#include <stdio.h>
#include <stdlib.h>

#include "lim_plan.h"

using namespace cmhip;

#define CHECK(c)                                                                       \
    do {                                                                               \
        if (!(c)) {                                                                    \
            fprintf(stderr, "%s:%d: %s (a %u hold %u channels %u)\n", __FILE__, __LINE__, #c, a, hold, ch); \
            return 1;                                                                  \
        }                                                                              \
    } while (0)

int main(void)
{
    unsigned long n = 0;
    uint32_t a = 0, hold = 0, ch = 1;
    LimGeom g;
    // the edges of the geometry
    CHECK(!lim_geom(2, 0, &g) && !lim_geom(10, 0, &g) && lim_geom(3, 0, &g) && lim_geom(9, 0, &g));
    CHECK(lim_geom(3, 2040, &g) && g.W == 2048 && !lim_geom(3, 2041, &g));
    CHECK(lim_geom(9, 1536, &g) && g.W == 2048 && g.hist == 2558 && g.halo == LIM_HALO_MAX && !lim_geom(9, 1537, &g));
    CHECK(!lim_geom(3, 0xffffffffu, &g) && !lim_geom(0xffffffffu, 0, &g));
    CHECK(lim_params_ok(1, 1) && lim_params_ok(32767, 65535) && !lim_params_ok(0, 1) && !lim_params_ok(32768, 1));
    CHECK(!lim_params_ok(1, 0) && !lim_params_ok(1, 65536));
    for (a = LIM_A_MIN; a <= LIM_A_MAX; a++) {
        const uint32_t A = 1u << a;
        for (hold = 0; hold <= LIM_W_MAX - A; hold++) {
            CHECK(lim_geom(a, hold, &g));
            CHECK(g.A == A && g.D == A - 1 && g.W == A + hold && g.hist == A + g.W - 2);
            CHECK(g.halo >= g.hist && g.halo < g.hist + 8 && g.halo % 8 == 0 && g.halo <= LIM_HALO_MAX);
            for (ch = 1; ch <= LIM_MAX_CH; ch += (hold % 97 == 0 ? 1 : 5)) {
                const uint32_t frames[] = {1, 4095, 4096, 4097, 100000, 0x7fffffffu / ch};
                for (uint32_t f : frames) {
                    const LimPlan p = plan_lim(3, ch, a, hold, f);
                    CHECK(p.err == 0 && p.block == LIM_BLOCK && p.fast == (ch <= 2 ? 1u : 0u));
                    const uint32_t t = p.tile_frames;
                    CHECK(t >= g.halo && t <= LIM_TILE_MAX && (t & (t - 1)) == 0 && p.halo == g.halo);
                    CHECK(p.lds_bytes == (t + g.halo) * 4 && p.lds_bytes <= LIM_LDS_LIMIT);
                    CHECK((t + g.halo) <= LIM_BLOCK * ((LIM_TILE_MAX + LIM_HALO_MAX) / LIM_BLOCK));
                    CHECK(p.chunks == (f + t - 1) / t && p.grid == 3 * p.chunks);
                    n++;
                }
            }
            ch = 1;
        }
    }
    a = 6; hold = 0; ch = 2;
    // no grid of 2^31 workgroups; nothing to launch for an empty run or a bad geometry
    CHECK(plan_lim(1u << 20, 2, 6, 0, 1u << 23).err == 1 && plan_lim(1u << 20, 2, 6, 0, 1u << 23).grid == 0);
    CHECK(plan_lim(1u << 20, 2, 6, 0, (1u << 23) - 4096).err == 0);
    CHECK(plan_lim(1u << 20, 2, 6, 0, (1u << 23) - 4096).grid == (1u << 20) * ((1u << 11) - 1));
    CHECK(plan_lim(0, 2, 6, 0, 100).grid == 0 && plan_lim(4, 2, 6, 0, 0).grid == 0 && plan_lim(4, 0, 6, 0, 100).grid == 0);
    CHECK(plan_lim(4, 17, 6, 0, 100).grid == 0 && plan_lim(4, 2, 2, 0, 100).grid == 0 && plan_lim(4, 2, 9, 1537, 100).grid == 0);
    CHECK(plan_lim(4, 2, 2, 0, 100).err == 0);
    printf("plans ok: %lu geometries\n", n);
    return 0;
}
