// limtp_plan_test.cpp -- csrc/lim_plan.h for the limiter's true-peak detector over every geometry, as a stand-alone
// program: g++ alone compiles it (the header includes no HIP), tests/test_limtp_host.py runs it plainly and under
// AddressSanitizer + UBSan.  The sample detector's entry points are held against their own formulas beside it.
//   limtp_plan_test  ->  "plans ok: N geometries"
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
    LimGeom g, o;
    // the edges of the geometry
    CHECK(!lim_geom_tp(2, 1, &g) && !lim_geom_tp(10, 1, &g) && lim_geom_tp(3, 1, &g) && lim_geom_tp(9, 1, &g));
    CHECK(!lim_geom_tp(3, 0, &g) && !lim_geom_tp(9, 0, &g) && !lim_geom_tp(6, 0, nullptr));
    CHECK(lim_geom_tp(3, 2040, &g) && g.W == 2048 && g.hist == 2067 && !lim_geom_tp(3, 2041, &g));
    CHECK(lim_geom_tp(8, 1792, &g) && g.W == 2048 && g.hist == 2315 && !lim_geom_tp(8, 1793, &g));
    CHECK(lim_geom_tp(9, 1525, &g) && g.W == 2037 && g.hist == 2560 && g.halo == LIM_HALO_MAX && g.D == 519);
    CHECK(!lim_geom_tp(9, 1526, &g) && lim_geom(9, 1526, &g));
    CHECK(!lim_geom_tp(3, 0xffffffffu, &g) && !lim_geom_tp(0xffffffffu, 1, &g));
    CHECK(lim_geom_of(0, 6, 0, &g) && !lim_geom_of(1, 6, 0, &g) && lim_geom_of(1, 6, 1, &g) && !lim_geom_of(2, 6, 1, &g));
    CHECK(!lim_geom_of(0xffffffffu, 6, 1, &g));
    CHECK(LIM_TP_AW_MAX == 2549);
    for (a = LIM_A_MIN; a <= LIM_A_MAX; a++) {
        const uint32_t A = 1u << a;
        for (hold = 0; hold <= LIM_W_MAX - A; hold++) {
            const bool ok = hold >= 1 && 2 * A + hold <= 2549;
            CHECK(lim_geom_tp(a, hold, &g) == ok);
            CHECK(lim_geom(a, hold, &o) && o.D == A - 1 && o.hist == A + o.W - 2 && o.halo == ((o.hist + 7) & ~7u));
            if (!ok) {
                CHECK(plan_limtp(3, 1, a, hold, 100).grid == 0 && plan_limtp(3, 1, a, hold, 100).err == 0);
                continue;
            }
            CHECK(g.a == a && g.A == A && g.D == A + 7 && g.H == hold && g.W == A + hold && g.hist == A + g.W - 2 + 13);
            CHECK((g.D + 1) % 8 == 0 && g.D <= g.hist);
            CHECK(g.halo >= g.hist && g.halo < g.hist + 8 && g.halo % 8 == 0 && g.halo <= LIM_HALO_MAX && g.halo >= 16);
            for (ch = 1; ch <= LIM_MAX_CH; ch += (hold % 97 == 0 ? 1 : 5)) {
                const uint32_t frames[] = {1, 4095, 4096, 4097, 100000, 0x7fffffffu / ch};
                for (uint32_t f : frames) {
                    const LimPlan p = plan_limtp(3, ch, a, hold, f);
                    CHECK(p.err == 0 && p.block == LIM_BLOCK && p.fast == (ch <= 2 ? 1u : 0u));
                    const uint32_t t = p.tile_frames;
                    CHECK(t >= g.halo && t <= LIM_TILE_MAX && (t & (t - 1)) == 0 && p.halo == g.halo);
                    CHECK(p.lds_bytes == (t + g.halo) * 4 && p.lds_bytes <= LIM_LDS_LIMIT);
                    CHECK((t + g.halo) <= LIM_BLOCK * ((LIM_TILE_MAX + LIM_HALO_MAX) / LIM_BLOCK));
                    CHECK(p.chunks == (f + t - 1) / t && p.grid == 3 * p.chunks);
                    // the fast forms: ceil(NV / 256) own vectors per thread, at most 4 (mono) / 7 (stereo)
                    if (ch <= 2)
                        CHECK(((t + g.halo) * ch / 8 + LIM_BLOCK - 1) / LIM_BLOCK <= (26 * ch + 7) / 8);
                    // the sample detector's plan of the same numbers is what it was
                    const LimPlan q = plan_lim(3, ch, a, hold, f);
                    CHECK(q.err == 0 && q.halo == o.halo && q.tile_frames == t && q.lds_bytes == (t + o.halo) * 4);
                    CHECK(q.chunks == p.chunks && q.grid == p.grid && q.fast == p.fast && q.block == LIM_BLOCK);
                    n++;
                }
            }
            ch = 1;
        }
    }
    a = 6; hold = 1; ch = 2;
    // no grid of 2^31 workgroups; nothing to launch for an empty run or a bad geometry
    CHECK(plan_limtp(1u << 20, 2, 6, 1, 1u << 23).err == 1 && plan_limtp(1u << 20, 2, 6, 1, 1u << 23).grid == 0);
    CHECK(plan_limtp(1u << 20, 2, 6, 1, (1u << 23) - 4096).err == 0);
    CHECK(plan_limtp(1u << 20, 2, 6, 1, (1u << 23) - 4096).grid == (1u << 20) * ((1u << 11) - 1));
    CHECK(plan_limtp(0, 2, 6, 1, 100).grid == 0 && plan_limtp(4, 2, 6, 1, 0).grid == 0 && plan_limtp(4, 0, 6, 1, 100).grid == 0);
    CHECK(plan_limtp(4, 17, 6, 1, 100).grid == 0 && plan_limtp(4, 2, 2, 1, 100).grid == 0 && plan_limtp(4, 2, 9, 1526, 100).grid == 0);
    CHECK(plan_limtp(4, 2, 6, 0, 100).grid == 0 && plan_limtp(4, 2, 6, 0, 100).err == 0);
    CHECK(plan_lim_of(2, 4, 2, 6, 1, 100).grid == 0 && plan_lim_of(0, 4, 2, 6, 0, 100).grid == 4);
    printf("plans ok: %lu geometries\n", n);
    return 0;
}
