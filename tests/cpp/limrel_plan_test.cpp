// limrel_plan_test.cpp -- csrc/lim_plan.h for the limiter's release stage over every (lookahead, release) pair, both
// detectors, as a stand-alone program: g++ alone compiles it (the header includes no HIP), tests/test_limrel_host.py runs
// it plainly and under AddressSanitizer + UBSan.  release_log2 0 is held against the plans without the stage.
//   limrel_plan_test  ->  "plans ok: N geometries"
#include <stdio.h>
#include <stdlib.h>

#include "lim_plan.h"

using namespace cmhip;

#define CHECK(c)                                                                       \
    do {                                                                               \
        if (!(c)) {                                                                    \
            fprintf(stderr, "%s:%d: %s (detector %u a %u hold %u rho %u channels %u)\n", __FILE__, __LINE__, #c, det, a, \
                    hold, rho, ch);                                                    \
            return 1;                                                                  \
        }                                                                              \
    } while (0)

// the largest hold a geometry allows, or -1 when hold 0 (1 for the true-peak detector) is already too much
static long top_hold(uint32_t det, uint32_t a, uint32_t rho)
{
    const long A = 1l << a, R = 1l << rho, front = det ? 13 : 0;
    long top = 2048 - A;                                              // W <= 2048
    if (det && 2549 - 2 * A < top)
        top = 2549 - 2 * A;                                           // A + W <= 2549
    if (4096 - (2 * A - 2 + R - 1 + front) < top)
        top = 4096 - (2 * A - 2 + R - 1 + front);                     // HIST <= 4096
    return top < (det ? 1 : 0) ? -1 : top;
}

int main(void)
{
    unsigned long n = 0;
    uint32_t det = 0, a = 0, hold = 0, rho = 0, ch = 1;
    LimGeom g, o;
    // the edges the header names
    CHECK(LIMREL_RHO_MAX == 11 && LIMREL_HIST_MAX == 4096 && LIMREL_SLOTS == 32);
    CHECK(lim_geom_rel(0, 9, 1027, 11, &g) && g.hist == 4096 && g.halo == 4096 && g.D == 511 && g.W == 1539);
    CHECK(!lim_geom_rel(0, 9, 1028, 11, &g) && !lim_geom_rel(0, 9, 1028, 11, nullptr));
    CHECK(lim_geom_rel(1, 9, 1014, 11, &g) && g.hist == 4096 && g.halo == 4096 && g.D == 519);
    CHECK(!lim_geom_rel(1, 9, 1015, 11, &g) && !lim_geom_rel(1, 9, 0, 11, &g) && !lim_geom_rel(1, 6, 0, 0, &g));
    CHECK(lim_geom_rel(0, 6, 0, 11, &g) && !lim_geom_rel(0, 6, 0, 12, &g) && !lim_geom_rel(0, 6, 0, 0xffffffffu, &g));
    CHECK(!lim_geom_rel(2, 6, 1, 5, &g) && !lim_geom_rel(0, 2, 0, 5, &g) && !lim_geom_rel(0, 10, 0, 5, &g));
    CHECK(!lim_geom_rel(0, 6, 1985, 1, &g) && !lim_geom_rel(0, 6, 0xffffffffu, 1, &g));
    for (det = 0; det <= 1; det++)
        for (a = LIM_A_MIN; a <= LIM_A_MAX; a++)
            for (rho = 0; rho <= LIMREL_RHO_MAX; rho++) {
                const uint32_t A = 1u << a, R = 1u << rho;
                const long top = top_hold(det, a, rho);
                CHECK(top >= (long)det);                              // every (a, rho) has a geometry
                CHECK(!lim_geom_rel(det, a, (uint32_t)top + 1u, rho, &g));
                const uint32_t holds[] = {0, 1, (uint32_t)top};
                for (uint32_t h : holds) {
                    hold = h;
                    if (det && hold == 0) {
                        CHECK(!lim_geom_rel(det, a, hold, rho, &g) && plan_limrel(det, 3, 1, a, hold, rho, 100).grid == 0);
                        continue;
                    }
                    CHECK(lim_geom_rel(det, a, hold, rho, &g) && lim_geom_of(det, a, hold, &o));
                    CHECK(g.a == a && g.A == A && g.H == hold && g.W == A + hold && g.D == o.D);
                    CHECK(g.hist == o.hist + R - 1 && g.hist == 2 * A + hold - 2 + R - 1 + (det ? 13u : 0u));
                    CHECK(g.hist <= LIMREL_HIST_MAX && g.halo >= g.hist && g.halo < g.hist + 8 && g.halo % 8 == 0);
                    CHECK((g.D + 1) % 8 == 0 && g.D <= g.hist);
                    for (ch = 1; ch <= LIM_MAX_CH; ch++) {
                        const uint32_t frames[] = {1, 4095, 4096, 4097, 100000, 0x7fffffffu / ch};
                        for (uint32_t f : frames) {
                            const LimPlan p = plan_limrel(det, 3, ch, a, hold, rho, f);
                            const LimPlan q = plan_lim_of(det, 3, ch, a, hold, f);
                            CHECK(p.err == 0 && p.block == LIM_BLOCK && p.fast == (ch <= 2 ? 1u : 0u));
                            CHECK(p.tile_frames == LIM_TILE_MAX && p.halo == g.halo && p.halo <= p.tile_frames);
                            CHECK(p.lds_bytes == (p.tile_frames + g.halo) * 4 && p.lds_bytes <= 32u * 1024u);
                            CHECK(p.tile_frames + g.halo <= LIM_BLOCK * LIMREL_SLOTS);   // the elements a thread keeps
                            CHECK(p.chunks == (f + 4095) / 4096 && p.grid == 3 * p.chunks);
                            if (ch <= 2)                             // own vectors per thread: at most 4 (mono), 8 (stereo)
                                CHECK(((p.tile_frames + g.halo) * ch / 8 + LIM_BLOCK - 1) / LIM_BLOCK <=
                                      (LIMREL_SLOTS * ch + 7) / 8);
                            if (rho == 0)                            // the limiter without the stage, field by field
                                CHECK(p.err == q.err && p.fast == q.fast && p.grid == q.grid && p.block == q.block &&
                                      p.chunks == q.chunks && p.tile_frames == q.tile_frames &&
                                      p.lds_bytes == q.lds_bytes && p.halo == q.halo);
                            // the plans without the stage are what they were
                            CHECK(q.halo == o.halo && q.lds_bytes == (q.tile_frames + o.halo) * 4 && o.halo <= LIM_HALO_MAX);
                            n++;
                        }
                    }
                    ch = 1;
                }
            }
    det = 0; a = 6; hold = 0; rho = 5; ch = 2;
    // no grid of 2^31 workgroups; nothing to launch for an empty run or a bad geometry
    CHECK(plan_limrel(0, 1u << 20, 2, 6, 0, 5, 1u << 23).err == 1 && plan_limrel(0, 1u << 20, 2, 6, 0, 5, 1u << 23).grid == 0);
    CHECK(plan_limrel(1, 1u << 20, 2, 6, 1, 5, (1u << 23) - 4096).err == 0);
    CHECK(plan_limrel(1, 1u << 20, 2, 6, 1, 5, (1u << 23) - 4096).grid == (1u << 20) * ((1u << 11) - 1));
    CHECK(plan_limrel(0, 0, 2, 6, 0, 5, 100).grid == 0 && plan_limrel(0, 4, 2, 6, 0, 5, 0).grid == 0);
    CHECK(plan_limrel(0, 4, 0, 6, 0, 5, 100).grid == 0 && plan_limrel(0, 4, 17, 6, 0, 5, 100).grid == 0);
    CHECK(plan_limrel(0, 4, 2, 6, 0, 12, 100).grid == 0 && plan_limrel(0, 4, 2, 6, 0, 12, 100).err == 0);
    CHECK(plan_limrel(0, 4, 2, 9, 1028, 11, 100).grid == 0 && plan_limrel(0, 4, 2, 9, 1027, 11, 100).grid == 4);
    CHECK(plan_limrel(2, 4, 2, 6, 1, 5, 100).grid == 0 && plan_limrel(1, 4, 2, 6, 0, 5, 100).grid == 0);
    printf("plans ok: %lu geometries\n", n);
    return 0;
}
