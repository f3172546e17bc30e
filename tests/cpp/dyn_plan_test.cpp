// dyn_plan_test.cpp -- csrc/dyn_plan.h over every geometry and every level, as a stand-alone program: g++ alone compiles
// it (the header includes no HIP), tests/test_dyn_host.py runs it plainly and under AddressSanitizer + UBSan.
//   dyn_plan_test  ->  "plans ok: N geometries, 32769 levels"
#include <stdio.h>
#include <stdlib.h>

#include "dyn_plan.h"

using namespace cmhip;

#define CHECK(c)                                                                       \
    do {                                                                               \
        if (!(c)) {                                                                    \
            fprintf(stderr, "%s:%d: %s (a %u b %u hold %u channels %u level %u)\n", __FILE__, __LINE__, #c, a, b, hold, ch, l); \
            return 1;                                                                  \
        }                                                                              \
    } while (0)

// the header's index, case by case, with a plain loop for floor(log2 l)
static DynIndex index_by_the_book(uint32_t l)
{
    DynIndex r = {0, 0, 0};
    if (l == 0)
        return r;
    uint32_t E = 0;
    while ((2u << E) <= l)
        E++;
    if (E >= 3) {
        r.idx = 1 + 8 * E + ((l >> (E - 3)) & 7);
        r.frac = l & ((1u << (E - 3)) - 1);
        r.sh = E - 3;
    } else {
        r.idx = 1 + 8 * E + ((l << (3 - E)) & 7);
    }
    return r;
}

int main(void)
{
    unsigned long n = 0;
    uint32_t a = 0, b = 0, hold = 0, ch = 1, l = 0;
    DynGeom g;
    // the edges of the geometry
    CHECK(!dyn_geom(2, 6, 0, &g) && !dyn_geom(11, 6, 0, &g) && dyn_geom(3, 6, 0, &g) && dyn_geom(10, 6, 0, &g));
    CHECK(!dyn_geom(6, 2, 0, &g) && !dyn_geom(6, 10, 0, &g) && dyn_geom(6, 3, 0, &g) && dyn_geom(6, 9, 0, &g));
    CHECK(dyn_geom(6, 3, 2040, &g) && g.W == 2048 && !dyn_geom(6, 3, 2041, &g));
    CHECK(dyn_geom(10, 9, 1536, &g) && g.W == 2048 && g.hist == 3581 && g.halo == DYN_HALO_MAX && !dyn_geom(10, 9, 1537, &g));
    CHECK(!dyn_geom(6, 6, 0xffffffffu, &g) && !dyn_geom(0xffffffffu, 6, 0, &g) && !dyn_geom(6, 0xffffffffu, 0, &g));
    for (a = DYN_A_MIN; a <= DYN_A_MAX; a++) {
        const uint32_t A = 1u << a;
        for (b = DYN_B_MIN; b <= DYN_B_MAX; b++) {
            const uint32_t B = 1u << b;
            const uint32_t holds[] = {0, 1, DYN_W_MAX - B};
            for (uint32_t h = 0; h < 3; h++) {
                hold = holds[h];
                CHECK(dyn_geom(a, b, hold, &g) && !dyn_geom(a, b, DYN_W_MAX - B + 1, &g));
                CHECK(g.A == A && g.B == B && g.D == B - 1 && g.W == B + hold && g.hist == (A - 1) + (g.W - 1) + (B - 1));
                CHECK(g.halo >= g.hist && g.halo < g.hist + 8 && g.halo % 8 == 0 && g.halo <= DYN_HALO_MAX);
                CHECK(g.hist >= B);                                      // the delayed samples never lie in front of the slot
                uint32_t lw = 0;
                while ((2u << lw) <= g.W)
                    lw++;
                for (ch = 1; ch <= DYN_MAX_CH; ch++) {
                    const uint32_t frames[] = {1, 4095, 4096, 4097, 100000, 0x7fffffffu / ch};
                    for (uint32_t f : frames) {
                        const DynPlan p = plan_dyn(3, ch, a, b, hold, f);
                        CHECK(p.err == 0 && p.block == DYN_BLOCK && p.fast == (ch <= 2 ? 1u : 0u));
                        const uint32_t t = p.tile_frames;
                        CHECK(t >= g.halo && t <= DYN_TILE_MAX && (t & (t - 1)) == 0 && p.halo == g.halo);
                        CHECK(t == DYN_TILE_MAX);                        // 4096 + 3584 frames are 30 KiB: never shrunk
                        CHECK(p.lds_bytes == (t + g.halo) * 4 && p.lds_bytes <= DYN_LDS_LIMIT && p.lds_bytes <= 30720);
                        CHECK((t + g.halo) <= DYN_BLOCK * ((DYN_TILE_MAX + DYN_HALO_MAX) / DYN_BLOCK));
                        CHECK(p.chunks == (f + t - 1) / t && p.grid == 3 * p.chunks);
                        CHECK(p.passes == a + lw + ((g.W & (g.W - 1)) ? 1u : 0u) + b);
                        n++;
                    }
                }
                ch = 1;
            }
        }
    }
    a = 6; b = 6; hold = 0; ch = 2;
    // no grid of 2^31 workgroups; nothing to launch for an empty run or a bad geometry
    CHECK(plan_dyn(1u << 20, 2, 6, 6, 0, 1u << 23).err == 1 && plan_dyn(1u << 20, 2, 6, 6, 0, 1u << 23).grid == 0);
    CHECK(plan_dyn(1u << 20, 2, 6, 6, 0, (1u << 23) - 4096).err == 0);
    CHECK(plan_dyn(1u << 20, 2, 6, 6, 0, (1u << 23) - 4096).grid == (1u << 20) * ((1u << 11) - 1));
    CHECK(plan_dyn(0, 2, 6, 6, 0, 100).grid == 0 && plan_dyn(4, 2, 6, 6, 0, 0).grid == 0 && plan_dyn(4, 0, 6, 6, 0, 100).grid == 0);
    CHECK(plan_dyn(4, 17, 6, 6, 0, 100).grid == 0 && plan_dyn(4, 2, 2, 6, 0, 100).grid == 0 && plan_dyn(4, 2, 6, 9, 1537, 100).grid == 0);
    CHECK(plan_dyn(4, 2, 11, 6, 0, 100).grid == 0 && plan_dyn(4, 2, 6, 10, 0, 100).grid == 0 && plan_dyn(4, 2, 2, 6, 0, 100).err == 0);

    // the curve's index: against the book for every level; monotone, at most 121, frac 0 at every knot, frac < 2^sh
    uint32_t prev = 0, knots = 0;
    for (l = 0; l <= DYN_UNITY; l++) {
        const DynIndex i = dyn_index(l), w = index_by_the_book(l);
        CHECK(i.idx == w.idx && i.frac == w.frac && i.sh == w.sh);
        CHECK(i.idx >= prev && i.idx <= prev + 8 && i.idx <= DYN_KNOT_MAX && i.frac < (1u << i.sh));
        if (i.idx != prev || l == 0) {                                   // the first level of a knot is the knot itself
            CHECK(i.frac == 0);
            if (i.idx >= 1) {
                const uint32_t k = i.idx - 1, m = 8 + k % 8, e = k / 8;  // level (8 + k % 8) * 2^(k / 8 - 3)
                CHECK(e >= 3 ? l == m << (e - 3) : l << (3 - e) == m);
            }
            knots++;
        }
        prev = i.idx;
    }
    l = DYN_UNITY;
    CHECK(prev == DYN_KNOT_MAX && dyn_index(DYN_UNITY).frac == 0 && DYN_KNOT_MAX + 1 < DYN_CURVE_USED);
    CHECK(knots == 1 + 1 + 2 + 4 + 8 * 12 + 1);                          // 0; 1; 2, 3; 4..7; 8 per octave from 8 on; 32768

    // what a set asks of a table
    uint16_t T[DYN_CURVE];
    for (uint32_t k = 0; k < DYN_CURVE; k++)
        T[k] = (uint16_t)DYN_UNITY;
    CHECK(dyn_curve_ok(T));
    const uint32_t bad[] = {0, 57, 122};
    for (uint32_t k : bad) {
        T[k] = 32769;
        CHECK(!dyn_curve_ok(T));
        T[k] = 0;
    }
    for (uint32_t k = DYN_CURVE_USED; k < DYN_CURVE; k++)
        T[k] = 65535;
    CHECK(dyn_curve_ok(T));
    // a lookup between two knots: levels 40 and 44 are neighbours
    for (uint32_t k = 0; k < DYN_CURVE_USED; k++)
        T[k] = (uint16_t)(1000 + 10 * k);
    CHECK(dyn_curve_at(T, 0) == 1000 && dyn_curve_at(T, DYN_UNITY) == 1000 + 10 * DYN_KNOT_MAX);
    CHECK(dyn_index(42).idx == dyn_index(40).idx && dyn_index(42).frac == 2 && dyn_index(42).sh == 2);
    CHECK(dyn_index(44).idx == dyn_index(40).idx + 1 && dyn_index(44).frac == 0);
    CHECK(dyn_curve_at(T, 42) == dyn_curve_at(T, 40) + 5 && dyn_curve_at(T, 43) == dyn_curve_at(T, 40) + 7);
    for (uint32_t k = 0; k < DYN_CURVE_USED; k++)
        T[k] = (uint16_t)(30000 - 10 * k);                               // falling: the shift is arithmetic
    CHECK(dyn_curve_at(T, 43) == dyn_curve_at(T, 40) - 8);               // (-10 * 3) >> 2 = -8
    printf("plans ok: %lu geometries, %u levels\n", n, DYN_UNITY + 1);
    return 0;
}
