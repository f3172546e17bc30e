// dyn_rms_test.cpp -- what csrc/dyn_plan.h adds for the RMS detector, as a stand-alone program: g++ alone compiles it (the
// header includes no HIP), tests/test_dyn_rms_host.py runs it plainly and under AddressSanitizer + UBSan.
//   dyn_isqrt against r * r <= v < (r + 1) * (r + 1) for every v in 0 .. 2^30 (what a mean square can be) and, thinned,
//   up to 2^32 - 1 (what a dword can hold); with DYN_RMS_THIN defined the first range is thinned too: every r * r,
//   r * r - 1, r * r + 1, r * r + 2 r and a stride between them.
//   dyn_mean_square: the two 32-bit sums of the split squares against one 64-bit sum, for extreme and for random inputs.
//   plan_dyn with the RMS detector over every geometry and channel count.
//   dyn_rms_test  ->  "rms ok: N roots, M sums, P plans"
#include <stdio.h>
#include <stdlib.h>

#include "dyn_plan.h"

using namespace cmhip;

#define CHECK(c)                                                                       \
    do {                                                                               \
        if (!(c)) {                                                                    \
            fprintf(stderr, "%s:%d: %s (v %llu a %u b %u hold %u channels %u)\n", __FILE__, __LINE__, #c, \
                    (unsigned long long)v, a, b, hold, ch);                            \
            return 1;                                                                  \
        }                                                                              \
    } while (0)

static bool root_ok(uint64_t v)
{
    const uint64_t r = dyn_isqrt((uint32_t)v);
    return r * r <= v && v < (r + 1) * (r + 1);
}

int main(void)
{
    unsigned long roots = 0, sums = 0, plans = 0;
    uint64_t v = 0;
    uint32_t a = 0, b = 0, hold = 0, ch = 1;

    // ---- the root
#ifdef DYN_RMS_THIN
    for (v = 0; v <= (1ull << 30); v += 997) {
        CHECK(root_ok(v));
        roots++;
    }
#else
    for (v = 0; v <= (1ull << 30); v++) {
        CHECK(root_ok(v));
        roots++;
    }
#endif
    for (uint64_t r = 0; r <= 65535; r++) {                              // every edge a 32-bit value has
        const uint64_t edges[] = {r * r, r * r + 1, r * r + 2 * r, r * r + r, r ? r * r - 1 : 0};
        for (uint64_t e : edges) {
            v = e;
            CHECK(v <= 0xffffffffull && root_ok(v));
            roots++;
        }
        v = r * r;
        CHECK(dyn_isqrt((uint32_t)v) == r && dyn_isqrt((uint32_t)(v + 2 * r)) == r);
        CHECK(r == 0 || dyn_isqrt((uint32_t)(v - 1)) == r - 1);
    }
    for (v = 1ull << 30; v <= 0xffffffffull; v += 65521) {               // a stride through the rest of a dword
        CHECK(root_ok(v));
        roots++;
    }
    v = 0xffffffffull;
    CHECK(dyn_isqrt(0xffffffffu) == 65535 && dyn_isqrt(0xfffe0001u) == 65535 && dyn_isqrt(0xfffe0000u) == 65534);
    CHECK(dyn_isqrt(0) == 0 && dyn_isqrt(1) == 1 && dyn_isqrt(3) == 1 && dyn_isqrt(4) == 2 && dyn_isqrt(1u << 30) == 32768);
    CHECK(dyn_isqrt((1u << 30) - 1) == 32767 && dyn_isqrt(23170u * 23170u) == 23170 && dyn_isqrt(23170u * 23170u - 1) == 23169);

    // ---- the sum of squares from its halves: A frames of magnitudes e[k], hi and lo summed apart in 32 bits
    uint32_t lcg = 2463534242u;
    for (a = DYN_A_MIN; a <= DYN_A_MAX; a++) {
        const uint32_t A = 1u << a;
        for (uint32_t kind = 0; kind < 40; kind++) {
            uint64_t wide = 0;
            uint32_t sum_hi = 0, sum_lo = 0;
            for (uint32_t k = 0; k < A; k++) {
                uint32_t e;
                lcg = lcg * 1664525u + 1013904223u;
                switch (kind) {
                case 0: e = 32768; break;                                // the largest sum: A * 2^30
                case 1: e = 32767; break;                                // lo and hi both near their tops
                case 2: e = 181; break;                                  // 32761: the largest square below 2^15, hi = 0
                case 3: e = 182; break;                                  // 33124: the first with hi = 1
                case 4: e = 0; break;
                case 5: e = k & 1 ? 32768 : 32767; break;
                case 6: e = k == A - 1 ? 32767 : 32768; break;           // one below the top
                case 7: e = k == 0 ? 1 : 0; break;                       // a mean square of 0 from a sum that is not
                default: e = (lcg >> 8) % 32769u; break;
                }
                const uint32_t q = e * e;
                wide += (uint64_t)e * e;
                sum_hi += q >> DYN_SQ_SPLIT;
                sum_lo += q & ((1u << DYN_SQ_SPLIT) - 1u);
                v = wide;
                CHECK(sum_hi <= (1u << 25) && sum_lo < (1u << 25));
            }
            v = wide;
            CHECK(wide <= (1ull << 40) && ((uint64_t)sum_hi << DYN_SQ_SPLIT) + sum_lo == wide);
            const uint32_t M = dyn_mean_square(sum_hi, sum_lo, a);
            CHECK(M == (uint32_t)(wide >> a) && M <= (1u << 30));
            CHECK(kind != 0 || (M == (1u << 30) && dyn_isqrt(M) == 32768));
            CHECK(kind != 1 || dyn_isqrt(M) == 32767);
            CHECK(kind != 6 || dyn_isqrt(M) == 32767);                   // just below 2^30
            CHECK(kind != 7 || M == 0);
            sums++;
        }
    }

    // ---- the plan: the mean detector's tile, grid and LDS, a more passes
    v = 0;
    for (a = DYN_A_MIN; a <= DYN_A_MAX; a++)
        for (b = DYN_B_MIN; b <= DYN_B_MAX; b++) {
            const uint32_t B = 1u << b;
            const uint32_t holds[] = {0, 1, DYN_W_MAX - B};
            for (uint32_t h = 0; h < 3; h++) {
                hold = holds[h];
                for (ch = 1; ch <= DYN_MAX_CH; ch++) {
                    const uint32_t frames[] = {1, 4096, 4097, 100000};
                    for (uint32_t f : frames) {
                        const DynPlan m = plan_dyn(3, ch, a, b, hold, f), p = plan_dyn(3, ch, a, b, hold, f, DYN_DETECT_RMS);
                        const DynPlan m0 = plan_dyn(3, ch, a, b, hold, f, DYN_DETECT_MEAN);
                        CHECK(p.err == 0 && p.grid == m.grid && p.block == m.block && p.chunks == m.chunks && p.fast == m.fast);
                        CHECK(p.tile_frames == m.tile_frames && p.halo == m.halo && p.lds_bytes == m.lds_bytes);
                        CHECK(p.lds_bytes == (p.tile_frames + p.halo) * 4 && p.lds_bytes <= 65536 && p.lds_bytes <= 30720);
                        CHECK(p.passes == m.passes + a && m0.passes == m.passes && m0.grid == m.grid);
                        plans++;
                    }
                }
                ch = 1;
            }
        }
    a = 6; b = 6; hold = 0; ch = 2;
    CHECK(plan_dyn(4, 2, 6, 6, 0, 100, 2).grid == 0 && plan_dyn(4, 2, 6, 6, 0, 100, 0xffffffffu).grid == 0);
    CHECK(plan_dyn(1u << 20, 2, 6, 6, 0, 1u << 23, DYN_DETECT_RMS).err == 1);
    printf("rms ok: %lu roots, %lu sums, %lu plans\n", roots, sums, plans);
    return 0;
}
