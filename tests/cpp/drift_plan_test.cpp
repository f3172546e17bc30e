// drift_plan_test.cpp -- csrc/drift_plan.h held against brute force, with g++ alone (no HIP):
//   the count formula against a walk over the outputs, for random pos, delta and F, delta = +-2^24, F = 0 and
//   pos >= F * 2^32; 0 <= pos' < step; counts and positions over random cuts of a stream; the table check's refusals
//   and the compiled table's row P; the servo's clamp and the frozen integrator; the plan's bounds.
// usage: drift_plan_test [rounds]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "drift_plan.h"

using namespace cmhip;

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            if (failures++ < 20)                                                 \
                fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
        }                                                                        \
    } while (0)

// outputs m = 0, 1, .. whose n = (pos + m * step) >> 32 lies below F, counted one by one
static uint32_t brute_count(uint64_t pos, int32_t delta, uint32_t F)
{
    const uint64_t step = DRIFT_ONE + (uint64_t)(int64_t)delta;
    uint32_t k = 0;
    for (uint64_t t = pos; (t >> 32) < F; t += step)
        k++;
    return k;
}

static int32_t pick_delta(std::mt19937_64 &rng)
{
    switch (rng() % 6) {
    case 0: return DRIFT_DELTA_MAX;
    case 1: return -DRIFT_DELTA_MAX;
    case 2: return 0;
    case 3: return (int32_t)(rng() % 3) - 1;
    default: return (int32_t)(rng() % (2u * DRIFT_DELTA_MAX + 1u)) - DRIFT_DELTA_MAX;
    }
}

static void test_counts(std::mt19937_64 &rng, int rounds)
{
    for (int i = 0; i < rounds; i++) {
        const int32_t delta = pick_delta(rng);
        const uint64_t step = DRIFT_ONE + (uint64_t)(int64_t)delta;
        const uint32_t F = (rng() % 8 == 0) ? (uint32_t)(rng() % 3) : (uint32_t)(rng() % 5000);
        uint64_t pos = rng() % step;
        if (rng() % 8 == 0)
            pos = ((uint64_t)F << 32) + rng() % 3 - (F && rng() % 2 ? 1 : 0);        // around the run's end
        if (rng() % 16 == 0)
            pos = rng() % 2 ? 0 : step - 1;
        const uint32_t k = drift_out_frames(pos, delta, F);
        CHECK(k == brute_count(pos, delta, F));
        if (pos >= ((uint64_t)F << 32))
            CHECK(k == 0);
        if (pos < step) {
            const uint64_t next = drift_next_pos(pos, delta, F);
            CHECK(next < step);
            if (k)
                CHECK(((pos + (uint64_t)(k - 1) * step) >> 32) < F);                 // the last output's frame exists
        }
    }
    CHECK(drift_out_frames(0, 0, 0) == 0 && drift_out_frames(5, 0, 0) == 0);
    CHECK(drift_out_frames(0, 0, 7) == 7 && drift_out_frames(1, 0, 7) == 7 && drift_out_frames(DRIFT_ONE, 0, 7) == 6);
    CHECK(drift_out_frames(0, -DRIFT_DELTA_MAX, 255) == 256);                        // F + 1
    CHECK(drift_out_frames(DRIFT_ONE - 1, DRIFT_DELTA_MAX, 1) == 1);
    CHECK(drift_out_frames(DRIFT_ONE, DRIFT_DELTA_MAX, 1) == 0);                     // frames, and no output
    CHECK(drift_out_frames(0, DRIFT_DELTA_MAX + 1, 9) == 0 && drift_out_frames(0, -DRIFT_DELTA_MAX - 1, 9) == 0);
    CHECK(drift_out_frames(0, -DRIFT_DELTA_MAX, 255u << 16) == (256u << 16));        // no 64-bit overflow on the way
}

// one stream cut at random: the counts add up to the count of the whole, and the mirror's totals follow
static void test_cuts(std::mt19937_64 &rng, int rounds)
{
    for (int i = 0; i < rounds; i++) {
        const int32_t delta = pick_delta(rng);
        const uint32_t F = (uint32_t)(rng() % 20000);
        DriftMirror m;
        m.init(2);
        m.delta[0] = m.delta[1] = delta;
        m.pos[0] = m.pos[1] = rng() % DRIFT_ONE;
        const uint32_t whole = m.advance(0, F);
        uint32_t left = F, sum = 0;
        while (left) {
            const uint32_t cut = rng() % 4 == 0 ? 0u : (uint32_t)(rng() % (left + 1));
            uint32_t rec[DRIFT_REC];
            m.record(1, cut, rec);
            const uint32_t k = m.advance(1, cut);
            CHECK(rec[0] == cut && rec[1] == k && (int32_t)rec[2] == delta);
            sum += k;
            left -= cut;
        }
        CHECK(sum == whole && m.pos[0] == m.pos[1]);
        CHECK(m.in_total[1] == F && m.out_total[1] == whole && m.in_total[0] == F);
        m.reset(1);
        CHECK(m.pos[1] == 0 && m.in_total[1] == 0 && m.out_total[1] == 0 && m.delta[1] == delta);
    }
}

static void test_table(std::mt19937_64 &rng)
{
    for (uint32_t phi = DRIFT_PHI_MIN; phi <= DRIFT_PHI_MAX; phi++)
        for (uint32_t T : {4u, 6u, 32u, 62u, 64u}) {
            const uint32_t P = 1u << phi, B = 65535u / T < 4096u ? 65535u / T : 4096u;
            std::vector<int16_t> h((size_t)P * T);
            for (auto &v : h)
                v = (int16_t)((rng() % 2 ? 1 : -1) * (int)(3 * B / 4 + rng() % (B / 4 + 1)));
            h[0] = 0;
            uint32_t where = 99999;
            CHECK(drift_table_check(phi, T, h.data(), &where) == DRIFT_TABLE_OK);
            h[0] = 1;
            CHECK(drift_table_check(phi, T, h.data(), &where) == DRIFT_TABLE_FIRST);
            h[0] = 0;
            const uint32_t row = (uint32_t)(rng() % P);
            std::vector<int16_t> g = h;
            for (uint32_t k = 0; k < T; k++)
                g[(size_t)row * T + k] = k < 2 ? (int16_t)-32768 : (int16_t)0;      // sum |h| = 65536
            if (row == 0)
                g[0] = 0, g[2] = -32768;
            CHECK(drift_table_check(phi, T, g.data(), &where) == DRIFT_TABLE_SUM && where == row);
            g[(size_t)row * T + 1] = -32767;                                         // 65535: allowed
            CHECK(drift_table_check(phi, T, g.data(), &where) == DRIFT_TABLE_OK);
            // the compiled table: every tap where the kernel looks for it, row P = row 0 moved by one tap
            std::vector<uint32_t> w(drift_table_words(phi, T), 0xdeadbeefu);
            drift_compile(phi, T, h.data(), w.data());
            const uint32_t rw = drift_row_words(T);
            CHECK((rw & 1u) == (T / 2u + 1u) % 2u && w.size() % 4 == 0 && w.size() >= (size_t)(P + 1) * rw);
            for (uint32_t p = 0; p <= P; p++)
                for (uint32_t k = 0; k < T; k++) {
                    const uint32_t d = w[(size_t)p * rw + k / 2];
                    const int16_t got = (int16_t)(k & 1 ? d & 0xffffu : d >> 16);
                    const int16_t want = p < P ? h[(size_t)p * T + k] : (k + 1 < T ? h[k + 1] : (int16_t)0);
                    CHECK(got == want);
                }
        }
    std::vector<int16_t> z(256 * 64, 0);
    CHECK(drift_table_check(4, 32, z.data(), nullptr) == DRIFT_TABLE_GEOMETRY);
    CHECK(drift_table_check(9, 32, z.data(), nullptr) == DRIFT_TABLE_GEOMETRY);
    CHECK(drift_table_check(7, 2, z.data(), nullptr) == DRIFT_TABLE_GEOMETRY);
    CHECK(drift_table_check(7, 66, z.data(), nullptr) == DRIFT_TABLE_GEOMETRY);
    CHECK(drift_table_check(7, 31, z.data(), nullptr) == DRIFT_TABLE_GEOMETRY);
    CHECK(drift_table_check(8, 64, z.data(), nullptr) == DRIFT_TABLE_OK);
}

static void test_servo(std::mt19937_64 &rng, int rounds)
{
    DriftServo v;
    CHECK(!drift_servo_init(&v, 0x80000000u, 1, 1, 1) && !drift_servo_init(&v, 1, 25, 1, 1) &&
          !drift_servo_init(&v, 1, 1, 25, 1) && !drift_servo_init(&v, 1, 1, 1, 0) &&
          !drift_servo_init(&v, 1, 1, 1, DRIFT_DELTA_MAX + 1));
    CHECK(drift_servo_init(&v, 1024, 14, 3, DRIFT_DELTA_MAX));
    CHECK(v.integ == 0 && v.delta == 0 && !v.clamped);
    // one step by hand: e = 10 -> raw = 10 * 2^14 + 10 * 2^3
    CHECK(drift_servo_step(&v, 1034) == 10 * 16384 + 80 && v.integ == 10 && !v.clamped);
    CHECK(drift_servo_step(&v, 1024 - 4) == -4 * 16384 + 6 * 8 && v.integ == 6);
    // far above the target: clamped at +limit, the integrator frozen however long it lasts
    for (int i = 0; i < 1000; i++) {
        CHECK(drift_servo_step(&v, 1024 + 100000) == DRIFT_DELTA_MAX && v.clamped == 1 && v.integ == 6);
    }
    CHECK(drift_servo_step(&v, 512) == -512 * 16384 - 506 * 8 && !v.clamped && v.integ == 6 - 512);  // free again at once
    CHECK(drift_servo_step(&v, -1) == v.delta && drift_servo_step(&v, (int64_t)1 << 31) == v.delta && v.integ == 6 - 512);
    drift_servo_reset(&v);
    CHECK(v.integ == 0 && v.delta == 0 && !v.clamped && v.target == 1024);
    for (int i = 0; i < rounds; i++) {
        DriftServo s;
        const int32_t limit = 1 + (int32_t)(rng() % DRIFT_DELTA_MAX);
        CHECK(drift_servo_init(&s, (uint32_t)(rng() % 100000), (uint32_t)(rng() % 25), (uint32_t)(rng() % 25), limit));
        for (int j = 0; j < 200; j++) {
            const int64_t before = s.integ, fill = (int64_t)(rng() % 200000);
            const int32_t d = drift_servo_step(&s, fill);
            CHECK(d >= -limit && d <= limit && d == s.delta);
            if (s.clamped)
                CHECK(s.integ == before && (d == limit || d == -limit));
            else
                CHECK(s.integ == before + fill - s.target);
        }
    }
}

static void test_plan()
{
    for (uint32_t phi = DRIFT_PHI_MIN; phi <= DRIFT_PHI_MAX; phi++)
        for (uint32_t T = DRIFT_T_MIN; T <= DRIFT_T_MAX; T += 2)
            for (uint32_t C = 1; C <= DRIFT_MAX_CH; C++)
                for (uint32_t out : {1u, 2u, 16u, 17u, 64u, 65u, 129u, 300u, 2048u, 2049u, 70000u}) {
                    const DriftPlan p = plan_drift(3, C, phi, T, out);
                    CHECK(!p.err && p.grid == 3 * p.chunks && p.block == DRIFT_BLOCK);
                    CHECK(p.tile_out >= 2 && !(p.tile_out & (p.tile_out - 1)) && p.tile_out <= DRIFT_TILE_MAX);
                    CHECK((uint64_t)p.chunks * p.tile_out >= out && (uint64_t)(p.chunks - 1) * p.tile_out < out);
                    CHECK(p.row > p.tile_in && !(p.row & 1u) && p.lds_bytes <= DRIFT_LDS_LIMIT);
                    CHECK(p.lds_bytes == (p.table_lds ? p.table_words * 4u : 0u) + 4u * C * p.row);
                    CHECK(p.table_lds == (2u * (out < p.tile_out ? out : p.tile_out) >= (1u << phi) + 1u ? 1u : 0u));
                    if (C <= 2)
                        CHECK((C * p.row) % 64u == 32u && p.fast == 1);
                    // the frames a tile can stage, at the largest step and the worst fraction
                    const uint64_t step = DRIFT_ONE + DRIFT_DELTA_MAX, tb = DRIFT_ONE - 1;
                    const uint64_t span = ((tb + (uint64_t)(p.tile_out - 1) * step) >> 32) - (tb >> 32) + 1 + (T - 1);
                    CHECK(span <= p.tile_in);
                }
    CHECK(plan_drift(1u << 30, 2, 7, 32, 4096).err == 1 && plan_drift(1u << 30, 2, 7, 32, 4096).grid == 0);
    CHECK(plan_drift(0, 2, 7, 32, 4096).grid == 0 && !plan_drift(0, 2, 7, 32, 4096).err);
    CHECK(plan_drift(1, 2, 7, 32, 0).grid == 0 && plan_drift(1, 17, 7, 32, 5).grid == 0);
}

int main(int argc, char **argv)
{
    const int rounds = argc > 1 ? atoi(argv[1]) : 2000;
    std::mt19937_64 rng(20261021);
    test_counts(rng, rounds * 10);
    test_cuts(rng, rounds);
    test_table(rng);
    test_servo(rng, rounds / 10 + 1);
    test_plan();
    if (failures) {
        fprintf(stderr, "drift plan: %d failures\n", failures);
        return 1;
    }
    printf("drift plan ok: %d rounds\n", rounds);
    return 0;
}
