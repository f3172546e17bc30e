// iir_ramp_test.cpp -- csrc/iir_ramp.h on its own (g++, no HIP; tests/test_iir_ramp_host.py builds it plain and under
// AddressSanitizer + UBSan): the section between two ends at EVERY position against the stability check, its two ends,
// the zero on z = 1 and a 128-bit restatement of the header's rule; the position, also as the kernels keep it (done and
// inc), against the mixer's formula restated; and the mirror through sequences of start, retarget, set and advance
// against a plain restatement.
//
//   iir_ramp_test [random pairs]
#include "iir_ramp.h"

#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

using namespace cmhip;

#define CHECK(c)                                                                   \
    do {                                                                           \
        if (!(c)) {                                                                \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c);  \
            exit(1);                                                               \
        }                                                                          \
    } while (0)

static std::mt19937_64 rng(4711);
static int64_t pick(int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); }

static bool same(const IirSec &a, const IirSec &b)
{
    return a.b0 == b.b0 && a.b1 == b.b1 && a.b2 == b.b2 && a.a1 == b.a1 && a.a2 == b.a2;
}

// ---- the rule restated in 128 bits, divisions instead of shifts
typedef __int128 i128;
static i128 toward_zero(i128 n, i128 d) { return n / d; }                 // (C++ division truncates)
static i128 upward(i128 n, i128 d) { return n / d + (n % d > 0 ? 1 : 0); }
static IirSec restated(const IirSec &c0, const IirSec &c1, uint32_t p)
{
    const i128 q = 32768 - (i128)p, P = p, D = 32768;
    const i128 b0 = toward_zero(c0.b0 * q + c1.b0 * P, D), b2 = toward_zero(c0.b2 * q + c1.b2 * P, D);
    const i128 a1 = toward_zero(c0.a1 * q + c1.a1 * P, D), a2 = upward(c0.a2 * q + c1.a2 * P, D);
    const i128 s0 = (i128)c0.b0 + c0.b1 + c0.b2, s1 = (i128)c1.b0 + c1.b1 + c1.b2;
    i128 b1 = toward_zero(s0 * q + s1 * P, D) - b0 - b2;
    b1 = b1 < -(i128)IIR_COEF_MAX ? -(i128)IIR_COEF_MAX : b1 > (i128)IIR_COEF_MAX ? (i128)IIR_COEF_MAX : b1;
    return IirSec{(int32_t)b0, (int32_t)b1, (int32_t)b2, (int32_t)a1, (int32_t)a2};
}

// the mixer's position restated: floor(n ceil(2^32 / R) / 2^17), at most 32768
static uint32_t position_restated(uint32_t n, uint32_t R)
{
    if (n == 0)
        return 0;
    if (R < 2 || n >= R)
        return 32768;
    const i128 inc = (((i128)1 << 32) + R - 1) / R;
    const i128 p = (i128)n * inc / 131072;
    return p > 32768 ? 32768u : (uint32_t)p;
}

static unsigned long long pairs_checked = 0, clamped = 0, over_by_most = 0;

// every p of a pair of valid ends
static void check_pair(const IirSec &c0, const IirSec &c1)
{
    CHECK(iir_section_ok(c0) && iir_section_ok(c1));
    const bool zero = iir_ramp_sum(c0) == 0 && iir_ramp_sum(c1) == 0;
    for (uint32_t p = 0; p <= IIR_RAMP_ONE; p++) {
        const IirSec c = iir_ramp_section(c0, c1, p);
        CHECK(iir_section_ok(c));
        CHECK(same(c, restated(c0, c1, p)));
        if (zero)
            CHECK((int64_t)c.b0 + c.b1 + c.b2 == 0);
        const int64_t raw = (int64_t)iir_ramp_trunc(iir_ramp_sum(c0), iir_ramp_sum(c1), p) - c.b0 - c.b2;
        if (raw != c.b1) {
            clamped++;
            const unsigned long long by = (unsigned long long)((raw < 0 ? -raw : raw) - IIR_COEF_MAX);
            over_by_most = by > over_by_most ? by : over_by_most;
        }
    }
    CHECK(same(iir_ramp_section(c0, c1, 0), c0) && same(iir_ramp_section(c0, c1, IIR_RAMP_ONE), c1));
    CHECK(same(iir_ramp_section(c0, c1, IIR_RAMP_ONE + 1), c1) && same(iir_ramp_section(c0, c1, 0xffffffffu), c1));
    pairs_checked++;
}

static IirSec random_section(int kind)
{
    const int64_t top = kind == 0 ? IIR_COEF_MAX : IIR_ONE;
    IirSec c;
    c.b0 = (int32_t)pick(-top, top);
    c.b1 = (int32_t)pick(-top, top);
    c.b2 = (int32_t)pick(-top, top);
    c.a2 = (int32_t)pick(-(IIR_ONE - 1), IIR_ONE - 1);
    const int64_t edge = (int64_t)IIR_ONE + c.a2 - 1;            // the largest |a1|
    c.a1 = (int32_t)(kind == 1 ? (pick(0, 1) ? edge : -edge) : pick(-edge, edge));
    if (kind == 2) {                                             // a zero on z = 1
        c.b0 = (int32_t)pick(-IIR_ONE, IIR_ONE);
        c.b2 = (int32_t)pick(-IIR_ONE, IIR_ONE);
        c.b1 = -(c.b0 + c.b2);
    }
    if (kind == 3) {                                             // b at the range's corners, off by a little
        c.b0 = (int32_t)(pick(0, 1) ? IIR_COEF_MAX - pick(0, 3) : -IIR_COEF_MAX + pick(0, 3));
        c.b1 = pick(0, 1) ? IIR_COEF_MAX : -IIR_COEF_MAX;
        c.b2 = (int32_t)(pick(0, 1) ? IIR_COEF_MAX - pick(0, 3) : -IIR_COEF_MAX + pick(0, 3));
    }
    return c;
}

static void check_sections(int rounds)
{
    const int32_t one = IIR_ONE, big = IIR_COEF_MAX;
    // the triangle's corners and edges, coefficients at +-2^28
    const std::vector<IirSec> fixed = {
        IIR_UNITY, {0, 0, 0, 0, 0}, {big, big, big, 0, 0}, {-big, -big, -big, 0, 0}, {big, -big, big, 0, 0},
        {big, big, big, 2 * one - 2, one - 1}, {-big, big, -big, -(2 * one - 2), one - 1}, {0, 0, 0, 0, -(one - 1)},
        {1, 2, 3, 1, -(one - 2)}, {1, 2, 3, -1, -(one - 2)}, {0, 0, 0, one - 1, 0}, {0, 0, 0, -(one - 1), 0},
        {big, big, big, (1 << 27) - 2, one - 1}, {-big, big, -big, -((1 << 27) - 2), one - 1}, {3, big, 3, 0, 0},
        {0, big, 0, 0, 0}, {-3, -big, -3, 1, 1}, {big - 1, big, big - 1, -1, -1}, {one, -2 * one, one, -(2 * one - 2), one - 1},
    };
    for (const IirSec &a : fixed)
        for (const IirSec &b : fixed)
            check_pair(a, b);
    CHECK(clamped > 0);
    for (int r = 0; r < rounds; r++) {
        const int ka = (int)pick(0, 3), kb = r % 3 == 0 ? ka : (int)pick(0, 3);
        check_pair(random_section(ka), random_section(kb));
    }
    CHECK(over_by_most <= 1);                                    // the clamp acts in corners only, and takes 1 at most
}

static void check_position()
{
    const uint32_t Rs[] = {0, 1, 2, 3, 4, 5, 7, 63, 64, 65, 480, 1000, 44100, 65535, 65536, 65537, (1u << 20) - 1, 1u << 20};
    for (uint32_t R : Rs) {
        if (R >= 2)
            CHECK(iir_ramp_inc(R) == (uint32_t)((((uint64_t)1 << 32) + R - 1) / R));
        uint32_t before = 0;
        for (uint32_t n = 0; n <= R + 3 && n < 70000; n++) {
            const uint32_t p = iir_ramp_position(n, R);
            CHECK(p == position_restated(n, R) && p >= before && p <= IIR_RAMP_ONE);
            before = p;
        }
        if (R >= 2) {                                            // n near R, also of the longest ramp
            for (uint32_t n = R - 2; n <= R + 2; n++)
                CHECK(iir_ramp_position(n, R) == position_restated(n, R));
            CHECK(iir_ramp_position(R, R) == IIR_RAMP_ONE && (R > 32768 || iir_ramp_position(R - 1, R) < IIR_RAMP_ONE));
            CHECK(iir_ramp_position(1, R) == (R <= 2 ? 16384u : position_restated(1, R)));
        }
        // as the kernels keep it: frame f of a run that the section enters at `done`
        const uint32_t dones[] = {0, 1, R / 2, R > 2 ? R - 2 : 0, R > 1 ? R - 1 : 0, R, R + 1};
        for (uint32_t done : dones) {
            const IirRampClock c = iir_ramp_clock(done, R);
            const bool ramping = done < R && R >= 2;
            const uint32_t fs[] = {0, 1, 2, 63, 64, R > done ? R - done - 1 : 0, R - done, R - done + 1, 0x7ffffffeu - (1u << 20)};
            for (uint32_t f : fs) {
                if (f > 0x7fffffffu)
                    continue;
                const uint32_t want = ramping ? position_restated(done + f + 1, R) : IIR_RAMP_ONE;
                CHECK(iir_ramp_at(c, f) == want);
            }
        }
    }
    // every n of the longest ramp's last stretch, and a sweep of a middle-sized one through both forms
    for (uint32_t n = (1u << 20) - 70000; n <= (1u << 20) + 2; n++)
        CHECK(iir_ramp_position(n, 1u << 20) == position_restated(n, 1u << 20));
    const IirRampClock c = iir_ramp_clock(0, 44100);
    for (uint32_t f = 0; f < 50000; f++)
        CHECK(iir_ramp_at(c, f) == iir_ramp_position(f + 1, 44100));
}

// ---- the mirror against a plain restatement
struct Plain {
    IirSec c0 = IIR_UNITY, c1 = IIR_UNITY;
    uint64_t done = 0, R = 0;
    IirSec now() const { return done < R ? restated(c0, c1, position_restated((uint32_t)done, (uint32_t)R)) : c1; }
    void ramp(const IirSec &c, uint32_t frames)
    {
        c0 = now();
        c1 = c;
        done = 0;
        R = frames;
    }
    void set(const IirSec &c)
    {
        c0 = c1 = c;
        done = R = 0;
    }
    void advance(uint32_t n)
    {
        if (done >= R)
            return;
        done = done + n > R ? R : done + n;
        if (done == R) {
            c0 = c1;
            done = R = 0;
        }
    }
};

static void check_mirror()
{
    const uint32_t Rs[] = {2, 3, 64, 1u << 20};
    IirRampMirror m;
    m.init(3);
    Plain plain[3];
    auto agree = [&]() {
        size_t active = 0;
        for (size_t i = 0; i < 3; i++) {
            CHECK(same(m.now(i), plain[i].now()) && m.e[i].done == plain[i].done && m.e[i].R == plain[i].R);
            CHECK(m.ramping(i) == (plain[i].done < plain[i].R));
            CHECK(iir_section_ok(m.now(i)));
            active += m.ramping(i);
        }
        CHECK(m.active == active && m.any() == (active != 0));
    };
    agree();
    for (uint32_t R : Rs) {
        const uint32_t steps[] = {0, 1, R - 1, R, R + 1, 0, R / 2, 0xffffffffu};
        for (int round = 0; round < 40; round++) {
            for (size_t i = 0; i < 3; i++) {
                const int what = (int)pick(0, 5);
                const IirSec c = random_section((int)pick(0, 3));
                if (what <= 2) {                                 // a ramp, or a retarget of one that runs
                    m.start(i, c, R);
                    plain[i].ramp(c, R);
                } else if (what == 3) {
                    m.cancel(i, c);
                    plain[i].set(c);
                }
                agree();
                const uint32_t n = steps[(size_t)pick(0, 7)];
                m.advance(i, n);
                plain[i].advance(n);
                agree();
            }
        }
        // one section step by step to the end of its ramp and past it
        const IirSec to = random_section(1);
        m.start(0, to, R);
        plain[0].ramp(to, R);
        const uint32_t stride = R > 1000 ? R / 7 + 1 : 1;
        for (uint64_t at = 0; at < (uint64_t)R + 2 * stride; at += stride) {
            agree();
            m.advance(0, stride);
            plain[0].advance(stride);
        }
        agree();
        CHECK(!m.ramping(0) && same(m.now(0), to));
        // n near the end of the ramp, also of the longest one
        m.start(1, to, R);
        plain[1].ramp(to, R);
        m.advance(1, R - 1);
        plain[1].advance(R - 1);
        agree();
        CHECK(m.ramping(1) && m.e[1].done == R - 1);
        m.advance(1, 0);
        plain[1].advance(0);
        agree();
        m.advance(1, 1);
        plain[1].advance(1);
        agree();
        CHECK(!m.ramping(1) && m.e[1].R == 0);
    }
}

int main(int argc, char **argv)
{
    const int rounds = argc > 1 ? atoi(argv[1]) : 300;
    check_position();
    check_sections(rounds);
    check_mirror();
    printf("iir ramp ok: %llu pairs at every p, %llu clamped b1 (by at most %llu)\n", pairs_checked, clamped, over_by_most);
    return 0;
}
