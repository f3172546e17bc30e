// delay_plan_test.cpp -- csrc/delay_plan.h over random geometries and positions, compiled by g++ alone (no HIP):
//   - every index a run forms stays inside the stream's input slot and inside its ring, aligned vectors included;
//   - the ring samples a run writes are exactly [P, P + N) mod CAP, each once, in whole 16-byte granules between a head
//     and a ragged end; the ring samples it USES are exactly [P - D, P) mod CAP restricted to the outputs in front of
//     the seam, and no sample is both read and written: one launch is free of races;
//   - the sample every output takes is x[n - d] of a plain list of all samples;
//   - the mirror against a model written out in full: positions, ramps, their ends, sets.
//   usage: delay_plan_test [iterations]
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "delay_plan.h"

using namespace cmhip;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}
static uint32_t pick(uint32_t lo, uint32_t hi) { return lo + rnd() % (hi - lo + 1u); }

#define CHECK(c)                                                                                                      \
    do {                                                                                                              \
        if (!(c)) {                                                                                                   \
            fprintf(stderr, "%s:%d: %s failed (iteration %lu)\n", __FILE__, __LINE__, #c, iteration);                 \
            exit(1);                                                                                                  \
        }                                                                                                             \
    } while (0)

static unsigned long iteration;

// one run of one stream as the kernel forms its indices; `all` is every sample the stream was given, the run's included
static void run_once(uint32_t C, uint32_t max_delay, uint32_t max_frames, uint32_t pos, uint32_t count, uint32_t d,
                     const std::vector<int> &ring_holds /* per ring sample: index into all, or -1 */, size_t first)
{
    const DelayPlan p = plan_delay(1, C, max_delay, max_frames, count ? count : 1);
    CHECK(p.err == 0 && p.ring_frames >= max_delay + max_frames && p.ring_frames % 8 == 0);
    const uint32_t CAP = p.ring_frames * C, P = pos * C, N = count * C, D = d * C;
    const uint32_t in_vecs = (max_frames * C + 7u) / 8u;                 // the smallest stride a run may have
    const uint32_t tile = p.tile_vecs * 8u;
    CHECK(tile == p.tile_frames * C && (uint64_t)D + N <= CAP);
    std::vector<char> wrote(CAP, 0), used(CAP, 0);

    auto fetch = [&](uint32_t nvec, uint32_t a, uint32_t sh, uint32_t i, bool *ok) {      // sample i of the shifted vector
        const uint32_t v = a + (sh + i) / 8u;
        *ok = v < nvec && ((sh + i) / 8u == 0 || sh != 0);
        return v * 8u + (sh + i) % 8u;
    };

    const uint32_t h = delay_ring_head(P);
    CHECK((P + h) % 8 == 0 && h < 8);
    for (uint32_t i = 0; i < h && i < N; i++) {                          // the head
        const uint32_t r = delay_ring_index(P, CAP, i);
        CHECK(r < CAP && !wrote[r]);
        wrote[r] = 1;
    }
    for (uint32_t e0 = 0; e0 < N; e0 += tile) {
        const uint32_t len = N - e0 < tile ? N - e0 : tile;
        const DelayTap tap = delay_tap(e0, len, D, P, CAP);
        CHECK(tap.cls <= DELAY_MIXED);
        for (uint32_t t = 0; t < p.tile_vecs; t++) {
            const uint32_t e = e0 + 8u * t;
            // in a mixed tile every vector is classified again by itself; its first source vector is then its own
            const DelayTap vt = tap.cls == DELAY_MIXED ? delay_tap(e, 8, D, P, CAP) : tap;
            const uint32_t va = tap.cls == DELAY_MIXED ? vt.q >> 3 : (tap.q >> 3) + t;
            if (tap.cls == DELAY_MIXED && vt.cls != DELAY_MIXED)
                CHECK((vt.q & 7u) == ((vt.cls == DELAY_BEHIND ? 0u - D : P + CAP - D % CAP) & 7u));     // the tile's shift
            for (uint32_t i = 0; i < 8 && e + i < N; i++) {              // the outputs the run owns
                const uint32_t ee = e + i;
                long src;                                                // index into `all`
                if (vt.cls == DELAY_BEHIND || (vt.cls == DELAY_MIXED && ee >= D)) {
                    uint32_t at = ee - D;
                    if (vt.cls == DELAY_BEHIND) {
                        bool ok;
                        at = fetch(in_vecs, va, vt.q & 7u, i, &ok);
                        CHECK(ok);
                    }
                    CHECK(at < N && at == ee - D);
                    src = (long)first + at;
                } else {
                    uint32_t r = delay_ring_index(P, CAP, (int64_t)ee - (int64_t)D);
                    if (vt.cls == DELAY_FRONT) {
                        bool ok;
                        const uint32_t at = fetch(CAP / 8u, va, vt.q & 7u, i, &ok);
                        CHECK(ok && at == r);
                    }
                    CHECK(r < CAP);
                    used[r] = 1;
                    src = ring_holds[r];
                }
                CHECK(src == (long)first + (long)ee - (long)D || (src < 0 && (long)first + (long)ee - (long)D < 0));
            }
            // the ring's granule of this vector: samples e + h .. e + h + 7 of the run
            const uint32_t es = e + h;
            if (es < N) {
                const uint32_t r = delay_ring_index(P, CAP, es), n = N - es < 8 ? N - es : 8;
                CHECK(r % 8 == 0 && r + 8 <= CAP);
                for (uint32_t i = 0; i < n; i++) {
                    bool ok;
                    const uint32_t at = fetch(in_vecs, e >> 3, h, i, &ok);
                    CHECK(ok && at == es + i && !wrote[r + i]);
                    wrote[r + i] = 1;
                }
            }
        }
    }
    for (uint32_t r = 0; r < CAP; r++) {
        const uint32_t off = delay_wrap((uint64_t)r + CAP - P, CAP);     // r = (P + off) mod CAP
        CHECK(wrote[r] == (off < N ? 1 : 0));
        CHECK(!(wrote[r] && used[r]));
        if (used[r])
            CHECK(CAP - off <= D);                                       // inside [P - D, P)
    }
}

struct Stream {
    uint32_t pos = 0;
    std::vector<int> holds;            // per ring sample: index into the list of all samples, -1: zero
    size_t given = 0;                  // samples so far
};

int main(int argc, char **argv)
{
    const unsigned long iterations = argc > 1 ? strtoul(argv[1], nullptr, 10) : 1000;
    unsigned long runs = 0;
    for (iteration = 0; iteration < iterations; iteration++) {
        const uint32_t C = pick(1, 16);
        const uint32_t t = C <= 2 ? DELAY_FAST_VECS * 8u / C : DELAY_ANY_FRAMES;
        const uint32_t max_delay = rnd() % 4 == 0 ? 0 : rnd() % 2 ? pick(1, 40) : pick(1, 3 * t);
        const uint32_t max_frames = rnd() % 2 ? pick(1, 40) : pick(1, 2 * t + 5);
        CHECK(delay_geometry_ok(1, C, max_delay, max_frames));
        const uint32_t cap = (uint32_t)delay_ring_frames(max_delay, max_frames);
        DelayMirror m;
        m.init(1, cap);
        Stream st;
        st.holds.assign((size_t)cap * C, -1);
        // the mirror's model, written out
        uint32_t d1 = 0, d0 = 0, R = 0, done = 0;
        for (unsigned k = 0; k < 12; k++, runs++) {
            const uint32_t d = rnd() % 3 == 0 ? max_delay : pick(0, max_delay);
            switch (rnd() % 3) {
            case 0:
                m.set(0, d);
                d1 = d0 = d;
                R = done = 0;
                break;
            case 1:
                if (!m.ramping(0)) {
                    const uint32_t frames = pick(2, 3 * max_frames + 2);
                    m.ramp(0, d, frames);
                    d0 = d1;
                    d1 = d;
                    R = frames;
                    done = 0;
                }
                break;
            default: break;
            }
            CHECK(m.ramping(0) == (done < R));
            const uint32_t count = rnd() % 5 == 0 ? 0 : rnd() % 2 ? max_frames : pick(0, max_frames);
            uint32_t rec[DELAY_REC];
            m.record(0, count, rec);
            CHECK(rec[DREC_COUNT] == count && rec[DREC_POS] == st.pos && rec[DREC_D1] == d1 && rec[DREC_D0] == d0 &&
                  rec[DREC_R] == R && rec[DREC_DONE] == done);
            if (done < R) {
                CHECK((uint64_t)rec[DREC_INC] * R >= (1ull << 32) && (uint64_t)(rec[DREC_INC] - 1u) * R < (1ull << 32));
                run_once(C, max_delay, max_frames, st.pos, count, d0, st.holds, st.given);
            }
            run_once(C, max_delay, max_frames, st.pos, count, d1, st.holds, st.given);
            for (uint32_t e = 0; e < count * C; e++)
                st.holds[delay_ring_index(st.pos * C, cap * C, e)] = (int)(st.given + e);
            st.given += (size_t)count * C;
            st.pos = (st.pos + count) % cap;
            m.advance(0, count);
            if (done < R) {
                done = done + count >= R ? R : done + count;
                if (done >= R) {
                    d0 = d1;
                    R = done = 0;
                }
            }
            CHECK(m.pos[0] == st.pos && m.d1[0] == d1 && m.d0[0] == d0 && m.R[0] == R && m.done[0] == done);
        }
    }
    // the geometry's refusals and the plan's
    CHECK(!delay_geometry_ok(0, 1, 1, 1) && !delay_geometry_ok(1, 0, 1, 1) && !delay_geometry_ok(1, 17, 1, 1));
    CHECK(!delay_geometry_ok(1, 1, 1, 0) && delay_geometry_ok(1, 1, 0, 1));
    CHECK(delay_geometry_ok(1, 1, (1ull << 31) - 2, 1) && !delay_geometry_ok(1, 1, (1ull << 31) - 1, 1));
    CHECK(delay_geometry_ok(1, 16, (1ull << 27) - 2, 1) && !delay_geometry_ok(1, 16, (1ull << 27) - 1, 1));
    CHECK(!delay_geometry_ok(1, 1, ~0ull, ~0ull) && !delay_geometry_ok(1, 1, 1ull << 63, 1ull << 63));
    CHECK(plan_delay(1u << 20, 2, 0, 1u << 21, 1u << 21).err == 1 && plan_delay(1u << 20, 2, 0, 1u << 21, 1u << 20).err == 0);
    printf("delay plan ok: %lu geometries, %lu runs\n", iterations, runs);
    return 0;
}
