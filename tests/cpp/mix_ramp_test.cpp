// mix_ramp_test.cpp -- drives csrc/mix_ramp.h (the arithmetic of the mixer's matrix ramps and the host's mirror of the
// streams' ramps; plain C++, no HIP) over random sequences of ramp / retarget / cancel / advance, against an
// independent restatement: positions by a 128-bit quotient instead of the 32-bit increment's habits, weights by a
// division instead of shifts, and a per-stream state kept as (W0, W1, done, R) in wide integers.  A stand-alone
// program: tests/test_mix_ramp_host.py builds it with g++ once plainly and once under AddressSanitizer + UBSan and runs
// it.   usage: mix_ramp_test [sequences]
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "mix_ramp.h"

using namespace cmhip;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            fprintf(stderr, "sequence %d: line %d: %s\n", seq, __LINE__, #cond);     \
            return 1;                                                                \
        }                                                                            \
    } while (0)

// the restatement
static long long ref_position(unsigned long long n, unsigned long long R)
{
    if (n == 0)
        return 0;
    if (R < 2)
        return 32768;
    if (n > R)
        n = R;
    const unsigned __int128 inc = (((unsigned __int128)1 << 32) + R - 1) / R;
    const unsigned __int128 q = (n * inc) / 131072;
    return q < 32768 ? (long long)q : 32768;
}
static long long ref_weight(long long w0, long long w1, long long p)
{
    if (p > 32768)
        p = 32768;
    return (w0 * (32768 - p) + w1 * p) / 32768;          // C++ division truncates towards zero
}
struct RefStream {
    std::vector<long long> w0, w1;
    unsigned long long done = 0, R = 0;
    bool ramping() const { return done < R; }
    long long now(size_t i) const { return ramping() ? ref_weight(w0[i], w1[i], ref_position(done, R)) : w1[i]; }
};

int main(int argc, char **argv)
{
    const int sequences = argc > 1 ? atoi(argv[1]) : 2000;
    std::mt19937 rng(20240923u);
    auto upto = [&](uint32_t hi) { return (uint32_t)(rng() % ((uint64_t)hi + 1u)); };       // 0 .. hi
    size_t steps = 0, ramps_ended = 0;
    int seq = -1;
    // the spec functions at their edges
    CHECK(mix_ramp_position(0, 5) == 0 && mix_ramp_position(5, 5) == 32768 && mix_ramp_position(9, 5) == 32768);
    CHECK(mix_ramp_position(0, 0) == 0 && mix_ramp_position(1, 0) == 32768 && mix_ramp_position(1, 1) == 32768);
    CHECK(mix_ramp_position(1, 2) == 16384 && mix_ramp_position(0xffffffffu, MIX_RAMP_MAX) == 32768);
    CHECK(mix_ramp_weight(-32768, 32767, 0) == -32768 && mix_ramp_weight(-32768, 32767, 32768) == 32767);
    CHECK(mix_ramp_weight(-32768, 32767, 0xffffffffu) == 32767 && mix_ramp_weight(-1, 0, 1) == 0);
    for (seq = 0; seq < sequences; seq++) {
        const size_t S = 1 + upto(4), n = 1 + upto(upto(3) == 0 ? 255 : 7);
        auto matrix = [&](std::vector<int16_t> &W) {
            W.resize(n);
            const uint32_t kind = upto(3);
            for (size_t i = 0; i < n; i++)
                W[i] = kind == 0 ? (int16_t)(upto(1) ? 32767 : -32768) : kind == 1 ? 0 : (int16_t)((int)upto(65535) - 32768);
        };
        std::vector<int16_t> W, init(S * n);
        for (size_t s = 0; s < S; s++) {
            matrix(W);
            for (size_t i = 0; i < n; i++)
                init[s * n + i] = W[i];
        }
        MixRampMirror mir;
        mir.init(S, n, init.data());
        std::vector<RefStream> ref(S);
        for (size_t s = 0; s < S; s++) {
            ref[s].w0.assign(init.begin() + s * n, init.begin() + (s + 1) * n);
            ref[s].w1 = ref[s].w0;
        }
        const uint32_t rmax = upto(2) == 0 ? MIX_RAMP_MAX : 300;
        for (int step = 0; step < 40; step++, steps++) {
            const size_t s = upto((uint32_t)S - 1);
            const uint32_t what = upto(5);
            if (what == 0) {                                     // a ramp, or a retarget when one runs
                matrix(W);
                const uint32_t R = 2 + upto(rmax - 2);
                std::vector<long long> cur(n);
                for (size_t i = 0; i < n; i++)
                    cur[i] = ref[s].now(i);
                ref[s].w0 = cur;
                ref[s].w1.assign(W.begin(), W.end());
                ref[s].done = 0;
                ref[s].R = R;
                mir.start(s, W.data(), R);
            } else if (what == 1) {                              // a step
                matrix(W);
                ref[s].w0.assign(W.begin(), W.end());
                ref[s].w1 = ref[s].w0;
                ref[s].done = ref[s].R = 0;
                mir.cancel(s, W.data());
            } else {                                             // a run: every stream its own count, zero included
                for (size_t t = 0; t < S; t++) {
                    const uint32_t c = upto(3) == 0 ? 0 : upto(2) == 0 ? upto(0xffffffffu) : upto(rmax / 2);
                    const bool was = ref[t].ramping();
                    if (was) {
                        ref[t].done += c;
                        if (ref[t].done >= ref[t].R) {
                            ref[t].done = ref[t].R;
                            ramps_ended++;
                        }
                    }
                    mir.advance(t, c);
                }
            }
            // the mirror against the restatement, every stream
            size_t active = 0;
            std::vector<int16_t> now(n);
            for (size_t t = 0; t < S; t++) {
                CHECK(mir.ramping(t) == ref[t].ramping());
                active += ref[t].ramping() ? 1 : 0;
                if (ref[t].ramping()) {
                    CHECK(mir.done[t] == ref[t].done && mir.R[t] == ref[t].R && mir.done[t] < mir.R[t]);
                }
                mir.now(t, now.data());
                for (size_t i = 0; i < n; i++) {
                    CHECK(now[i] == ref[t].now(i));
                    CHECK(mir.w1[t * n + i] == ref[t].w1[i]);
                    // between the two ends, never outside them
                    const long long lo = ref[t].w0[i] < ref[t].w1[i] ? ref[t].w0[i] : ref[t].w1[i];
                    const long long hi = ref[t].w0[i] < ref[t].w1[i] ? ref[t].w1[i] : ref[t].w0[i];
                    CHECK(now[i] >= lo && now[i] <= hi);
                }
            }
            CHECK(mir.active == active && mir.any() == (active != 0));
        }
    }
    printf("ramps ok: %d sequences, %zu steps, %zu ramps ran to their end\n", sequences, steps, ramps_ended);
    return 0;
}
