// bus_ramp_test.cpp -- drives csrc/bus_ramp.h and csrc/bus_route.h's bounds-taking compile (the host side of the mix
// bus's send ramps; plain C++, no HIP).  A stand-alone program: tests/test_bus_ramp_host.py builds it with g++ once
// plainly and once under AddressSanitizer + UBSan and runs it.
//
//   bus_ramp_test [sequences]      random tables and random independent ramps / retargets / steps / runs: the mirror
//       against a restatement in wide integers (positions by a 128-bit quotient, weights by a division); after every
//       step the two-ended split -- every group's bound sum stays <= 65535 per row, the split is the greedy one, every
//       send's rows evaluated at EVERY position of its ramp (R <= 64 exhaustively, longer ones at 64 positions) stay
//       within the send's bound, and the rows in force within their group -- and every send's device record
//   bus_ramp_test replay FILE      a script of operations, one per line, the mirror's state printed after each (the
//       plain-Python model of tests/test_bus_ramp_host.py compares):
//           init SENDS C_OUT C_IN BUSES  bus[SENDS]  W[SENDS * C_OUT * C_IN]
//           start J R w[C_OUT * C_IN]  |  step J w[C_OUT * C_IN]  |  adv count[BUSES]
//       answer per operation, one line per send: done R ramping  now[C_OUT * C_IN]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "bus_ramp.h"

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
    if (n > R)
        n = R;
    const unsigned __int128 inc = (((unsigned __int128)1 << 32) + R - 1) / R;
    const unsigned __int128 q = (n * inc) / 131072;
    return q < 32768 ? (long long)q : 32768;
}
static long long ref_weight(long long w0, long long w1, long long p)
{
    return (w0 * (32768 - p) + w1 * p) / 32768;          // C++ division truncates towards zero
}
struct RefSend {
    std::vector<long long> w0, w1;
    unsigned long long done = 0, R = 0;
    bool ramping() const { return done < R; }
    long long at(size_t i, unsigned long long n) const { return ref_weight(w0[i], w1[i], ref_position(n, R)); }
    long long now(size_t i) const { return ramping() ? at(i, done) : w1[i]; }
};

static int replay(const char *path)
{
    FILE *f = fopen(path, "r");
    if (!f)
        return 2;
    BusRampMirror mir;
    unsigned sends = 0, co = 0, ci = 0, buses = 0;
    char op[16];
    std::vector<int16_t> W;
    auto matrix = [&](size_t n) {
        W.resize(n);
        for (size_t i = 0; i < n; i++) {
            int v;
            if (fscanf(f, "%d", &v) != 1)
                return false;
            W[i] = (int16_t)v;
        }
        return true;
    };
    while (fscanf(f, "%15s", op) == 1) {
        if (!strcmp(op, "init")) {
            if (fscanf(f, "%u %u %u %u", &sends, &co, &ci, &buses) != 4)
                return 2;
            std::vector<uint32_t> bus(sends);
            for (unsigned j = 0; j < sends; j++)
                if (fscanf(f, "%u", &bus[j]) != 1)
                    return 2;
            if (!matrix((size_t)sends * co * ci))
                return 2;
            mir.init(sends, (size_t)co * ci, bus.data(), W.data());
        } else if (!strcmp(op, "start")) {
            unsigned j, R;
            if (fscanf(f, "%u %u", &j, &R) != 2 || !matrix((size_t)co * ci) || j >= sends)
                return 2;
            mir.start(j, W.data(), R);
        } else if (!strcmp(op, "step")) {
            unsigned j;
            if (fscanf(f, "%u", &j) != 1 || !matrix((size_t)co * ci) || j >= sends)
                return 2;
            mir.step(j, W.data());
        } else if (!strcmp(op, "adv")) {
            std::vector<uint32_t> c(buses);
            for (unsigned b = 0; b < buses; b++)
                if (fscanf(f, "%u", &c[b]) != 1)
                    return 2;
            mir.advance(c.data());
        } else {
            return 2;
        }
        std::vector<int16_t> now((size_t)co * ci);
        for (unsigned j = 0; j < sends; j++) {
            mir.now(j, now.data());
            printf("%u %u %d ", mir.ramping(j) ? mir.r.done[j] : 0u, mir.ramping(j) ? mir.r.R[j] : 0u, mir.ramping(j) ? 1 : 0);
            for (size_t i = 0; i < now.size(); i++)
                printf(" %d", now[i]);
            printf("\n");
        }
    }
    fclose(f);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 2 && !strcmp(argv[1], "replay"))
        return replay(argv[2]);
    const int sequences = argc > 1 ? atoi(argv[1]) : 1000;
    std::mt19937 rng(20241019u);
    auto upto = [&](uint32_t hi) { return (uint32_t)(rng() % ((uint64_t)hi + 1u)); };       // 0 .. hi
    size_t steps = 0, ramps_ended = 0, positions = 0, groups_seen = 0, two_ended = 0;
    int seq = -1;
    for (seq = 0; seq < sequences; seq++) {
        const uint32_t ci = 1 + upto(upto(2) == 0 ? 15 : 2), co = 1 + upto(upto(2) == 0 ? 15 : 1);
        const uint32_t cp = (ci + 1) / 2, B = 1 + upto(3);
        const size_t S = 1 + upto(11), n = (size_t)co * ci;
        // a matrix whose rows have sum |w| <= 65535: heavy rows, light rows and zero ones
        auto matrix = [&](std::vector<int16_t> &W) {
            W.assign(n, 0);
            for (uint32_t o = 0; o < co; o++) {
                const uint32_t kind = upto(3);
                uint32_t left = kind == 0 ? 65535u : kind == 1 ? 0u : upto(3) == 0 ? upto(65535) : upto(20000);
                for (uint32_t c = 0; c < ci && left; c++) {
                    uint32_t mag = c + 1 == ci ? left : upto(left);
                    mag = mag > 32767 ? 32767 : mag;
                    left -= mag;
                    W[o * ci + c] = (int16_t)(upto(1) ? -(int)mag : (int)mag);
                }
            }
        };
        std::vector<int16_t> W, table(S * n);
        std::vector<uint32_t> bus(S), stream(S);
        for (size_t j = 0; j < S; j++) {
            matrix(W);
            memcpy(&table[j * n], W.data(), n * sizeof(int16_t));
            bus[j] = upto(B - 1);
            stream[j] = upto(7);
        }
        BusRampMirror mir;
        mir.init(S, n, bus.data(), table.data());
        std::vector<RefSend> ref(S);
        for (size_t j = 0; j < S; j++) {
            ref[j].w0.assign(table.begin() + j * n, table.begin() + (j + 1) * n);
            ref[j].w1 = ref[j].w0;
        }
        const uint32_t rmax = upto(3) == 0 ? MIX_RAMP_MAX : 64;
        for (int step = 0; step < 30; step++, steps++) {
            const size_t j = upto((uint32_t)S - 1);
            const uint32_t what = upto(4);
            if (what <= 1) {                                     // a ramp, or a retarget when one runs
                matrix(W);
                const uint32_t R = 2 + upto(rmax - 2);
                std::vector<long long> cur(n);
                for (size_t i = 0; i < n; i++)
                    cur[i] = ref[j].now(i);
                ref[j].w0 = cur;
                ref[j].w1.assign(W.begin(), W.end());
                ref[j].done = 0;
                ref[j].R = R;
                mir.start(j, W.data(), R);
                memcpy(&table[j * n], W.data(), n * sizeof(int16_t));
            } else if (what == 2) {                              // a step
                matrix(W);
                ref[j].w0.assign(W.begin(), W.end());
                ref[j].w1 = ref[j].w0;
                ref[j].done = ref[j].R = 0;
                mir.step(j, W.data());
                memcpy(&table[j * n], W.data(), n * sizeof(int16_t));
            } else {                                             // a run: every bus its own count, zero included
                std::vector<uint32_t> count(B);
                for (uint32_t b = 0; b < B; b++)
                    count[b] = upto(3) == 0 ? 0 : upto(3) == 0 ? upto(0xffffffffu) : upto(rmax / 2);
                for (size_t t = 0; t < S; t++) {
                    if (!ref[t].ramping())
                        continue;
                    ref[t].done += count[bus[t]];
                    if (ref[t].done >= ref[t].R) {
                        ref[t].done = ref[t].R;
                        ramps_ended++;
                    }
                }
                mir.advance(count.data());
            }
            // ---- the mirror against the restatement, every send
            bool any = false;
            std::vector<int16_t> now(n);
            for (size_t t = 0; t < S; t++) {
                CHECK(mir.ramping(t) == ref[t].ramping());
                any = any || ref[t].ramping();
                if (ref[t].ramping())
                    CHECK(mir.r.done[t] == ref[t].done && mir.r.R[t] == ref[t].R);
                mir.now(t, now.data());
                for (size_t i = 0; i < n; i++) {
                    CHECK(now[i] == ref[t].now(i));
                    CHECK(mir.r.w1[t * n + i] == ref[t].w1[i] && table[t * n + i] == ref[t].w1[i]);
                }
            }
            CHECK(mir.any() == any);
            // ---- the two-ended split
            std::vector<uint32_t> bound, pos;
            bus_ramp_bounds(mir, ci, co, bound);
            BusTable t, plain;
            bus_route_compile_bounds(B, ci, co, S, bus.data(), stream.data(), table.data(), bound.data(), t, &pos);
            bus_route_compile(B, ci, co, S, bus.data(), stream.data(), table.data(), plain);
            CHECK(t.first == plain.first && t.stream == plain.stream && t.wk == plain.wk);       // only the split differs
            if (!any)
                CHECK(t.flag == plain.flag && t.groups == plain.groups);
            else if (t.flag != plain.flag)
                two_ended++;
            std::vector<size_t> from(S);
            for (size_t c = 0; c < S; c++) {
                CHECK(pos[c] < S && t.stream[pos[c]] == stream[c] && pos[c] >= t.first[bus[c]] && pos[c] < t.first[bus[c] + 1]);
                from[pos[c]] = c;
            }
            for (size_t c = 1; c < S; c++)
                if (bus[from[c]] == bus[from[c - 1]])
                    CHECK(from[c] > from[c - 1]);                // stable inside a bus
            for (size_t c = 0; c < S; c++) {
                // a send's rows at every position of its ramp stay within its bound
                const RefSend &r = ref[c];
                const unsigned long long Rr = r.ramping() ? r.R : 0, stride = Rr > 64 ? Rr / 64 : 1;
                for (unsigned long long k = 0; k <= Rr; k += (k + stride > Rr && k < Rr) ? Rr - k : stride) {
                    for (uint32_t o = 0; o < co; o++) {
                        long long sum = 0, want0 = 0, want1 = 0;
                        for (uint32_t cc = 0; cc < ci; cc++) {
                            const long long w = r.ramping() ? r.at(o * ci + cc, k) : r.w1[o * ci + cc];
                            sum += w < 0 ? -w : w;
                            want0 += r.w0[o * ci + cc] < 0 ? -r.w0[o * ci + cc] : r.w0[o * ci + cc];
                            want1 += r.w1[o * ci + cc] < 0 ? -r.w1[o * ci + cc] : r.w1[o * ci + cc];
                        }
                        CHECK(sum <= (long long)bound[c * co + o] && bound[c * co + o] <= BUS_ROW_MAX);
                        CHECK((long long)bound[c * co + o] == (r.ramping() && want0 > want1 ? want0 : want1));
                    }
                    positions++;
                }
            }
            for (uint32_t b = 0; b < B; b++) {
                uint32_t groups = 0;
                std::vector<long long> run(co, 0), force(co, 0);
                for (uint32_t p = t.first[b]; p < t.first[b + 1]; p++) {
                    const size_t c = from[p];
                    bool fits = p != t.first[b];
                    for (uint32_t o = 0; o < co; o++)
                        fits = fits && run[o] + bound[c * co + o] <= 65535;
                    CHECK(t.flag[p] == (fits ? 0u : 1u));        // greedy: a group ends only where the next send does not fit
                    groups += t.flag[p];
                    for (uint32_t o = 0; o < co; o++) {
                        long long f = 0;
                        for (uint32_t cc = 0; cc < ci; cc++) {
                            const long long w = ref[c].now(o * ci + cc);
                            f += w < 0 ? -w : w;
                        }
                        run[o] = (fits ? run[o] : 0) + bound[c * co + o];
                        force[o] = (fits ? force[o] : 0) + f;
                        CHECK(run[o] <= 65535 && force[o] <= run[o]);
                    }
                }
                CHECK(t.groups[b] == groups);
                groups_seen += groups;
            }
            // ---- the device's records
            const uint32_t recw = bus_ramp_record_dwords(ci, co);
            CHECK(recw == 4 + 2 * co * cp);
            std::vector<uint32_t> rec(recw);
            for (size_t c = 0; c < S; c++) {
                mir.record(c, ci, co, rec.data());
                const RefSend &r = ref[c];
                CHECK(rec[BUSR_BUS] == bus[c]);
                CHECK(rec[BUSR_R] == (r.ramping() ? r.R : 0) && rec[BUSR_DONE] == (r.ramping() ? r.done : 0));
                CHECK(rec[BUSR_INC] == (r.ramping() ? (uint32_t)((((unsigned long long)1 << 32) + r.R - 1) / r.R) : 0u));
                for (uint32_t o = 0; o < co; o++)
                    for (uint32_t k = 0; k < cp; k++)
                        for (uint32_t h = 0; h < 2; h++) {
                            const uint32_t cc = 2 * k + h;
                            const long long w0 = cc < ci ? (r.ramping() ? r.w0[o * ci + cc] : r.w1[o * ci + cc]) : 0;
                            const long long w1 = cc < ci ? r.w1[o * ci + cc] : 0;
                            CHECK((int16_t)(rec[BUSR_HDR + o * cp + k] >> (16 * h)) == w0);
                            CHECK((int16_t)(rec[BUSR_HDR + co * cp + o * cp + k] >> (16 * h)) == w1);
                            CHECK((int16_t)(t.wk[(pos[c] * co + o) * cp + k] >> (16 * h)) == w1);
                        }
            }
        }
    }
    printf("send ramps ok: %d sequences, %zu steps, %zu ramps ran to their end, %zu positions, %zu groups, "
           "%zu splits moved by a ramp's other end\n", sequences, steps, ramps_ended, positions, groups_seen, two_ended);
    return 0;
}
