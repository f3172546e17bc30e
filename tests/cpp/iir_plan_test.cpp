// iir_plan_test.cpp -- csrc/iir_plan.h on its own (g++, no HIP; tests/test_iir_host.py builds it plain and under
// AddressSanitizer + UBSan): the section against a 128-bit restatement of the header's arithmetic, the output step, the
// stability check, the tiles' vectors, the plan, and a launch as the kernels decompose it -- workgroups of spw
// streams, tiles staged through an LDS image in 16-byte vectors with ragged ends, the skewed pipeline of (row,
// section) lanes with its drain or the row loop -- against a plain walk of every row, however the streams are cut
// into runs.
//
//   iir_plan_test [rounds]
#include "iir_plan.h"

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

static std::mt19937_64 rng(12345);
static int64_t pick(int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); }

static IirSec random_section()
{
    for (;;) {
        IirSec c;
        const int kind = (int)pick(0, 3);
        const int64_t top = kind == 0 ? IIR_COEF_MAX : IIR_ONE;
        c.b0 = (int32_t)pick(-top, top);
        c.b1 = (int32_t)pick(-top, top);
        c.b2 = (int32_t)pick(-top, top);
        c.a2 = (int32_t)pick(-(IIR_ONE - 1), IIR_ONE - 1);
        const int64_t edge = (int64_t)IIR_ONE + c.a2 - 1;
        c.a1 = (int32_t)(kind == 1 ? edge : kind == 2 ? -edge : pick(-edge, edge));
        if (kind == 3)
            c = IIR_UNITY;
        if (iir_section_ok(c))
            return c;
    }
}

static void test_section()
{
    for (int n = 0; n < 20000; n++) {
        const IirSec c = random_section();
        IirState s;
        s.u1 = (int32_t)pick(-IIR_V_MAX, IIR_V_MAX);
        s.u2 = (int32_t)pick(-IIR_V_MAX, IIR_V_MAX);
        s.v1 = (int32_t)pick(-IIR_V_MAX, IIR_V_MAX);
        s.v2 = (int32_t)pick(-IIR_V_MAX, IIR_V_MAX);
        s.e = (uint32_t)pick(0, IIR_ONE - 1);
        const int32_t u = (int32_t)(n & 1 ? pick(-IIR_V_MAX, IIR_V_MAX) : iir_input((int32_t)pick(-32768, 32767)));
        const __int128 acc = (__int128)c.b0 * u + (__int128)c.b1 * s.u1 + (__int128)c.b2 * s.u2 - (__int128)c.a1 * s.v1 -
                             (__int128)c.a2 * s.v2 + s.e;
        const __int128 lim = (__int128)1 << 62;
        CHECK(acc < lim && acc > -lim);
        __int128 q = acc >> 26;
        const uint32_t e = (uint32_t)(acc & (IIR_ONE - 1));
        const bool over = q > IIR_V_MAX || q < -(__int128)IIR_V_MAX;
        q = q > IIR_V_MAX ? IIR_V_MAX : q < -(__int128)IIR_V_MAX ? -(__int128)IIR_V_MAX : q;
        IirState t = s;
        uint32_t o;
        const int32_t v = iir_section(c, u, t, &o);
        CHECK(v == (int32_t)q && o == (over ? 1u : 0u) && t.e == e && t.e < (uint32_t)IIR_ONE);
        CHECK(t.u1 == u && t.u2 == s.u1 && t.v1 == v && t.v2 == s.v1);
    }
    // unity is the identity on u and leaves no remainder
    IirState s = {1, 2, 3, 4, 0};
    uint32_t o;
    CHECK(iir_section(IIR_UNITY, -12345678, s, &o) == -12345678 && o == 0 && s.e == 0);
    CHECK(iir_section(IIR_UNITY, IIR_V_MAX, s, &o) == IIR_V_MAX && o == 0);
}

static void test_output()
{
    const int64_t edges[] = {-IIR_V_MAX, IIR_V_MAX, -2049, -2048, -2047, -1, 0, 2047, 2048, 32767 * 4096 + 2047,
                             32767 * 4096 + 2048, -32768 * 4096 - 2048, -32768 * 4096 - 2049};
    for (int n = 0; n < 20000; n++) {
        const int64_t v = n < 13 ? edges[n] : pick(-IIR_V_MAX, IIR_V_MAX) >> (n % 20);
        const int64_t r = (v + 2048) >> 12, y = r < -32768 ? -32768 : r > 32767 ? 32767 : r;
        uint32_t clip;
        CHECK(iir_output((int32_t)v, &clip) == (int32_t)y && clip == (y != r ? 1u : 0u));
    }
    for (int x = -32768; x <= 32767; x++) {
        uint32_t clip;
        CHECK(iir_output(iir_input(x), &clip) == x && clip == 0);
    }
}

static void test_check()
{
    const int32_t one = IIR_ONE, big = IIR_COEF_MAX;
    CHECK(iir_section_ok(IIR_UNITY) && iir_section_ok(IirSec{big, -big, big, 0, 0}));
    CHECK(!iir_section_ok(IirSec{big + 1, 0, 0, 0, 0}) && !iir_section_ok(IirSec{0, 0, -big - 1, 0, 0}));
    CHECK(iir_section_ok(IirSec{0, 0, 0, 2 * one - 2, one - 1}) && !iir_section_ok(IirSec{0, 0, 0, 2 * one - 1, one - 1}));
    CHECK(iir_section_ok(IirSec{0, 0, 0, -(2 * one - 2), one - 1}) && !iir_section_ok(IirSec{0, 0, 0, -(2 * one - 1), one - 1}));
    CHECK(!iir_section_ok(IirSec{0, 0, 0, 0, one}) && !iir_section_ok(IirSec{0, 0, 0, 0, -one}));
    CHECK(iir_section_ok(IirSec{0, 0, 0, one - 1, 0}) && !iir_section_ok(IirSec{0, 0, 0, one, 0}));
    CHECK(iir_section_ok(IirSec{0, 0, 0, 0, -(one - 1)}) && !iir_section_ok(IirSec{0, 0, 0, 1, -(one - 1)}));
    CHECK(!iir_section_ok(IirSec{INT32_MIN, 0, 0, 0, 0}) && !iir_section_ok(IirSec{0, 0, 0, INT32_MIN, 0}));
}

static void test_plan()
{
    for (uint32_t c = 1; c <= 16; c++)
        for (uint32_t n = 1; n <= 8; n++) {
            const IirPlan p = plan_iir(70, c, n, 1000);
            CHECK(!p.err && p.fast == (c <= 2 ? 1u : 0u) && p.np == (p.fast ? iir_np(n) : 1u) && p.np >= (p.fast ? n : 1u));
            CHECK(p.spw >= 1 && p.spw * c * p.np <= IIR_BLOCK && p.grid == (70 + p.spw - 1) / p.spw);
            CHECK(p.tile == IIR_TILE && (IIR_TILE * c) % 8 == 0 && p.lds_bytes == p.spw * iir_lds_pitch(c) * 2 &&
                  p.lds_bytes <= (IIR_BLOCK * IIR_TILE + 2 * IIR_BLOCK) * 2 && iir_lds_pitch(c) % 2 == 0);
            CHECK(p.tiles == (1000 + IIR_TILE - 1) / IIR_TILE);
        }
    CHECK(plan_iir(3, 2, 2, 0).grid == 0 && plan_iir(0, 2, 2, 5).grid == 0 && plan_iir(3, 17, 2, 5).grid == 0 &&
          plan_iir(3, 2, 9, 5).grid == 0);
    CHECK(iir_geometry_ok(1, 16, 8, (1u << 27) - 1) && !iir_geometry_ok(1, 16, 8, 1u << 27) && !iir_geometry_ok(1, 1, 1, 0));
    // the last samples below 2^31
    const uint32_t count = 0x7ffffffu, last = (count - 1) / IIR_TILE;
    uint64_t covered = 0;
    for (uint32_t q = 0; q < iir_tile_vecs(16); q++) {
        const IirVec v = iir_tile_vec(count, 16, last, q);
        CHECK(v.n == 0 || (uint64_t)v.off + v.n <= (uint64_t)count * 16);
        covered += v.n;
    }
    CHECK(covered == (uint64_t)(count - last * IIR_TILE) * 16);
}

// ---- a launch as the kernels decompose it
struct Streams {
    uint32_t S, C, N;
    std::vector<IirSec> coef;          // [S][N]
    std::vector<IirState> st;          // [S][C][N]
    std::vector<uint64_t> clips, overs;
};

static const int16_t SENTINEL = -21555;

// every row walked plainly
static void reference(Streams &m, const std::vector<std::vector<int16_t>> &in, std::vector<std::vector<int16_t>> &out)
{
    for (uint32_t s = 0; s < m.S; s++) {
        const size_t frames = in[s].size() / m.C;
        out[s].assign(in[s].size(), 0);
        for (size_t f = 0; f < frames; f++)
            for (uint32_t c = 0; c < m.C; c++) {
                int32_t u = iir_input(in[s][f * m.C + c]);
                for (uint32_t k = 0; k < m.N; k++) {
                    uint32_t over;
                    u = iir_section(m.coef[s * m.N + k], u, m.st[(s * m.C + c) * m.N + k], &over);
                    m.overs[s] += over;
                }
                uint32_t clip;
                out[s][f * m.C + c] = (int16_t)iir_output(u, &clip);
                m.clips[s] += clip;
            }
    }
}

static void move(std::vector<int16_t> &lds, std::vector<std::vector<int16_t>> &slots, const std::vector<uint32_t> &counts,
                 uint32_t s0, const IirPlan &p, uint32_t S, uint32_t C, uint32_t t, bool out)
{
    const uint32_t nv = iir_tile_vecs(C);
    for (uint32_t i = 0; i < p.spw * nv; i++) {
        const uint32_t j = i / nv, q = i % nv, s = s0 + j;
        if (s >= S)
            break;
        const IirVec v = iir_tile_vec(counts[s], C, t, q);
        CHECK(v.n == 0 || (uint64_t)v.off + v.n <= (uint64_t)counts[s] * C);
        for (uint32_t k = 0; k < v.n; k++) {             // (through the vectors' own bounds: ASan watches both arrays)
            if (out) {
                CHECK(slots[s].at(v.off + k) == SENTINEL);
                slots[s].at(v.off + k) = lds.at((size_t)j * iir_lds_pitch(C) + (size_t)q * 8 + k);
            } else {
                lds.at((size_t)j * iir_lds_pitch(C) + (size_t)q * 8 + k) = slots[s].at(v.off + k);
            }
        }
    }
}

static void launch(Streams &m, std::vector<std::vector<int16_t>> &in, std::vector<std::vector<int16_t>> &out)
{
    std::vector<uint32_t> counts(m.S);
    uint32_t frames = 0;
    for (uint32_t s = 0; s < m.S; s++) {
        counts[s] = (uint32_t)(in[s].size() / m.C);
        frames = counts[s] > frames ? counts[s] : frames;
        out[s].assign(in[s].size(), SENTINEL);
    }
    const IirPlan p = plan_iir(m.S, m.C, m.N, frames);
    CHECK(!p.err && (frames == 0) == (p.grid == 0));
    const uint32_t NP = p.np, C = m.C, N = m.N;
    for (uint32_t wg = 0; wg < p.grid; wg++) {
        const uint32_t s0 = wg * p.spw;
        uint32_t most = 0;
        for (uint32_t s = s0; s < s0 + p.spw && s < m.S; s++)
            most = counts[s] > most ? counts[s] : most;
        std::vector<int32_t> vprev(IIR_BLOCK, 0), seen(IIR_BLOCK, 0);
        std::vector<int16_t> lds(p.lds_bytes / 2);
        for (uint32_t t = 0; t < (most + IIR_TILE - 1) / IIR_TILE; t++) {
            lds.assign(lds.size(), 0x5a5a);
            move(lds, in, counts, s0, p, m.S, C, t, false);
            const uint32_t steps = iir_tile_frames(most, t) + NP - 1;
            for (uint32_t i = 0; i < steps; i++) {
                seen = vprev;                            // the cross-lane move reads what the step before has left
                for (uint32_t lane = 0; lane < p.spw * C * NP; lane++) {
                    const uint32_t k = lane % NP, r = lane / NP, j = r / C, c = r % C, s = s0 + j;
                    if (s >= m.S)
                        continue;
                    const uint32_t len = iir_tile_frames(counts[s], t), f = i - k;
                    if (f >= len)
                        continue;
                    int16_t &cell = lds.at((size_t)j * iir_lds_pitch(C) + (size_t)f * C + c);
                    int32_t u = k == 0 ? iir_input(cell) : seen[lane - 1];
                    uint32_t over = 0;
                    if (p.fast) {
                        IirState none = {0, 0, 0, 0, 0};
                        u = iir_section(k < N ? m.coef[s * N + k] : IIR_UNITY, u, k < N ? m.st[(s * C + c) * N + k] : none, &over);
                        m.overs[s] += over;
                        CHECK(k < N || none.e == 0);
                    } else {
                        for (uint32_t kk = 0; kk < N; kk++) {
                            u = iir_section(m.coef[s * N + kk], u, m.st[(s * C + c) * N + kk], &over);
                            m.overs[s] += over;
                        }
                    }
                    vprev[lane] = u;
                    if (k == NP - 1) {
                        uint32_t clip;
                        cell = (int16_t)iir_output(u, &clip);
                        m.clips[s] += clip;
                    }
                }
            }
            move(lds, out, counts, s0, p, m.S, C, t, true);
        }
    }
}

static void test_launches(int rounds)
{
    const uint32_t lens[] = {0, 1, 2, 7, 8, 9, IIR_TILE - 1, IIR_TILE, IIR_TILE + 1, 2 * IIR_TILE + 1};
    for (int round = 0; round < rounds; round++) {
        Streams a;
        a.S = (uint32_t)pick(1, 9) + (round % 7 == 0 ? 64 : 0);
        a.C = round % 3 == 0 ? (uint32_t)pick(1, 2) : (uint32_t)pick(1, 16);
        a.N = (uint32_t)pick(1, 8);
        a.coef.resize(a.S * a.N);
        for (IirSec &c : a.coef)
            c = random_section();
        a.st.assign((size_t)a.S * a.C * a.N, IirState{0, 0, 0, 0, 0});
        a.clips.assign(a.S, 0);
        a.overs.assign(a.S, 0);
        Streams b = a;
        for (int run = 0; run < 3; run++) {
            std::vector<std::vector<int16_t>> in(a.S), want(a.S), got(a.S);
            for (uint32_t s = 0; s < a.S; s++) {
                in[s].resize((size_t)lens[pick(0, 9)] * a.C);
                const int amp = (int)pick(1, 32767);
                for (int16_t &x : in[s])
                    x = (int16_t)(pick(0, 9) == 0 ? (pick(0, 1) ? 32767 : -32768) : pick(-amp, amp));
            }
            if (run == 1) {                              // a set and a reset between two runs
                const uint32_t s = (uint32_t)pick(0, a.S - 1), k = (uint32_t)pick(0, a.N - 1);
                a.coef[s * a.N + k] = b.coef[s * b.N + k] = random_section();
                for (uint32_t i = 0; i < a.C * a.N; i++)
                    a.st[(size_t)s * a.C * a.N + i] = b.st[(size_t)s * a.C * a.N + i] = IirState{0, 0, 0, 0, 0};
            }
            reference(a, in, want);
            launch(b, in, got);
            for (uint32_t s = 0; s < a.S; s++) {
                CHECK(want[s] == got[s]);
                CHECK(a.clips[s] == b.clips[s] && a.overs[s] == b.overs[s]);
            }
            for (size_t i = 0; i < a.st.size(); i++)
                CHECK(a.st[i].u1 == b.st[i].u1 && a.st[i].u2 == b.st[i].u2 && a.st[i].v1 == b.st[i].v1 &&
                      a.st[i].v2 == b.st[i].v2 && a.st[i].e == b.st[i].e);
        }
    }
}

int main(int argc, char **argv)
{
    const int rounds = argc > 1 ? atoi(argv[1]) : 200;
    test_section();
    test_output();
    test_check();
    test_plan();
    test_launches(rounds);
    printf("iir plan ok: %d rounds\n", rounds);
    return 0;
}
