// failover_plan_test.cpp -- csrc/failover_plan.h, compiled by g++ alone (no HIP):
//   - the packed counters: a candidate's counters move alone, stay at 65535 (planted at 65534, not walked there), and
//     LIVE is m > quiet^2, not >=;
//   - failover_step against a restatement of the header's rule 2 over an exhaustive grid: K <= 4, every cur, force,
//     counters in {0, 1, R - 1, R, 65535};
//   - the plan word, failover_edge: a fade keeps the length it began with, takes no decision inside (force included),
//     and a fade may begin at the edge where one ends;
//   - failover_fade against the delay stage's crossfade formula, first frame and range;
//   - the record: pack and unpack; the rows' records: count 0 and a checked slot for a candidate the list lacks;
//   - the mirror: lists are checked, a new list restarts the output and makes it automatic;
//   - an output walked run by run as k_failover_step walks it (the counters taken at the edge with that run's
//     parameters, the plan words per window of the run, the carried plan) equals the output walked window by window,
//     whatever the cuts.
//   usage: failover_plan_test [iterations]
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "failover_plan.h"

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

static unsigned long iteration;

#define CHECK(c)                                                                                                      \
    do {                                                                                                              \
        if (!(c)) {                                                                                                   \
            fprintf(stderr, "%s:%d: %s failed (iteration %lu)\n", __FILE__, __LINE__, #c, iteration);                 \
            exit(1);                                                                                                  \
        }                                                                                                             \
    } while (0)

static FailoverParams defaults(uint32_t w)
{
    FailoverParams p;
    for (uint32_t i = 0; i < FO_SRC; i++)
        p.quiet[i] = 33;
    p.fail_windows = p.return_windows = 1;
    p.fade_log2 = (uint16_t)w;
    p.force = -1;
    return p;
}

static uint64_t packed(const uint32_t *v)
{
    uint64_t r = 0;
    for (uint32_t i = 0; i < FO_SRC; i++)
        r = failover_run_set(r, i, v[i]);
    return r;
}

// the header's rule 2, restated with the list of candidates built first
static uint32_t step_model(uint32_t K, const FailoverParams &p, uint32_t cur, const uint32_t *live, const uint32_t *dead)
{
    if (p.force >= 0)
        return (uint32_t)p.force;
    int b = -1;
    for (uint32_t i = 0; i < K && b < 0; i++)
        if (live[i] >= p.return_windows)
            b = (int)i;
    if (b >= 0 && (uint32_t)b < cur)
        return (uint32_t)b;
    if (dead[cur] >= p.fail_windows) {
        std::vector<uint32_t> alive;
        for (uint32_t i = 0; i < K; i++)
            if (i != cur && live[i] >= 1)
                alive.push_back(i);
        return alive.empty() ? cur : alive.front();
    }
    return cur;
}

static void test_counters()
{
    uint64_t live = 0, dead = 0;
    failover_count(50, 7, 2, live, dead);            // 50 > 49
    CHECK(failover_run(live, 2) == 1 && failover_run(dead, 2) == 0 && (live & ~(0xffffull << 32)) == 0);
    failover_count(49, 7, 2, live, dead);            // 49 = quiet^2: not live
    CHECK(failover_run(live, 2) == 0 && failover_run(dead, 2) == 1);
    failover_count(0, 0, 1, live, dead);             // quiet 0: m = 0 is not live, m = 1 is
    CHECK(failover_run(dead, 1) == 1);
    failover_count(1, 0, 1, live, dead);
    CHECK(failover_run(live, 1) == 1 && failover_run(dead, 1) == 0 && failover_run(dead, 2) == 1);
    failover_count(1u << 30, 32767, 0, live, dead);  // full scale against the largest quiet: 2^30 > 32767^2
    CHECK(failover_run(live, 0) == 1);
    for (uint32_t i = 0; i < FO_SRC; i++) {
        uint32_t l[4] = {3, 3, 3, 3}, d[4] = {5, 5, 5, 5};
        l[i] = 65534;
        uint64_t lv = packed(l), dd = packed(d);
        failover_count(100, 1, i, lv, dd);
        CHECK(failover_run(lv, i) == 65535 && failover_run(dd, i) == 0);
        failover_count(100, 1, i, lv, dd);
        CHECK(failover_run(lv, i) == 65535);         // it stays
        for (uint32_t j = 0; j < FO_SRC; j++)
            if (j != i)
                CHECK(failover_run(lv, j) == 3 && failover_run(dd, j) == 5);
        d[i] = 65534;
        lv = packed(l);
        dd = packed(d);
        failover_count(1, 1, i, lv, dd);
        failover_count(1, 1, i, lv, dd);
        CHECK(failover_run(dd, i) == 65535 && failover_run(lv, i) == 0);
    }
}

static unsigned long test_step_grid()
{
    unsigned long n = 0;
    const uint32_t Rs[] = {1, 2, 3, 65535};
    for (uint32_t K = 1; K <= 4; K++)
        for (uint32_t R : Rs)
            for (uint32_t Fw : Rs) {
                const uint32_t vals[5] = {0, 1, R - 1, R, 65535};
                const uint32_t dvals[5] = {0, 1, Fw - 1, Fw, 65535};
                uint32_t combos = 1;
                for (uint32_t i = 0; i < K; i++)
                    combos *= 5;
                for (uint32_t lc = 0; lc < combos; lc++)
                    for (uint32_t di = 0; di < 5; di++)
                        for (uint32_t cur = 0; cur < K; cur++)
                            for (int force = -1; force < (int)K; force++) {
                                uint32_t live[4] = {0, 0, 0, 0}, dead[4] = {0, 0, 0, 0};
                                uint32_t c = lc;
                                for (uint32_t i = 0; i < K; i++) {
                                    live[i] = vals[c % 5];
                                    dead[i] = live[i] ? 0u : pick(1, 9);       // (one of the two is 0)
                                    c /= 5;
                                }
                                if (!live[cur])
                                    dead[cur] = dvals[di] ? dvals[di] : 1u;
                                FailoverParams p = defaults(6);
                                p.return_windows = (uint16_t)R;
                                p.fail_windows = (uint16_t)Fw;
                                p.force = (int16_t)force;
                                const uint32_t want = step_model(K, p, cur, live, dead);
                                CHECK(failover_step(K, p, cur, packed(live), packed(dead)) == want);
                                CHECK(want < K);
                                n++;
                            }
            }
    return n;
}

static void test_plan_and_edge()
{
    for (uint32_t from = 0; from < 4; from++)
        for (uint32_t to = 0; to < 4; to++)
            for (uint32_t phi = 6; phi <= 16; phi++)
                for (uint32_t q : {0u, 1u, 1023u}) {
                    const FailoverPlan b = failover_plan_unpack(failover_plan_pack(from, to, phi, q));
                    CHECK(b.from == from && b.to == to && b.phi == phi && b.q == q);
                }
    const uint32_t w = 6;
    FailoverParams p = defaults(w);
    p.fade_log2 = w + 2;
    uint32_t live[4] = {0, 1, 0, 0}, dead[4] = {1, 0, 1, 1}, sw;
    // candidate 0 has died: a fade of four windows to candidate 1 begins
    uint32_t pl = failover_edge(failover_plan_steady(0), 2, p, w, packed(live), packed(dead), &sw);
    CHECK(sw == 1 && pl == failover_plan_pack(0, 1, w + 2, 0));
    // inside it phi is set to w, force to 0, and candidate 0 is back: nothing moves but q
    p.fade_log2 = w;
    p.force = 0;
    live[0] = 9;
    dead[0] = 0;
    for (uint32_t q = 1; q < 4; q++) {
        pl = failover_edge(pl, 2, p, w, packed(live), packed(dead), &sw);
        CHECK(sw == 0 && pl == failover_plan_pack(0, 1, w + 2, q));
    }
    // the edge behind the fade's last window: the next fade begins there, with the new length
    pl = failover_edge(pl, 2, p, w, packed(live), packed(dead), &sw);
    CHECK(sw == 1 && pl == failover_plan_pack(1, 0, w, 0));
    pl = failover_edge(pl, 2, p, w, packed(live), packed(dead), &sw);
    CHECK(sw == 0 && pl == failover_plan_steady(0));
    CHECK(failover_first(p) == failover_plan_steady(0));
    p.force = 3;
    CHECK(failover_first(p) == failover_plan_steady(3));
    p.force = -1;
    CHECK(failover_first(p) == failover_plan_steady(0));
}

static void test_fade()
{
    for (unsigned it = 0; it < 200000; it++) {
        const int a = (int)pick(0, 65535) - 32768, b = (int)pick(0, 65535) - 32768;
        const uint32_t phi = pick(6, 16), d = pick(0, (1u << phi) - 1u);
        const uint32_t p = (d << 15) >> phi;
        CHECK(p < 32768);
        const long long N = (long long)a * (32768 - (long long)p) + (long long)b * p;
        const long long want = (N + 16384) >> 15;
        CHECK(failover_fade(a, b, d, phi) == (int32_t)want && want >= -32768 && want <= 32767);
    }
    CHECK(failover_fade(-32768, 32767, 0, 16) == -32768 && failover_fade(32767, -32768, 0, 6) == 32767);
    CHECK(failover_fade(-32768, 32767, 32768, 16) == 0);             // half way: (-32768 + 32767) * 16384 + 16384 >> 15
}

static void test_records_and_mirror()
{
    for (unsigned it = 0; it < 20000; it++) {
        FailoverParams p;
        for (uint32_t i = 0; i < FO_SRC; i++)
            p.quiet[i] = (uint16_t)pick(0, 32767);
        p.fail_windows = (uint16_t)pick(1, 65535);
        p.return_windows = (uint16_t)pick(1, 65535);
        p.fade_log2 = (uint16_t)pick(6, 16);
        const uint32_t K = pick(1, 4);
        p.force = (int16_t)((int)pick(0, K) - 1);
        uint32_t rec[FO_REC] = {0}, k2 = 0;
        failover_pack(p, K, rec);
        const FailoverParams q = failover_unpack(rec, &k2);
        CHECK(k2 == K && q.force == p.force && q.fade_log2 == p.fade_log2 && q.fail_windows == p.fail_windows &&
              q.return_windows == p.return_windows);
        for (uint32_t i = 0; i < FO_SRC; i++)
            CHECK(q.quiet[i] == p.quiet[i] && failover_quiet(rec, i) == p.quiet[i]);
        CHECK(failover_params_ok(p, 6, K));
        if (p.force >= 0)
            CHECK(!failover_params_ok(p, 6, (uint32_t)p.force));     // a list too short for the force
    }
    FailoverParams bad = defaults(8);
    CHECK(failover_params_ok(bad, 8, 1));
    bad.fade_log2 = 7;
    CHECK(!failover_params_ok(bad, 8, 1));
    bad.fade_log2 = 17;
    CHECK(!failover_params_ok(bad, 8, 1));
    bad = defaults(8);
    bad.quiet[3] = 32768;
    CHECK(!failover_params_ok(bad, 8, 4));
    bad = defaults(8);
    bad.fail_windows = 0;
    CHECK(!failover_params_ok(bad, 8, 4));
    bad = defaults(8);
    bad.return_windows = 0;
    CHECK(!failover_params_ok(bad, 8, 4));
    bad = defaults(8);
    bad.force = -2;
    CHECK(!failover_params_ok(bad, 8, 4) && !failover_params_ok(defaults(8), 8, 0) && !failover_params_ok(defaults(8), 8, 5));

    FailoverMirror m;
    m.init(5, 3, defaults(6));
    for (size_t o = 0; o < 5; o++)
        CHECK(m.K[o] == 1 && m.src[o * FO_SRC] == (o < 3 ? o : 2) && m.pos[o] == 0);
    const uint32_t twice[3] = {0, 2, 0}, far[2] = {1, 3}, good[3] = {2, 0, 1};
    CHECK(!FailoverMirror::sources_ok(3, twice, 3) && !FailoverMirror::sources_ok(2, far, 3) &&
          !FailoverMirror::sources_ok(0, good, 3) && !FailoverMirror::sources_ok(5, good, 3) &&
          FailoverMirror::sources_ok(3, good, 3) && FailoverMirror::sources_ok(2, far, 4));
    m.advance(1, 777);
    m.par[1].force = 0;
    m.set_sources(1, 3, good);
    CHECK(m.K[1] == 3 && m.pos[1] == 0 && m.par[1].force == -1 && m.src[FO_SRC + 3] == 2);
    m.advance(1, (1ull << 32) - 5);
    m.advance(1, 70);
    uint32_t rec[FO_REC], row[AGC_REC];
    m.record(1, 99, rec);
    CHECK(rec[AREC_COUNT] == 99 && rec[AREC_POS_LO] == 65 && rec[AREC_POS_HI] == 1 && rec[FREC_SRC] == 2 &&
          rec[FREC_SRC + 1] == 0 && rec[FREC_SRC + 2] == 1 && rec[FREC_SRC + 3] == 2);
    for (uint32_t i = 0; i < FO_SRC; i++) {
        m.record_row(1, i, 99, row);
        CHECK(row[AREC_COUNT] == (i < 3 ? 99u : 0u) && row[AREC_POS_LO] == 65 && row[AREC_POS_HI] == 1 && row[AREC_SLOT] < 3);
    }
    m.reset(1);
    CHECK(m.pos[1] == 0 && m.K[1] == 3);
}

// ---- an output's windows, walked two ways
struct Walk {
    uint64_t live = 0, dead = 0;
    uint32_t level[4] = {0, 0, 0, 0};
    uint32_t plan = 0;
    uint64_t switches = 0;
};

static void test_walks(unsigned long iterations)
{
    for (iteration = 0; iteration < iterations; iteration++) {
        const uint32_t w = pick(6, 8), W = 1u << w, K = pick(1, 4), NWIN = pick(3, 40);
        std::vector<uint32_t> m(NWIN * 4);
        for (auto &v : m)
            v = pick(0, 3) ? pick(0, 5) : 0;
        // parameters change at window edges chosen in advance: a set between two runs, with a cut there in both walks
        std::vector<FailoverParams> par(NWIN);
        FailoverParams p = defaults(w);
        for (uint32_t k = 0; k < NWIN; k++) {
            if (k == 0 || pick(0, 5) == 0) {
                for (uint32_t i = 0; i < 4; i++)
                    p.quiet[i] = (uint16_t)pick(0, 2);
                p.fail_windows = (uint16_t)pick(1, 3);
                p.return_windows = (uint16_t)pick(1, 3);
                p.fade_log2 = (uint16_t)(w + pick(0, 2));
                p.force = pick(0, 3) ? (int16_t)-1 : (int16_t)pick(0, K - 1);
            }
            par[k] = p;
        }
        // window by window
        std::vector<uint32_t> want(NWIN);
        Walk a;
        for (uint32_t k = 0; k < NWIN; k++) {
            if (k == 0) {
                a.plan = failover_first(par[0]);
            } else {
                for (uint32_t i = 0; i < K; i++)
                    failover_count(m[(k - 1) * 4 + i], par[k].quiet[i], i, a.live, a.dead);
                uint32_t sw;
                a.plan = failover_edge(a.plan, K, par[k], w, a.live, a.dead, &sw);
                a.switches += sw;
            }
            want[k] = a.plan;
            const FailoverPlan pl = failover_plan_unpack(a.plan);
            CHECK(pl.from < K && pl.to < K && (pl.from == pl.to ? pl.q == 0 : pl.q < (1u << (pl.phi - w))));
        }
        // run by run, as the kernel: cuts anywhere, but a run never spans a change of parameters at an edge
        Walk b;
        uint64_t pos = 0;
        const uint64_t total = (uint64_t)NWIN * W;
        while (pos < total) {
            const uint32_t k0 = (uint32_t)(pos >> w);
            uint64_t limit = total;                  // the frame where the parameters next change
            for (uint32_t k = k0 + 1; k < NWIN; k++)
                if (par[k].quiet[0] != par[k0].quiet[0] || par[k].quiet[1] != par[k0].quiet[1] ||
                    par[k].quiet[2] != par[k0].quiet[2] || par[k].quiet[3] != par[k0].quiet[3] ||
                    par[k].fail_windows != par[k0].fail_windows || par[k].return_windows != par[k0].return_windows ||
                    par[k].fade_log2 != par[k0].fade_log2 || par[k].force != par[k0].force) {
                    limit = (uint64_t)k * W;
                    break;
                }
            uint32_t count = pick(1, 3 * W + 3);
            if (pos + count > limit)
                count = (uint32_t)(limit - pos);
            const FailoverParams &q = par[k0];
            const AgcRun r = agc_run(pos, count, w);
            const bool fresh = pos == 0, carried = ((uint32_t)pos & (W - 1u)) != 0;
            uint64_t live = fresh ? 0 : b.live, dead = fresh ? 0 : b.dead;
            uint32_t pl = fresh ? failover_first(q) : b.plan;
            for (uint32_t i = 0; i < r.nwin; i++) {
                if ((i > 0 || !carried) && r.first + i >= 1u) {
                    for (uint32_t c = 0; c < K; c++)
                        failover_count(b.level[c], q.quiet[c], c, live, dead);
                    uint32_t sw;
                    pl = failover_edge(pl, K, q, w, live, dead, &sw);
                    b.switches += sw;
                }
                CHECK(pl == want[r.first + i]);
                if (i < r.complete)
                    for (uint32_t c = 0; c < K; c++)
                        b.level[c] = m[(r.first + i) * 4 + c];
            }
            b.live = live;
            b.dead = dead;
            b.plan = pl;
            pos += count;
        }
        CHECK(b.plan == a.plan && b.switches == a.switches);
        // (a's counters hold window NWIN - 2 as the last edge left them, and so do b's)
        CHECK(b.live == a.live && b.dead == a.dead);
    }
}

int main(int argc, char **argv)
{
    const unsigned long iterations = argc > 1 ? strtoul(argv[1], nullptr, 10) : 2000;
    test_counters();
    const unsigned long grid = test_step_grid();
    test_plan_and_edge();
    test_fade();
    test_records_and_mirror();
    test_walks(iterations);
    printf("failover plan ok: %lu decisions, %lu walks\n", grid, iterations);
    return 0;
}
