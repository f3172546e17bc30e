// failover_plan.h -- the arithmetic, a run's records and the host's mirror of the failover switch
// (include/coolmic_hip.h, "failover switch").  Plain C++17, no HIP: tests/cpp/failover_plan_test.cpp compiles it with g++
// alone; the kernels (k_failover.hip) use the same counter, decision and edge functions.  The windows, the tiles and the
// launch plan are the leveller's (agc_plan.h).
//
//   An output's record (FO_REC dwords, sent through the counts ring with every run): count, pos (two dwords), the four
//   candidate slots (an unused one repeats candidate 0, so that every index names a slot the host checked), quiet packed
//   in two dwords, fail | return << 16, fade_log2 | K << 8 | (force & 0xff) << 16.
//   An (output, candidate) row's record, which the energy pass reads: the leveller's AGC_REC dwords with the output's
//   count (0 for a candidate the list does not have: the pass reads nothing of it) and position, and in AREC_SLOT the
//   input slot of the candidate.
//   A window's plan, one dword: from | to << 2 | phi' << 4 | q << 16; steady: from = to, phi' = q = 0.
#ifndef CMHIP_FAILOVER_PLAN_H
#define CMHIP_FAILOVER_PLAN_H

#include "agc_plan.h"

namespace cmhip {

constexpr uint32_t FO_SRC = 4;                       // candidates of an output at most
constexpr uint32_t FO_FADE_MAX = 16;                 // fade_log2 at most
constexpr uint32_t FO_RUN_MAX = 65535;               // where live_run and dead_run stay
constexpr uint32_t FO_QUIET_DEFAULT = 33;            // the leveller's gate
constexpr uint32_t FO_REC = 12;
constexpr uint32_t FREC_SRC = 3, FREC_Q0 = 7, FREC_Q1 = 8, FREC_WIN = 9, FREC_MODE = 10;
constexpr uint32_t AREC_SLOT = 7;                    // (the leveller's and the automixer's records keep 0 there)

// cmhip_failover_params_t, field by field (cmhip_failover.hip holds the two layouts against each other)
struct FailoverParams {
    uint16_t quiet[FO_SRC];
    uint16_t fail_windows, return_windows, fade_log2;
    int16_t  force;
};

CMHIP_AGC_HD constexpr bool failover_params_ok(const FailoverParams &p, uint32_t w, uint32_t K)
{
    return K >= 1 && K <= FO_SRC && p.quiet[0] <= 32767 && p.quiet[1] <= 32767 && p.quiet[2] <= 32767 &&
           p.quiet[3] <= 32767 && p.fail_windows >= 1 && p.return_windows >= 1 && p.fade_log2 >= w &&
           p.fade_log2 <= FO_FADE_MAX && p.force >= -1 && p.force < (int)K;
}

// ---- a window's plan
struct FailoverPlan {
    uint32_t from, to, phi, q;
};
CMHIP_AGC_HD constexpr uint32_t failover_plan_pack(uint32_t from, uint32_t to, uint32_t phi, uint32_t q)
{
    return from | (to << 2) | (phi << 4) | (q << 16);
}
CMHIP_AGC_HD constexpr uint32_t failover_plan_steady(uint32_t c) { return failover_plan_pack(c, c, 0, 0); }
CMHIP_AGC_HD inline FailoverPlan failover_plan_unpack(uint32_t v)
{
    return {v & 3u, (v >> 2) & 3u, (v >> 4) & 31u, v >> 16};
}

// the plan of window 0
CMHIP_AGC_HD inline uint32_t failover_first(const FailoverParams &p)
{
    return failover_plan_steady(p.force >= 0 ? (uint32_t)p.force : 0u);
}

// An output's four live_run (or dead_run) counters in one 64-bit word, candidate i in bits 16 i .. 16 i + 15: a lane of
// k_failover_step indexes them by a candidate it has just chosen, and a word needs no memory for that.
CMHIP_AGC_HD constexpr uint32_t failover_run(uint64_t v, uint32_t i) { return (uint32_t)(v >> (16u * i)) & 0xffffu; }
CMHIP_AGC_HD constexpr uint64_t failover_run_set(uint64_t v, uint32_t i, uint32_t n)
{
    return (v & ~(0xffffull << (16u * i))) | ((uint64_t)n << (16u * i));
}

// the counters of candidate i, moved on by a complete window of level m
CMHIP_AGC_HD inline void failover_count(uint32_t m, uint32_t quiet, uint32_t i, uint64_t &live, uint64_t &dead)
{
    const uint32_t l = failover_run(live, i), d = failover_run(dead, i);
    const bool is_live = m > quiet * quiet;          // (quiet <= 32767: the square fits)
    live = failover_run_set(live, i, is_live ? (l < FO_RUN_MAX ? l + 1u : FO_RUN_MAX) : 0u);
    dead = failover_run_set(dead, i, is_live ? 0u : (d < FO_RUN_MAX ? d + 1u : FO_RUN_MAX));
}

// the header's rule 2: the candidate wanted at an edge outside a fade (K in 1..4, cur < K, force < K)
CMHIP_AGC_HD inline uint32_t failover_step(uint32_t K, const FailoverParams &p, uint32_t cur, uint64_t live, uint64_t dead)
{
    if (p.force >= 0)
        return (uint32_t)p.force;
    for (uint32_t i = 0; i < cur; i++)               // the smallest i with a long enough live run, where it is below cur
        if (failover_run(live, i) >= p.return_windows)
            return i;
    if (failover_run(dead, cur) >= p.fail_windows)
        for (uint32_t i = 0; i < K; i++)
            if (i != cur && failover_run(live, i) >= 1u)
                return i;
    return cur;
}

// the plan of window k >= 1 from the plan of window k - 1 and the counters, which hold window k - 1 already.
// *switched: 1 where a changeover begins.
CMHIP_AGC_HD inline uint32_t failover_edge(uint32_t before, uint32_t K, const FailoverParams &p, uint32_t w,
                                           uint64_t live, uint64_t dead, uint32_t *switched)
{
    const FailoverPlan b = failover_plan_unpack(before);
    *switched = 0;
    if (b.from != b.to && b.q + 1u < (1u << (b.phi - w)))
        return failover_plan_pack(b.from, b.to, b.phi, b.q + 1u);
    const uint32_t want = failover_step(K, p, b.to, live, dead);
    if (want == b.to)
        return failover_plan_steady(b.to);
    *switched = 1;
    return failover_plan_pack(b.to, want, p.fade_log2, 0);
}

// one sample of a fade: frame d of the fade, 0 <= d < 2^phi <= 2^16.  The delay stage's crossfade in the form of its
// header's note: p (b - a) + 16384 stays below 2^31.
CMHIP_AGC_HD inline int32_t failover_fade(int32_t a, int32_t b, uint32_t d, uint32_t phi)
{
    const int32_t p = (int32_t)((d << 15) >> phi);
    return a + ((p * (b - a) + 16384) >> 15);
}

// ---- records
CMHIP_AGC_HD inline void failover_pack(const FailoverParams &p, uint32_t K, uint32_t *rec)
{
    rec[FREC_Q0] = (uint32_t)p.quiet[0] | ((uint32_t)p.quiet[1] << 16);
    rec[FREC_Q1] = (uint32_t)p.quiet[2] | ((uint32_t)p.quiet[3] << 16);
    rec[FREC_WIN] = (uint32_t)p.fail_windows | ((uint32_t)p.return_windows << 16);
    rec[FREC_MODE] = (uint32_t)p.fade_log2 | (K << 8) | (((uint32_t)p.force & 0xffu) << 16);
}
// quiet of candidate i straight from the record (the device indexes memory, not a register array)
CMHIP_AGC_HD inline uint32_t failover_quiet(const uint32_t *rec, uint32_t i)
{
    return (rec[FREC_Q0 + (i >> 1)] >> (16u * (i & 1u))) & 0xffffu;
}
CMHIP_AGC_HD inline FailoverParams failover_unpack(const uint32_t *rec, uint32_t *K)
{
    FailoverParams p;
    p.quiet[0] = (uint16_t)rec[FREC_Q0];
    p.quiet[1] = (uint16_t)(rec[FREC_Q0] >> 16);
    p.quiet[2] = (uint16_t)rec[FREC_Q1];
    p.quiet[3] = (uint16_t)(rec[FREC_Q1] >> 16);
    p.fail_windows = (uint16_t)rec[FREC_WIN];
    p.return_windows = (uint16_t)(rec[FREC_WIN] >> 16);
    p.fade_log2 = (uint16_t)(rec[FREC_MODE] & 0xffu);
    *K = (rec[FREC_MODE] >> 8) & 0xffu;
    p.force = (int16_t)(int8_t)(rec[FREC_MODE] >> 16);
    return p;
}

// ---- the outputs as the host knows them
struct FailoverMirror {
    std::vector<uint64_t> pos;
    std::vector<FailoverParams> par;
    std::vector<uint32_t> K;
    std::vector<uint32_t> src;                       // [O][FO_SRC]

    void init(size_t outputs, size_t streams, const FailoverParams &p)           // may throw std::bad_alloc
    {
        pos.assign(outputs, 0);
        par.assign(outputs, p);
        K.assign(outputs, 1);
        src.assign(outputs * FO_SRC, 0);
        for (size_t o = 0; o < outputs; o++)
            for (uint32_t i = 0; i < FO_SRC; i++)
                src[o * FO_SRC + i] = (uint32_t)(o < streams ? o : streams - 1);
    }
    // 0: a list of n candidates below `streams`, no stream twice
    static bool sources_ok(uint32_t n, const uint32_t *streams_in, size_t streams)
    {
        if (n < 1 || n > FO_SRC)
            return false;
        for (uint32_t i = 0; i < n; i++) {
            if (streams_in[i] >= streams)
                return false;
            for (uint32_t j = 0; j < i; j++)
                if (streams_in[j] == streams_in[i])
                    return false;
        }
        return true;
    }
    // (the list was checked.)  The output starts afresh and is automatic again.
    void set_sources(size_t o, uint32_t n, const uint32_t *streams_in)
    {
        K[o] = n;
        for (uint32_t i = 0; i < FO_SRC; i++)
            src[o * FO_SRC + i] = streams_in[i < n ? i : 0];
        par[o].force = -1;
        pos[o] = 0;
    }
    void reset(size_t o) { pos[o] = 0; }
    void record(size_t o, uint32_t count, uint32_t *rec) const
    {
        rec[AREC_COUNT] = count;
        rec[AREC_POS_LO] = (uint32_t)pos[o];
        rec[AREC_POS_HI] = (uint32_t)(pos[o] >> 32);
        for (uint32_t i = 0; i < FO_SRC; i++)
            rec[FREC_SRC + i] = src[o * FO_SRC + i];
        failover_pack(par[o], K[o], rec);
        rec[11] = 0;
    }
    // the energy pass's record of candidate i of output o
    void record_row(size_t o, uint32_t i, uint32_t count, uint32_t *rec) const
    {
        rec[AREC_COUNT] = i < K[o] ? count : 0u;
        rec[AREC_POS_LO] = (uint32_t)pos[o];
        rec[AREC_POS_HI] = (uint32_t)(pos[o] >> 32);
        rec[AREC_P0] = rec[AREC_P1] = rec[AREC_P2] = rec[AREC_P3] = 0;
        rec[AREC_SLOT] = src[o * FO_SRC + i];
    }
    void advance(size_t o, uint32_t count) { pos[o] += count; }
};

}  // namespace cmhip
#endif
