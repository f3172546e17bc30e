// automix_plan.h -- the arithmetic, a run's record and the host's mirror of the automixer (include/coolmic_hip.h,
// "automixer").  Plain C++17, no HIP: tests/cpp/automix_plan_test.cpp compiles it with g++ alone; the kernels
// (k_automix.hip) use the same power and share functions.  The windows, the tiles and the launch plan are the
// leveller's (agc_plan.h): a run's record keeps AGC_REC dwords with the count and the position in the leveller's
// places, so the leveller's tile context serves both stages.
//
//   record: count, pos (two dwords), weight | floor << 16, attack | release << 16, initial, the group id
//   (AUTOMIX_NO_GROUP for none), 0.
//
// A group has ONE clock: its members have the same position and get the same count in every run.  The mirror keeps that
// true by construction -- set_group and reset restart whole groups, a run with unequal counts inside a group is refused
// before anything changes -- so window i of a run is the same window for every member, and one entry gsum[group][i] holds
// the members' sum for it.
#ifndef CMHIP_AUTOMIX_PLAN_H
#define CMHIP_AUTOMIX_PLAN_H

#include "agc_plan.h"

namespace cmhip {

constexpr uint32_t AUTOMIX_UNITY = AGC_UNITY;        // 4096: the gain unit, and the weight's unit on power
constexpr uint32_t AUTOMIX_SHIFT_MAX = 8;            // attack, release
constexpr uint32_t AUTOMIX_NO_GROUP = 0xffffffffu;
constexpr uint32_t XREC_P0 = 3, XREC_P1 = 4, XREC_INITIAL = 5, XREC_GROUP = 6;

// cmhip_automix_params_t, field by field (cmhip_automix.hip holds the two layouts against each other)
struct AutomixParams {
    uint16_t weight, floor, attack, release, initial;
};

CMHIP_AGC_HD constexpr bool automix_params_ok(const AutomixParams &p)
{
    return p.weight <= AUTOMIX_UNITY && p.floor <= AUTOMIX_UNITY && p.attack <= AUTOMIX_SHIFT_MAX &&
           p.release <= AUTOMIX_SHIFT_MAX && p.initial <= AUTOMIX_UNITY;
}

// the parameters as a record carries them, and back
CMHIP_AGC_HD inline void automix_pack(const AutomixParams &p, uint32_t *rec)
{
    rec[XREC_P0] = (uint32_t)p.weight | ((uint32_t)p.floor << 16);
    rec[XREC_P1] = (uint32_t)p.attack | ((uint32_t)p.release << 16);
    rec[XREC_INITIAL] = (uint32_t)p.initial;
}
CMHIP_AGC_HD inline AutomixParams automix_unpack(const uint32_t *rec)
{
    AutomixParams p;
    p.weight = (uint16_t)rec[XREC_P0];
    p.floor = (uint16_t)(rec[XREC_P0] >> 16);
    p.attack = (uint16_t)rec[XREC_P1];
    p.release = (uint16_t)(rec[XREC_P1] >> 16);
    p.initial = (uint16_t)rec[XREC_INITIAL];
    return p;
}

// m of a complete window from its loudest channel's sum of squares: the leveller's E and shift, m <= 2^30
CMHIP_AGC_HD inline uint32_t automix_mean(uint64_t E, uint32_t w) { return (uint32_t)(E >> w); }

// P[k] from P[k-1] and the window's m: v = (m u) >> 12 <= 2^30, V = v << 8 <= 2^38, and P moves towards V by
// (V - P) >> sh, arithmetic: P stays in 0..2^38 (a floor of a step towards V never passes V, nor leaves the side of it
// P was on).
CMHIP_AGC_HD inline uint64_t automix_power(uint64_t P, uint32_t m, const AutomixParams &p)
{
    const uint64_t V = (((uint64_t)m * p.weight) >> 12) << 8;
    const uint32_t sh = V > P ? p.attack : p.release;
    return (uint64_t)((int64_t)P + (((int64_t)V - (int64_t)P) >> sh));
}

// D[k] from the stream's P[k], its group's sum, the floor and D[k-1].  P <= sum (P is one of its terms) and P <= 2^38:
// P << 24 fits 64 bits and the quotient is at most 2^24, so the root is at most 4096.
CMHIP_AGC_HD inline uint32_t automix_share(uint64_t P, uint64_t sum, uint32_t floor, uint32_t D_before)
{
    if (sum == 0)
        return D_before;
    const uint32_t D = dyn_isqrt((uint32_t)((P << 24) / sum));
    return D > floor ? D : floor;
}

// ---- the streams as the host knows them
struct AutomixMirror {
    std::vector<uint64_t> pos;
    std::vector<AutomixParams> par;
    std::vector<uint32_t> group;                     // AUTOMIX_NO_GROUP: none
    mutable std::vector<uint32_t> seen;              // the equal-counts check's first member per group

    void init(size_t streams, const AutomixParams &p)              // may throw std::bad_alloc
    {
        pos.assign(streams, 0);
        par.assign(streams, p);
        group.assign(streams, AUTOMIX_NO_GROUP);
        seen.assign(streams, AUTOMIX_NO_GROUP);
    }
    void record(size_t s, uint32_t count, uint32_t *rec) const
    {
        rec[AREC_COUNT] = count;
        rec[AREC_POS_LO] = (uint32_t)pos[s];
        rec[AREC_POS_HI] = (uint32_t)(pos[s] >> 32);
        automix_pack(par[s], rec);
        rec[XREC_GROUP] = group[s];
        rec[7] = 0;
    }
    // position 0 in the next record for every member of group g
    void reset_group(uint32_t g)
    {
        for (size_t s = 0; s < pos.size(); s++)
            if (group[s] == g)
                pos[s] = 0;
    }
    // the stream's whole group; an ungrouped stream alone
    void reset(size_t s)
    {
        if (group[s] == AUTOMIX_NO_GROUP)
            pos[s] = 0;
        else
            reset_group(group[s]);
    }
    // stream s joins group g (AUTOMIX_NO_GROUP: leaves).  The group left, the group joined and the stream restart, so
    // both groups stay on one clock each.
    void set_group(size_t s, uint32_t g)
    {
        if (group[s] != AUTOMIX_NO_GROUP)
            reset_group(group[s]);
        group[s] = g;
        reset(s);
    }
    // a run's counts (count(s) for every stream): true where every group's members agree; else *a and *b are two
    // members of one group with different counts, a < b
    template <typename Count>
    bool counts_agree(Count &&count, size_t *a, size_t *b) const
    {
        bool ok = true;
        for (size_t s = 0; s < pos.size() && ok; s++) {
            const uint32_t g = group[s];
            if (g == AUTOMIX_NO_GROUP)
                continue;
            if (seen[g] == AUTOMIX_NO_GROUP) {
                seen[g] = (uint32_t)s;
            } else if (count(seen[g]) != count(s)) {
                *a = seen[g];
                *b = s;
                ok = false;
            }
        }
        for (size_t s = 0; s < pos.size(); s++)
            if (group[s] != AUTOMIX_NO_GROUP)
                seen[group[s]] = AUTOMIX_NO_GROUP;
        return ok;
    }
    void advance(size_t s, uint32_t count) { pos[s] += count; }
};

}  // namespace cmhip
#endif
