// iir_ramp.h -- the arithmetic of a coefficient ramp and the host's mirror of the sections' ramps (include/coolmic_hip.h,
// "filter", coefficient ramps).  Plain C++17, no HIP: tests/cpp/iir_ramp_test.cpp compiles it with g++ alone; the ramp
// kernels (k_iirramp.hip) use the same position and section functions.
//
//   inc  = ceil(2^32 / R)                       R in 2..2^20: inc <= 2^31
//   p(n) = min(32768, (n * inc) >> 17)          n = 1..R the ramp's frame, p in units of 2^-15, p(0) = 0: the mixer's
//   N(x0, x1) = x0 * (32768 - p) + x1 * p       int64, |N| < 2^45
//   b0, b2, a1:  sgn(N) * (|N| >> 15)           towards zero: |a1(p)| is at most the exact convex combination
//   a2:          -((-N) >> 15)                  rounded up: a2(p) is not below it -- the triangle is convex, so c(p) is
//                                               inside whenever both ends are
//   s:           towards zero from s0 = b0 + b1 + b2 of c0 and s1 of c1
//   b1 = clamp(s - b0 - b2, -2^28, 2^28)        ends with s0 = s1 = 0 keep their zero on z = 1 at every p
// c(0) = c0 and c(32768) = c1 exactly.  A section ramps while done < R: frame f (from 0) of its stream's next run uses
// c(p(done + f + 1)), frames past the ramp c1.  The device advances nothing: the table that travels with a run's counts
// holds both ends, done and R as the mirror has them (IIR_RAMP_WORDS per section), and the mirror advances by the counts.
#ifndef CMHIP_IIR_RAMP_H
#define CMHIP_IIR_RAMP_H

#include "iir_plan.h"

#include <vector>

namespace cmhip {

constexpr uint32_t IIR_RAMP_MAX = 1u << 20;          // frames of a ramp at most
constexpr uint32_t IIR_RAMP_ONE = 32768;             // p at the ramp's end
constexpr uint32_t IIR_RAMP_WORDS = 12;              // a section in a ramp run's table: c0[5], c1[5], done, R

// ceil(2^32 / R), R >= 2, without leaving 32 bits
CMHIP_IIR_HD inline uint32_t iir_ramp_inc(uint32_t R) { return 0xffffffffu / R + 1u; }

// p(n), the mixer's; n above R counts as R, R below 2 is a step (0 before it, the end from frame 1 on)
CMHIP_IIR_HD inline uint32_t iir_ramp_position(uint32_t n, uint32_t R)
{
    if (n == 0)
        return 0;
    if (R < 2)
        return IIR_RAMP_ONE;
    if (n > R)
        n = R;
    const uint64_t q = ((uint64_t)n * iir_ramp_inc(R)) >> 17;
    return q < IIR_RAMP_ONE ? (uint32_t)q : IIR_RAMP_ONE;
}

// What a kernel keeps of a section's (done, R): done and inc.  R * inc >= 2^32, so the product alone clamps p at the
// ramp's end and R is not needed; a section at rest counts as a ramp of 2 frames that is over.  Frame f of the run:
// p(done + f + 1), done + f + 1 < 2^32 and inc <= 2^31.
struct IirRampClock {
    uint32_t done, inc;
};
CMHIP_IIR_HD inline IirRampClock iir_ramp_clock(uint32_t done, uint32_t R)
{
    return done < R && R >= 2 ? IirRampClock{done, iir_ramp_inc(R)} : IirRampClock{2u, 1u << 31};
}
CMHIP_IIR_HD inline uint32_t iir_ramp_at(const IirRampClock &c, uint32_t f)
{
    const uint64_t q = ((uint64_t)(c.done + f + 1u) * c.inc) >> 17;
    return q < IIR_RAMP_ONE ? (uint32_t)q : IIR_RAMP_ONE;
}

// N(x0, x1) >> 15 towards zero and rounded up; |x| <= 3 * 2^28, p <= 32768.  (Two products: x0 * 32768 + (x1 - x0) * p
// is one, and measured slower in both kernels -- DESIGN 4.20.1.)
CMHIP_IIR_HD inline int64_t iir_ramp_num(int32_t x0, int32_t x1, uint32_t p)
{
    return (int64_t)x0 * (int32_t)(IIR_RAMP_ONE - p) + (int64_t)x1 * (int32_t)p;
}
CMHIP_IIR_HD inline int32_t iir_ramp_trunc(int32_t x0, int32_t x1, uint32_t p)
{
    const int64_t N = iir_ramp_num(x0, x1, p);
    return (int32_t)(N < 0 ? -((-N) >> 15) : N >> 15);
}
CMHIP_IIR_HD inline int32_t iir_ramp_up(int32_t x0, int32_t x1, uint32_t p)
{
    return (int32_t)-((-iir_ramp_num(x0, x1, p)) >> 15);           // (arithmetic: floor of -N, negated)
}

// b0 + b1 + b2 of a section whose |c| <= 2^28
CMHIP_IIR_HD inline int32_t iir_ramp_sum(const IirSec &c) { return c.b0 + c.b1 + c.b2; }

// c(p) between two sections whose |c| <= 2^28, s0 and s1 their sums; p above 32768 counts as 32768
CMHIP_IIR_HD inline IirSec iir_ramp_section(const IirSec &c0, const IirSec &c1, int32_t s0, int32_t s1, uint32_t p)
{
    if (p > IIR_RAMP_ONE)
        p = IIR_RAMP_ONE;
    IirSec c;
    c.b0 = iir_ramp_trunc(c0.b0, c1.b0, p);
    c.b2 = iir_ramp_trunc(c0.b2, c1.b2, p);
    c.a1 = iir_ramp_trunc(c0.a1, c1.a1, p);
    c.a2 = iir_ramp_up(c0.a2, c1.a2, p);
    const int32_t b1 = iir_ramp_trunc(s0, s1, p) - c.b0 - c.b2;      // |b1| <= 5 * 2^28
    c.b1 = b1 < -IIR_COEF_MAX ? -IIR_COEF_MAX : b1 > IIR_COEF_MAX ? IIR_COEF_MAX : b1;
    return c;
}
CMHIP_IIR_HD inline IirSec iir_ramp_section(const IirSec &c0, const IirSec &c1, uint32_t p)
{
    return iir_ramp_section(c0, c1, iir_ramp_sum(c0), iir_ramp_sum(c1), p);
}

// a section of a ramp run's table
struct IirRampEntry {
    IirSec   c0, c1;
    uint32_t done, R;                                // R = 0: at rest on c1
};
static_assert(sizeof(IirRampEntry) == IIR_RAMP_WORDS * sizeof(uint32_t), "a table entry is IIR_RAMP_WORDS words");

// The sections' ramps as the host knows them, entry i = stream * N + section.
struct IirRampMirror {
    std::vector<IirRampEntry> e;
    size_t active = 0;                               // entries with done < R

    // every section at rest on unity; may throw std::bad_alloc
    void init(size_t entries)
    {
        e.assign(entries, IirRampEntry{IIR_UNITY, IIR_UNITY, 0, 0});
        active = 0;
    }
    bool ramping(size_t i) const { return e[i].done < e[i].R; }
    bool any() const { return active != 0; }
    // the section in force: c(p(done)) while the section ramps, its target otherwise
    IirSec now(size_t i) const
    {
        const IirRampEntry &r = e[i];
        return ramping(i) ? iir_ramp_section(r.c0, r.c1, iir_ramp_position(r.done, r.R)) : r.c1;
    }
    // a ramp of `frames` >= 2 frames to c, from the section in force (a retarget when one is running)
    void start(size_t i, const IirSec &c, uint32_t frames)
    {
        const IirSec from = now(i);
        if (!ramping(i))
            active++;
        e[i] = IirRampEntry{from, c, 0, frames};
    }
    // a step to c: whatever ramp runs is over
    void cancel(size_t i, const IirSec &c)
    {
        if (ramping(i))
            active--;
        e[i] = IirRampEntry{c, c, 0, 0};
    }
    // the section's stream was given `count` frames
    void advance(size_t i, uint32_t count)
    {
        if (!ramping(i))
            return;
        IirRampEntry &r = e[i];
        r.done = count >= r.R - r.done ? r.R : r.done + count;
        if (!ramping(i)) {
            active--;
            r = IirRampEntry{r.c1, r.c1, 0, 0};
        }
    }
};

}  // namespace cmhip
#endif
