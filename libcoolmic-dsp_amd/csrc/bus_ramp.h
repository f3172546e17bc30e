// bus_ramp.h -- the host's side of the mix bus's send ramps (include/coolmic_hip.h, "send ramps"): the mirror of every
// send's ramp, the bounds the group split runs on while sends ramp, and the record a send has on the device.  Host
// only, plain C++17, no HIP: tests/cpp/bus_ramp_test.cpp compiles it with g++ alone.
//
// The arithmetic is the mixer's (csrc/mix_ramp.h: position, weight and the per-stream mirror); a send takes the place
// of a stream, and its clock is the output count of its BUS, not of its own stream.
//
// The group split under ramps.  Over a group the kernels chain an int32 accumulator, which is exact while the group's
// per-row sum of sum_c |w| stays <= 65535 (csrc/bus_route.h).  A ramp's rows stay within the convex combination of the
// two ends' row sums (truncation towards zero, mix_ramp.h), so a send between W0 and W1 never passes
// max(sum |W0 row|, sum |W1 row|) in a row.  Sends ramp independently -- one may be at its start while another is at
// its end -- so no common bound is tighter than the sum of these maxima, and the split is made on them
// (bus_route_compile_bounds), again at every ramp call.  When a ramp has ended the split may stay the more
// conservative one until the next call that compiles: results do not depend on it, the int64 across groups is exact.
//
// The device's record of a send, in compiled order (BusRampArgs::ramp, csrc/cmhip_internal.h):
//     inc, R, done, bus,  W0[n], W1[n]       n = C_out * CP dwords, the matrices in the kernels' packed form
// The send ramps while done < R; a send at rest has inc = R = done = 0 and its matrix in both.
#ifndef CMHIP_BUS_RAMP_H
#define CMHIP_BUS_RAMP_H

#include "bus_route.h"
#include "mix_ramp.h"

namespace cmhip {

constexpr uint32_t BUSR_HDR = 4;
constexpr uint32_t BUSR_INC = 0, BUSR_R = 1, BUSR_DONE = 2, BUSR_BUS = 3;

inline uint32_t bus_ramp_record_dwords(uint32_t ci, uint32_t co) { return BUSR_HDR + 2u * co * ((ci + 1u) / 2u); }

// a matrix int16 [C_out][C_in] in the kernels' packed form, uint32 [C_out][CP] (bus_route_compile's wk)
inline void bus_ramp_pack(const int16_t *W, uint32_t ci, uint32_t co, uint32_t *k)
{
    const uint32_t cp = (ci + 1) / 2;
    for (uint32_t i = 0; i < co * cp; i++)
        k[i] = 0;
    for (uint32_t o = 0; o < co; o++)
        for (uint32_t c = 0; c < ci; c++)
            k[o * cp + (c >> 1)] |= (uint32_t)(uint16_t)W[o * ci + c] << (16u * (c & 1u));
}

// The sends' ramps as the host knows them, in the caller's order of the table in force.
struct BusRampMirror {
    MixRampMirror r;                                 // per send: W0, W1 int16 [C_out * C_in], done, R
    std::vector<uint32_t> bus;                       // the send's bus

    // every send at rest on its matrix; may throw std::bad_alloc
    void init(size_t sends, size_t entries, const uint32_t *bus_of, const int16_t *W)
    {
        r.init(sends, entries, W);
        bus.assign(bus_of, bus_of + sends);
    }
    size_t sends() const { return bus.size(); }
    bool ramping(size_t j) const { return r.ramping(j); }
    bool any() const { return r.any(); }
    void now(size_t j, int16_t *W) const { r.now(j, W); }
    // a ramp of `frames` >= 2 of the bus's frames to W, from the matrix in force (a retarget when one is running)
    void start(size_t j, const int16_t *W, uint32_t frames) { r.start(j, W, frames); }
    // a step to W between two frames: whatever ramp runs is over
    void step(size_t j, const int16_t *W) { r.cancel(j, W); }
    // a run produced bus_count[b] frames of bus b: every send moves on by its bus's count (0 keeps its position)
    void advance(const uint32_t *bus_count)
    {
        if (!any())
            return;
        for (size_t j = 0; j < bus.size(); j++)
            r.advance(j, bus_count[bus[j]]);
    }
    // what row o of send j may reach: the larger of its two ends' sums while it ramps, its matrix's own otherwise
    void bounds(size_t j, uint32_t ci, uint32_t co, uint32_t *row) const
    {
        const int16_t *a = &r.w0[j * r.n], *b = &r.w1[j * r.n];
        for (uint32_t o = 0; o < co; o++) {
            uint32_t s0 = 0, s1 = 0;
            for (uint32_t c = 0; c < ci; c++) {
                s0 += bus_abs16(a[o * ci + c]);
                s1 += bus_abs16(b[o * ci + c]);
            }
            row[o] = ramping(j) && s0 > s1 ? s0 : s1;
        }
    }
    // the device's record of send j (bus_ramp_record_dwords(ci, co) dwords)
    void record(size_t j, uint32_t ci, uint32_t co, uint32_t *rec) const
    {
        const uint32_t n = co * ((ci + 1) / 2);
        const bool on = ramping(j);
        rec[BUSR_INC] = on ? mix_ramp_inc(r.R[j]) : 0u;
        rec[BUSR_R] = on ? r.R[j] : 0u;
        rec[BUSR_DONE] = on ? r.done[j] : 0u;
        rec[BUSR_BUS] = bus[j];
        bus_ramp_pack(on ? &r.w0[j * r.n] : &r.w1[j * r.n], ci, co, rec + BUSR_HDR);
        bus_ramp_pack(&r.w1[j * r.n], ci, co, rec + BUSR_HDR + n);
    }
};

// the bounds of every send, uint32 [sends][C_out], for bus_route_compile_bounds
inline void bus_ramp_bounds(const BusRampMirror &m, uint32_t ci, uint32_t co, std::vector<uint32_t> &bound)
{
    bound.assign(m.sends() * co, 0);
    for (size_t j = 0; j < m.sends(); j++)
        m.bounds(j, ci, co, &bound[j * co]);
}

}  // namespace cmhip
#endif
