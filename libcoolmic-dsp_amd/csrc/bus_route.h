// bus_route.h -- the routing compiler of the mix bus (include/coolmic_hip.h, "mix bus"): the caller's sends
// (bus, stream, W[C_out][C_in]) in any order -> the form k_bus.hip's kernels walk.  Host only, plain C++17, no HIP:
// tests/cpp/bus_route_test.cpp compiles it with g++ alone.
//
//   first[B+1]        sends of bus b are first[b] .. first[b+1]-1 of the arrays below (CSR); sorted by bus with a STABLE
//                     sort, so inside a bus the caller's order is kept
//   stream[n]         the send's input slot
//   flag[n]           1: the send starts a GROUP.  Inside a bus the sends are split greedily, in table order, into
//                     maximal runs whose running per-row sum of sum_c |w| stays <= 65535 in every row: over a group
//                     an int32 accumulator chained through dot instructions is exact (the mixer's bound,
//                     |acc + 8192| < 2^31); at a group's end it is added into an int64
//   groups[B]         groups per bus (0 for a bus without sends): a bus of one group never needs the int64
//   wk[n][C_out][CP]  the matrices in the mixer's packed form, CP = ceil(C_in / 2): dword k of row o is
//                     W[o][2k] | W[o][2k+1] << 16, an odd C_in padded with a zero weight
#ifndef CMHIP_BUS_ROUTE_H
#define CMHIP_BUS_ROUTE_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace cmhip {

constexpr uint32_t BUS_MAX_CH = 16;
constexpr uint32_t BUS_ROW_MAX = 65535;              // sum_c |w| of a row of a send, and of a row over a group
constexpr uint64_t BUS_MAX_ENTRIES = 1ull << 31;     // the table's sizes stay below this

struct BusTable {
    std::vector<uint32_t> first, stream, flag, groups, wk;
};

enum BusRouteError : int {
    BUS_ROUTE_OK = 0,
    BUS_ROUTE_GEOMETRY,        // buses, streams or a channel count out of range
    BUS_ROUTE_SIZE,            // n sends of C_out * CP dwords would reach 2^31 entries
    BUS_ROUTE_NULL,            // n > 0 and an array is NULL
    BUS_ROUTE_BUS,             // a bus index out of range      (*where: the send)
    BUS_ROUTE_STREAM,          // a stream index out of range   (*where: the send)
    BUS_ROUTE_ROW,             // a row above 65535             (*where: the send)
};

inline uint32_t bus_abs16(int16_t w) { return (uint32_t)(w < 0 ? -(int)w : (int)w); }

// the validity rules of the header; reads nothing of the arrays before the sizes are known to be in range
inline BusRouteError bus_route_check(uint32_t buses, uint32_t streams, uint32_t ci, uint32_t co, size_t n,
                                     const uint32_t *bus, const uint32_t *stream, const int16_t *W, size_t *where)
{
    if (buses == 0 || streams == 0 || ci == 0 || ci > BUS_MAX_CH || co == 0 || co > BUS_MAX_CH)
        return BUS_ROUTE_GEOMETRY;
    if (buses >= BUS_MAX_ENTRIES - 1 || streams >= BUS_MAX_ENTRIES || (uint64_t)n >= BUS_MAX_ENTRIES / (co * ((ci + 1) / 2)))
        return BUS_ROUTE_SIZE;
    if (n && (!bus || !stream || !W))
        return BUS_ROUTE_NULL;
    for (size_t j = 0; j < n; j++) {
        if (where)
            *where = j;
        if (bus[j] >= buses)
            return BUS_ROUTE_BUS;
        if (stream[j] >= streams)
            return BUS_ROUTE_STREAM;
        for (uint32_t o = 0; o < co; o++) {
            uint32_t sum = 0;
            for (uint32_t c = 0; c < ci; c++)
                sum += bus_abs16(W[(j * co + o) * ci + c]);
            if (sum > BUS_ROW_MAX)
                return BUS_ROUTE_ROW;
        }
    }
    return BUS_ROUTE_OK;
}

// a table that passed bus_route_check -> its kernel form
inline void bus_route_compile(uint32_t buses, uint32_t ci, uint32_t co, size_t n, const uint32_t *bus,
                              const uint32_t *stream, const int16_t *W, BusTable &t)
{
    const uint32_t cp = (ci + 1) / 2;
    t.first.assign((size_t)buses + 1, 0);
    t.groups.assign(buses, 0);
    t.stream.assign(n, 0);
    t.flag.assign(n, 0);
    t.wk.assign(n * co * cp, 0);
    // a counting sort by bus: stable
    for (size_t j = 0; j < n; j++)
        t.first[bus[j] + 1]++;
    for (uint32_t b = 0; b < buses; b++)
        t.first[b + 1] += t.first[b];
    std::vector<uint32_t> next(t.first.begin(), t.first.end() - 1);
    std::vector<size_t> from(n);
    for (size_t j = 0; j < n; j++)
        from[next[bus[j]]++] = j;
    uint32_t run[BUS_MAX_CH], row[BUS_MAX_CH];
    for (uint32_t b = 0; b < buses; b++) {
        for (uint32_t p = t.first[b]; p < t.first[b + 1]; p++) {
            const int16_t *w = W + from[p] * co * ci;
            bool fits = p != t.first[b];             // (a bus's first send always starts a group)
            for (uint32_t o = 0; o < co; o++) {
                row[o] = 0;
                for (uint32_t c = 0; c < ci; c++) {
                    row[o] += bus_abs16(w[o * ci + c]);
                    t.wk[((size_t)p * co + o) * cp + (c >> 1)] |= (uint32_t)(uint16_t)w[o * ci + c] << (16u * (c & 1u));
                }
                if (fits && run[o] + row[o] > BUS_ROW_MAX)
                    fits = false;
            }
            for (uint32_t o = 0; o < co; o++)
                run[o] = fits ? run[o] + row[o] : row[o];
            t.stream[p] = stream[from[p]];
            t.flag[p] = fits ? 0u : 1u;
            t.groups[b] += t.flag[p];
        }
    }
}

// The same table with the group split taken from BOUNDS instead of from W (send ramps, csrc/bus_ramp.h): bound[j][o]
// is what row o of the caller's send j may reach while its matrix moves -- the larger of its two ends' sums for a
// send that ramps, its own sum for one at rest -- and the greedy split above runs on these.  first, stream and wk
// are bus_route_compile's own (wk holds W, the targets); only flag and groups differ, and with bounds equal to the
// rows' sums not even they.  pos (may be nullptr) receives the compiled position of every send of the caller's order.
inline void bus_route_compile_bounds(uint32_t buses, uint32_t ci, uint32_t co, size_t n, const uint32_t *bus,
                                     const uint32_t *stream, const int16_t *W, const uint32_t *bound, BusTable &t,
                                     std::vector<uint32_t> *pos)
{
    bus_route_compile(buses, ci, co, n, bus, stream, W, t);
    std::vector<uint32_t> next(t.first.begin(), t.first.end() - 1);
    std::vector<size_t> from(n);
    for (size_t j = 0; j < n; j++)                   // (the same stable counting sort)
        from[next[bus[j]]++] = j;
    if (pos) {
        pos->assign(n, 0);
        for (size_t p = 0; p < n; p++)
            (*pos)[from[p]] = (uint32_t)p;
    }
    uint32_t run[BUS_MAX_CH] = {0};
    for (uint32_t b = 0; b < buses; b++) {
        t.groups[b] = 0;
        for (uint32_t p = t.first[b]; p < t.first[b + 1]; p++) {
            const uint32_t *row = bound + from[p] * co;
            bool fits = p != t.first[b];
            for (uint32_t o = 0; o < co && fits; o++)
                fits = run[o] + row[o] <= BUS_ROW_MAX;
            for (uint32_t o = 0; o < co; o++)
                run[o] = fits ? run[o] + row[o] : row[o];
            t.flag[p] = fits ? 0u : 1u;
            t.groups[b] += t.flag[p];
        }
    }
}

// the words the kernels read: bit 31 of first[b] says that bus b has more than one group, bit 31 of a send's word
// that it starts a group (both indices stay below 2^31)
constexpr uint32_t BUS_BIT = 0x80000000u;
inline uint32_t bus_first_word(const BusTable &t, uint32_t b)
{
    return t.first[b] | (b < t.groups.size() && t.groups[b] > 1 ? BUS_BIT : 0u);
}
inline uint32_t bus_send_word(const BusTable &t, size_t p) { return t.stream[p] | (t.flag[p] ? BUS_BIT : 0u); }

// a bus's frame count: the largest count among its sends' streams (counts == nullptr: every stream has `frames`)
inline uint32_t bus_out_frames(const BusTable &t, uint32_t b, const uint32_t *counts, uint32_t frames)
{
    uint32_t m = 0;
    for (uint32_t p = t.first[b]; p < t.first[b + 1]; p++) {
        const uint32_t c = counts ? counts[t.stream[p]] : frames;
        m = c > m ? c : m;
    }
    return m;
}

}  // namespace cmhip
#endif
