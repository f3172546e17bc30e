// k_automix.hip -- gfx950 (MI355X, wave64) automixer kernels: S streams of C interleaved int16 channels, each multiplied
// by the share of its group's gain that its level earns, once per window of W = 2^w frames (include/coolmic_hip.h,
// "automixer", has the arithmetic to the bit; csrc/automix_plan.h the power, the share and the record as code;
// csrc/agc_plan.h the windows and the tiles, which are the leveller's).  Four launches per run, behind one clearing of
// the groups' sums:
//
//   k_automix_energy_fast<C> / k_automix_energy_any   per tile: the sums of squares per channel, into the run's table
//   k_automix_level                                   per stream, one lane: m, v and P of every window that completes,
//                                                     P into power[s][i] and, one 64-bit add, into gsum[group][i]
//   k_automix_share                                   per stream, one lane: the run's gain nodes; D of every window that
//                                                     completes from power[s][i] and gsum[group][i]
//   k_automix_apply_fast<C> / k_automix_apply_any     per tile: y = (x g + 2048) >> 12, g between the window's two nodes
//
// The energy and the apply pass are the leveller's tile bodies (k_agc.h), instantiated here and not copied.
//
// Why two lane-per-stream kernels and not one: D of a window needs the sum over ALL members of the group, and the
// members' lanes lie in any workgroup.  The kernel boundary is the only barrier across workgroups there is: every add of
// k_automix_level has happened before any lane of k_automix_share reads.  No lane loops over its group's members, the
// work is O(S NW) per run.
//
// gsum is zero before the adds because the launcher clears it on the run's stream in front of the run (hipMemsetAsync):
// stream order puts the clearing behind the reads of the run before and in front of the adds of this one, and nothing
// else touches it.  No lane clears an entry, so none can clear what another member has still to read.
//
// A group is on one clock (csrc/automix_plan.h): its members' records hold the same position and count, so window i of
// the run is the same window for each of them.  A stream in no group: the energy pass sees count 0 for it (rec_energy)
// and reads nothing, k_automix_level returns at once, k_automix_share writes the unity node 4096 for every window, and
// the apply pass gives (4096 x + 2048) >> 12 = x.
#include "k_agc.h"

namespace cmhip {

static AgcArgs automix_energy_args(const AutomixArgs &a)
{
    AgcArgs e = a.tile;
    e.rec = a.rec_energy;
    return e;
}

// ---------------------------------------------------------------------------
// energy and apply (agc_energy_body, agc_apply_body: k_agc.h)

template <int C>
__global__ __launch_bounds__(AGC_FAST_BLOCK) void k_automix_energy_fast(AgcArgs a)
{
    agc_energy_body<C, AGC_FAST_BLOCK, AGC_FAST_VECS / AGC_FAST_BLOCK>(a, nullptr);
}

__global__ __launch_bounds__(AGC_ANY_BLOCK) void k_automix_energy_any(AgcArgs a)
{
    __shared__ u64 lds[AGC_MAX_CH * AGC_ANY_BLOCK];
    agc_energy_body<0, AGC_ANY_BLOCK, AGC_ANY_VECS>(a, lds);
}

template <int C>
__global__ __launch_bounds__(AGC_FAST_BLOCK) void k_automix_apply_fast(AgcArgs a)
{
    agc_apply_body<C, AGC_FAST_BLOCK, AGC_FAST_VECS / AGC_FAST_BLOCK>(a, nullptr);
}

__global__ __launch_bounds__(AGC_ANY_BLOCK) void k_automix_apply_any(AgcArgs a)
{
    __shared__ u32 lds[AGC_ANY_BLOCK / 64u];
    agc_apply_body<0, AGC_ANY_BLOCK, AGC_ANY_VECS>(a, lds);
}

// ---------------------------------------------------------------------------
// level: a lane per stream walks the windows the run touches, in order.  Where window i of the run completes, E is the
// largest channel's table entry -- plus the carried sums where the window was begun in an earlier run -- and m, v and P
// follow; P goes to power[s][i] and into gsum[group][i].  Where the window stays open (the run's last one) its sums are
// carried.  Every table entry read is left zero.  A stream without frames or in no group returns before it touched
// anything.  (group < S: the host checked it, cmhip_automix_set_group.)
__global__ __launch_bounds__(AGC_STEP_BLOCK) void k_automix_level(AutomixArgs a)
{
    const u32 s = blockIdx.x * AGC_STEP_BLOCK + threadIdx.x;
    if (s >= a.tile.streams)
        return;
    const u32 *rec = a.tile.rec + (u64)s * AGC_REC;
    const u32 count = rec[AREC_COUNT], group = rec[XREC_GROUP];
    if (count == 0 || group >= a.tile.streams)
        return;
    const u64 pos = (u64)rec[AREC_POS_LO] | ((u64)rec[AREC_POS_HI] << 32);
    const AutomixParams p = automix_unpack(rec);
    const u32 C = a.tile.channels, w = a.tile.w, nw = a.tile.nw;
    AutomixState *st = a.state + s;
    u64 *row = a.tile.table + (u64)s * nw * C;
    u64 *pw = a.power + (u64)s * nw, *gs = a.gsum + (u64)group * nw;
    u64 P = pos == 0 ? 0ull : st->power;             // frame 0: creation, or a reset since the last run
    const AgcRun r = agc_run(pos, count, w);
    const bool carried = ((u32)pos & ((1u << w) - 1u)) != 0;         // window 0 of the run began in an earlier run
    for (u32 i = 0; i < r.nwin && i < nw; i++) {
        const bool add = i == 0 && carried;
        if (i < r.complete) {
            u64 E = 0;
            for (u32 ch = 0; ch < C; ch++) {
                const u64 e = row[i * C + ch] + (add ? st->psum[ch] : 0ull);
                row[i * C + ch] = 0;
                E = e > E ? e : E;
            }
            P = automix_power(P, automix_mean(E, w), p);
            pw[i] = P;
            if (P)
                atomicAdd(gs + i, P);
        } else {
            for (u32 ch = 0; ch < C; ch++) {
                st->psum[ch] = row[i * C + ch] + (add ? st->psum[ch] : 0ull);
                row[i * C + ch] = 0;
            }
        }
    }
    st->power = P;
}

// ---------------------------------------------------------------------------
// share: a lane per stream, behind k_automix_level on the same stream.  Window i of the run: where its first frame is
// processed in this run (every window but a carried first one) and it is not the stream's window 0, the nodes move on:
// a_lo = a_hi, a_hi = pending; then its nodes are written; then, where it ends inside the run, pending = D from the
// stream's own P and the group's sum.  A stream in no group writes 4096 everywhere and keeps no state.
__global__ __launch_bounds__(AGC_STEP_BLOCK) void k_automix_share(AutomixArgs a)
{
    const u32 s = blockIdx.x * AGC_STEP_BLOCK + threadIdx.x;
    if (s >= a.tile.streams)
        return;
    const u32 *rec = a.tile.rec + (u64)s * AGC_REC;
    const u32 count = rec[AREC_COUNT], group = rec[XREC_GROUP];
    if (count == 0)
        return;
    const u64 pos = (u64)rec[AREC_POS_LO] | ((u64)rec[AREC_POS_HI] << 32);
    const u32 w = a.tile.w, nw = a.tile.nw;
    u32 *nodes = a.tile.nodes + (u64)s * (nw + 1u);
    const AgcRun r = agc_run(pos, count, w);
    if (group >= a.tile.streams) {
        for (u32 i = 0; i <= r.nwin && i <= nw; i++)
            nodes[i] = AUTOMIX_UNITY;
        return;
    }
    const AutomixParams p = automix_unpack(rec);
    AutomixState *st = a.state + s;
    const u64 *pw = a.power + (u64)s * nw, *gs = a.gsum + (u64)group * nw;
    const bool fresh = pos == 0;
    u32 a_lo = fresh ? (u32)p.initial : st->a_lo, a_hi = fresh ? (u32)p.initial : st->a_hi;
    u32 pending = fresh ? (u32)p.initial : st->pending;
    const bool carried = ((u32)pos & ((1u << w) - 1u)) != 0;
    for (u32 i = 0; i < r.nwin && i < nw; i++) {
        if ((i > 0 || !carried) && r.first + i >= 1u) {
            a_lo = a_hi;
            a_hi = pending;
        }
        nodes[i] = a_lo;
        nodes[i + 1u] = a_hi;
        if (i < r.complete)
            pending = automix_share(pw[i], gs[i], p.floor, pending);
    }
    st->a_lo = a_lo;
    st->a_hi = a_hi;
    st->pending = pending;
}

// ---------------------------------------------------------------------------
// launcher

hipError_t launch_automix(const AutomixArgs &a, uint64_t max_frames, uint32_t frames, hipStream_t st, hipEvent_t *ev)
{
    const AgcPlan p = plan_agc(a.tile.streams, a.tile.channels, a.tile.w, max_frames, frames);
    if (p.grid == 0)
        return p.err ? hipErrorInvalidValue : hipSuccess;
    AutomixArgs b = a;
    b.tile.nw = p.nw;
    b.tile.chunks = p.chunks;
    b.tile.tile_log2 = p.tile_log2;
    const AgcArgs en = automix_energy_args(b);
    const u32 C = a.tile.channels;
    // (ev: tools/bench_automix.py's five events around the four launches; no run of the library's own has any)
    auto mark = [&](unsigned i) { return ev ? hipEventRecord(ev[i], st) : hipSuccess; };
    hipError_t e = mark(0);
    if (e != hipSuccess)
        return e;
    // the groups' sums of this run: zero before k_automix_level adds (the file's head has the ordering argument)
    e = hipMemsetAsync(b.gsum, 0, (size_t)a.tile.streams * p.nw * sizeof(u64), st);
    if (e != hipSuccess)
        return e;
    if (!p.fast)
        hipLaunchKernelGGL(k_automix_energy_any, dim3(p.grid), dim3(p.block), 0, st, en);
    else if (C == 1)
        hipLaunchKernelGGL(k_automix_energy_fast<1>, dim3(p.grid), dim3(p.block), 0, st, en);
    else
        hipLaunchKernelGGL(k_automix_energy_fast<2>, dim3(p.grid), dim3(p.block), 0, st, en);
    e = hipGetLastError();
    if (e != hipSuccess || (e = mark(1)) != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_automix_level, dim3(p.step_grid), dim3(AGC_STEP_BLOCK), 0, st, b);
    e = hipGetLastError();
    if (e != hipSuccess || (e = mark(2)) != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_automix_share, dim3(p.step_grid), dim3(AGC_STEP_BLOCK), 0, st, b);
    e = hipGetLastError();
    if (e != hipSuccess || (e = mark(3)) != hipSuccess)
        return e;
    if (!p.fast)
        hipLaunchKernelGGL(k_automix_apply_any, dim3(p.grid), dim3(p.block), 0, st, b.tile);
    else if (C == 1)
        hipLaunchKernelGGL(k_automix_apply_fast<1>, dim3(p.grid), dim3(p.block), 0, st, b.tile);
    else
        hipLaunchKernelGGL(k_automix_apply_fast<2>, dim3(p.grid), dim3(p.block), 0, st, b.tile);
    e = hipGetLastError();
    return e != hipSuccess ? e : mark(4);
}

}  // namespace cmhip
