// k_agc.hip -- gfx950 (MI355X, wave64) leveller kernels: S streams of C interleaved int16 channels, each multiplied by a
// gain that moves once per window of W = 2^w frames towards target / level (include/coolmic_hip.h, "leveller", has the
// arithmetic to the bit; csrc/agc_plan.h the windows, the tiles and the step as code).  Three launches per run:
//
//   k_agc_energy_fast<C> / k_agc_energy_any   per tile: the sums of squares per channel, into the run's table
//   k_agc_step                                per stream, one lane: levels, steps, the run's gain nodes, the state
//   k_agc_apply_fast<C> / k_agc_apply_any     per tile: y = clamp((x g + 2048) >> 12), g between the window's two nodes
//
// The energy and the apply pass are tile bodies in csrc/k_agc.h, which k_automix.hip instantiates as well.
//
// _fast: C in {1, 2}, one wave per tile of at most 256 input vectors, four per lane.  _any: every other channel count up
// to 16, 256 threads per tile of at most 256 frames, two vectors per thread; no speed goal.
//
// A tile lies between multiples of its length in the stream's absolute position and so inside one window (agc_tile):
// its sums go to ONE table entry per channel and its two gain nodes are uniform.  In the run's own samples such a tile
// begins and ends anywhere in a 16-byte vector (agc_tile_span): the whole vectors inside it are read -- and in the
// apply pass written -- as vectors, the up to 7 samples in front and behind one by one, a lane each.  Two tiles that
// share a vector write disjoint samples of it.
//
// Every sum is of integers: squares in uint64 per lane, a DPP wave reduction, then one 64-bit integer add per
// workgroup, window and channel into the table.  No order can change a bit.  k_agc_step reads the table behind the
// energy pass on the same stream, adds the stream's carried partial window, and leaves every entry it read zero.
#include "k_agc.h"

namespace cmhip {

// ---------------------------------------------------------------------------
// energy (agc_energy_body, k_agc.h)
template <int C>
__global__ __launch_bounds__(AGC_FAST_BLOCK) void k_agc_energy_fast(AgcArgs a)
{
    agc_energy_body<C, AGC_FAST_BLOCK, AGC_FAST_VECS / AGC_FAST_BLOCK>(a, nullptr);
}

__global__ __launch_bounds__(AGC_ANY_BLOCK) void k_agc_energy_any(AgcArgs a)
{
    __shared__ u64 lds[AGC_MAX_CH * AGC_ANY_BLOCK];
    agc_energy_body<0, AGC_ANY_BLOCK, AGC_ANY_VECS>(a, lds);
}

// ---------------------------------------------------------------------------
// step: a lane per stream walks the windows the run touches, in order.  Window i of the run: where its first frame is
// processed in this run (every window but a carried first one) and it is not the stream's window 0, the nodes move on by
// one step from the level of the last complete window; then its nodes are written; then, where it ends inside the run,
// its level is taken -- otherwise it is the run's last window and its sums are carried.  A stream with no frames
// returns before it touched anything.
__global__ __launch_bounds__(AGC_STEP_BLOCK) void k_agc_step(AgcArgs a)
{
    const u32 s = blockIdx.x * AGC_STEP_BLOCK + threadIdx.x;
    if (s >= a.streams)
        return;
    const u32 *rec = a.rec + (u64)s * AGC_REC;
    const u32 count = rec[AREC_COUNT];
    if (count == 0)
        return;
    const u64 pos = (u64)rec[AREC_POS_LO] | ((u64)rec[AREC_POS_HI] << 32);
    const AgcParams p = agc_unpack(rec[AREC_P0], rec[AREC_P1], rec[AREC_P2], rec[AREC_P3]);
    const u32 C = a.channels, w = a.w;
    AgcState *st = a.state + s;
    u64 *row = a.table + (u64)s * a.nw * C;
    u32 *nodes = a.nodes + (u64)s * (a.nw + 1u);
    const bool fresh = pos == 0;                     // frame 0: creation, or a reset since the last run
    u32 a_lo = fresh ? (u32)p.initial : st->a_lo, a_hi = fresh ? (u32)p.initial : st->a_hi;
    u32 level = fresh ? 0u : st->level;
    const AgcRun r = agc_run(pos, count, w);
    const bool carried = ((u32)pos & ((1u << w) - 1u)) != 0;         // window 0 of the run began in an earlier run
    for (u32 i = 0; i < r.nwin && i < a.nw; i++) {
        if ((i > 0 || !carried) && r.first + i >= 1u) {
            const u32 next = agc_step(a_hi, level, p);
            a_lo = a_hi;
            a_hi = next;
        }
        nodes[i] = a_lo;
        nodes[i + 1u] = a_hi;
        const bool add = i == 0 && carried;
        if (i < r.complete) {
            u64 E = 0;
            for (u32 ch = 0; ch < C; ch++) {
                const u64 e = row[i * C + ch] + (add ? st->psum[ch] : 0ull);
                row[i * C + ch] = 0;
                E = e > E ? e : E;
            }
            level = agc_level(E, w);
        } else {
            for (u32 ch = 0; ch < C; ch++) {
                st->psum[ch] = row[i * C + ch] + (add ? st->psum[ch] : 0ull);
                row[i * C + ch] = 0;
            }
        }
    }
    st->a_lo = a_lo;
    st->a_hi = a_hi;
    st->level = level;
}

// ---------------------------------------------------------------------------
// apply (agc_apply_body, k_agc.h)

template <int C>
__global__ __launch_bounds__(AGC_FAST_BLOCK) void k_agc_apply_fast(AgcArgs a)
{
    agc_apply_body<C, AGC_FAST_BLOCK, AGC_FAST_VECS / AGC_FAST_BLOCK>(a, nullptr);
}

__global__ __launch_bounds__(AGC_ANY_BLOCK) void k_agc_apply_any(AgcArgs a)
{
    __shared__ u32 lds[AGC_ANY_BLOCK / 64u];
    agc_apply_body<0, AGC_ANY_BLOCK, AGC_ANY_VECS>(a, lds);
}

// ---------------------------------------------------------------------------
// launcher

hipError_t launch_agc(const AgcArgs &a, uint64_t max_frames, uint32_t frames, hipStream_t st, hipEvent_t *ev)
{
    const AgcPlan p = plan_agc(a.streams, a.channels, a.w, max_frames, frames);
    if (p.grid == 0)
        return p.err ? hipErrorInvalidValue : hipSuccess;
    AgcArgs b = a;
    b.nw = p.nw;
    b.chunks = p.chunks;
    b.tile_log2 = p.tile_log2;
    // (ev: tools/bench_agc.py's four events around the three launches; no run of the library's own has any)
    auto mark = [&](unsigned i) { return ev ? hipEventRecord(ev[i], st) : hipSuccess; };
    hipError_t e = mark(0);
    if (e != hipSuccess)
        return e;
    if (!p.fast)
        hipLaunchKernelGGL(k_agc_energy_any, dim3(p.grid), dim3(p.block), 0, st, b);
    else if (a.channels == 1)
        hipLaunchKernelGGL(k_agc_energy_fast<1>, dim3(p.grid), dim3(p.block), 0, st, b);
    else
        hipLaunchKernelGGL(k_agc_energy_fast<2>, dim3(p.grid), dim3(p.block), 0, st, b);
    e = hipGetLastError();
    if (e != hipSuccess || (e = mark(1)) != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_agc_step, dim3(p.step_grid), dim3(AGC_STEP_BLOCK), 0, st, b);
    e = hipGetLastError();
    if (e != hipSuccess || (e = mark(2)) != hipSuccess)
        return e;
    if (!p.fast)
        hipLaunchKernelGGL(k_agc_apply_any, dim3(p.grid), dim3(p.block), 0, st, b);
    else if (a.channels == 1)
        hipLaunchKernelGGL(k_agc_apply_fast<1>, dim3(p.grid), dim3(p.block), 0, st, b);
    else
        hipLaunchKernelGGL(k_agc_apply_fast<2>, dim3(p.grid), dim3(p.block), 0, st, b);
    e = hipGetLastError();
    return e != hipSuccess ? e : mark(3);
}

// test hooks (host logic, need no GPU): the plan of a run whose longest stream has `frames` frames, a run's windows,
// a tile and its span, and the step, the gain and a sample as code
extern "C" void cmhip_test_plan_agc(uint32_t streams, uint32_t channels, uint32_t window_log2, uint64_t max_frames,
                                    uint32_t frames, AgcPlan *plan)
{
    if (plan)
        *plan = plan_agc(streams, channels, window_log2, max_frames, frames);
}

extern "C" void cmhip_test_agc_run(uint64_t pos, uint32_t count, uint32_t window_log2, AgcRun *run)
{
    if (run)
        *run = agc_run(pos, count, window_log2);
}

extern "C" void cmhip_test_agc_tile(uint32_t pos_lo, uint32_t count, uint32_t window_log2, uint32_t tile_log2, uint32_t t,
                                    uint32_t channels, AgcTile *tile, AgcSpan *span)
{
    const AgcTile tl = agc_tile(pos_lo, count, window_log2, tile_log2, t);
    if (tile)
        *tile = tl;
    if (span)
        *span = agc_tile_span(tl.fa, tl.fb, channels);
}

}  // namespace cmhip
