// k_failover.hip -- gfx950 (MI355X, wave64) failover switch kernels: O outputs of C interleaved int16 channels, each a
// copy of one of up to four candidate input slots, or a crossfade between two of them, chosen once per window of
// W = 2^w frames from the candidates' levels (include/coolmic_hip.h, "failover switch", has the arithmetic to the bit;
// csrc/failover_plan.h the counters, the decision, the plan word and the records as code; csrc/agc_plan.h the windows
// and the tiles, which are the leveller's).  Three launches per run:
//
//   k_failover_energy_fast<C> / k_failover_energy_any   per tile of an (output, candidate) row: the sums of squares per
//                                                       channel, into the run's table
//   k_failover_step                                     per output, one lane: m, the counters, the decision at every
//                                                       window edge of the run, the windows' plan words, the state
//   k_failover_apply_fast<C> / k_failover_apply_any     per tile of an output: a copy of the plan's source, or the
//                                                       crossfade of its two
//
// The energy pass is the leveller's tile body (k_agc.h) over O * 4 rows with its slot indirection: row (o, i) has
// output o's count and position and reads the input slot of candidate i; a candidate the list does not have carries
// count 0 and reads nothing.  An input that is a candidate of two outputs is summed twice, each on its output's clock:
// no two outputs have to agree on counts.  k_failover_step reads the table behind the energy pass on the same stream,
// adds the carried partial windows, and leaves every entry it read zero, as k_agc_step does.
//
// The apply pass.  A tile lies inside one window (agc_tile), so it has ONE plan word, wave-uniform.  What stands
// between a workgroup and its loads: the output's record (count, position, the four candidate slots: one scalar load,
// its address known from blockIdx alone), then the plan word, whose index is the tile's window and so depends on the
// record's position.  The slot base is then a select among the four ids the record brought in registers, not a third
// dependent load.  A steady tile issues its 16-byte non-temporal loads from the one slot and stores them; a fade tile
// issues the loads of both slots back to back before the first crossfade.  The ragged ends go a sample per lane, as in
// agc_apply_body.  Nothing is indexed at run time but global memory: no scratch.
#include "k_agc.h"

namespace cmhip {

// ---------------------------------------------------------------------------
// energy (agc_energy_body with the slot indirection, k_agc.h)

template <int C>
__global__ __launch_bounds__(AGC_FAST_BLOCK) void k_failover_energy_fast(AgcArgs a)
{
    agc_energy_body<C, AGC_FAST_BLOCK, AGC_FAST_VECS / AGC_FAST_BLOCK, true>(a, nullptr);
}

__global__ __launch_bounds__(AGC_ANY_BLOCK) void k_failover_energy_any(AgcArgs a)
{
    __shared__ u64 lds[AGC_MAX_CH * AGC_ANY_BLOCK];
    agc_energy_body<0, AGC_ANY_BLOCK, AGC_ANY_VECS, true>(a, lds);
}

// ---------------------------------------------------------------------------
// step: a lane per output walks the windows the run touches, in order.  Window i of the run: where its first frame is
// processed in this run (every window but a carried first one) and it is not the output's window 0, the counters take
// the last complete window's levels -- with the quiet of THIS run -- and the plan moves on (failover_edge); then its plan
// word is written; then, where it ends inside the run, its m is taken per candidate -- otherwise it is the run's last
// window and its sums are carried.  An output with no frames returns before it touched anything.
__global__ __launch_bounds__(AGC_STEP_BLOCK) void k_failover_step(FailoverArgs a)
{
    const u32 o = blockIdx.x * AGC_STEP_BLOCK + threadIdx.x;
    if (o >= a.outputs)
        return;
    const u32 *rec = a.rec + (u64)o * FO_REC;
    const u32 count = rec[AREC_COUNT];
    if (count == 0)
        return;
    const u64 pos = (u64)rec[AREC_POS_LO] | ((u64)rec[AREC_POS_HI] << 32);
    u32 K;
    const FailoverParams p = failover_unpack(rec, &K);
    K = K < FO_SRC ? K : FO_SRC;
    const u32 C = a.energy.channels, w = a.energy.w, nw = a.energy.nw;
    FailoverState *st = a.state + o;
    u64 *table = a.energy.table + (u64)o * FO_SRC * nw * C;
    u32 *plan = a.plan + (u64)o * (nw + 1u);
    const bool fresh = pos == 0;                     // frame 0: creation, a reset or a new list since the last run
    uint64_t live = fresh ? 0u : (uint64_t)st->live, dead = fresh ? 0u : (uint64_t)st->dead;
    u32 pl = fresh ? failover_first(p) : st->plan;
    if (fresh)
        for (u32 c = 0; c < FO_SRC; c++)
            st->level[c] = 0;
    u32 begun = 0;
    const AgcRun r = agc_run(pos, count, w);
    const bool carried = ((u32)pos & ((1u << w) - 1u)) != 0;         // window 0 of the run began in an earlier run
    for (u32 i = 0; i < r.nwin && i < nw; i++) {
        if ((i > 0 || !carried) && r.first + i >= 1u) {
            for (u32 c = 0; c < K; c++)
                failover_count(st->level[c], failover_quiet(rec, c), c, live, dead);
            u32 sw;
            pl = failover_edge(pl, K, p, w, live, dead, &sw);
            begun += sw;
        }
        plan[i] = pl;
        const bool add = i == 0 && carried;
        for (u32 c = 0; c < K; c++) {
            u64 *row = table + ((u64)c * nw + i) * C;
            if (i < r.complete) {
                u64 E = 0;
                for (u32 ch = 0; ch < C; ch++) {
                    const u64 e = row[ch] + (add ? st->psum[c][ch] : 0ull);
                    row[ch] = 0;
                    E = e > E ? e : E;
                }
                st->level[c] = (u32)(E >> w);
            } else {
                for (u32 ch = 0; ch < C; ch++) {
                    st->psum[c][ch] = row[ch] + (add ? st->psum[c][ch] : 0ull);
                    row[ch] = 0;
                }
            }
        }
    }
    st->live = live;
    st->dead = dead;
    st->plan = pl;
    if (begun)
        a.switches[o] += begun;
}

// ---------------------------------------------------------------------------
// apply.  CT: the channel count of the fast forms, 0 for the any-channel-count form.  NT threads, NV vectors each.

__device__ __forceinline__ int fo_sample(const u32x4 &x, u32 i) { return (int)(short)(x[i >> 1] >> (16u * (i & 1u))); }

template <int CT, u32 NT, u32 NV>
__device__ __forceinline__ void failover_apply_body(const FailoverArgs &a)
{
    const AgcArgs &g = a.energy;
    const u32 C = CT ? (u32)CT : g.channels;
    const u32 o = blockIdx.x / g.chunks, t = blockIdx.x - o * g.chunks;
    const u32 *rec = a.rec + (u64)o * FO_REC;
    const u32 count = uniform(rec[AREC_COUNT]), pos_lo = uniform(rec[AREC_POS_LO]);
    const u32 s0 = uniform(rec[FREC_SRC]), s1 = uniform(rec[FREC_SRC + 1]), s2 = uniform(rec[FREC_SRC + 2]),
              s3 = uniform(rec[FREC_SRC + 3]);
    const AgcTile tl = agc_tile(pos_lo, count, g.w, g.tile_log2, t);
    if (tl.fa >= tl.fb)
        return;
    const FailoverPlan pl = failover_plan_unpack(uniform(a.plan[(u64)o * (g.nw + 1u) + tl.win]));
    const AgcSpan sp = agc_tile_span(tl.fa, tl.fb, C);
    const u32 slot_to = pl.to == 0 ? s0 : pl.to == 1 ? s1 : pl.to == 2 ? s2 : s3;
    const int16_t *xt = g.in + (u64)slot_to * g.in_stride;
    int16_t *outs = a.out + (u64)o * a.out_stride;
    const u32x4 *vt = reinterpret_cast<const u32x4 *>(xt);
    u32x4 *vout = reinterpret_cast<u32x4 *>(outs);
    const u32 tid = threadIdx.x;
    const u32 nh = sp.hend - sp.sa, nt = sp.sb - sp.tb;
    // the ragged ends, a sample per lane
    u32 e = 0xffffffffu;
    if (tid < nh)
        e = sp.sa + tid;
    else if (tid - nh < nt)
        e = sp.tb + (tid - nh);

    if (pl.from == pl.to) {                          // steady (uniform): a copy
        u32x4 x[NV];
#pragma unroll
        for (u32 j = 0; j < NV; j++) {
            const u32 v = sp.vb + tid + NT * j;
            x[j] = u32x4{0, 0, 0, 0};
            if (v < sp.ve)
                x[j] = __builtin_nontemporal_load(vt + v);
        }
        int16_t xe = 0;
        if (e != 0xffffffffu)
            xe = xt[e];
#pragma unroll
        for (u32 j = 0; j < NV; j++) {
            const u32 v = sp.vb + tid + NT * j;
            if (v < sp.ve)
                __builtin_nontemporal_store(x[j], vout + v);
        }
        if (e != 0xffffffffu)
            outs[e] = xe;
        return;
    }

    // a fade: both slots' loads first
    const u32 slot_from = pl.from == 0 ? s0 : pl.from == 1 ? s1 : pl.from == 2 ? s2 : s3;
    const int16_t *xf = g.in + (u64)slot_from * g.in_stride;
    const u32x4 *vf = reinterpret_cast<const u32x4 *>(xf);
    u32x4 xa[NV], xb[NV];
#pragma unroll
    for (u32 j = 0; j < NV; j++) {
        const u32 v = sp.vb + tid + NT * j;
        xa[j] = u32x4{0, 0, 0, 0};
        xb[j] = u32x4{0, 0, 0, 0};
        if (v < sp.ve) {
            xa[j] = __builtin_nontemporal_load(vf + v);
            xb[j] = __builtin_nontemporal_load(vt + v);
        }
    }
    int ea = 0, eb = 0;
    if (e != 0xffffffffu) {
        ea = (int)xf[e];
        eb = (int)xt[e];
    }
    const u32 d0 = (pl.q << g.w) + tl.j - tl.fa;     // run frame f is the fade's frame d0 + f (mod 2^32; f >= fa)
#pragma unroll
    for (u32 j = 0; j < NV; j++) {
        const u32 v = sp.vb + tid + NT * j;
        if (v < sp.ve) {
            u32 f = CT == 1 ? v * 8u : CT == 2 ? v * 4u : (v * 8u) / C;          // the frame of the vector's first sample
            u32 ch = CT ? 0u : v * 8u - f * C;
            u32 y[4] = {0, 0, 0, 0};
#pragma unroll
            for (u32 i = 0; i < 8; i++) {
                const u32 fi = CT == 1 ? f + i : CT == 2 ? f + (i >> 1) : f;
                const int yi = failover_fade(fo_sample(xa[j], i), fo_sample(xb[j], i), d0 + fi, pl.phi);
                y[i >> 1] |= ((u32)yi & 0xffffu) << (16u * (i & 1u));
                if constexpr (CT == 0) {
                    if (++ch == C) {
                        ch = 0;
                        f++;
                    }
                }
            }
            const u32x4 ov = {y[0], y[1], y[2], y[3]};
            __builtin_nontemporal_store(ov, vout + v);
        }
    }
    if (e != 0xffffffffu) {
        const u32 f = CT == 1 ? e : CT == 2 ? e >> 1 : e / C;
        outs[e] = (int16_t)failover_fade(ea, eb, d0 + f, pl.phi);
    }
}

template <int C>
__global__ __launch_bounds__(AGC_FAST_BLOCK) void k_failover_apply_fast(FailoverArgs a)
{
    failover_apply_body<C, AGC_FAST_BLOCK, AGC_FAST_VECS / AGC_FAST_BLOCK>(a);
}

__global__ __launch_bounds__(AGC_ANY_BLOCK) void k_failover_apply_any(FailoverArgs a)
{
    failover_apply_body<0, AGC_ANY_BLOCK, AGC_ANY_VECS>(a);
}

// ---------------------------------------------------------------------------
// launcher

hipError_t launch_failover(const FailoverArgs &a, uint64_t max_frames, uint32_t frames, hipStream_t st, hipEvent_t *ev)
{
    const u32 C = a.energy.channels;
    const AgcPlan p = plan_agc(a.outputs * FO_SRC, C, a.energy.w, max_frames, frames);
    if (p.grid == 0)
        return p.err ? hipErrorInvalidValue : hipSuccess;
    FailoverArgs b = a;
    b.energy.streams = a.outputs * FO_SRC;
    b.energy.nw = p.nw;
    b.energy.chunks = p.chunks;
    b.energy.tile_log2 = p.tile_log2;
    const u32 apply_grid = a.outputs * p.chunks;     // (a quarter of p.grid)
    // (ev: tools/bench_failover.py's four events around the three launches; no run of the library's own has any)
    auto mark = [&](unsigned i) { return ev ? hipEventRecord(ev[i], st) : hipSuccess; };
    hipError_t e = mark(0);
    if (e != hipSuccess)
        return e;
    if (!p.fast)
        hipLaunchKernelGGL(k_failover_energy_any, dim3(p.grid), dim3(p.block), 0, st, b.energy);
    else if (C == 1)
        hipLaunchKernelGGL(k_failover_energy_fast<1>, dim3(p.grid), dim3(p.block), 0, st, b.energy);
    else
        hipLaunchKernelGGL(k_failover_energy_fast<2>, dim3(p.grid), dim3(p.block), 0, st, b.energy);
    e = hipGetLastError();
    if (e != hipSuccess || (e = mark(1)) != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_failover_step, dim3((a.outputs + AGC_STEP_BLOCK - 1u) / AGC_STEP_BLOCK), dim3(AGC_STEP_BLOCK), 0,
                       st, b);
    e = hipGetLastError();
    if (e != hipSuccess || (e = mark(2)) != hipSuccess)
        return e;
    if (!p.fast)
        hipLaunchKernelGGL(k_failover_apply_any, dim3(apply_grid), dim3(p.block), 0, st, b);
    else if (C == 1)
        hipLaunchKernelGGL(k_failover_apply_fast<1>, dim3(apply_grid), dim3(p.block), 0, st, b);
    else
        hipLaunchKernelGGL(k_failover_apply_fast<2>, dim3(apply_grid), dim3(p.block), 0, st, b);
    e = hipGetLastError();
    return e != hipSuccess ? e : mark(3);
}

}  // namespace cmhip
