// k_tpeak.hip -- gfx950 (MI355X, wave64) true-peak kernels: ITU-R BS.1770 Annex 2's 4x oversampling as a 48-tap
// polyphase FIR in exact integers over the TRANSFORMED stream (channel map, gain, saturation), and the running
// maximum of |y| per stream and channel.  A pass of its own, launched ahead of the block kernel of the same run: it
// reads the run's INPUT slots and transforms them itself with the block kernels' arithmetic (cmhip_device.h), so the
// samples are bit-identical to theirs and an in-place batch needs nothing special.
//
//   k_tpeak_fast<C>  mono, stereo: one wave per 8 KiB tile of one stream
//   k_tpeak_any      any channel count (3..16 in practice): one workgroup per 1024 frames, staged through LDS
//
// No recurrence, so the work is cut along time; what a tile needs of its predecessor is the 11-frame halo, read
// again from the same slot (the stream's first tile: from the stream's history).  Integer max is order independent:
// one atomicMax per channel and wave, results reproducible.  The mono / stereo kernel is VALU-issue-bound (24 dot
// instructions per sample), not bandwidth-bound: DESIGN 4.5.
#include "cmhip_device.h"

namespace cmhip {

// The stream's new history: the last 11 transformed frames of (old history, this run's frames), into the slot the
// next run reads.  Done by the workgroup of the stream's last tile (its first when the stream got no frame: the
// history moves over unchanged); fewer than 11 frames shift the old history by that many.
__device__ __forceinline__ void tp_history(const TpArgs &a, u32 s, u32 nfr, u32 C, const int16_t *ins)
{
    const int16_t *hrd = a.hist + ((u64)a.parity * a.streams + s) * (MAX_CH * TP_HIST);
    int16_t *hwr = a.hist + ((u64)(a.parity ^ 1u) * a.streams + s) * (MAX_CH * TP_HIST);
    const StreamParam *p = a.param + s;
    for (u32 idx = threadIdx.x; idx < C * TP_HIST; idx += blockDim.x) {
        const u32 c = idx / TP_HIST, i = idx - c * TP_HIST;
        int val;
        if (nfr + i < TP_HIST) {                     // frame nfr - 11 + i lies before this run
            val = hrd[c * TP_HIST + i + nfr];
        } else {
            const u64 m = (u64)nfr - TP_HIST + i;
            val = gain1(ins[m * C + p->chmap[c]], p->mi[c], p->mf[c]);
        }
        hwr[c * TP_HIST + i] = (int16_t)val;
    }
}

// ---------------------------------------------------------------------------
// Mono and stereo.
//
// A wave owns a contiguous tile of TP_U * 64 16-byte vectors of one stream; a lane owns TP_U consecutive vectors of
// it (128 bytes: one line) and loads the 2 (mono) / 3 (stereo) vectors before them as well: its halo.  Pairs of
// consecutive samples of one channel sit in a dword, P[t] = x[t-1] | x[t] << 16, and one v_dot2c_i32_i16 does two
// taps: y_p[t] = sum_{i<6} dot2(P[t - 2i], K[p][i]) with K[p][i] = H[p][2i+1] | H[p][2i] << 16, 24 constants.  Mono:
// P[t] is a loaded dword for odd t and one v_alignbit_b32 of two for even t; stereo: one v_perm_b32 per channel
// and frame.  The maximum of |y| is kept as a running maximum and a running minimum per lane (v_max3_i32 /
// v_min3_i32 take two values each), folded once at the end.
constexpr u32 TP_U = 8;                          // 16-byte vectors per lane
constexpr u32 TP_TILE_VEC = 64 * TP_U;           // vectors per wave: 8 KiB of PCM

constexpr u32 tp_pair(unsigned p, unsigned i)
{
    return (u32)(uint16_t)tp_h(p, 2 * i + 1) | ((u32)(uint16_t)tp_h(p, 2 * i) << 16);
}

__device__ __forceinline__ int tp_dot2(u32 x, u32 k, int acc)
{
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(v2s, x), __builtin_bit_cast(v2s, k), acc, false);
}

// FULL: every frame of the tile lies inside the stream's count -- no bounds tests.  Otherwise vectors past the
// count are not loaded and outputs past it do not count (what lies there is not the stream's).
template <int C, bool FULL>
__device__ __forceinline__ void tp_tile(const TpArgs &a, u32 s, u32 k, u32 nfr, u32 nvec, const int16_t *ins)
{
    constexpr u32 HV = C == 1 ? 2 : 3;           // halo vectors: 16 / 12 frames, 11 needed
    constexpr u32 FPV = 8 / C;                   // frames per vector
    constexpr u32 NV = TP_U + HV;
    constexpr u32 H = HV * FPV;                  // local index of the lane's first own frame
    constexpr u32 F = TP_U * FPV;                // own frames per lane
    const u32 lane = threadIdx.x & 63u;
    const u32 vl = k * TP_TILE_VEC + lane * TP_U;
    const u32x4 *src = reinterpret_cast<const u32x4 *>(ins);

    u32 d[NV * 4];
#pragma unroll
    for (u32 i = 0; i < NV; i++) {
        const int v = (int)vl + (int)i - (int)HV;
        u32x4 w = {0, 0, 0, 0};
        if (v >= 0 && (FULL || (u32)v < nvec))
            w = __builtin_nontemporal_load(src + v);
        d[4 * i] = w.x; d[4 * i + 1] = w.y; d[4 * i + 2] = w.z; d[4 * i + 3] = w.w;
    }

    // the stream's parameters, read behind the tile's loads (as fast_tile does, k_block.hip)
    __builtin_amdgcn_sched_barrier(0);
    const StreamParam *p = a.param + s;
    const u32 perm2 = p->perm2;
    const u32 mi01 = p->mi01;
    const u32 mf0 = p->mf[0], mf1 = p->mf[C - 1];
    const u32 mipk = C == 1 ? (mi01 & 0xffffu) * 0x10001u : mi01;

#pragma unroll
    for (u32 i = 0; i < NV * 4; i++) {
        u32 w = d[i];
        if constexpr (C == 2)
            w = __builtin_amdgcn_perm(w, w, perm2);      // stereo channel map
        (void)gain2<true>(w, mipk, mf0, mf1, d[i]);
        asm volatile("" : "+v"(d[i]));           // (finished here: sunk towards its uses the tail of every gain2
                                                 // stays pending, three registers per dword)
        if ((i & 3u) == 3u)                      // (a vector at a time: see the barrier in the loop below)
            __builtin_amdgcn_sched_barrier(0);
    }

    // the stream's first lane: its halo is the stream's history (transformed samples, as they were produced)
    if (k == 0) {                                // (uniform)
        const int16_t *h = a.hist + ((u64)a.parity * a.streams + s) * (MAX_CH * TP_HIST);
        if (lane == 0) {
#pragma unroll
            for (u32 i = 0; i < TP_HIST; i++) {
#pragma unroll
                for (u32 c = 0; c < (u32)C; c++) {
                    const u32 t = H - TP_HIST + i;           // local frame
                    const u32 idx = C == 1 ? t >> 1 : t, sh = C == 1 ? 16u * (t & 1u) : 16u * c;
                    const u32 val = (u32)(uint16_t)h[c * TP_HIST + i];
                    d[idx] = (d[idx] & ~(0xffffu << sh)) | (val << sh);
                }
            }
        }
    }

    int mx[C], mn[C];
#pragma unroll
    for (int c = 0; c < C; c++)
        mx[c] = mn[c] = 0;
    const u32 n0 = vl * FPV;                     // the lane's first own frame in the stream
    auto pair = [&](u32 t, u32 c) -> u32 {       // x_c[t-1] | x_c[t] << 16
        if constexpr (C == 1) {
            (void)c;
            return (t & 1u) ? d[t >> 1] : __builtin_amdgcn_alignbit(d[t >> 1], d[(t >> 1) - 1u], 16);
        } else {
            return __builtin_amdgcn_perm(d[t], d[t - 1u], c == 0 ? 0x05040100u : 0x07060302u);
        }
    };
#pragma unroll
    for (u32 t = H; t < H + F; t++) {
#pragma unroll
        for (u32 c = 0; c < (u32)C; c++) {
            int y[4] = {0, 0, 0, 0};
#pragma unroll
            for (u32 i = 0; i < TP_TAPS / 2; i++) {
                const u32 pr = pair(t - 2u * i, c);
                y[0] = tp_dot2(pr, tp_pair(0, i), y[0]);
                y[1] = tp_dot2(pr, tp_pair(1, i), y[1]);
                y[2] = tp_dot2(pr, tp_pair(2, i), y[2]);
                y[3] = tp_dot2(pr, tp_pair(3, i), y[3]);
            }
            if constexpr (!FULL) {               // (a mask, not a branch: the loop stays one basic block)
                const int keep = n0 + (t - H) < nfr ? -1 : 0;
                y[0] &= keep; y[1] &= keep; y[2] &= keep; y[3] &= keep;
            }
            mx[c] = max(max(mx[c], y[0]), y[1]);
            mx[c] = max(max(mx[c], y[2]), y[3]);
            mn[c] = min(min(mn[c], y[0]), y[1]);
            mn[c] = min(min(mn[c], y[2]), y[3]);
            // (one sample at a time: left to itself the scheduler interleaves all of the tile's dot chains and
            // needs 256 registers for it)
            __builtin_amdgcn_sched_barrier(0);
        }
    }

#pragma unroll
    for (int c = 0; c < C; c++) {
        const u32 pk = wave_max_u32(max((u32)mx[c], (u32)-mn[c]));
        if (lane == 0 && pk)
            atomicMax(&a.peak[(u64)s * MAX_CH + c], pk);
    }
}

template <int C>
__global__ __launch_bounds__(64) void k_tpeak_fast(TpArgs a)
{
    const int16_t *a_in = a.in;
    const u64 a_stride = a.stride;
    const u32 a_frames = a.frames;
    const u32 s = blockIdx.x / a.chunks;         // stream
    const u32 k = blockIdx.x - s * a.chunks;     // tile inside the stream
    const u32 nfr = a.nframes ? a.nframes[s] : a_frames;
    const u32 nsamp = nfr * (u32)C;
    const u32 nvec = (nsamp + 7u) >> 3;          // 16-byte vectors that hold a sample of the stream
    const u32 v0 = k * TP_TILE_VEC;
    const int16_t *ins = a_in + (u64)s * a_stride;
    if (v0 < nvec) {
        if (v0 + TP_TILE_VEC <= (nsamp >> 3))
            tp_tile<C, true>(a, s, k, nfr, nvec, ins);
        else
            tp_tile<C, false>(a, s, k, nfr, nvec, ins);
    }
    if (k == (nvec ? (nvec - 1u) / TP_TILE_VEC : 0u))
        tp_history(a, s, nfr, (u32)C, ins);
}

// ---------------------------------------------------------------------------
// Any channel count.  A workgroup of 256 threads takes TP_ANY_FRAMES frames of one stream: the transformed tile and
// its 11-frame halo go into LDS as planes, [C][TP_ANY_FRAMES + 11]; then one thread per channel and run of 16
// frames.  Bit-exact by the same integer arithmetic; no speed goal.
constexpr u32 TP_ANY_FRAMES = 1024;
constexpr u32 TP_ANY_RUN = 16;
constexpr u32 TP_ANY_ROW = TP_ANY_FRAMES + TP_HIST;

__global__ __launch_bounds__(256) void k_tpeak_any(TpArgs a)
{
    __shared__ int16_t plane[MAX_CH * TP_ANY_ROW];
    __shared__ u32 lpeak[MAX_CH];
    const u32 C = a.channels;
    const u32 s = blockIdx.x / a.chunks;
    const u32 k = blockIdx.x - s * a.chunks;
    const u32 nfr = a.nframes ? a.nframes[s] : a.frames;
    const u32 f0 = k * TP_ANY_FRAMES;            // the tile's first frame
    const int16_t *ins = a.in + (u64)s * a.stride;
    const StreamParam *p = a.param + s;
    const int16_t *hrd = a.hist + ((u64)a.parity * a.streams + s) * (MAX_CH * TP_HIST);

    if (f0 < nfr) {                              // (uniform)
        if (threadIdx.x < MAX_CH)
            lpeak[threadIdx.x] = 0;
        for (u32 idx = threadIdx.x; idx < C * TP_ANY_ROW; idx += blockDim.x) {
            const u32 lf = idx / C, c = idx - lf * C;        // local frame (0: the tile's frame -11), channel
            int val = 0;
            if (f0 + lf < TP_HIST)                           // before this run (only the stream's first tile)
                val = hrd[c * TP_HIST + f0 + lf];
            else if (f0 + lf - TP_HIST < nfr)
                val = gain1(ins[(u64)(f0 + lf - TP_HIST) * C + p->chmap[c]], p->mi[c], p->mf[c]);
            plane[c * TP_ANY_ROW + lf] = (int16_t)val;
        }
        __syncthreads();
        for (u32 idx = threadIdx.x; idx < C * (TP_ANY_FRAMES / TP_ANY_RUN); idx += blockDim.x) {
            const u32 r = idx / C, c = idx - r * C;
            const int16_t *x = plane + c * TP_ANY_ROW + r * TP_ANY_RUN;      // x[f + 11] is the run's frame f
            int xs[TP_ANY_RUN + TP_HIST];
#pragma unroll
            for (u32 j = 0; j < TP_ANY_RUN + TP_HIST; j++)
                xs[j] = x[j];
            u32 pk = 0;
#pragma unroll
            for (u32 f = 0; f < TP_ANY_RUN; f++) {
                if (f0 + r * TP_ANY_RUN + f >= nfr)
                    break;
#pragma unroll
                for (u32 ph = 0; ph < 4; ph++) {
                    int y = 0;
#pragma unroll
                    for (u32 t = 0; t < TP_TAPS; t++)
                        y += (int)tp_h(ph, t) * xs[f + TP_HIST - t];
                    pk = max(pk, (u32)(y < 0 ? -y : y));
                }
            }
            if (pk)
                atomicMax(&lpeak[c], pk);
        }
        __syncthreads();
        if (threadIdx.x < C && lpeak[threadIdx.x])
            atomicMax(&a.peak[(u64)s * MAX_CH + threadIdx.x], lpeak[threadIdx.x]);
    }
    if (k == (nfr ? (nfr - 1u) / TP_ANY_FRAMES : 0u))
        tp_history(a, s, nfr, C, ins);
}

// ---------------------------------------------------------------------------
// launcher

TpPlan plan_tpeak(const TpArgs &a)
{
    TpPlan p{};
    p.err = hipSuccess;
    if (a.streams == 0 || a.frames == 0 || a.channels == 0 || a.channels > MAX_CH)
        return p;
    p.fast = a.channels <= 2 ? 1u : 0u;
    const u64 nvec = ((u64)a.frames * a.channels + 7) / 8;
    const u64 tiles = p.fast ? (nvec + TP_TILE_VEC - 1) / TP_TILE_VEC : ((u64)a.frames + TP_ANY_FRAMES - 1) / TP_ANY_FRAMES;
    if (tiles * a.streams >= (1ull << 31)) {     // (as plan_run: no grid of 2^31 workgroups)
        TpPlan refused{};
        refused.err = hipErrorInvalidValue;
        return refused;
    }
    p.chunks = (u32)tiles;
    p.grid = a.streams * p.chunks;
    p.block = p.fast ? 64u : 256u;
    return p;
}

hipError_t launch_tpeak(const TpArgs &a, hipStream_t st)
{
    const TpPlan p = plan_tpeak(a);
    if (p.grid == 0)
        return p.err;
    TpArgs b = a;
    b.chunks = p.chunks;
    if (!p.fast)
        hipLaunchKernelGGL(k_tpeak_any, dim3(p.grid), dim3(p.block), 0, st, b);
    else if (a.channels == 1)
        hipLaunchKernelGGL(k_tpeak_fast<1>, dim3(p.grid), dim3(p.block), 0, st, b);
    else
        hipLaunchKernelGGL(k_tpeak_fast<2>, dim3(p.grid), dim3(p.block), 0, st, b);
    return hipGetLastError();
}

// test hook: the plan of a true-peak pass (host logic, needs no GPU)
extern "C" void cmhip_test_plan_tpeak(uint32_t streams, uint32_t channels, uint32_t frames, TpPlan *plan)
{
    TpArgs a{};
    a.streams = streams;
    a.channels = channels;
    a.frames = frames;
    if (plan)
        *plan = plan_tpeak(a);
}

}  // namespace cmhip
