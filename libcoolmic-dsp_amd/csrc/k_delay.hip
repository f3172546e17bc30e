// k_delay.hip -- gfx950 (MI355X, wave64) delay-line kernels: S streams of C interleaved int16 channels come out d_s frames
// later, with a ring of the last frames per stream as the only state (include/coolmic_hip.h, "delay", has the arithmetic
// to the bit; csrc/delay_plan.h the ring, the positions and the tile classes):
//     y[n][c] = x[n - d][c]                                          outside a ramp
//     y = x0 + ((p * (x1 - x0) + 16384) >> 15)                       inside one: x0, x1 the taps d0, d1, p per frame
//
//   k_delay_fast<C>  C in {1, 2}: one short-lived wave per tile of 256 output vectors, four per lane
//   k_delay_any      every other channel count up to 16: 256 threads per tile of 256 frames; no speed goal
//
// Both are ONE tile body (delay_body) over SAMPLES: a delay of d frames shifts the interleaved stream by D = d * C samples
// whatever C is, so the channel count only sizes the tile and, in a ramp, tells a sample's frame.  The work is a copy.
// Per tile and tap the source is classified once, wave-uniformly (delay_tap): behind the seam it is the input, in front
// of it an unwrapped stretch of the ring, and either is read with ALIGNED 16-byte loads -- the vector that holds a
// granule's first sample and, where the source is misaligned, the next one -- and one funnel shift (v_alignbyte) by the
// tile's uniform amount.  In a tile on the seam or on the ring's wrap each vector is classified by itself and only the
// one vector that holds the seam or the wrap gathers its samples one by one.  The crossfade is a
// second path of the same body; a stream outside a ramp never takes it.
//
// The ring is written from the input by the same workgroup: the run's samples [P, P + N) modulo CAP, in the ring's own
// 16-byte granules (again aligned loads and a uniform shift), the ragged ends sample by sample.  A run reads only
// [P - D, P): no workgroup reads what another writes.  Aligned loads may cover ring samples that another workgroup
// writes in this launch; the shift or the count drops exactly those.
#include "k_mix.h"

namespace cmhip {

struct DelayCtx {                                    // a stream's run (wave-uniform)
    const int16_t *ins;
    int16_t *outs, *rs;
    u32 N, P, CAP, in_vecs;
};

// vector a of `base` and, where the shift needs it, the one behind it -- each only while it lies below nvec
__device__ __forceinline__ void delay_fetch(const int16_t *base, u32 nvec, u32 a, u32 sh, u32 (&w)[8])
{
    const u32x4 *p = reinterpret_cast<const u32x4 *>(base);
    u32x4 lo = {0, 0, 0, 0}, hi = {0, 0, 0, 0};
    if (a < nvec)
        lo = p[a];
    if (sh != 0 && a + 1u < nvec)
        hi = p[a + 1u];
    w[0] = lo.x; w[1] = lo.y; w[2] = lo.z; w[3] = lo.w;
    w[4] = hi.x; w[5] = hi.y; w[6] = hi.z; w[7] = hi.w;
}

// output samples e .. e + 7 at a delay of D samples, one by one: the input behind the seam, the ring in front of it
__device__ __forceinline__ void delay_gather(const DelayCtx &c, u32 D, u32 e, u32 (&w)[8])
{
#pragma unroll
    for (u32 i = 0; i < 8; i++)
        w[i] = 0;
#pragma unroll
    for (u32 i = 0; i < 8; i++) {
        const u32 ee = e + i;
        u32 val = 0;
        if (ee < c.N) {
            if (ee >= D)
                val = (u32)(uint16_t)c.ins[ee - D];
            else
                val = (u32)(uint16_t)c.rs[delay_ring_index(c.P, c.CAP, (int64_t)ee - (int64_t)D)];
        }
        w[i >> 1] |= val << (16u * (i & 1u));
    }
}

// samples sh .. sh + 7 of the sixteen in w (sh uniform outside a mixed tile): a choice of dwords and a funnel shift by
// 0 or 2 bytes
template <u32 DW>
__device__ __forceinline__ void delay_shift_dw(const u32 (&w)[8], u32 bytes, u32 (&x)[4])
{
#pragma unroll
    for (u32 i = 0; i < 4; i++)
        x[i] = __builtin_amdgcn_alignbyte(w[i + DW + 1u], w[i + DW], bytes);
}
__device__ __forceinline__ void delay_shift(const u32 (&w)[8], u32 sh, u32 (&x)[4])
{
    const u32 bytes = (sh & 1u) * 2u;
    switch (sh >> 1) {
    case 0: delay_shift_dw<0>(w, bytes, x); break;
    case 1: delay_shift_dw<1>(w, bytes, x); break;
    case 2: delay_shift_dw<2>(w, bytes, x); break;
    default: delay_shift_dw<3>(w, bytes, x); break;
    }
}

// vector t of a tile for one tap (e: the vector's first output sample): loads and shift.  The tile's class is uniform
// over the wave.  In a tile on the seam or on the wrap every vector is classified again by itself, per lane: class,
// source and shift then differ between the lanes -- a vector behind the seam has the shift (-D) mod 8, one in front of
// it (P - D) mod 8 -- and the branches below and the switch of delay_shift diverge.  Only the vector that holds the seam
// or the wrap goes sample by sample.
__device__ __forceinline__ void delay_source(const DelayCtx &c, DelayTap tap, u32 D, u32 t, u32 e, u32 (&x)[4])
{
    u32 w[8];
    u32 sh = tap.q & 7u;
    if (tap.cls == DELAY_MIXED) {                    // (uniform; what follows inside is per lane)
        const DelayTap v = delay_tap(e, 8u, D, c.P, c.CAP);
        sh = v.q & 7u;
        if (v.cls == DELAY_BEHIND)
            delay_fetch(c.ins, c.in_vecs, v.q >> 3, sh, w);
        else if (v.cls == DELAY_FRONT)
            delay_fetch(c.rs, c.CAP >> 3, v.q >> 3, sh, w);
        else
            delay_gather(c, D, e, w);                // (sh = 0: delay_tap gives q = 0 here)
    } else if (tap.cls == DELAY_BEHIND) {
        delay_fetch(c.ins, c.in_vecs, (tap.q >> 3) + t, sh, w);
    } else {
        delay_fetch(c.rs, c.CAP >> 3, (tap.q >> 3) + t, sh, w);
    }
    delay_shift(w, sh, x);
}

// the crossfade of two vectors whose first sample is sample e of the run; frame f of the run is the ramp's done + f + 1
template <int CT>
__device__ __forceinline__ void delay_fade(u32 C, u32 e, u32 done, u32 R, u32 inc, const u32 (&x0)[4], const u32 (&x1)[4],
                                           u32 (&y)[4])
{
#pragma unroll
    for (u32 i = 0; i < 4; i++)
        y[i] = 0;
#pragma unroll
    for (u32 i = 0; i < 8; i++) {
        const u32 f = CT == 1 ? e + i : CT == 2 ? (e + i) >> 1 : (e + i) / C;
        const int p = (int)mixr_pos(done + f + 1u, R, inc);
        const int a = (int)(short)(x0[i >> 1] >> (16u * (i & 1u))), b = (int)(short)(x1[i >> 1] >> (16u * (i & 1u)));
        const int v = a + ((p * (b - a) + 16384) >> 15);             // |p (b - a)| <= 2^15 * 65535: int32 is exact
        y[i >> 1] |= ((u32)v & 0xffffu) << (16u * (i & 1u));
    }
}

// output vector e / 8: whole and non-temporal, or the stream's ragged end sample by sample; nothing past the count
__device__ __forceinline__ void delay_store_out(const DelayCtx &c, u32 e, const u32 (&x)[4])
{
    if (e + 8u <= c.N) {
        const u32x4 ov = {x[0], x[1], x[2], x[3]};
        __builtin_nontemporal_store(ov, reinterpret_cast<u32x4 *>(c.outs) + (e >> 3));
    } else if (e < c.N) {
        store_tail(c.outs, e >> 3, x, c.N - e);
    }
}

// the ring granule that begins at sample es of the run (es + P is a multiple of 8): whole, or the run's ragged end
__device__ __forceinline__ void delay_store_ring(const DelayCtx &c, u32 es, const u32 (&x)[4])
{
    if (es >= c.N)
        return;
    const u32 r = delay_ring_index(c.P, c.CAP, (int64_t)es);         // a multiple of 8, at most CAP - 8
    if (es + 8u <= c.N) {
        const u32x4 rv = {x[0], x[1], x[2], x[3]};
        *reinterpret_cast<u32x4 *>(c.rs + r) = rv;
    } else {
        const u32 n = c.N - es;
        for (u32 j = 0; j < n; j++)
            c.rs[r + j] = (int16_t)half_at(x, j);
    }
}

// ---------------------------------------------------------------------------
// The tile.  CT: the channel count of the fast forms, 0 for the any-channel-count form.  NT threads, NV vectors each.
template <int CT, u32 NT, u32 NV, bool RAMP>
__device__ __forceinline__ void delay_tile(const DelayCtx &c, u32 C, u32 tile_vecs, u32 e0, DelayTap tap0, DelayTap tap1,
                                           u32 D0, u32 D1, u32 done, u32 R, u32 inc)
{
    const u32 tid = threadIdx.x;
    const u32 h = delay_ring_head(c.P);
    const DelayTap tin = {DELAY_BEHIND, e0 + h};                     // the ring's granules: the input from e0 + h on

    // ---- every load of the tile, shifted into place.  A vector past the stream's count owns no output and no ring
    // granule (e + h >= N with it): it loads nothing, so a short last tile moves what it needs and reads no ring
    // granule that another workgroup writes.
    u32 x1[NV][4] = {}, x0[RAMP ? NV : 1u][4] = {}, xr[NV][4] = {};
#pragma unroll
    for (u32 j = 0; j < NV; j++) {
        const u32 t = tid + NT * j, e = e0 + 8u * t;
        if ((CT != 0 || t < tile_vecs) && e < c.N) {
            delay_source(c, tap1, D1, t, e, x1[j]);
            if constexpr (RAMP)
                delay_source(c, tap0, D0, t, e, x0[j]);
            delay_source(c, tin, 0u, t, e, xr[j]);
        }
    }

    // ---- the crossfade, stores
#pragma unroll
    for (u32 j = 0; j < NV; j++) {
        const u32 t = tid + NT * j, e = e0 + 8u * t;
        if ((CT != 0 || t < tile_vecs) && e < c.N) {
            if constexpr (RAMP) {
                u32 y[4];
                delay_fade<CT>(C, e, done, R, inc, x0[j], x1[j], y);
                delay_store_out(c, e, y);
            } else {
                delay_store_out(c, e, x1[j]);
            }
            delay_store_ring(c, e + h, xr[j]);
        }
    }
}

template <int CT, u32 NT, u32 NV>
__device__ __forceinline__ void delay_body(const DelayArgs &a)
{
    const u32 C = CT ? (u32)CT : a.channels;
    const u32 tile_vecs = CT ? DELAY_FAST_VECS : a.tile_vecs;
    const u32 s = blockIdx.x / a.chunks;             // stream
    const u32 k = blockIdx.x - s * a.chunks;         // tile inside the stream
    const u32 *rec = a.rec + (u64)s * DELAY_REC;
    const u32 F = uniform(rec[DREC_COUNT]);
    const u32 N = F * C, e0 = k * tile_vecs * 8u;
    if (e0 >= N)                                     // (uniform)
        return;
    const u32 pos = uniform(rec[DREC_POS]), d1 = uniform(rec[DREC_D1]), d0 = uniform(rec[DREC_D0]);
    const u32 R = uniform(rec[DREC_R]), done = uniform(rec[DREC_DONE]), inc = uniform(rec[DREC_INC]);
    DelayCtx c;
    c.ins = a.in + (u64)s * a.in_stride;
    c.outs = a.out + (u64)s * a.out_stride;
    c.rs = a.ring + (u64)s * a.ring_samples;
    c.N = N;
    c.P = pos * C;
    c.CAP = a.ring_samples;
    c.in_vecs = (u32)min(a.in_stride >> 3, (u64)0xffffffffu);
    const u32 len = min(tile_vecs * 8u, N - e0);
    const u32 D1 = d1 * C, D0 = d0 * C;
    const DelayTap tap1 = delay_tap(e0, len, D1, c.P, c.CAP);

    // the run's samples in front of the ring's first whole granule
    if (k == 0 && threadIdx.x < delay_ring_head(c.P) && threadIdx.x < N)
        c.rs[delay_ring_index(c.P, c.CAP, (int64_t)threadIdx.x)] = c.ins[threadIdx.x];

    if (done < R)                                    // (uniform) the stream ramps
        delay_tile<CT, NT, NV, true>(c, C, tile_vecs, e0, delay_tap(e0, len, D0, c.P, c.CAP), tap1, D0, D1, done, R, inc);
    else
        delay_tile<CT, NT, NV, false>(c, C, tile_vecs, e0, tap1, tap1, D1, D1, 0, 0, 0);
}

template <int C>
__global__ __launch_bounds__(DELAY_FAST_BLOCK) void k_delay_fast(DelayArgs a)
{
    delay_body<C, DELAY_FAST_BLOCK, DELAY_FAST_VECS / DELAY_FAST_BLOCK>(a);
}

__global__ __launch_bounds__(DELAY_ANY_BLOCK) void k_delay_any(DelayArgs a)
{
    delay_body<0, DELAY_ANY_BLOCK, DELAY_ANY_FRAMES * DELAY_MAX_CH / 8u / DELAY_ANY_BLOCK>(a);
}

// ---------------------------------------------------------------------------
// launcher

hipError_t launch_delay(const DelayArgs &a, uint32_t max_delay, uint32_t max_frames, uint32_t frames, hipStream_t st)
{
    const DelayPlan p = plan_delay(a.streams, a.channels, max_delay, max_frames, frames);
    if (p.grid == 0)
        return p.err ? hipErrorInvalidValue : hipSuccess;
    DelayArgs b = a;
    b.chunks = p.chunks;
    b.tile_vecs = p.tile_vecs;
    if (!p.fast)
        hipLaunchKernelGGL(k_delay_any, dim3(p.grid), dim3(p.block), 0, st, b);
    else if (a.channels == 1)
        hipLaunchKernelGGL(k_delay_fast<1>, dim3(p.grid), dim3(p.block), 0, st, b);
    else
        hipLaunchKernelGGL(k_delay_fast<2>, dim3(p.grid), dim3(p.block), 0, st, b);
    return hipGetLastError();
}

// test hooks (host logic, need no GPU): the plan of a run whose longest stream has `frames` frames, and the class of a
// tile for one tap
extern "C" void cmhip_test_plan_delay(uint32_t streams, uint32_t channels, uint32_t max_delay, uint32_t max_frames,
                                      uint32_t frames, DelayPlan *plan)
{
    if (plan)
        *plan = plan_delay(streams, channels, max_delay, max_frames, frames);
}

extern "C" void cmhip_test_delay_tap(uint32_t e0, uint32_t len, uint32_t D, uint32_t P, uint32_t CAP, uint32_t *cls,
                                     uint32_t *q)
{
    const DelayTap t = delay_tap(e0, len, D, P, CAP);
    if (cls)
        *cls = t.cls;
    if (q)
        *q = t.q;
}

}  // namespace cmhip
