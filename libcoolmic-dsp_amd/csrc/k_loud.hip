// k_loud.hip -- gfx950 (MI355X, wave64) loudness kernels: ITU-R BS.1770's K-weighting (two biquads in double, Direct
// Form I, every product and sum rounded once) over the TRANSFORMED stream (channel map, gain, saturation), and the
// sum of squares of its output per 100 ms sub-block, stream and channel.  A pass of its own, launched ahead of the
// block kernel of the same run: it reads the run's INPUT slots and transforms them itself with the block kernels'
// arithmetic (gain1, cmhip_device.h), so the samples are bit-identical to theirs and an in-place batch needs nothing
// special.
//
//   k_loud_vec<C>  mono, stereo: a lane walks its stream's slot in 16-byte vectors, the next one loaded ahead
//   k_loud_any     any channel count: 2-byte loads, the next sample loaded ahead
//
// The arithmetic is specified to the bit (include/coolmic_hip.h) and time is a recurrence, so there is no
// parallelism along a stream: a ROW -- one channel of one stream -- is one lane, rows are the parallelism, and a
// workgroup is one wave so that the waves spread over all CUs.  Exactly one lane owns a row's LoudState in a launch:
// it is read at the start and written back at the end, no atomics.  The file is built with -ffp-contract=off like
// the rest: no fused multiply-add may appear in the recurrence (tests/test_loudness_host.py reads the assembly).
#include "cmhip_device.h"

namespace cmhip {

// a row in registers
struct LoudLane {
    double u1, u2, y1, y2, v1, v2, e;
    u32 pos, slot;
    u64 done;
    double *ring;                                // the row's element of ring slot 0; slots are `step` doubles apart
};

struct LoudCoef {
    double b0, b1, b2, a1, a2;                   // section 1
    double c1, c2;                               // section 2's a1, a2 (its numerator is exactly 1, -2, 1)
};

__device__ __forceinline__ LoudCoef loud_coef(const LoudArgs &a)
{
    return {a.coef[0], a.coef[1], a.coef[2], a.coef[3], a.coef[4], a.coef[8], a.coef[9]};
}

// one transformed sample x into the row:
//   f = (b0*u + b1*u1) + b2*u2    y = (f - a2*y2) - a1*y1      section 1, u = x / 32768 (exact)
//   g = (y - 2*y1) + y2           v = (g - c2*v2) - c1*v1      section 2: the products by 1 and -2 are exact
//   e += v*v, and at the sub-block's last frame e goes to the ring and starts again from 0.0
__device__ __forceinline__ void loud_step(LoudLane &r, const LoudCoef &k, int x, u32 sub, u32 slots, u64 step)
{
    const double u = (double)x * 0x1p-15;
    const double f = (k.b0 * u + k.b1 * r.u1) + k.b2 * r.u2;
    const double y = (f - k.a2 * r.y2) - k.a1 * r.y1;
    const double g = (y - 2.0 * r.y1) + r.y2;
    const double v = (g - k.c2 * r.v2) - k.c1 * r.v1;
    r.u2 = r.u1;
    r.u1 = u;
    r.y2 = r.y1;
    r.y1 = y;
    r.v2 = r.v1;
    r.v1 = v;
    r.e += v * v;
    if (++r.pos == sub) {
        r.ring[(u64)r.slot * step] = r.e;
        r.e = 0.0;
        r.pos = 0;
        r.slot = r.slot + 1u == slots ? 0u : r.slot + 1u;
        r.done++;
    }
}

__device__ __forceinline__ LoudLane loud_open(const LoudArgs &a, u32 row, u32 s, u32 c)
{
    const LoudState st = a.state[row];
    LoudLane r;
    r.u1 = st.u1; r.u2 = st.u2; r.y1 = st.y1; r.y2 = st.y2; r.v1 = st.v1; r.v2 = st.v2;
    r.e = st.e;
    r.pos = st.pos;
    r.done = st.done;
    r.slot = (u32)(st.done % a.ring_slots);
    r.ring = a.ring + (u64)s * a.ring_slots * a.channels + c;
    return r;
}

__device__ __forceinline__ void loud_close(const LoudArgs &a, u32 row, const LoudLane &r)
{
    LoudState st;
    st.u1 = r.u1; st.u2 = r.u2; st.y1 = r.y1; st.y2 = r.y2; st.v1 = r.v1; st.v2 = r.v2;
    st.e = r.e;
    st.pos = r.pos;
    st.pad = 0;
    st.done = r.done;
    a.state[row] = st;
}

// ---------------------------------------------------------------------------
// Mono and stereo: a fixed position of a 16-byte vector has a fixed channel.  The whole vectors of the lane's count
// are loaded as such, the next one before the current one's 8 / C steps of the recurrence; the frames of a ragged last
// vector are read sample by sample (nothing past the stream's count is read).  A stereo row takes the half of each
// dword that its channel map names; both rows of a stream read the same vectors.
template <int C>
__global__ __launch_bounds__(64) void k_loud_vec(LoudArgs a)
{
    constexpr u32 FPV = 8 / C;                   // frames per vector
    const u32 row = blockIdx.x * 64u + threadIdx.x;
    if (row >= a.streams * (u32)C)
        return;
    const u32 s = row / (u32)C, c = row - s * (u32)C;
    const u32 nfr = a.nframes ? a.nframes[s] : a.frames;
    if (nfr == 0)                                // a stream that gets no frame keeps everything
        return;
    const StreamParam *p = a.param + s;
    const u32 in_ch = C == 1 ? 0u : (p->chmap[c] & 1u);
    const u32 sh = 16u * in_ch;
    const u32 mi = p->mi[c], mf = p->mf[c];
    const int16_t *ins = a.in + (u64)s * a.stride;
    const u32x4 *src = reinterpret_cast<const u32x4 *>(ins);
    const LoudCoef k = loud_coef(a);
    const u32 sub = a.sub, slots = a.ring_slots;
    const u64 step = a.channels;
    LoudLane r = loud_open(a, row, s, c);

    const u32 nfull = nfr / FPV;
    u32x4 cur = {0, 0, 0, 0};
    if (nfull)
        cur = src[0];
    for (u32 v = 0; v < nfull; v++) {
        u32x4 nxt = cur;
        if (v + 1u < nfull)
            nxt = src[v + 1u];
        const u32 d[4] = {cur.x, cur.y, cur.z, cur.w};
#pragma unroll
        for (u32 j = 0; j < FPV; j++) {
            int x;
            if constexpr (C == 1)
                x = (int)(short)(d[j >> 1] >> (16u * (j & 1u)));
            else
                x = (int)(short)(d[j] >> sh);
            loud_step(r, k, gain1(x, mi, mf), sub, slots, step);
        }
        cur = nxt;
    }
    for (u32 f = nfull * FPV; f < nfr; f++)
        loud_step(r, k, gain1(ins[(u64)f * C + in_ch], mi, mf), sub, slots, step);
    loud_close(a, row, r);
}

// ---------------------------------------------------------------------------
// Any channel count: the lanes of a stream's rows read neighbouring samples of a frame, 2 bytes each.
__global__ __launch_bounds__(64) void k_loud_any(LoudArgs a)
{
    const u32 C = a.channels;
    const u32 row = blockIdx.x * 64u + threadIdx.x;
    if (row >= a.streams * C)
        return;
    const u32 s = row / C, c = row - s * C;
    const u32 nfr = a.nframes ? a.nframes[s] : a.frames;
    if (nfr == 0)
        return;
    const StreamParam *p = a.param + s;
    const u32 mi = p->mi[c], mf = p->mf[c];
    const int16_t *src = a.in + (u64)s * a.stride + p->chmap[c];
    const LoudCoef k = loud_coef(a);
    const u32 sub = a.sub, slots = a.ring_slots;
    const u64 step = C;
    LoudLane r = loud_open(a, row, s, c);

    int cur = src[0];
    for (u32 f = 0; f < nfr; f++) {
        int nxt = cur;
        if (f + 1u < nfr)
            nxt = src[(u64)(f + 1u) * C];
        loud_step(r, k, gain1(cur, mi, mf), sub, slots, step);
        cur = nxt;
    }
    loud_close(a, row, r);
}

// ---------------------------------------------------------------------------
// launcher

LoudPlan plan_loud(const LoudArgs &a)
{
    LoudPlan p{};
    p.err = hipSuccess;
    if (a.streams == 0 || a.frames == 0 || a.channels == 0 || a.channels > MAX_CH)
        return p;
    const u64 rows = (u64)a.streams * a.channels;
    const u64 waves = (rows + 63) / 64;
    if (waves >= (1ull << 31) || rows >= (1ull << 32)) {     // (as plan_run: no grid of 2^31 workgroups)
        LoudPlan refused{};
        refused.err = hipErrorInvalidValue;
        return refused;
    }
    p.vec = a.channels <= 2 ? 1u : 0u;
    p.grid = (u32)waves;
    p.block = 64;
    return p;
}

hipError_t launch_loud(const LoudArgs &a, hipStream_t st)
{
    const LoudPlan p = plan_loud(a);
    if (p.grid == 0)
        return p.err;
    if (a.sub == 0 || a.ring_slots == 0)
        return hipErrorInvalidValue;
    if (!p.vec)
        hipLaunchKernelGGL(k_loud_any, dim3(p.grid), dim3(p.block), 0, st, a);
    else if (a.channels == 1)
        hipLaunchKernelGGL(k_loud_vec<1>, dim3(p.grid), dim3(p.block), 0, st, a);
    else
        hipLaunchKernelGGL(k_loud_vec<2>, dim3(p.grid), dim3(p.block), 0, st, a);
    return hipGetLastError();
}

// test hook: the plan of a loudness pass (host logic, needs no GPU)
extern "C" void cmhip_test_plan_loud(uint32_t streams, uint32_t channels, uint32_t frames, LoudPlan *plan)
{
    LoudArgs a{};
    a.streams = streams;
    a.channels = channels;
    a.frames = frames;
    if (plan)
        *plan = plan_loud(a);
}

}  // namespace cmhip
