// k_spec.hip -- gfx950 (MI355X, wave64) spectrum kernel: per stream, selected channel and block of N = 2^n frames a
// Hann-windowed radix-2 FFT in exact integers through LDS, the bins' powers summed into bands, one 64-bit atomic add
// per band and workgroup into the stream's window.  A pass of its own, launched ahead of the block kernel of the same
// run: it reads the run's INPUT slots and transforms them itself with the block kernels' arithmetic (cmhip_device.h),
// as k_corr.hip does.  The arithmetic is include/coolmic_hip.h's ("spectrum"), the bookkeeping csrc/spec_plan.h's.
//
//   k_spec<n>   n = 8..12: workgroup (s, c, k) of a run takes block k of channel c of stream s, k below the stream's
//               block count of the run; workgroup (s, c, chunks - 1) writes the state the run leaves for (s, c).
//
// A block's samples come from two places: the stream's state (the N - 1 transformed samples before the run, slot
// `parity`) and the run's slot.  Both are only read in this launch -- the state workgroups write slot `parity ^ 1` --
// so a run longer than N has nothing to overwrite under a block that still reads it.  Integer sums merged by integer
// atomics do not depend on the order the workgroups arrive in: the windows are reproducible to the bit.  DESIGN 4.21.
#include "cmhip_device.h"

namespace cmhip {

typedef long long i64;

// an index into the padded LDS arrays: one word more per 32, against the power-of-two strides of the late stages
__device__ __forceinline__ u32 spec_pad(u32 i) { return i + (i >> 5); }

template <u32 LN>
__global__ __launch_bounds__(256) void k_spec(SpecArgs a)
{
    constexpr u32 N = 1u << LN, H = N / 2, NP = N + N / 32;
    __shared__ int zr[NP], zi[NP];
    __shared__ unsigned long long lband[SPEC_MAX_BANDS];
    __shared__ u32 ledge[SPEC_MAX_BANDS + 1];
    __shared__ u32 lmf[MAX_CH], lmi[MAX_CH], lmap[MAX_CH];

    const u32 tid = threadIdx.x;
    const u32 C = a.channels;
    const u32 row = blockIdx.x / a.chunks;       // (stream, selected channel)
    const u32 k = blockIdx.x - row * a.chunks;
    const u32 s = row / a.nch;
    const u32 ci = row - s * a.nch;
    const u32 nfr = a.nframes ? a.nframes[s] : a.frames;
    const u32 back = a.back[a.parity * a.streams + s];
    const u32 nblk = spec_run_blocks(LN, back, nfr);
    const bool state = k == a.chunks - 1u;       // (uniform)
    if (!state && k >= nblk)
        return;

    // The stream's map and gains go through LDS: the selected channel is a uniform run-time value, and a table in
    // LDS is indexed without a scalar load at a register offset (k_corr_any).
    const StreamParam *p = a.param + s;
    if (tid < C) {
        lmf[tid] = p->mf[tid];
        lmi[tid] = p->mi[tid];
        lmap[tid] = p->chmap[tid];
    }
    if (tid < SPEC_MAX_BANDS)
        lband[tid] = 0;
    if (tid <= a.nb)
        ledge[tid] = (u32)a.table[2 * N + tid];
    __syncthreads();
    const u32 ch = (u32)(a.chpack >> (8u * ci)) & 0xffu;
    const u32 im = lmap[ch], mi = lmi[ch], mf = lmf[ch];
    const int16_t *ins = a.in + (u64)s * a.stride;
    const int16_t *hold = a.hist + ((u64)(a.parity * a.streams + s) * a.nch + ci) * N;

    if (state) {
        // the last N - 1 transformed samples of (state, run): from the run where it reaches, from the state above that
        int16_t *hnew = a.hist + ((u64)((a.parity ^ 1u) * a.streams + s) * a.nch + ci) * N;
        for (u32 j = tid; j < N - 1u; j += 256u) {
            const int rel = (int)spec_state_frame(LN, nfr, j);
            hnew[j] = rel >= 0 ? (int16_t)gain1(ins[(u64)(u32)rel * C + im], mi, mf) : hold[j + nfr];
        }
        if (ci == 0 && tid == 0)
            a.back[(a.parity ^ 1u) * a.streams + s] = spec_next_back(LN, back, nfr);
        return;
    }

    // gather, window, bit-reversed into LDS
    const int32_t *wr = a.table, *wi = a.table + H, *win = a.table + N;
    for (u32 t = tid; t < N; t += 256u) {
        const int rel = (int)spec_block_frame(LN, back, k, t);
        const int x = rel >= 0 ? gain1(ins[(u64)(u32)rel * C + im], mi, mf) : (int)hold[(int)(N - 1u) + rel];
        const u32 r = spec_pad(__brev(t) >> (32u - LN));
        zr[r] = x * win[t];
        zi[r] = 0;
    }
    __syncthreads();

    // the n stages, in place: butterfly b of stage st pairs z[g m + j] and z[g m + j + m / 2], m = 2^st
#pragma unroll 1
    for (u32 st = 1; st <= LN; st++) {
        const u32 h = 1u << (st - 1u);
        for (u32 b = tid; b < H; b += 256u) {
            const u32 j = b & (h - 1u);
            const u32 ia = spec_pad(((b >> (st - 1u)) << st) + j), ib = spec_pad(((b >> (st - 1u)) << st) + j + h);
            const u32 kw = j << (LN - st);
            const i64 cr = wr[kw], cw = wi[kw];
            const i64 br = zr[ib], bi = zi[ib];
            const i64 pr = br * cr - bi * cw;
            const i64 pi = br * cw + bi * cr;
            const i64 ar = (i64)zr[ia] * SPEC_ONE + SPEC_ONE, ai = (i64)zi[ia] * SPEC_ONE + SPEC_ONE;
            zr[ia] = spec_round(ar, pr);
            zr[ib] = spec_round(ar, -pr);
            zi[ia] = spec_round(ai, pi);
            zi[ib] = spec_round(ai, -pi);
        }
        __syncthreads();
    }

    // Powers and bands: a thread takes PER consecutive bins of 0 .. N / 2 and walks the band table beside them (bd:
    // the band of the bin, -1 below the table, nb past it); a sum leaves for LDS when the band changes.
    constexpr u32 PER = (H + 1u + 255u) / 256u;
    const int nb = (int)a.nb;
    int bd = -1;
    u64 acc = 0;
    for (u32 q = 0; q < PER; q++) {
        const u32 bin = tid * PER + q;
        if (bin > H)
            break;
        int nd = bd;
        while (nd < nb && bin >= ledge[nd + 1])
            nd++;
        if (nd != bd) {
            if (acc && bd >= 0 && bd < nb)
                atomicAdd(&lband[bd], acc);
            acc = 0;
            bd = nd;
        }
        const i64 re = zr[spec_pad(bin)], ig = zi[spec_pad(bin)];
        acc += (u64)(re * re + ig * ig) >> 16;
    }
    if (acc && bd >= 0 && bd < nb)
        atomicAdd(&lband[bd], acc);
    __syncthreads();
    if (tid < a.nb && lband[tid])
        atomicAdd(&a.sums[((u64)s * SPEC_MAX_CH + ci) * SPEC_MAX_BANDS + tid], lband[tid]);
}

// ---------------------------------------------------------------------------
// launcher

SpecPlan plan_spec(const SpecArgs &a, uint32_t max_blocks)
{
    SpecPlan p{};
    p.err = hipSuccess;
    if (a.streams == 0 || a.frames == 0 || a.channels == 0 || a.channels > MAX_CH || a.nch == 0 ||
        a.nch > SPEC_MAX_CH || a.nb == 0 || a.nb > SPEC_MAX_BANDS || a.log2n < SPEC_MIN_LOG2 || a.log2n > SPEC_MAX_LOG2)
        return p;
    const u64 chunks = (u64)max_blocks + 1;
    if (chunks * a.streams * a.nch >= (1ull << 31)) {    // (as plan_run: no grid of 2^31 workgroups)
        SpecPlan refused{};
        refused.err = hipErrorInvalidValue;
        return refused;
    }
    p.chunks = (u32)chunks;
    p.grid = a.streams * a.nch * p.chunks;
    p.block = 256u;
    return p;
}

hipError_t launch_spec(const SpecArgs &a, uint32_t max_blocks, hipStream_t st)
{
    const SpecPlan p = plan_spec(a, max_blocks);
    if (p.grid == 0)
        return p.err;
    SpecArgs b = a;
    b.chunks = p.chunks;
    switch (a.log2n) {
    case 8: hipLaunchKernelGGL(k_spec<8>, dim3(p.grid), dim3(p.block), 0, st, b); break;
    case 9: hipLaunchKernelGGL(k_spec<9>, dim3(p.grid), dim3(p.block), 0, st, b); break;
    case 10: hipLaunchKernelGGL(k_spec<10>, dim3(p.grid), dim3(p.block), 0, st, b); break;
    case 11: hipLaunchKernelGGL(k_spec<11>, dim3(p.grid), dim3(p.block), 0, st, b); break;
    default: hipLaunchKernelGGL(k_spec<12>, dim3(p.grid), dim3(p.block), 0, st, b); break;
    }
    return hipGetLastError();
}

// test hook: the plan of a spectrum pass (host logic, needs no GPU)
extern "C" void cmhip_test_plan_spec(uint32_t streams, uint32_t channels, uint32_t frames, uint32_t fft_log2,
                                     uint32_t nch, uint32_t nb, uint32_t max_blocks, SpecPlan *plan)
{
    SpecArgs a{};
    a.streams = streams;
    a.channels = channels;
    a.frames = frames;
    a.log2n = fft_log2;
    a.nch = nch;
    a.nb = nb;
    if (plan)
        *plan = plan_spec(a, max_blocks);
}

}  // namespace cmhip
