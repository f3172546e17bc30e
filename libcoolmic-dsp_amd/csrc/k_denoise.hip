// k_denoise.hip -- gfx950 (MI355X, wave64) noise suppressor kernel: per row (stream, channel) the run's blocks of
// N = 2^n frames in order -- the spectrum's forward transform under a sine window, the per-bin gain law and its
// smoothing, the learning of the profile, the removed spectrum, the inverse transform, the synthesis window and the
// overlap-add -- and the output, the delayed input less the removed part.  The arithmetic is include/coolmic_hip.h's
// ("noise suppressor"), the bookkeeping csrc/spec_plan.h's, the steps csrc/denoise_plan.h's.
//
//   k_denoise<n>   n = 8..12: workgroup `row` of 256 threads takes row (s, c) through the whole run.
//
// The shape and its reason.  A row's gains and profile are recurrences over its blocks: block i needs g and Np as block
// i - 1 left them, and the overlap-add needs the block before.  One workgroup that walks a row's blocks in order keeps
// both transforms' planes in LDS (two int32 planes of N words, padded: 33 KiB at N = 4096, so four workgroups fit a CU),
// needs no second pass and no scratch array, and writes everything the row carries between runs itself: there is no
// order between workgroups to get wrong.  The parallelism is the project's regime: S * C rows, thousands of them.
// What it costs: 256 threads on N / 2 butterflies leave half the threads idle at n = 8, and a barrier per stage.  The
// forward stages are k_spec.hip's body to the bit (tests/cpp/denoise_plan_test.cpp holds denoise_block_ref, which
// calls spec_block_ref, and the device tests hold the kernel to the model).  DESIGN 4.26.
//
// A row's input history has two slots (the run reads slot `parity`, writes the other): entries move by the run's count,
// which in place would race between threads.  tail, g, Np and acc are the row's own and are updated in place, each
// entry by the thread that read it, or behind a barrier.
#include "cmhip_device.h"

namespace cmhip {

typedef long long i64;

// an index into the padded LDS planes: one word more per 32, against the power-of-two strides of the late stages
__device__ __forceinline__ u32 dn_pad(u32 i) { return i + (i >> 5); }

template <u32 LN>
__global__ __launch_bounds__(256) void k_denoise(DenoiseArgs a)
{
    constexpr u32 N = 1u << LN, H = N / 2, NP = N + N / 32;
    __shared__ int zr[NP], zi[NP];
    __shared__ u32 lsat, lclip;

    const u32 tid = threadIdx.x;
    const u32 C = a.channels;
    const u32 row = blockIdx.x;                  // (stream, channel)
    const u32 s = row / C, c = row - s * C;
    const uint32_t *rec = a.rec + (u64)s * DENOISE_REC;
    const u32 count = rec[NREC_COUNT], back = rec[NREC_BACK], flags = rec[NREC_FLAGS];
    u32 cnt = rec[NREC_CNT];
    const DenoiseParams par = denoise_unpack(rec[NREC_PAR]);
    const bool fresh = (flags & DENOISE_FRESH) != 0u, learn = (flags & DENOISE_LEARN) != 0u;

    const int16_t *ins = a.in + (u64)s * a.in_stride + c;
    int16_t *outs = a.out + (u64)s * a.out_stride + c;
    const int16_t *hold = a.hist + ((u64)a.parity * a.streams * C + row) * N;
    int16_t *hnew = a.hist + ((u64)(a.parity ^ 1u) * a.streams * C + row) * N;
    int32_t *tail = a.tail + (u64)row * N;
    uint32_t *g = a.gain + (u64)row * (H + 1u);
    unsigned long long *np = a.np + (u64)row * (H + 1u), *acc = a.acc + (u64)row * (H + 1u);

    if (count == 0) {                            // nothing arrives: the history changes slots, everything else stays
        for (u32 j = tid; j < N - 1u; j += 256u)
            hnew[j] = hold[j];
        return;
    }
    if (tid == 0) {
        lsat = 0;
        lclip = 0;
    }
    if (fresh) {                                 // frame 0: what the row's arrays hold is older than the reset
        for (u32 j = tid; j < N; j += 256u)
            tail[j] = 0;
        for (u32 k = tid; k <= H; k += 256u)
            g[k] = DENOISE_UNITY;
    }
    __syncthreads();

    const int32_t *wr = a.table, *wi = a.table + H, *sw = a.table + N;
    const u32 nblk = spec_run_blocks(LN, back, count);
    const u32 e0 = N - 1u - back;                // the last frame of the run's block 0, as a frame of the run
    u32 nsat = 0, nclip = 0;
    const bool mono = C == 1u;                   // (uniform)

    // Outputs in front of e0: their removed part was finished by the block before this run (tail's lower half), their
    // dry sample lies in the history.
    const u32 lim = count < e0 ? count : e0;
    for (u32 q = tid; q < lim; q += 256u) {
        const int u = (int)denoise_tail_entry(LN, back, q);
        const int r = u >= 0 ? tail[u] : 0;
        const int xd = fresh ? 0 : (int)hold[q];
        outs[(u64)q * C] = denoise_out(xd, r, &nclip);
    }

#pragma unroll 1
    for (u32 i = 0; i < nblk; i++) {
        // gather, window, bit-reversed into LDS
        for (u32 t = tid; t < N; t += 256u) {
            const int rel = (int)spec_block_frame(LN, back, i, t);
            const int x = rel >= 0 ? (int)ins[(u64)(u32)rel * C] : fresh ? 0 : (int)hold[(int)(N - 1u) + rel];
            const u32 r = dn_pad(__brev(t) >> (32u - LN));
            zr[r] = x * sw[t];
            zi[r] = 0;
        }
        __syncthreads();

        // the spectrum's n stages, in place: butterfly b of stage st pairs z[q m + j] and z[q m + j + m / 2], m = 2^st
#pragma unroll 1
        for (u32 st = 1; st <= LN; st++) {
            const u32 h = 1u << (st - 1u);
            for (u32 b = tid; b < H; b += 256u) {
                const u32 j = b & (h - 1u);
                const u32 ia = dn_pad(((b >> (st - 1u)) << st) + j), ib = dn_pad(((b >> (st - 1u)) << st) + j + h);
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

        // Per bin 0 .. H: the power, the gain's step under the profile in force, the learning, and the removed spectrum
        // with its mirror image.  A thread reads bins <= H and writes bin k and bin N - k >= H: nothing another thread
        // still reads (bin H is its own mirror).
        const bool learns = learn && cnt < DENOISE_CNT_MAX;      // (uniform)
        for (u32 k = tid; k <= H; k += 256u) {
            const int re = zr[dn_pad(k)], ig = zi[dn_pad(k)];
            const u64 p = (u64)((i64)re * re + (i64)ig * ig) >> 16;
            const u32 gk = denoise_smooth(g[k], denoise_target(p, np[k], par.over, par.floor), par.rise_shift, par.fall_shift);
            g[k] = gk;
            if (learns) {
                const u64 sum = cnt ? acc[k] + p : p;
                acc[k] = sum;
                np[k] = sum / (cnt + 1u);
            }
            const int ur = denoise_removed(re, gk);
            const int ui = k == 0u || k == H ? 0 : denoise_removed(ig, gk);
            const u32 km = dn_pad((N - k) & (N - 1u));
            zr[dn_pad(k)] = ur;
            zi[dn_pad(k)] = ui;
            zr[km] = ur;
            zi[km] = k == 0u ? 0 : -ui;
        }
        if (learns)
            cnt++;
        __syncthreads();

        // bit-reversed for the decimation in time: the lower index of a pair swaps it
        for (u32 t = tid; t < N; t += 256u) {
            const u32 r = __brev(t) >> (32u - LN);
            if (t < r) {
                const u32 pa = dn_pad(t), pb = dn_pad(r);
                const int vr = zr[pa], vi = zi[pa];
                zr[pa] = zr[pb];
                zi[pa] = zi[pb];
                zr[pb] = vr;
                zi[pb] = vi;
            }
        }
        __syncthreads();

        // the inverse: the same stages with the twiddles conjugated, no halving, every output clamped and counted
#pragma unroll 1
        for (u32 st = 1; st <= LN; st++) {
            const u32 h = 1u << (st - 1u);
            for (u32 b = tid; b < H; b += 256u) {
                const u32 j = b & (h - 1u);
                const u32 ia = dn_pad(((b >> (st - 1u)) << st) + j), ib = dn_pad(((b >> (st - 1u)) << st) + j + h);
                const u32 kw = j << (LN - st);
                const i64 cr = wr[kw], cw = -(i64)wi[kw];
                const i64 br = zr[ib], bi = zi[ib];
                const i64 pr = br * cr - bi * cw;
                const i64 pi = br * cw + bi * cr;
                const i64 ar = (i64)zr[ia] * SPEC_ONE + (SPEC_ONE >> 1), ai = (i64)zi[ia] * SPEC_ONE + (SPEC_ONE >> 1);
                zr[ia] = denoise_inv_round(ar, pr, &nsat);
                zr[ib] = denoise_inv_round(ar, -pr, &nsat);
                zi[ia] = denoise_inv_round(ai, pi, &nsat);
                zi[ib] = denoise_inv_round(ai, -pi, &nsat);
            }
            __syncthreads();
        }

        // Synthesis and overlap-add.  The block's lower half completes the sums the block before left (tail's upper
        // half) and is final: it leaves with the dry samples N - 1 frames back, from frame ei on; what lies behind the
        // run's end waits in tail's lower half (the last block only: the next one ends H frames later, inside the run).
        // Its upper half is the next block's to complete.  Thread t owns tail[t] and tail[H + t] here.
        // A mono row's outputs are consecutive samples: they meet in the imaginary plane, which nothing reads any more,
        // and leave as 16-byte vectors below.  Other rows are every C-th sample of their slot and leave one by one.
        const u32 ei = e0 + i * H;
        for (u32 t = tid; t < H; t += 256u) {
            const int lo = denoise_synth(zr[dn_pad(t)], sw[t]), hi = denoise_synth(zr[dn_pad(t + H)], sw[t + H]);
            const int r = denoise_r((i64)tail[H + t] + lo);
            tail[H + t] = hi;
            const u32 q = ei + t;
            if (q < count) {
                const int rel = (int)q - (int)(N - 1u);
                const int xd = rel >= 0 ? (int)ins[(u64)(u32)rel * C] : fresh ? 0 : (int)hold[q];
                const int16_t y = denoise_out(xd, r, &nclip);
                if (mono)
                    zi[dn_pad(t)] = y;
                else
                    outs[(u64)q * C] = y;
            } else {
                tail[t] = r;
            }
        }
        __syncthreads();
        if (mono) {
            // samples [ei, qe) of the slot: whole vectors [q1, q2) by the thread of their first sample, the ragged ends
            // [ei, q1) and [q2, qe) sample by sample.  The slot's base is 16-byte aligned and ei < count.
            const u32 qe = count - ei < H ? count : ei + H;
            const u32 q1 = (ei + 7u) & ~7u, q2 = qe > q1 ? q1 + ((qe - q1) & ~7u) : q1;
            for (u32 t = tid; t < qe - ei; t += 256u) {
                const u32 q = ei + t;
                if (q < q1 || q >= q2) {
                    outs[q] = (int16_t)zi[dn_pad(t)];
                } else if ((q & 7u) == 0u) {
                    u32x4 v;
                    v.x = ((u32)zi[dn_pad(t)] & 0xffffu) | ((u32)zi[dn_pad(t + 1u)] << 16);
                    v.y = ((u32)zi[dn_pad(t + 2u)] & 0xffffu) | ((u32)zi[dn_pad(t + 3u)] << 16);
                    v.z = ((u32)zi[dn_pad(t + 4u)] & 0xffffu) | ((u32)zi[dn_pad(t + 5u)] << 16);
                    v.w = ((u32)zi[dn_pad(t + 6u)] & 0xffffu) | ((u32)zi[dn_pad(t + 7u)] << 16);
                    *(u32x4 *)(outs + q) = v;
                }
            }
            __syncthreads();
        }
    }

    // the last N - 1 inputs of (history, run): from the run where it reaches, from the history above that
    for (u32 j = tid; j < N - 1u; j += 256u) {
        const int rel = (int)spec_state_frame(LN, count, j);
        hnew[j] = rel >= 0 ? ins[(u64)(u32)rel * C] : fresh ? (int16_t)0 : hold[j + count];
    }

    if (nsat)
        atomicAdd(&lsat, nsat);
    if (nclip)
        atomicAdd(&lclip, nclip);
    __syncthreads();
    if (tid == 0) {
        if (lsat)
            atomicAdd(&a.sat[s], (unsigned long long)lsat);
        if (lclip)
            atomicAdd(&a.clips[s], (unsigned long long)lclip);
    }
}

// ---------------------------------------------------------------------------
// launcher

hipError_t launch_denoise(const DenoiseArgs &a, hipStream_t st)
{
    if (!denoise_geometry_ok(a.streams, a.channels, a.log2n, 1))
        return hipErrorInvalidValue;
    const dim3 grid(a.streams * a.channels), block(DENOISE_BLOCK);
    switch (a.log2n) {
    case 8: hipLaunchKernelGGL(k_denoise<8>, grid, block, 0, st, a); break;
    case 9: hipLaunchKernelGGL(k_denoise<9>, grid, block, 0, st, a); break;
    case 10: hipLaunchKernelGGL(k_denoise<10>, grid, block, 0, st, a); break;
    case 11: hipLaunchKernelGGL(k_denoise<11>, grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL(k_denoise<12>, grid, block, 0, st, a); break;
    }
    return hipGetLastError();
}

}  // namespace cmhip
