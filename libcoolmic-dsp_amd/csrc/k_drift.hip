// k_drift.hip -- gfx950 (MI355X, wave64) clock-drift compensation kernels: a resampler in exact integers whose ratio is
// close to 1 and moves per stream between runs, over interleaved int16 (include/coolmic_hip.h, "clock-drift
// compensation", has the arithmetic to the bit; csrc/drift_plan.h the table's form, the counts and the plan).  Output m
// of a run has t = pos + m * step in units of 2^-32 input frames, reads input frame n = t >> 32 through the table rows
// p and p + 1 of its fraction, and mixes the two sums by the fraction's next 15 bits:
//     a0 = sum_k H[p][k] x[n-k]   a1 = sum_k H[p+1][k] x[n-k]   y = saturate((a0 (32768 - mu) + a1 mu + 2^28) >> 29)
//
//   k_drift_fast<C>  mono, stereo: a lane owns one dword of output (two mono frames / one stereo frame)
//   k_drift_any      any channel count (3..16 in practice): a lane owns one output sample; no speed goal
//
// k_src.hip's decomposition: one workgroup of 256 threads per stream and tile of DriftArgs::tile_out output frames.  The
// stream's record of the run (F, K, delta, pos) comes from the host with the run; the device keeps no position.
//
// LDS (dynamic, plan_drift sizes it): the table of P + 1 rows, when the plan puts it there; then the tile's input
// frames j_lo .. j_hi as channel planes, TWICE: copy A as it is and copy B delayed by one sample, so that the pair
// (x[n-k-1], x[n-k]) of an even k is an aligned dword of A when its first index is even and of B when it is odd.
// j_lo = n_first - (T-1) may be negative in ANY tile: negative frames come from the stream's history, which holds
// exactly the T-1 frames a tile can ask for.  The phase differs from lane to lane, so the taps are read per lane.
#include "cmhip_device.h"

namespace cmhip {

__device__ __forceinline__ int drift_dot2(u32 x, u32 k, int acc)
{
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(v2s, x), __builtin_bit_cast(v2s, k), acc, false);
}

__device__ __forceinline__ int drift_round(int a0, int a1, u32 mu)
{
    const long long num = (long long)a0 * (int)(32768u - mu) + (long long)a1 * (int)mu;
    const long long y = (num + (1ll << 28)) >> 29;
    return (int)min(max(y, -32768ll), 32767ll);
}

// The stream's new history: the last T-1 frames of (old history, this run's frames), into the slot the next run reads.
// Done by the workgroup of the stream's last tile (its first when the run gives the stream no output); a stream
// without a frame copies its slot over.
__device__ __forceinline__ void drift_history(const DriftArgs &a, u32 s, u32 F, u32 C, const int16_t *ins)
{
    const u32 HT = a.T - 1u;
    const int16_t *hrd = a.hist + ((u64)a.parity * a.streams + s) * C * HT;
    int16_t *hwr = a.hist + ((u64)(a.parity ^ 1u) * a.streams + s) * C * HT;
    for (u32 idx = threadIdx.x; idx < C * HT; idx += blockDim.x) {
        const u32 c = idx / HT, i = idx - c * HT;
        int16_t val;
        if (F + i < HT)                              // frame F - (T-1) + i lies before this run
            val = hrd[c * HT + i + F];
        else
            val = ins[(u64)(F - HT + i) * C + c];
        hwr[c * HT + i] = val;
    }
}

// one tile: staging, then the lanes' outputs.  CT: the channel count when it is 1 or 2, 0: a.channels.  TLDS: the
// table sits in LDS.
template <int CT, bool TLDS>
__device__ __forceinline__ void drift_tile(const DriftArgs &a, u32x4 *lds, u32 s, u32 q0, u32 K, u32 F, u64 pos, u64 step,
                                           const int16_t *ins)
{
    const u32 C = CT ? (u32)CT : a.channels;
    const u32 T = a.T, phi = a.phi, row = a.row, rw = drift_row_words(T);
    const u32 tid = threadIdx.x;
    const u32 nq = min(a.tile_out, K - q0);          // the tile's output frames
    const u64 tb = pos + (u64)q0 * step;             // t of the tile's first output
    const u32 jf = (u32)(tb >> 32);                  // run frame of the tile's first output
    const u32 jh = (u32)((tb + (u64)(nq - 1u) * step) >> 32);    // ... of its last: the last frame staged (< F)
    const int j_lo = (int)jf - (int)(T - 1u);        // the first frame staged (plane index 0), >= -(T-1)
    const u32 staged = (u32)((int)jh - j_lo + 1);
    const u64 tfrac = (u32)tb;                       // t counted from frame jf
    int16_t *pl = reinterpret_cast<int16_t *>(lds) + (TLDS ? a.table_words * 2u : 0u);

    if constexpr (TLDS) {
        const u32x4 *src = reinterpret_cast<const u32x4 *>(a.table);
        for (u32 i = tid; i < a.table_words / 4u; i += DRIFT_BLOCK)
            lds[i] = src[i];
    }
    // frames before the run: the history
    const u32 npre = j_lo < 0 ? min(staged, (u32)-j_lo) : 0u;
    if (npre) {
        const u32 HT = T - 1u;
        const int16_t *hrd = a.hist + ((u64)a.parity * a.streams + s) * C * HT;
        for (u32 idx = tid; idx < npre * C; idx += DRIFT_BLOCK) {
            const u32 i = idx / C, c = idx - i * C;
            const int16_t val = hrd[c * HT + (u32)((int)HT + j_lo + (int)i)];
            pl[c * row + i] = val;
            pl[(C + c) * row + i + 1u] = val;
        }
    }
    // the run's frames jb .. jh: whole 16-byte vectors of the slot, the ragged last one sample by sample
    if (staged > npre) {
        const u32 jb = j_lo < 0 ? 0u : (u32)j_lo;
        const u32 nsamp = F * C, nfull = nsamp >> 3, ntail = nsamp & 7u;
        const u32 v_hi = ((jh + 1u) * C + 7u) >> 3;
        for (u32 v = ((jb * C) >> 3) + tid; v < v_hi; v += DRIFT_BLOCK) {
            u32 x[4];
            load_vec(x, ins, v, v < nfull, v == nfull && ntail != 0, ntail);
#pragma unroll
            for (u32 i = 0; i < 8; i++) {
                const u32 e = v * 8u + i;
                const u32 j = e / C, c = e - j * C;
                if (j >= jb && j <= jh) {
                    const int16_t val = (int16_t)(x[i >> 1] >> (16u * (i & 1u)));
                    const u32 at = (u32)((int)j - j_lo);
                    pl[c * row + at] = val;
                    pl[(C + c) * row + at + 1u] = val;
                }
            }
        }
    }
    __syncthreads();

    // output frame q of the tile, channels c .. c + NC - 1: t = tfrac + q * step, n = jf + (t >> 32).  x[n] is plane
    // index a0 = n - j_lo = (t >> 32) + T - 1; tap pair (k, k+1) is the dword that holds plane indices a0-k-1 and a0-k:
    // dword (a0 >> 1) - k/2 of copy A for an odd a0, of copy B (one sample later) for an even one.
    const u32 *tab = TLDS ? reinterpret_cast<const u32 *>(lds) : a.table;
    auto frame = [&](u32 q, u32 c, auto nc, int (&y)[2]) {
        constexpr u32 NC = decltype(nc)::value;
        const u64 t = tfrac + (u64)q * step;
        const u32 a0 = (u32)(t >> 32) + T - 1u, f = (u32)t;
        const u32 p = f >> (32u - phi), mu = (f >> (17u - phi)) & 32767u;
        const u32 *xp = reinterpret_cast<const u32 *>(pl + (((a0 & 1u) ? 0u : C) + c) * row) + (a0 >> 1);
        const u32 *kp = tab + p * rw;                // rows p and p + 1, adjacent
        int acc0[2] = {0, 0}, acc1[2] = {0, 0};
        for (u32 kk = 0; kk < T / 2u; kk++) {
            const u32 k0 = kp[kk], k1 = kp[rw + kk];
#pragma unroll
            for (u32 ch = 0; ch < NC; ch++) {
                const u32 x = *(xp + ch * (row / 2u) - kk);
                acc0[ch] = drift_dot2(x, k0, acc0[ch]);
                acc1[ch] = drift_dot2(x, k1, acc1[ch]);
            }
        }
#pragma unroll
        for (u32 ch = 0; ch < NC; ch++)
            y[ch] = drift_round(acc0[ch], acc1[ch], mu);
    };

    int16_t *outs = a.out + (u64)s * a.out_stride;
    if constexpr (CT == 2) {
        u32 *dst = reinterpret_cast<u32 *>(outs) + q0;
        for (u32 w = tid; w < nq; w += DRIFT_BLOCK) {
            int y[2];
            frame(w, 0u, std::integral_constant<u32, 2>{}, y);
            dst[w] = ((u32)y[0] & 0xffffu) | ((u32)y[1] << 16);
        }
    } else if constexpr (CT == 1) {
        u32 *dst = reinterpret_cast<u32 *>(outs) + (q0 >> 1);        // (tile_out is even)
        for (u32 w = tid; 2u * w < nq; w += DRIFT_BLOCK) {
            int y0[2], y1[2];
            frame(2u * w, 0u, std::integral_constant<u32, 1>{}, y0);
            if (2u * w + 1u < nq) {
                frame(2u * w + 1u, 0u, std::integral_constant<u32, 1>{}, y1);
                dst[w] = ((u32)y0[0] & 0xffffu) | ((u32)y1[0] << 16);
            } else {
                outs[q0 + 2u * w] = (int16_t)y0[0];                  // outputs past the count are not written
            }
        }
    } else {
        for (u32 e = tid; e < nq * C; e += DRIFT_BLOCK) {
            const u32 q = e / C, c = e - q * C;
            int y[2];
            frame(q, c, std::integral_constant<u32, 1>{}, y);
            outs[(u64)(q0 + q) * C + c] = (int16_t)y[0];
        }
    }
}

template <int CT>
__device__ __forceinline__ void drift_body(const DriftArgs &a)
{
    extern __shared__ u32x4 drift_lds[];
    const u32 C = CT ? (u32)CT : a.channels;
    const u32 s = blockIdx.x / a.chunks;             // stream
    const u32 k = blockIdx.x - s * a.chunks;         // tile inside the stream
    const u32 *rec = a.rec + (u64)s * DRIFT_REC;
    const u32 F = rec[0], K = rec[1];
    const u64 step = DRIFT_ONE + (u64)(long long)(int)rec[2];
    const u64 pos = (u64)rec[3] | (u64)rec[4] << 32;
    const int16_t *ins = a.in + (u64)s * a.in_stride;
    const u32 q0 = k * a.tile_out;
    if (q0 < K) {                                    // (uniform)
        if (a.table_lds)
            drift_tile<CT, true>(a, drift_lds, s, q0, K, F, pos, step, ins);
        else
            drift_tile<CT, false>(a, drift_lds, s, q0, K, F, pos, step, ins);
    }
    if (k == (K ? (K - 1u) / a.tile_out : 0u))
        drift_history(a, s, F, C, ins);
}

template <int C>
__global__ __launch_bounds__(DRIFT_BLOCK) void k_drift_fast(DriftArgs a)
{
    drift_body<C>(a);
}

__global__ __launch_bounds__(DRIFT_BLOCK) void k_drift_any(DriftArgs a)
{
    drift_body<0>(a);
}

// ---------------------------------------------------------------------------
// launcher

hipError_t launch_drift(const DriftArgs &a, uint32_t out_frames, hipStream_t st)
{
    const DriftPlan p = plan_drift(a.streams, a.channels, a.phi, a.T, out_frames);
    if (p.grid == 0)
        return p.err ? hipErrorInvalidValue : hipSuccess;
    DriftArgs b = a;
    b.chunks = p.chunks;
    b.tile_out = p.tile_out;
    b.row = p.row;
    b.table_lds = p.table_lds;
    b.table_words = p.table_words;
    if (!p.fast)
        hipLaunchKernelGGL(k_drift_any, dim3(p.grid), dim3(p.block), p.lds_bytes, st, b);
    else if (a.channels == 1)
        hipLaunchKernelGGL(k_drift_fast<1>, dim3(p.grid), dim3(p.block), p.lds_bytes, st, b);
    else
        hipLaunchKernelGGL(k_drift_fast<2>, dim3(p.grid), dim3(p.block), p.lds_bytes, st, b);
    return hipGetLastError();
}

}  // namespace cmhip
