// denoise_plan.h -- the window, the gain law, the smoothing, the learning, a plain reference of one block (the
// spectrum's forward transform, the removed spectrum, the inverse transform and the synthesis), the host's mirror and
// the run record of the noise suppressor (include/coolmic_hip.h, "noise suppressor").  Plain C++17, no HIP:
// tests/cpp/denoise_plan_test.cpp compiles it with g++ alone; the kernel (k_denoise.hip) uses the same functions.
//
//   S streams of C interleaved int16 channels; every (stream, channel) is a row.  N = 2^n frames per block, n = 8..12,
//   hop H = N / 2.  Block j of a row covers its frames [j H, j H + N) and is computed in the run in which its last
//   frame arrives: the bookkeeping is csrc/spec_plan.h's (spec_run_blocks, spec_next_back, spec_block_frame,
//   spec_state_frame), with `back` kept by the host and handed down with every run.
//
// What a row carries from run to run:
//   its last N - 1 inputs (spec_plan.h's state: entry j is the sample N - 1 - j frames before the next run's first);
//   tail[N], int32, the overlap-add of the span of the last block completed, J: tail[u], u < H, is the finished
//     r[J H + u]; tail[H + u] is c[H + u] of block J alone, which block J + 1 completes.  The output is D = N - 1 frames
//     behind the input and block J ends at frame J H + N - 1 = J H + D: the frame that completes block J is the one
//     whose output needs r[J H], so of the H values block J finishes up to H - 1 are still to be written when the run
//     ends -- the lower half -- and the upper half is what the specification calls the not-yet-completed overlap sums.
//     Before block 0 the tail is zero;
//   g[H + 1], Np[H + 1], acc[H + 1].
// The host keeps per stream: back, whether the stream is at frame 0 (fresh), the learn flag, cnt and the parameters;
// they travel with the run's counts (DENOISE_REC dwords per stream).  The device keeps no position.
#ifndef CMHIP_DENOISE_PLAN_H
#define CMHIP_DENOISE_PLAN_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "dyn_plan.h"
#include "spec_plan.h"

#if defined(__HIPCC__)
#define CMHIP_DN_HD __host__ __device__
#else
#define CMHIP_DN_HD
#endif

namespace cmhip {

constexpr uint32_t DENOISE_MAX_CH = 16;
constexpr uint32_t DENOISE_UNITY = 32768;            // a gain of one
constexpr uint64_t DENOISE_NP_MAX = 1ull << 52;      // the largest profile value
constexpr uint32_t DENOISE_CNT_MAX = 65536;          // learning blocks that count
constexpr uint32_t DENOISE_SHIFT_MAX = 8;
constexpr uint32_t DENOISE_BLOCK = 256;              // threads of k_denoise: a workgroup per row
constexpr uint32_t DENOISE_REC = 8;                  // dwords of a stream's record
constexpr uint32_t NREC_COUNT = 0, NREC_BACK = 1, NREC_FLAGS = 2, NREC_CNT = 3, NREC_PAR = 4;
constexpr uint32_t DENOISE_FRESH = 1u, DENOISE_LEARN = 2u;

// cmhip_denoise_params_t, field by field (cmhip_denoise.hip holds the two layouts against each other)
struct DenoiseParams {
    uint16_t floor;
    uint8_t  over, rise_shift, fall_shift;
};

CMHIP_DN_HD constexpr bool denoise_log2_ok(uint32_t n) { return n >= SPEC_MIN_LOG2 && n <= SPEC_MAX_LOG2; }
CMHIP_DN_HD constexpr bool denoise_params_ok(const DenoiseParams &p)
{
    return p.floor <= DENOISE_UNITY && p.rise_shift <= DENOISE_SHIFT_MAX && p.fall_shift <= DENOISE_SHIFT_MAX;
}
CMHIP_DN_HD constexpr uint32_t denoise_pack(const DenoiseParams &p)
{
    return (uint32_t)p.floor | ((uint32_t)p.over << 16) | ((uint32_t)p.rise_shift << 24) | ((uint32_t)p.fall_shift << 28);
}
CMHIP_DN_HD inline DenoiseParams denoise_unpack(uint32_t w)
{
    DenoiseParams p;
    p.floor = (uint16_t)(w & 0xffffu);
    p.over = (uint8_t)((w >> 16) & 0xffu);
    p.rise_shift = (uint8_t)((w >> 24) & 0xfu);
    p.fall_shift = (uint8_t)((w >> 28) & 0xfu);
    return p;
}
constexpr bool denoise_geometry_ok(uint64_t streams, uint64_t channels, uint64_t n, uint64_t max_frames)
{
    return streams != 0 && channels >= 1 && channels <= DENOISE_MAX_CH && streams * channels < (1ull << 31) &&
           n >= SPEC_MIN_LOG2 && n <= SPEC_MAX_LOG2 && max_frames != 0 && max_frames * channels < (1ull << 31);
}

// sw[i] = min(32767, rint(32768 sin(pi i / N))), the upper half mirrored: sw[N - i] = sw[i], sw[0] = 0
inline void denoise_window(uint32_t n, int16_t *sw)
{
    const uint32_t N = 1u << n;
    for (uint32_t i = 0; i <= N / 2; i++) {
        const double v = rint(32768.0 * sin(M_PI * (double)i / (double)N));
        sw[i] = (int16_t)(v > 32767.0 ? 32767.0 : v);
    }
    for (uint32_t i = N / 2 + 1; i < N; i++)
        sw[i] = sw[N - i];
}

// bits of v: 0 for 0
CMHIP_DN_HD inline uint32_t denoise_bitlength(uint64_t v)
{
    return v ? 64u - (uint32_t)__builtin_clzll((unsigned long long)v) : 0u;
}

// The target gain of a bin of power p under the profile value np (at most 2^52).  np * over < 2^60.  Behind the shift
// p >> sh is below 2^34 and t >> sh at most that, so the difference shifted up by 30 fits uint64; the quotient is at
// most 2^30 and its root at most 32768.
CMHIP_DN_HD inline uint32_t denoise_target(uint64_t p, uint64_t np, uint32_t over, uint32_t floor)
{
    const uint64_t t = (np * over) >> 4;
    if (p <= t)
        return floor;
    const uint32_t bl = denoise_bitlength(p), sh = bl > 34u ? bl - 34u : 0u;
    const uint64_t ps = p >> sh, ts = t >> sh;
    const uint32_t r = dyn_isqrt((uint32_t)(((ps - ts) << 30) / ps));
    return r > floor ? r : floor;
}

// one step of a bin's gain towards its target: no dead band, a shift of 0 is instant
CMHIP_DN_HD inline uint32_t denoise_smooth(uint32_t g, uint32_t target, uint32_t rise_shift, uint32_t fall_shift)
{
    if (target > g) {
        const uint32_t d = (target - g) >> rise_shift;
        return g + (d ? d : 1u);
    }
    if (target < g) {
        const uint32_t d = (g - target) >> fall_shift;
        return g - (d ? d : 1u);
    }
    return g;
}

// a component of the removed spectrum: (X (32768 - g) + 2^16) >> 17, arithmetic shift; |X| <= 2^30
CMHIP_DN_HD inline int32_t denoise_removed(int32_t X, uint32_t g)
{
    return (int32_t)(((int64_t)X * (int64_t)(DENOISE_UNITY - g) + 65536) >> 17);
}

// one output of an inverse butterfly: (a 2^30 +- P + 2^29) >> 30 clamped to int32; *sat counts the clamps.
// |a| <= 2^31 and |P| <= 2^61.5, so the int64 sum is exact.
CMHIP_DN_HD inline int32_t denoise_sat32(int64_t v, uint32_t *sat)
{
    if (v > 2147483647ll) {
        ++*sat;
        return 2147483647;
    }
    if (v < -2147483648ll) {
        ++*sat;
        return (int32_t)(-2147483648ll);
    }
    return (int32_t)v;
}
CMHIP_DN_HD inline int32_t denoise_inv_round(int64_t a30, int64_t p, uint32_t *sat)
{
    return denoise_sat32((a30 + p) >> 30, sat);
}

// the synthesis: c = (t sw + 2^14) >> 15, an int64 product, an int32 result
CMHIP_DN_HD inline int32_t denoise_synth(int32_t t, int32_t sw) { return (int32_t)(((int64_t)t * sw + 16384) >> 15); }
// r from the sum of the one or two c that cover a frame
CMHIP_DN_HD inline int32_t denoise_r(int64_t sum) { return (int32_t)((sum + 4096) >> 13); }
// y = clamp16(x - r); *clip counts the clamps
CMHIP_DN_HD inline int16_t denoise_out(int32_t x, int32_t r, uint32_t *clip)
{
    const int32_t v = x - r;
    const int32_t y = v < -32768 ? -32768 : v > 32767 ? 32767 : v;
    *clip += y != v ? 1u : 0u;
    return (int16_t)y;
}

// What a run's output frame q (q below e0 = N - 1 - back, the last frame of the first block the run may complete)
// reads of the tail the run found: entry q + back + H + 1 - N, or nothing (r = 0) where that is negative -- frames
// before frame 0.
CMHIP_DN_HD constexpr int64_t denoise_tail_entry(uint32_t n, uint32_t back, uint32_t q)
{
    return (int64_t)q + (int64_t)back + (int64_t)(1ull << (n - 1)) + 1 - (int64_t)(1ull << n);
}

// ---------------------------------------------------------------------------
// The reference of one block, stage by stage as the specification states it.  x[N]: the block's samples; g, np, acc:
// the row's H + 1 gains, profile values and learning sums, updated; *cnt the stream's learning count as this row sees
// it.  c[N]: the synthesised block; p[H + 1]: its powers.  zr, zi: N words of work space each.  Returns the clamps of
// the inverse transform.
inline uint32_t denoise_block_ref(uint32_t n, const int16_t *x, const int16_t *sw, const int32_t *wr, const int32_t *wi,
                                  const DenoiseParams &par, bool learn, uint32_t *cnt, uint32_t *g, uint64_t *np,
                                  uint64_t *acc, int32_t *zr, int32_t *zi, uint64_t *p, int32_t *c)
{
    const uint32_t N = 1u << n, H = N / 2;
    spec_block_ref(n, x, sw, wr, wi, zr, zi, p);     // the spectrum's transform to the bit, under this stage's window
    for (uint32_t k = 0; k <= H; k++)
        g[k] = denoise_smooth(g[k], denoise_target(p[k], np[k], par.over, par.floor), par.rise_shift, par.fall_shift);
    if (learn && *cnt < DENOISE_CNT_MAX) {
        for (uint32_t k = 0; k <= H; k++) {
            acc[k] = *cnt ? acc[k] + p[k] : p[k];    // (the first block of a learning phase clears the sums)
            np[k] = acc[k] / (*cnt + 1u);
        }
        ++*cnt;
    }
    // the removed spectrum, conjugate symmetric, bit-reversed for the decimation in time
    std::vector<int32_t> ur(N), ui(N);
    for (uint32_t k = 0; k <= H; k++) {
        const int32_t re = denoise_removed(zr[k], g[k]);
        const int32_t im = k == 0 || k == H ? 0 : denoise_removed(zi[k], g[k]);
        ur[k] = re;
        ui[k] = im;
        ur[(N - k) & (N - 1u)] = re;
        ui[(N - k) & (N - 1u)] = k == 0 ? 0 : -im;
    }
    for (uint32_t i = 0; i < N; i++) {
        uint32_t r = 0;
        for (uint32_t b = 0; b < n; b++)
            r |= ((i >> b) & 1u) << (n - 1 - b);
        zr[r] = ur[i];
        zi[r] = ui[i];
    }
    uint32_t sat = 0;
    for (uint32_t s = 1; s <= n; s++) {
        const uint32_t m = 1u << s, h = m / 2;
        for (uint32_t q = 0; q < N; q += m)
            for (uint32_t j = 0; j < h; j++) {
                const uint32_t ia = q + j, ib = ia + h, k = j * (N / m);
                const int64_t cr = wr[k], cw = -(int64_t)wi[k];      // the twiddle conjugated
                const int64_t pr = (int64_t)zr[ib] * cr - (int64_t)zi[ib] * cw;
                const int64_t pi = (int64_t)zr[ib] * cw + (int64_t)zi[ib] * cr;
                const int64_t ar = (int64_t)zr[ia] * SPEC_ONE + (SPEC_ONE >> 1), ai = (int64_t)zi[ia] * SPEC_ONE + (SPEC_ONE >> 1);
                zr[ia] = denoise_inv_round(ar, pr, &sat);
                zr[ib] = denoise_inv_round(ar, -pr, &sat);
                zi[ia] = denoise_inv_round(ai, pi, &sat);
                zi[ib] = denoise_inv_round(ai, -pi, &sat);
            }
    }
    for (uint32_t i = 0; i < N; i++)
        c[i] = denoise_synth(zr[i], sw[i]);
    return sat;
}

// ---------------------------------------------------------------------------
// the streams as the host knows them
struct DenoiseMirror {
    uint32_t n = 0;
    std::vector<uint32_t> back, cnt;
    std::vector<uint8_t> fresh, learn;
    std::vector<DenoiseParams> par;

    void init(size_t streams, uint32_t fft_log2, const DenoiseParams &p)      // may throw std::bad_alloc
    {
        n = fft_log2;
        back.assign(streams, 0);
        cnt.assign(streams, 0);
        fresh.assign(streams, 1);
        learn.assign(streams, 0);
        par.assign(streams, p);
    }
    void record(size_t s, uint32_t count, uint32_t *rec) const
    {
        rec[NREC_COUNT] = count;
        rec[NREC_BACK] = back[s];
        rec[NREC_FLAGS] = (fresh[s] ? DENOISE_FRESH : 0u) | (learn[s] ? DENOISE_LEARN : 0u);
        rec[NREC_CNT] = cnt[s];
        rec[NREC_PAR] = denoise_pack(par[s]);
        rec[5] = rec[6] = rec[7] = 0;
    }
    // behind a launched run of `count` frames for stream s
    void advance(size_t s, uint32_t count)
    {
        if (count == 0)
            return;
        const uint32_t nb = spec_run_blocks(n, back[s], count);
        if (learn[s]) {
            const uint64_t c = (uint64_t)cnt[s] + nb;
            cnt[s] = c > DENOISE_CNT_MAX ? DENOISE_CNT_MAX : (uint32_t)c;
        }
        back[s] = spec_next_back(n, back[s], count);
        fresh[s] = 0;
    }
    void set_learn(size_t s, bool on)
    {
        if (on && !learn[s])
            cnt[s] = 0;                              // the first learning block starts the sums anew
        learn[s] = on ? 1 : 0;
    }
    void reset(size_t s)
    {
        back[s] = 0;
        fresh[s] = 1;
        learn[s] = 0;
    }
};

}  // namespace cmhip
#endif
