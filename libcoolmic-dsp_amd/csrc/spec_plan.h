// spec_plan.h -- the tables, the band design, the position bookkeeping and a plain reference of the spectrum meter's
// transform (include/coolmic_hip.h, "spectrum").  Plain C++17, no HIP: tests/cpp/spec_plan_test.cpp compiles it with g++
// alone; the kernel (k_spec.hip) uses the same bookkeeping functions, cmhip_spec.hip the tables and the design.
//
//   N = 2^n frames per block, n = 8..12, hop H = N / 2.  Block j of a stream covers its frames [j H, j H + N) and is
//   computed in the run in which its last frame arrives.
//
// Bookkeeping.  Between two runs a stream keeps, per selected channel, its last N - 1 transformed samples (entry j of
// the state is the sample N - 1 - j frames before the next run's first) and one number, `back`: how many frames of the
// next block to complete lie before the next run's first frame, 0 <= back <= N - 1.  A run of f frames then completes
//     nb = back + f >= N ? (back + f - N) / H + 1 : 0
// blocks, block i of the run starting back - i H frames BEFORE the run's first frame (negative: inside the run), and
// leaves back' = back + f - nb H.  Nothing here knows the stream's absolute position: two cuts of a stream that reach
// the same frame have the same back, state and blocks behind them.
#ifndef CMHIP_SPEC_PLAN_H
#define CMHIP_SPEC_PLAN_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CMHIP_SPEC_HD __host__ __device__
#else
#define CMHIP_SPEC_HD
#endif

namespace cmhip {

constexpr uint32_t SPEC_MIN_LOG2 = 8, SPEC_MAX_LOG2 = 12, SPEC_DEFAULT_LOG2 = 10;
constexpr uint32_t SPEC_MAX_CH = 8;                  // selected channels per stream
constexpr uint32_t SPEC_MAX_BANDS = 32;
constexpr int32_t  SPEC_ONE = 1 << 30;               // a twiddle of 1.0
constexpr double   SPEC_DB_REF = 1649267441664.0;    // 1.5 * 2^40: one block of a full-scale sine, all three bins

// ---------------------------------------------------------------------------
// bookkeeping

// blocks a run of f frames completes for a stream whose next block began `back` frames ago
CMHIP_SPEC_HD constexpr uint32_t spec_run_blocks(uint32_t n, uint32_t back, uint32_t f)
{
    const uint64_t N = 1ull << n, reach = (uint64_t)back + f;
    return reach >= N ? (uint32_t)((reach - N) / (N / 2) + 1) : 0u;
}
// ... and the back it leaves
CMHIP_SPEC_HD constexpr uint32_t spec_next_back(uint32_t n, uint32_t back, uint32_t f)
{
    const uint64_t N = 1ull << n;
    return (uint32_t)((uint64_t)back + f - (uint64_t)spec_run_blocks(n, back, f) * (N / 2));
}
// Sample t of the run's block i, as a frame of the run; negative: entry N - 1 + (the value) of the state.  For a block
// the run completes the value is below f, and never below -(N - 1): back <= N - 1.
CMHIP_SPEC_HD constexpr int64_t spec_block_frame(uint32_t n, uint32_t back, uint32_t i, uint32_t t)
{
    return (int64_t)t - (int64_t)back + (int64_t)i * (int64_t)(1ull << (n - 1));
}
// Entry j (0 .. N - 2) of the state a run of f frames leaves, as a frame of the run; negative: entry j + f of the state
// the run found (which is below N - 1 exactly then).
CMHIP_SPEC_HD constexpr int64_t spec_state_frame(uint32_t n, uint32_t f, uint32_t j)
{
    return (int64_t)f - (int64_t)((1ull << n) - 1) + (int64_t)j;
}

// ---------------------------------------------------------------------------
// tables

// win[i] = min(32767, rint(32768 * 0.5 * (1 - cos(2 pi i / N)))): the periodic Hann window.  The upper half mirrors
// the lower one (win[N - i] = win[i]), so the table is symmetric whatever the libm.
inline void spec_window(uint32_t n, int16_t *win)
{
    const uint32_t N = 1u << n;
    for (uint32_t i = 0; i <= N / 2; i++) {
        const double v = rint(32768.0 * 0.5 * (1.0 - cos(2.0 * M_PI * (double)i / (double)N)));
        win[i] = (int16_t)(v > 32767.0 ? 32767.0 : v);
    }
    for (uint32_t i = N / 2 + 1; i < N; i++)
        win[i] = win[N - i];
}

// Wr[k] = llround(2^30 cos(2 pi k / N)), Wi[k] = llround(-2^30 sin(2 pi k / N)), k < N / 2.  One octant is computed
// (c[k], s[k] for k <= N / 8, with s[N / 8] = c[N / 8]) and mirrored:
//     k <= N / 8           ( c[k],         -s[k])
//     N / 8 < k <= N / 4   ( s[N / 4 - k], -c[N / 4 - k])
//     N / 4 < k < N / 2    ( Wi[k - N / 4], -Wr[k - N / 4])        (a quarter turn: W[k] = -i W[k - N / 4])
// so k = 0 is exactly (2^30, 0), k = N / 4 exactly (0, -2^30), and Wr[N / 4 - k] = -Wi[k] holds to the bit.
inline void spec_twiddles(uint32_t n, int32_t *wr, int32_t *wi)
{
    const uint32_t N = 1u << n, Q = N / 4, O = N / 8;
    for (uint32_t k = 0; k <= O; k++) {
        const double th = 2.0 * M_PI * (double)k / (double)N;
        const int32_t c = (int32_t)llround((double)SPEC_ONE * cos(th));
        const int32_t s = k == O ? c : (int32_t)llround((double)SPEC_ONE * sin(th));
        wr[k] = c;
        wi[k] = -s;
        wr[Q - k] = s;
        wi[Q - k] = -c;
    }
    for (uint32_t k = Q + 1; k < N / 2; k++) {
        wr[k] = wi[k - Q];
        wi[k] = -wr[k - Q];
    }
}

// the default band table: the bin octaves 1, 2, 4, ..., N / 2, N / 2 + 1 -- n bands, DC left out
inline uint32_t spec_default_bands(uint32_t n, uint16_t *edges)
{
    for (uint32_t b = 0; b < n; b++)
        edges[b] = (uint16_t)(1u << b);
    edges[n] = (uint16_t)((1u << (n - 1)) + 1u);
    return n;
}

// 0 <= e[0] < e[1] < ... < e[nb] <= N / 2 + 1, nb in 1..32
inline bool spec_bands_ok(uint32_t n, uint32_t nb, const uint16_t *edges)
{
    if (nb == 0 || nb > SPEC_MAX_BANDS)
        return false;
    for (uint32_t b = 0; b < nb; b++)
        if (edges[b] >= edges[b + 1])
            return false;
    return edges[nb] <= (1u << (n - 1)) + 1u;
}

// Fractional-octave bands around 1 kHz: f(i) = 1000 * 2^((2 i - 1) / (2 per_octave)) for every integer i, the bin edge
// ceil(f(i) N / rate) clamped to 1 .. N / 2 + 1, the table the strictly ascending list of the distinct values (all but
// finitely many i give 1 or N / 2 + 1; +-SPEC_DESIGN_SPAN covers 2^-100 .. 2^100 kHz at per_octave 1 and a third of that
// at 3, far past every rate an uint32 holds).  The band count, or -1: more than 32 bands or an argument out of range.
constexpr int SPEC_DESIGN_SPAN = 100;
inline int spec_design_bands(uint32_t rate, uint32_t n, uint32_t per_octave, uint16_t *edges)
{
    if (rate == 0 || n < SPEC_MIN_LOG2 || n > SPEC_MAX_LOG2 || per_octave < 1 || per_octave > 3)
        return -1;
    const uint32_t N = 1u << n, top = N / 2 + 1;
    uint16_t tmp[SPEC_MAX_BANDS + 1];
    uint32_t ne = 0, last = 0;
    for (int i = -SPEC_DESIGN_SPAN; i <= SPEC_DESIGN_SPAN; i++) {
        const double f = 1000.0 * pow(2.0, (double)(2 * i - 1) / (2.0 * (double)per_octave));
        const double e = ceil(f * (double)N / (double)rate);
        const uint32_t edge = e < 1.0 ? 1u : e > (double)top ? top : (uint32_t)e;
        if (edge == last)
            continue;
        if (ne == SPEC_MAX_BANDS + 1)
            return -1;
        tmp[ne++] = (uint16_t)edge;
        last = edge;
    }
    for (uint32_t k = 0; k < ne; k++)
        edges[k] = tmp[k];
    return (int)ne - 1;
}

// the host finish: 10 log10(power / (blocks * 1.5 * 2^40)), -inf for power 0, 0.0 for blocks 0
inline double spec_db(uint64_t power, uint64_t blocks)
{
    if (blocks == 0)
        return 0.0;
    return 10.0 * log10((double)power / ((double)blocks * SPEC_DB_REF));
}

// ---------------------------------------------------------------------------
// the transform

// one butterfly output: (a 2^30 +- P + 2^30) >> 31, an arithmetic shift of the exact 64-bit sum
CMHIP_SPEC_HD constexpr int32_t spec_round(int64_t a30, int64_t p)
{
    return (int32_t)((a30 + p) >> 31);
}

// The reference: x[N] transformed samples -> p[N / 2 + 1] bin powers, stage by stage as the specification states it.
// zr, zi: N words of work space each.
inline void spec_block_ref(uint32_t n, const int16_t *x, const int16_t *win, const int32_t *wr, const int32_t *wi,
                           int32_t *zr, int32_t *zi, uint64_t *p)
{
    const uint32_t N = 1u << n;
    for (uint32_t i = 0; i < N; i++) {
        uint32_t r = 0;
        for (uint32_t b = 0; b < n; b++)
            r |= ((i >> b) & 1u) << (n - 1 - b);
        zr[r] = (int32_t)x[i] * (int32_t)win[i];
        zi[r] = 0;
    }
    for (uint32_t s = 1; s <= n; s++) {
        const uint32_t m = 1u << s, h = m / 2;
        for (uint32_t g = 0; g < N; g += m)
            for (uint32_t j = 0; j < h; j++) {
                const uint32_t ia = g + j, ib = ia + h, k = j * (N / m);
                const int64_t pr = (int64_t)zr[ib] * wr[k] - (int64_t)zi[ib] * wi[k];
                const int64_t pi = (int64_t)zr[ib] * wi[k] + (int64_t)zi[ib] * wr[k];
                const int64_t ar = (int64_t)zr[ia] * SPEC_ONE + SPEC_ONE, ai = (int64_t)zi[ia] * SPEC_ONE + SPEC_ONE;
                zr[ia] = spec_round(ar, pr);
                zr[ib] = spec_round(ar, -pr);
                zi[ia] = spec_round(ai, pi);
                zi[ib] = spec_round(ai, -pi);
            }
    }
    for (uint32_t k = 0; k <= N / 2; k++)
        p[k] = (uint64_t)((int64_t)zr[k] * zr[k] + (int64_t)zi[k] * zi[k]) >> 16;
}

}  // namespace cmhip
#endif
