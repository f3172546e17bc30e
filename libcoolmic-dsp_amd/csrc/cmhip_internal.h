// cmhip_internal.h -- device-side records and launcher prototypes shared by the gfx950 kernels (k_block.hip, k_eq.hip,
// k_misc.hip, k_tpeak.hip, k_corr.hip, k_loud.hip, k_src.hip, k_mix.hip, k_mixramp.hip, k_bus.hip, k_busramp.hip, k_lim.hip, k_limtp.hip, k_limrel.hip, k_dyn.hip, k_split.hip, k_delay.hip, k_agc.hip, k_automix.hip, k_failover.hip, k_drift.hip, k_iir.hip, k_iirramp.hip, k_spec.hip, k_watch.hip, k_denoise.hip) and the host code that
// launches them (cmhip_engine.h includes it).  Nothing host-only lives here.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include "lim_plan.h"
#include "dyn_plan.h"
#include "split_plan.h"
#include "delay_plan.h"
#include "agc_plan.h"
#include "automix_plan.h"
#include "failover_plan.h"
#include "drift_plan.h"
#include "iir_plan.h"
#include "iir_ramp.h"
#include "spec_plan.h"
#include "watch_plan.h"
#include "denoise_plan.h"

namespace cmhip {

constexpr unsigned MAX_CH = 16;
constexpr unsigned MAX_EQ = 4;

// Per-stream transform parameters, rebuilt on the host whenever a setter runs.
// The reference's q = trunc(x * gain / scale) (ref: src/transform.c:111-119) is done on magnitudes with
// the division split at the integer part of the gain:
//     gain = mi * scale + r   (r < scale),   mf = ceil(r * 2^32 / scale)   (< 2^32 because r <= scale - 1)
//     floor(|x| * gain / scale) = |x| * mi + mulhi(|x|, mf)
// exact for every |x| <= 32768, gain <= 65535, scale in 1..65535: with e = mf * scale - r * 2^32 in
// [0, scale) the product |x| * mf / 2^32 lies |x| * e / (scale * 2^32) < 2^31 / (scale * 2^32) < 1 / scale
// above |x| * r / scale, which is itself at least 1 / scale below the next integer when it is not one
// (cmhip_test_gain_consts / test_division_constants_are_exact prove it per class of gain and scale).
// Two VALU instructions per sample (v_mul_hi_u32, v_mad_u32_u16) instead of the three of a division
// by magic number and shift.  A disabled gain (scale 0 in the reference, ref: src/transform.c:107-108) is
// stored as mi 1 / mf 0, the identity through the same code.
//
// mode names the shorter forms the read-only runs take where the VALU binds (a VU window and no PCM
// result).  GAIN_IDENTITY: the gain is disabled or every gain equals the scale -- the magnitudes are the
// samples' own.  GAIN_BELOW_SCALE: every gain of the stream is below its scale -- mi is 0 everywhere, one
// v_mul_hi_u32 per sample, and the quotient never reaches the saturation limits.  GAIN_GENERAL: the rest.
// 128 bytes, one cache line per stream (round 3 kept the short forms in a table of their own, 96 + 68 bytes).
struct alignas(128) StreamParam {
    uint32_t mode;             // GAIN_GENERAL / GAIN_BELOW_SCALE / GAIN_IDENTITY
    uint32_t perm2;            // stereo channel map as a v_perm_b32 selector
    uint32_t map_identity;     // 1 when chmap is the identity
    uint32_t mi01;             // mi[0] | mi[1] << 16: what the mono / stereo kernels need sits in the first 32 bytes
    uint32_t mf[MAX_CH];       // ceil((gain[c] % scale) * 2^32 / scale)
    uint16_t mi[MAX_CH];       // gain[c] / scale
    uint8_t  chmap[MAX_CH];    // out channel c reads in channel chmap[c]
};
static_assert(sizeof(StreamParam) == 128, "one line per stream");
constexpr uint32_t GAIN_GENERAL = 0, GAIN_BELOW_SCALE = 1, GAIN_IDENTITY = 2;

// Per-stream VU window, all 64-bit so that every update is an integer atomic
// (add / max are associative and commutative: results do not depend on the order
// in which waves arrive).
//   key = |peak| << 47 | (~sample_index & (2^46-1)) << 1 | negative
// sample_index counts interleaved samples since the window opened, so the largest
// key is the largest magnitude and, among equals, the earliest sample: the
// reference's strict-greater update (ref: src/vumeter.c:163-168).
struct VuState {
    unsigned long long power[MAX_CH];
    unsigned long long key[MAX_CH];
    // interleaved samples accounted so far.  Two slots: a run reads slot `parity` and the
    // stream's first tile writes slot `parity^1`, so no wave can see a half-updated value
    // and no extra kernel is needed to advance the window; the host flips parity per run.
    unsigned long long samples[2];
};

constexpr int      KEY_ABS_SHIFT = 47;
constexpr uint64_t KEY_IDX_MASK  = (1ull << 46) - 1;
constexpr int      NODE_KEY_ABS_SHIFT = 46;      // |peak| of a node record's key (k_node_partial)

struct EqParam {
    uint32_t nsec;
    float    coef[MAX_EQ][5];  // b0 b1 b2 a1 a2
};
struct EqState {
    float s[MAX_EQ][4];        // x1 x2 y1 y2 per section
};

struct RunArgs {
    const int16_t *in;
    int16_t       *out;            // may equal in; nullptr: PCM not written
    float         *f32;            // planar float output or nullptr
    const StreamParam *param;
    VuState       *vu;             // nullptr: no VU
    const uint32_t *nframes;       // per-stream frame counts or nullptr
    uint32_t       frames;         // uniform count when nframes == nullptr
    uint32_t       streams;
    uint32_t       channels;
    uint64_t       stride;         // samples between stream slots (multiple of 8)
    uint64_t       plane;          // floats between planes of the f32 output
    uint32_t       chunks;         // 4 KiB tiles (one wave each) per stream slot
    uint32_t       parity;         // which VuState::samples slot is current
    uint32_t       identity_maps;  // 1 when no stream of the batch has a channel map
    // Completion by flag, for launches of ONE workgroup (the 1 KiB pulls of the per-stream stages): when not
    // null the workgroup, at its very end, makes its stores visible to the host and stores done_seq there
    // (pinned, device-mapped host memory).  The host spins on the word instead of waiting for the stream:
    // 4-5 us less per launch-and-wait on MI355X (tools/ubench_roundtrip.hip).  The launcher clears it
    // when the grid has more than one workgroup.
    uint32_t      *done_flag;
    uint32_t       done_seq;
};

struct EqArgs {
    const int16_t *in;
    int16_t       *out;            // int16 result or nullptr
    float         *f32;            // float result or nullptr
    const StreamParam *param;
    const EqParam *eq;
    EqState       *state;
    VuState       *vu;             // VU of the int16 result, or nullptr
    const uint32_t *nframes;
    uint32_t       frames;
    uint32_t       streams;
    uint32_t       channels;       // every channel of a stream runs the stream's filter, with state of its own
    uint32_t       nsec;           // biquad sections, same for every stream of the batch
    uint32_t       whole_streams;  // keep the channels of a stream in one workgroup (in place + channel maps)
    uint32_t       parity;
    uint64_t       stride;
    uint64_t       plane;
    uint32_t      *done_flag;      // as RunArgs::done_flag
    uint32_t       done_seq;
};

// True peak (ITU-R BS.1770 Annex 2, 4x oversampling): a 48-tap polyphase FIR over the TRANSFORMED stream (map,
// gain, saturation -- the samples the VU window accounts), coefficients in units of 2^-13.  Row p of TP_H is phase
// p: y_p[n] = sum_k TP_H[p][k] * x[n - k]; rows 2 and 3 are rows 1 and 0 reversed.  sum|h| <= 16571 per row, so
// |y| <= 16571 * 32768 < 2^31: int32 accumulators are exact.  (k_tpeak.hip; cmhip_tp.hip hands the table out.)
constexpr unsigned TP_TAPS = 12;
constexpr unsigned TP_HIST = TP_TAPS - 1;      // frames of history a stream keeps per channel
constexpr int16_t TP_P0[TP_TAPS] = {14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68};
constexpr int16_t TP_P1[TP_TAPS] = {-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155};
constexpr int16_t tp_h(unsigned p, unsigned k)
{
    return p == 0 ? TP_P0[k] : p == 1 ? TP_P1[k] : p == 2 ? TP_P1[TP_TAPS - 1 - k] : TP_P0[TP_TAPS - 1 - k];
}

struct TpArgs {
    const int16_t *in;             // the run's INPUT slots: the kernel applies map and gain itself
    const StreamParam *param;
    const uint32_t *nframes;       // per-stream frame counts or nullptr
    uint32_t      *peak;           // [S][MAX_CH] window maxima of |y|
    // [2][S][MAX_CH][TP_HIST] the last 11 transformed frames per channel, oldest first.  Two slots: a run reads slot
    // `parity`, the stream's last tile writes slot `parity ^ 1` (as VuState::samples); the host flips parity per run.
    int16_t       *hist;
    uint32_t       frames;         // uniform count when nframes == nullptr
    uint32_t       streams;
    uint32_t       channels;
    uint32_t       parity;
    uint64_t       stride;         // samples between stream slots (multiple of 8)
    uint32_t       chunks;         // tiles per stream (the launcher fills it in)
};

// Phase correlation (k_corr.hip; the specification: include/coolmic_hip.h): per stream and channel pair (a, b) the
// window sums of x_a^2, x_b^2 and x_a * x_b over the TRANSFORMED stream, exact 64-bit integers merged by integer
// atomics.  No filter, no history, no parity slot.
constexpr unsigned CORR_MAX_PAIRS = 8;
constexpr unsigned CORR_SUMS = 3;              // energy_a, energy_b, cross (two's complement) per pair
struct CorrArgs {
    const int16_t *in;             // the run's INPUT slots: the kernel applies map and gain itself
    const StreamParam *param;
    const uint32_t *nframes;       // per-stream frame counts or nullptr
    unsigned long long *sums;      // [S][CORR_MAX_PAIRS][CORR_SUMS] the windows
    uint32_t       frames;         // uniform count when nframes == nullptr
    uint32_t       streams;
    uint32_t       channels;
    uint32_t       npairs;
    uint8_t        a[CORR_MAX_PAIRS], b[CORR_MAX_PAIRS];     // transformed channels of pair i (for k_corr_any)
    uint64_t       stride;         // samples between stream slots (multiple of 8)
    uint32_t       chunks;         // tiles per stream (the launcher fills it in)
};

// Signal watch (k_watch.hip; the specification: include/coolmic_hip.h, the arithmetic: csrc/watch_plan.h): per stream
// the run-length and sum statistics of dead air, quiet channels and samples at the rail over the TRANSFORMED stream.
// The tile pass writes one summary per stream, tile and predicate and adds the channel sums by integer atomics; the
// fold walks a stream's summaries in order.  No workgroup waits for another: the stream orders the two kernels.
struct WatchArgs {
    const int16_t *in;             // the run's INPUT slots: the kernel applies map and gain itself
    const StreamParam *param;
    const uint32_t *nframes;       // per-stream frame counts or nullptr
    unsigned long long *words;     // [S][WATCH_WINDOW_WORDS] the windows
    unsigned long long *state;     // [S][WATCH_SLOTS] the run lengths the streams brought along
    WatchSum      *scratch;        // [S][chunks][2C + 1] the run's tile summaries
    uint32_t       frames;         // uniform count when nframes == nullptr
    uint32_t       streams;
    uint32_t       channels;
    uint32_t       quiet, rail, clip_run;
    uint64_t       stride;         // samples between stream slots (multiple of 8)
    uint32_t       chunks;         // tiles per stream (the launcher fills it in)
};

// Spectrum (k_spec.hip; the specification: include/coolmic_hip.h, the bookkeeping: csrc/spec_plan.h): per stream,
// selected channel and band the window sums of the blocks' bin powers over the TRANSFORMED stream, exact 64-bit integers
// merged by integer atomics.
struct SpecArgs {
    const int16_t *in;             // the run's INPUT slots: the kernel applies map and gain itself
    const StreamParam *param;
    const uint32_t *nframes;       // per-stream frame counts or nullptr
    unsigned long long *sums;      // [S][SPEC_MAX_CH][SPEC_MAX_BANDS] the windows
    // [2][S][nch][N] the last N - 1 transformed samples per selected channel, oldest first (entry N - 1 unused), and
    // [2][S] the streams' back (spec_plan.h).  Two slots each: a run reads slot `parity`, the state workgroups write
    // slot `parity ^ 1` (as TpArgs::hist); the host flips parity per run.
    int16_t       *hist;
    uint32_t      *back;
    // the tables, made when the meter is turned on: Wr[N / 2], Wi[N / 2], win[N] (as int32), edges[nb + 1]
    const int32_t *table;
    uint64_t       chpack;         // the selected channels, channel i in byte i
    uint32_t       frames;         // uniform count when nframes == nullptr
    uint32_t       streams;
    uint32_t       channels;
    uint32_t       log2n;          // n
    uint32_t       nch, nb;        // selected channels, bands
    uint32_t       parity;
    uint64_t       stride;         // samples between stream slots (multiple of 8)
    // workgroups per stream and channel: the run's largest block count + 1 (the launcher fills it in)
    uint32_t       chunks;
};

// Loudness (ITU-R BS.1770 K-weighting, 100 ms sub-block sums): one row is one channel of one stream.
// LoudState [S][C]: the two biquads' Direct Form I history in double (section 2's inputs are section 1's outputs, so
// six values), the open sub-block's sum of squares, the frames it holds, and the sub-blocks the row has completed.
// Exactly one lane owns a row in a launch, so the state is updated in place.  All zero = freshly reset.
struct LoudState {
    double   u1, u2;               // section 1 inputs n-1, n-2
    double   y1, y2;               // section 1 outputs n-1, n-2 (= section 2's inputs)
    double   v1, v2;               // section 2 outputs n-1, n-2
    double   e;                    // sum of squares of the open sub-block, in frame order from 0.0
    uint32_t pos;                  // frames in the open sub-block (< LoudArgs::sub)
    uint32_t pad;
    uint64_t done;                 // sub-blocks completed since enable / reset; number j went to ring slot j % ring
};
static_assert(sizeof(LoudState) == 72, "nine 8-byte words");

struct LoudArgs {
    const int16_t *in;             // the run's INPUT slots: the kernel applies map and gain itself
    const StreamParam *param;
    const uint32_t *nframes;       // per-stream frame counts or nullptr
    LoudState     *state;          // [S][C]
    double        *ring;           // [S][ring][C] completed sub-block sums
    double         coef[10];       // cmhip_loud_coefficients: {b0,b1,b2,a1,a2} of section 1, of section 2
    uint32_t       frames;         // uniform count when nframes == nullptr
    uint32_t       streams;
    uint32_t       channels;
    uint32_t       sub;            // frames per sub-block: (rate + 5) / 10
    uint32_t       ring_slots;
    uint64_t       stride;         // samples between stream slots (multiple of 8)
};

// Sample-rate conversion (k_src.hip; the arithmetic: include/coolmic_hip.h): a resampler's run over S stream slots.
struct SrcArgs {
    const int16_t *in;             // int16 [S][in_stride]
    int16_t       *out;            // int16 [S][out_stride]
    const uint32_t *nframes;       // per-stream input frame counts or nullptr
    // [L][T8 + 8] the table in the kernel's form: rows padded with zero taps to T8 = T rounded up to 8 and by 8 more
    // samples, every tap pair swapped (H[p][k+1], H[p][k]) -- the order v_dot2c_i32_i16 meets a pair of samples in
    const int16_t *table;
    // [2][S][C][T-1] the last T-1 input frames per channel, oldest first, and [2][S] r = (frames so far) mod M.  Two
    // slots each: a run reads slot `parity`, the stream's last tile writes slot `parity ^ 1`; the host flips parity.
    int16_t       *hist;
    uint32_t      *rpos;
    uint64_t       in_stride, out_stride;    // samples between stream slots (multiples of 8)
    uint32_t       frames;         // uniform count when nframes == nullptr
    uint32_t       streams;
    uint32_t       channels;
    uint32_t       parity;
    uint32_t       L, M, T;
    // (the launcher fills these in)
    uint32_t       inv_l;          // ceil(2^32 / L), 0 for L == 1
    uint32_t       chunks;         // tiles per stream
    uint32_t       tile_out;       // output frames per tile
    uint32_t       row;            // samples between the planes of a tile in LDS
    uint32_t       table_lds;      // the table is copied into LDS
};

// Channel mixing (k_mix.hip; the arithmetic: include/coolmic_hip.h): a mixer's run over S stream slots.
struct MixArgs {
    const int16_t *in;             // int16 [S][in_stride]
    int16_t       *out;            // int16 [S][out_stride]
    const uint32_t *nframes;       // per-stream frame counts or nullptr
    // [S][C_out][CP] the matrices in the kernel's form, CP = ceil(C_in / 2): dword k of row o is
    // W[o][2k] | W[o][2k+1] << 16, an odd C_in padded with a zero weight
    const uint32_t *wk;
    uint64_t       in_stride, out_stride;    // samples between stream slots (multiples of 8)
    uint32_t       frames;         // uniform count when nframes == nullptr
    uint32_t       streams;
    uint32_t       channels_in, channels_out;
    // (the launcher fills these in)
    uint32_t       chunks;         // tiles per stream
    uint32_t       tile_frames;    // frames per tile
};

// Matrix ramps (k_mixramp.hip; the arithmetic: include/coolmic_hip.h, csrc/mix_ramp.h): a mixer's run while at least
// one stream ramps.  Per stream a record of MIXR_HDR + 2 n dwords, n = C_out * CP:
//     inc, R, done, 0,  W0[n], W1[n]       (the matrices in the kernel's form, MixArgs::wk)
// The stream ramps while done < R; frame f of the run uses w(p(done + f + 1)).  MixArgs::wk holds the targets.
constexpr uint32_t MIXR_HDR = 4;
constexpr uint32_t MIXR_INC = 0, MIXR_R = 1, MIXR_DONE = 2;
struct MixRampArgs {
    MixArgs         m;
    const uint32_t *ramp;          // [S][MIXR_HDR + 2 n]
};

// Mix bus (k_bus.hip; the arithmetic: include/coolmic_hip.h): a run that sums S input slots into B bus slots by the
// routing table csrc/bus_route.h compiled.
struct BusArgs {
    const int16_t *in;             // int16 [S][in_stride]
    int16_t       *out;            // int16 [B][out_stride]
    const uint32_t *nframes;       // per-stream frame counts or nullptr
    const uint32_t *bus_frames;    // per-bus frame counts (read when nframes != nullptr)
    const uint32_t *first;         // [B+1] sends of bus b: first[b] .. first[b+1]-1; bit 31: the bus has several groups
    const uint32_t *send;          // [n] the send's stream; bit 31: the send starts a group
    const uint32_t *wk;            // [n][C_out][CP] the sends' matrices in the mixer's form (MixArgs::wk)
    uint64_t       in_stride, out_stride;    // samples between slots (multiples of 8)
    uint32_t       frames;         // uniform count when nframes == nullptr
    uint32_t       buses;
    uint32_t       channels_in, channels_out;
    uint32_t       nt_loads;       // k_bus_fast loads its input non-temporally (tools/bench_bus.py; default: plain)
    // (the launcher fills these in)
    uint32_t       chunks;         // tiles per bus
    uint32_t       tile_frames;    // frames per tile
};

// Send ramps (k_busramp.hip; the arithmetic: include/coolmic_hip.h, "send ramps"): a bus's run while at least one send
// ramps.  Per send, in the table's compiled order, a record of BUSR_HDR + 2 n dwords, n = C_out * CP, whose layout
// csrc/bus_ramp.h states: inc, R, done, bus, W0[n], W1[n].  The send ramps while done < R; frame f of its bus uses
// w(p(done + f + 1)).  BusArgs::wk holds the targets.
struct BusRampArgs {
    BusArgs         b;
    const uint32_t *ramp;          // [n sends][BUSR_HDR + 2 n]
};

// Peak limiter (k_lim.hip, k_limtp.hip, k_limrel.hip; the arithmetic: include/coolmic_hip.h): a limiter's run over S stream slots.
struct LimArgs {
    const int16_t *in;             // int16 [S][in_stride]
    int16_t       *out;            // int16 [S][out_stride]
    const uint32_t *nframes;       // per-stream frame counts or nullptr
    const uint32_t *par;           // [S] threshold | drive << 16
    // [2][S][halo * C] the last halo input frames per stream, interleaved, oldest first.  Two slots: a run reads slot
    // `parity`, the stream's last tile (or its first, for a stream with 0 frames) writes slot `parity ^ 1`; the host
    // flips parity (the mechanism of SrcArgs::hist).
    int16_t       *hist;
    uint32_t      *gmin;           // [S] the gain-reduction meter: minimum s[n], Q15
    uint64_t       in_stride, out_stride;    // samples between stream slots (multiples of 8)
    uint32_t       frames;         // uniform count when nframes == nullptr
    uint32_t       streams;
    uint32_t       channels;
    uint32_t       parity;
    uint32_t       a, W;           // lookahead_log2, A + hold
    // (the launcher fills these in)
    uint32_t       halo;           // LimGeom::halo
    uint32_t       chunks;         // tiles per stream
    uint32_t       tile_frames;    // frames per tile
};

// Dynamics (k_dyn.hip; the arithmetic: include/coolmic_hip.h): a run of a dynamics stage over S stream slots.
struct DynArgs {
    const int16_t *in;             // int16 [S][in_stride]
    int16_t       *out;            // int16 [S][out_stride]
    const uint32_t *nframes;       // per-stream frame counts or nullptr
    const uint16_t *curve;         // [S][DYN_CURVE] the streams' curves
    // [2][S][halo * C] the last halo input frames per stream, interleaved, oldest first; the two slots of LimArgs::hist
    int16_t       *hist;
    uint32_t      *gmin;           // [S] the gain meter: minimum s[n], Q15
    uint64_t       in_stride, out_stride;    // samples between stream slots (multiples of 8)
    uint32_t       frames;         // uniform count when nframes == nullptr
    uint32_t       streams;
    uint32_t       channels;
    uint32_t       parity;
    uint32_t       a, b, W;        // detector_log2, smooth_log2, B + hold
    // (the launcher fills these in)
    uint32_t       halo;           // DynGeom::halo
    uint32_t       chunks;         // tiles per stream
    uint32_t       tile_frames;    // frames per tile
};
// a curve as it travels: a kernel argument of 256 bytes, entries k and k + 1 in dword k / 2
struct DynCurveArg {
    uint32_t w[DYN_CURVE / 2];
};

// Band split (k_split.hip; the arithmetic: include/coolmic_hip.h): a run of a band split over S stream slots.
struct SplitArgs {
    const int16_t *in;             // int16 [S][in_stride]
    int16_t       *out;            // int16 [B][S][out_stride]
    const uint32_t *nframes;       // per-stream frame counts or nullptr
    const uint32_t *table;         // the filters in the kernel's form (csrc/split_plan.h)
    // [2][S][C][T-1] the last T-1 input frames per channel, oldest first; the two slots of SrcArgs::hist
    int16_t       *hist;
    uint32_t      *clips;          // [S][B] saturated samples per stream and band
    uint64_t       in_stride, out_stride;    // samples between slots (multiples of 8)
    uint32_t       frames;         // uniform count when nframes == nullptr
    uint32_t       streams;
    uint32_t       channels;
    uint32_t       bands, taps;
    uint32_t       parity;
    // (the launcher fills these in)
    uint32_t       chunks;         // tiles per stream
    uint32_t       tile_frames;    // frames per tile
    uint32_t       row;            // samples between the planes of a tile in LDS
    uint32_t       table_words;    // dwords of the table in LDS
};

// Delay (k_delay.hip; the arithmetic: include/coolmic_hip.h, the geometry: csrc/delay_plan.h): a run of a delay stage
// over S stream slots.
struct DelayArgs {
    const int16_t *in;             // int16 [S][in_stride]
    int16_t       *out;            // int16 [S][out_stride]
    int16_t       *ring;           // int16 [S][ring_samples] the streams' rings
    const uint32_t *rec;           // [S][DELAY_REC] the run's records: count, pos, d1, d0, R, done, inc
    uint64_t       in_stride, out_stride;    // samples between stream slots (multiples of 8)
    uint32_t       ring_samples;   // CAP: samples of a stream's ring (a multiple of 8)
    uint32_t       streams;
    uint32_t       channels;
    // (the launcher fills these in)
    uint32_t       chunks;         // tiles per stream
    uint32_t       tile_vecs;      // 16-byte vectors per tile
};

// Leveller (k_agc.hip; the arithmetic: include/coolmic_hip.h, the windows and tiles: csrc/agc_plan.h).  What a stream
// carries from run to run, written by k_agc_step alone:
struct AgcState {
    unsigned long long psum[16];   // the open window's sums of squares so far, per channel
    uint32_t a_lo, a_hi;           // the gain nodes of the window the stream's last frame lies in: A[k], A[k+1]
    uint32_t level;                // L of the last complete window
    uint32_t pad;
};
// a run of a leveller over S stream slots
struct AgcArgs {
    const int16_t *in;             // int16 [S][in_stride]
    int16_t       *out;            // int16 [S][out_stride]
    const uint32_t *rec;           // [S][AGC_REC] the run's records: count, pos, the parameters
    unsigned long long *table;     // [S][nw][C] the run's sums of squares per window and channel; zero between runs
    uint32_t      *nodes;          // [S][nw + 1] the run's gain nodes: window i has nodes i and i + 1
    AgcState      *state;          // [S]
    unsigned long long *clips;     // [S] clamped samples
    uint64_t       in_stride, out_stride;    // samples between stream slots (multiples of 8)
    uint32_t       streams;
    uint32_t       channels;
    uint32_t       w;              // window_log2
    // (the launcher fills these in)
    uint32_t       nw;             // windows per stream in the tables
    uint32_t       chunks;         // tiles per stream
    uint32_t       tile_log2;      // frames per tile, as a power of two
};

// Automixer (k_automix.hip; the arithmetic: include/coolmic_hip.h, the record and the mirror: csrc/automix_plan.h).  What
// a stream carries from run to run: k_automix_level writes psum and power, k_automix_share the rest
struct AutomixState {
    unsigned long long psum[16];   // the open window's sums of squares so far, per channel
    unsigned long long power;      // P of the last complete window
    uint32_t a_lo, a_hi;           // the gain nodes of the window the stream's last frame lies in: A[k], A[k+1]
    uint32_t pending;              // D of the last complete window: the node the next window edge brings in
    uint32_t pad;
};
// Noise suppressor (k_denoise.hip; the arithmetic: include/coolmic_hip.h, the block and the mirror:
// csrc/denoise_plan.h).  A row is a (stream, channel); everything a row carries from run to run is written by the one
// workgroup that owns the row.
struct DenoiseArgs {
    const int16_t *in;             // int16 [S][in_stride]
    int16_t       *out;            // int16 [S][out_stride]
    const uint32_t *rec;           // [S][DENOISE_REC] the run's records: count, back, flags, cnt, the parameters
    const int32_t *table;          // Wr[N/2], Wi[N/2], sw[N]
    int16_t       *hist;           // [2][S][C][N] the rows' last N - 1 inputs, oldest first (entry N - 1 unused); a run
                                   // reads slot `parity` and writes the other one
    int32_t       *tail;           // [S][C][N] the overlap-add of the last completed block's span (denoise_plan.h)
    uint32_t      *gain;           // [S][C][N/2 + 1] g
    unsigned long long *np;        // [S][C][N/2 + 1] the profile
    unsigned long long *acc;       // [S][C][N/2 + 1] the learning sums
    unsigned long long *clips;     // [S] clamped output samples
    unsigned long long *sat;       // [S] clamped components of the inverse transform
    uint64_t       in_stride, out_stride;    // samples between stream slots (multiples of 8)
    uint32_t       streams, channels;
    uint32_t       log2n;
    uint32_t       parity;
};

// a run of an automixer over S stream slots
struct AutomixArgs {
    AgcArgs        tile;           // what the leveller's tile bodies read (state: unused, nullptr); tile.rec: every stream's
                                   // record, as the apply pass and the two lane-per-stream kernels read it
    const uint32_t *rec_energy;    // [S][AGC_REC] the same records with count 0 for a stream in no group: the energy pass
                                   // reads nothing of such a stream and leaves its table row alone
    unsigned long long *power;     // [S][nw] P of the run's complete windows, level's word to share
    unsigned long long *gsum;      // [S][nw] per group id and window of the run: the members' sum of P; zero before level
    AutomixState  *state;          // [S]
};

// Failover switch (k_failover.hip; the arithmetic: include/coolmic_hip.h, the records, the plan word and the mirror:
// csrc/failover_plan.h).  What an output carries from run to run, written by k_failover_step alone:
struct FailoverState {
    unsigned long long psum[4][16];    // the open window's sums of squares so far, per candidate and channel
    uint32_t level[4];                 // m of the last complete window, per candidate
    unsigned long long live, dead;     // the counters as the last edge processed left them, packed (failover_run)
    uint32_t plan;                     // the plan word of the window the output's last frame lies in
    uint32_t pad[3];
};
// a run of a failover switch: S input slots, O output slots
struct FailoverArgs {
    AgcArgs        energy;         // what the leveller's energy body reads: O * 4 rows, rec: the rows' records, in: the
                                   // input array, table [O * 4][nw][C]; out, nodes, state and clips unused (nullptr)
    int16_t       *out;            // int16 [O][out_stride]
    const uint32_t *rec;           // [O][FO_REC] the outputs' records
    uint32_t      *plan;           // [O][nw + 1] the run's plan words: window i of the run has entry i
    FailoverState *state;          // [O]
    unsigned long long *switches;  // [O] changeovers begun
    uint64_t       out_stride;     // samples between output slots (a multiple of 8)
    uint32_t       outputs;
};

// Drift stage (k_drift.hip; the arithmetic: include/coolmic_hip.h, the table's form, the record and the plan:
// csrc/drift_plan.h): a run over S stream slots.
struct DriftArgs {
    const int16_t *in;             // int16 [S][in_stride]
    int16_t       *out;            // int16 [S][out_stride]
    const uint32_t *rec;           // [S][DRIFT_REC] the run's F, K, delta and pos per stream, from the host's mirror
    const uint32_t *table;         // [P + 1][T/2 + 1] the table in the kernel's form (drift_compile)
    int16_t       *hist;           // [2][S][C][T-1] the last T-1 input frames; the two slots of SrcArgs::hist
    uint64_t       in_stride, out_stride;    // samples between stream slots (multiples of 8)
    uint32_t       streams;
    uint32_t       channels;
    uint32_t       parity;
    uint32_t       phi, T;
    // (the launcher fills these in)
    uint32_t       chunks;         // tiles per stream
    uint32_t       tile_out;       // output frames per tile
    uint32_t       row;            // samples between the planes of a tile in LDS
    uint32_t       table_lds;      // the table is copied into LDS
    uint32_t       table_words;    // its dwords
};

// Filter (k_iir.hip; the arithmetic: include/coolmic_hip.h, the tiles: csrc/iir_plan.h): a run of a biquad cascade over
// S stream slots
struct IirArgs {
    const int16_t *in;             // int16 [S][in_stride]
    int16_t       *out;            // int16 [S][out_stride]
    const uint32_t *counts;        // [S] the run's frames per stream
    const int32_t *coef;           // [S][N][5] b0, b1, b2, a1, a2 in units of 2^-26; in a ramp run [S][N][12], IirRampEntry
    IirState      *state;          // [S * C][N] the rows' sections between two runs
    unsigned long long *clips;     // [S] outputs the last clamp changed
    unsigned long long *overs;     // [S] section results the inner clamp changed
    uint64_t       in_stride, out_stride;    // samples between stream slots (multiples of 8)
    uint32_t       streams;
    uint32_t       channels;
    uint32_t       sections;       // N
};

struct GenArgs {
    int16_t *dst;
    uint32_t streams, channels, frames;
    uint64_t stride;
    uint32_t seed;
    uint64_t first_global, global_step, frame_offset;
    int16_t  sine[48];
};

// launchers (k_block.hip, k_eq.hip, k_misc.hip)
// (ev_start / ev_stop: optional events that take the kernel's own start and end -- hipExtLaunchKernelGGL
// stamps them from the dispatch itself, without the extra packets of hipEventRecord around the launch)
// (*flagged: the launch was one workgroup and carries the completion flag of RunArgs::done_flag)
// What launch_run launches for a run (plan_run, k_block.hip): the kernel, its grid and its tiles.
enum RunFamily : uint32_t { RUN_NONE = 0, RUN_FAST, RUN_FAST_RO, RUN_WIDE, RUN_ROWS };
struct RunPlan {
    hipError_t err;                // hipErrorInvalidValue: refused, the grid would reach 2^31 workgroups
    uint32_t   family;             // RunFamily; RUN_NONE: nothing to launch (or refused)
    uint32_t   channels;           // template C of k_run_fast / k_run_fast_ro / k_run_wide (0 for k_run_rows)
    uint32_t   tile_u;             // 16-byte vectors per lane of a tile (k_run_fast, k_run_fast_ro, k_run_wide)
    uint32_t   waves;              // waves per workgroup (k_run_fast's NW)
    uint32_t   map, stage;         // k_run_rows' MAP and STAGE
    uint32_t   grid, block;        // workgroups, threads per workgroup
    uint32_t   chunks;             // RunArgs::chunks: tiles per stream
    uint32_t   W, rows_per_tile;   // k_run_rows' arguments
    uint32_t   keep_flag;          // the launch is one workgroup and carries RunArgs::done_flag
};
RunPlan plan_run(const RunArgs &a);
hipError_t launch_run(const RunArgs &a, hipStream_t st, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr,
                      bool *flagged = nullptr);
// (the first launch of an EQ kernel variant on a device raises its dynamic-LDS limit there:
// prepare_eq does that for a batch's device when the batch is created, launch_eq checks it)
hipError_t prepare_eq(int device);
hipError_t launch_eq(const EqArgs &a, hipStream_t st, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr,
                     bool *flagged = nullptr);
// True peak (k_tpeak.hip): the kernel of a run and its grid.  fast: the mono / stereo kernel (one wave per 8 KiB tile);
// otherwise the any-channel-count kernel (one workgroup per 1024 frames).
struct TpPlan {
    hipError_t err;                // hipErrorInvalidValue: refused, the grid would reach 2^31 workgroups
    uint32_t   fast;
    uint32_t   grid, block;        // grid 0: nothing to launch (or refused)
    uint32_t   chunks;             // TpArgs::chunks: tiles per stream
};
TpPlan plan_tpeak(const TpArgs &a);
hipError_t launch_tpeak(const TpArgs &a, hipStream_t st);
// Phase correlation (k_corr.hip): the kernel of a run and its grid.  fast: stereo with one pair (one wave per 8 KiB
// tile, sums of channel 0 / channel 1 / their product into pair 0 whichever way round the pair names them); otherwise
// the any-channel-count kernel (one workgroup per 1024 frames).  A mono run has no pair: nothing to launch.
struct CorrPlan {
    hipError_t err;                // hipErrorInvalidValue: refused, the grid would reach 2^31 workgroups
    uint32_t   fast;
    uint32_t   grid, block;        // grid 0: nothing to launch (or refused)
    uint32_t   chunks;             // CorrArgs::chunks: tiles per stream
};
CorrPlan plan_corr(const CorrArgs &a);
hipError_t launch_corr(const CorrArgs &a, hipStream_t st);
// Spectrum (k_spec.hip): one workgroup of 256 threads per stream, selected channel and block of the run, and one more
// per stream and channel that writes the state the run leaves.  max_blocks: the largest block count of the run's streams
// (spec_run_blocks over the host's mirror of the streams' back).
struct SpecPlan {
    hipError_t err;                // hipErrorInvalidValue: refused, the grid would reach 2^31 workgroups
    uint32_t   grid, block;        // grid 0: nothing to launch (or refused)
    uint32_t   chunks;             // SpecArgs::chunks
};
SpecPlan plan_spec(const SpecArgs &a, uint32_t max_blocks);
hipError_t launch_spec(const SpecArgs &a, uint32_t max_blocks, hipStream_t st);
// Noise suppressor (k_denoise.hip): one workgroup of DENOISE_BLOCK threads per row, streams * channels of them (below
// 2^31: the object's geometry says so).
hipError_t launch_denoise(const DenoiseArgs &a, hipStream_t st);
// Signal watch (k_watch.hip): the plan is csrc/watch_plan.h's, shared with the CPU tests.  launch_watch queues the
// tile pass and the fold; a.scratch holds at least plan.scratch summaries.  ev: nullptr, or three events recorded
// ahead of the tile pass, between the two kernels and behind the fold (the measurement of tools/bench_watch.py).
hipError_t launch_watch(const WatchArgs &a, const WatchPlan &p, hipStream_t st, hipEvent_t *ev = nullptr);
// Loudness (k_loud.hip): one lane per row, one wave per workgroup.
struct LoudPlan {
    hipError_t err;                // hipErrorInvalidValue: refused, the grid would reach 2^31 workgroups
    uint32_t   vec;                // mono / stereo: the lanes walk their slots in 16-byte vectors
    uint32_t   grid, block;        // grid 0: nothing to launch (or refused)
};
LoudPlan plan_loud(const LoudArgs &a);
hipError_t launch_loud(const LoudArgs &a, hipStream_t st);
// Sample-rate conversion (k_src.hip): one workgroup per stream and tile of tile_out output frames.  fast: the mono /
// stereo kernel; otherwise the any-channel-count kernel.  out_frames: what the run gives its longest stream.
struct SrcPlan {
    hipError_t err;                // hipErrorInvalidValue: refused, the grid would reach 2^31 workgroups
    uint32_t   fast;
    uint32_t   grid, block;        // grid 0: nothing to launch (or refused)
    uint32_t   chunks;             // SrcArgs::chunks: tiles per stream
    uint32_t   tile_out;           // output frames per tile
    uint32_t   tile_in;            // input frames a tile stages at most, its halo included
    uint32_t   row;                // SrcArgs::row
    uint32_t   table_lds;          // SrcArgs::table_lds
    uint32_t   lds_bytes;          // dynamic LDS of the launch
};
SrcPlan plan_src(const SrcArgs &a, uint32_t out_frames);
hipError_t launch_src(const SrcArgs &a, uint32_t out_frames, hipStream_t st);
// Channel mixing (k_mix.hip): one workgroup per stream and tile of tile_frames frames.  fast: the kernel for mono /
// stereo on both sides (one wave per workgroup, no LDS); otherwise the any-channel-count kernel (256 threads).
struct MixPlan {
    hipError_t err;                // hipErrorInvalidValue: refused, the grid would reach 2^31 workgroups
    uint32_t   fast;
    uint32_t   grid, block;        // grid 0: nothing to launch (or refused)
    uint32_t   chunks;             // MixArgs::chunks: tiles per stream
    uint32_t   tile_frames;        // MixArgs::tile_frames (a multiple of 8)
    uint32_t   lds_bytes;          // dynamic LDS of the launch
};
MixPlan plan_mix(const MixArgs &a);
hipError_t launch_mix(const MixArgs &a, hipStream_t st);
// (one matrix W[C_out][C_in] into the kernel-form rows of streams first .. first + count - 1, in stream order; the
// matrix travels as a kernel argument, so W may change as soon as the call returns)
hipError_t launch_mix_set(uint32_t *wk, uint32_t first, uint32_t count, uint32_t channels_in, uint32_t channels_out,
                          const int16_t *W, hipStream_t st);
// Matrix ramps (k_mixramp.hip).  launch_mixramp: a run with plan_mix's own grid and tile (lds_bytes: the dynamic LDS
// of the any-channel-count ramp kernel, two matrices beside the target); the caller launches it only while a stream
// ramps.  The small kernels, all in stream order: start (or retarget) a ramp of R >= 2 frames to W for streams first
// .. first + count - 1, each from its own matrix in force; advance every stream's position by its count of the run
// (nframes nullptr: by frames); cancel the ramps of a range of streams.
uint32_t mixramp_record_dwords(uint32_t channels_in, uint32_t channels_out);
uint32_t mixramp_lds_bytes(uint32_t channels_in, uint32_t channels_out, uint32_t tile_frames);
hipError_t launch_mixramp(const MixRampArgs &a, hipStream_t st);
hipError_t launch_mixramp_start(uint32_t *ramp, uint32_t *wk, uint32_t first, uint32_t count, uint32_t channels_in,
                                uint32_t channels_out, const int16_t *W, uint32_t R, hipStream_t st);
hipError_t launch_mixramp_advance(uint32_t *ramp, const uint32_t *nframes, uint32_t frames, uint32_t streams,
                                  uint32_t channels_in, uint32_t channels_out, hipStream_t st);
hipError_t launch_mixramp_cancel(uint32_t *ramp, uint32_t first, uint32_t count, uint32_t channels_in,
                                 uint32_t channels_out, hipStream_t st);
// Mix bus (k_bus.hip): one workgroup per bus and tile of tile_frames frames.  fast: the kernel for mono / stereo on
// both sides (one wave per workgroup, no LDS); otherwise the any-channel-count kernel (256 threads).
struct BusPlan {
    hipError_t err;                // hipErrorInvalidValue: refused, the grid would reach 2^31 workgroups
    uint32_t   fast;
    uint32_t   grid, block;        // grid 0: nothing to launch (or refused)
    uint32_t   chunks;             // BusArgs::chunks: tiles per bus
    uint32_t   tile_frames;        // BusArgs::tile_frames (a multiple of 8)
    uint32_t   lds_bytes;          // dynamic LDS of the launch
};
BusPlan plan_bus(const BusArgs &a);
hipError_t launch_bus(const BusArgs &a, hipStream_t st);
// Send ramps (k_busramp.hip).  plan_busramp: plan_bus's grid and block; the mono / stereo forms keep its tile, the
// any-channel-count form chooses its own with W0 and W1 counted beside the send's matrix in LDS.  launch_busramp: a run;
// the caller launches it only while a send ramps.  launch_busramp_advance, behind it on the stream: every ramping
// send's position moves on by its bus's count of the run (bus_frames nullptr: by frames), capped at R.
BusPlan plan_busramp(const BusArgs &a);
hipError_t launch_busramp(const BusRampArgs &a, hipStream_t st);
hipError_t launch_busramp_advance(uint32_t *ramp, const uint32_t *bus_frames, uint32_t frames, uint32_t sends,
                                  uint32_t channels_in, uint32_t channels_out, hipStream_t st);
// Peak limiter (k_lim.hip): one workgroup of 256 threads per stream and tile; the plan is csrc/lim_plan.h's.
hipError_t launch_lim(const LimArgs &a, hipStream_t st);
// The same with the true-peak detector (k_limtp.hip): LimArgs as they are, halo and delay are lim_geom_tp's.
hipError_t launch_limtp(const LimArgs &a, hipStream_t st);
// Either of them with a release stage of 2^release_log2 frames (k_limrel.hip): halo is lim_geom_rel's, the plan
// plan_limrel's; release_log2 0 is launch_lim or launch_limtp itself.
hipError_t launch_limrel(const LimArgs &a, uint32_t detector, uint32_t release_log2, hipStream_t st);
// (threshold and drive into the parameter words of streams first .. first + count - 1; they travel as kernel arguments)
hipError_t launch_lim_set(uint32_t *par, uint32_t first, uint32_t count, uint32_t threshold, uint32_t drive,
                          hipStream_t st);
// Dynamics (k_dyn.hip): one workgroup of 256 threads per stream and tile; the plan is csrc/dyn_plan.h's.  detector is
// DYN_DETECT_*.  key == nullptr: every stream's detector reads the stream itself; otherwise the detector of stream s
// reads stream key[s] (uint32 [S] on the device; a keyed stream and its key have equal counts).
hipError_t launch_dyn(const DynArgs &a, uint32_t detector, const uint32_t *key, hipStream_t st);
// (one curve into the tables of streams first .. first + count - 1; it travels as a kernel argument)
hipError_t launch_dyn_set(uint16_t *curve, uint32_t first, uint32_t count, const uint16_t *table, hipStream_t st);
// (the key map's writer: streams first .. first + count - 1 get `key`, or each itself where own is set; both values
// travel as kernel arguments)
hipError_t launch_dyn_set_key(uint32_t *map, uint32_t first, uint32_t count, uint32_t key, bool own, hipStream_t st);
// Band split (k_split.hip): one workgroup of 256 threads per stream and tile; the plan is csrc/split_plan.h's.
hipError_t launch_split(const SplitArgs &a, hipStream_t st);
// Delay (k_delay.hip): one workgroup per stream and tile; the plan is csrc/delay_plan.h's.  frames: the run's largest
// count, max_delay and max_frames the object's.
hipError_t launch_delay(const DelayArgs &a, uint32_t max_delay, uint32_t max_frames, uint32_t frames, hipStream_t st);
// Leveller (k_agc.hip): k_agc_energy, k_agc_step and k_agc_apply, in that order; the plan is csrc/agc_plan.h's.  frames:
// the run's largest count, max_frames the object's.  ev: nullptr, or four events recorded in front of, between and behind
// the three launches (tools/bench_agc.py).
hipError_t launch_agc(const AgcArgs &a, uint64_t max_frames, uint32_t frames, hipStream_t st, hipEvent_t *ev = nullptr);
// Automixer (k_automix.hip): gsum cleared, then k_automix_energy, k_automix_level, k_automix_share and k_automix_apply, in
// that order on `st`; the plan is the leveller's.  ev: nullptr, or five events around the four launches
// (tools/bench_automix.py); the clearing of gsum lies between the first two.
hipError_t launch_automix(const AutomixArgs &a, uint64_t max_frames, uint32_t frames, hipStream_t st, hipEvent_t *ev = nullptr);
// Failover switch (k_failover.hip): k_failover_energy, k_failover_step and k_failover_apply, in that order.  ev (may be
// nullptr): four events recorded in front of, between and behind the three launches (tools/bench_failover.py).
hipError_t launch_failover(const FailoverArgs &a, uint64_t max_frames, uint32_t frames, hipStream_t st, hipEvent_t *ev = nullptr);
// Drift stage (k_drift.hip): one workgroup of 256 threads per stream and tile of output frames; the plan is
// csrc/drift_plan.h's.  out_frames: what the run gives its longest stream.
hipError_t launch_drift(const DriftArgs &a, uint32_t out_frames, hipStream_t st);
// Filter (k_iir.hip): one launch, a workgroup per iir_plan's spw streams.  frames: the run's largest count.  ramp: some
// section ramps at the run's start, a.coef is the ramp table (csrc/iir_ramp.h) and the kernels are k_iirramp.hip's.
hipError_t launch_iir(const IirArgs &a, uint32_t frames, bool ramp, hipStream_t st);
hipError_t launch_generate(const GenArgs &a, int mode, hipStream_t st);
hipError_t launch_node_partial(const VuState *vu, uint32_t streams, uint32_t channels,
                               uint32_t parity, uint64_t first_global, uint64_t global_step,
                               long long *dst_sum, long long *dst_key, bool clear, hipStream_t st,
                               hipEvent_t ev_stop = nullptr);
// (a set of windows -> [1 + 2C][streams] words in pinned, device-mapped host memory; clears the set)
hipError_t launch_vu_pack(VuState *vu, uint32_t streams, uint32_t channels, uint32_t parity,
                          unsigned long long *dst_host_mapped, hipStream_t st, hipEvent_t ev_stop);
// (the same with the dB finish on the device: finished doubles and int16 peaks, the layout stated at k_vu_finish)
hipError_t launch_vu_finish(VuState *vu, uint32_t streams, uint32_t channels, uint32_t parity,
                            unsigned long long *dst_host_mapped, hipStream_t st, hipEvent_t ev_stop);
// (test hook: the device finish over n (sum, count) pairs in device memory; lg may be nullptr)
hipError_t launch_test_power_db(const unsigned long long *sum, const unsigned long long *count, uint32_t n, double *db,
                                double *lg, hipStream_t st);
hipError_t launch_ceiling(int mode, const void *src, void *dst, size_t bytes,
                          unsigned long long *sink, hipStream_t st);

}  // namespace cmhip
