/*
 * coolmic_hip.h -- C ABI of the MI355X batch engine behind the transform -> vumeter path.
 *
 * Plain pointers and sizes only.  One cmhip_batch_t owns, on one GPU, a block of
 * S independent capture streams that share a channel count: their PCM slots in
 * HBM, their gain / channel-map / EQ parameters and their VU accumulators.  One
 * cmhip_batch_run() is one pass of the reference's per-sample loops over every
 * stream of the batch:
 *
 *   replaces, per stream and per block:
 *     __process()            ref: src/transform.c:101-124   (gain, saturate)
 *     the accumulate loop    ref: src/vumeter.c:161-177     (peak, sum of squares)
 *     int16 -> float planar  ref: src/enc_vorbis.c:108-115  (optional output)
 *   and cmhip_batch_vu_result() replaces
 *     coolmic_vumeter_result ref: src/vumeter.c:189-218     (dB on the host, double)
 *
 * The per-stream objects of <coolmic-dsp/transform.h> and <coolmic-dsp/vumeter.h>
 * sit on top of this engine.  Every function returns a COOLMIC_ERROR_* number
 * (<coolmic-dsp/coolmic-dsp.h>) unless stated; cmhip_last_error() has the text.
 *
 * HBM layout: pcm[stream][frame][channel], int16, each stream's slot contiguous
 * and 16-byte aligned (cmhip_batch_stride() samples apart).  Planar float output:
 * f32[stream][channel][frame], planes cmhip_batch_max_frames() apart.
 */
#ifndef COOLMIC_HIP_H
#define COOLMIC_HIP_H

#include <stddef.h>
#include <stdint.h>
#include <coolmic-dsp/vumeter.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cmhip_batch cmhip_batch_t;

/* what a run produces */
#define CMHIP_OUT_PCM      0x0001u   /* materialise the transformed int16 PCM */
#define CMHIP_OUT_F32      0x0002u   /* planar float copy of the transformed PCM */
#define CMHIP_VU           0x0004u   /* accumulate the VU meters */
#define CMHIP_INPLACE      0x0008u   /* PCM output overwrites the input slots (as the reference does) */
#define CMHIP_EQ           0x0010u   /* biquad EQ after map and gain, every channel with state of its own */
#define CMHIP_HOSTPCM      0x0020u   /* PCM slots in pinned host memory the kernels access directly (zero copy):
                                      * for small batches fed block by block, e.g. the per-stream stages */
#define CMHIP_EXTSLOTS     0x0040u   /* no PCM slots of its own: every run names them (cmhip_batch_run_slots) */
#define CMHIP_PLACE_SEARCH 0x0080u   /* at creation, look for a faster physical placement of the two PCM arrays
                                      * (cmhip_batch_placement below).  OFF unless asked for: the search takes
                                      * memory and time for a few per cent of the kernel */

/* synthetic inputs generated on the device */
#define CMHIP_GEN_NULL     0         /* zeros, as snddev "null" */
#define CMHIP_GEN_SINE     1         /* 48-sample sine period, stream s starts at phase 7*s */
#define CMHIP_GEN_NOISE    2         /* per-stream LCG, seed + global stream id */

#define CMHIP_MAX_EQ_SECTIONS 4

typedef struct cmhip_batch_desc {
    int          device;          /* HIP device ordinal */
    unsigned int streams;         /* S >= 1 */
    unsigned int channels;        /* 1..16, shared by the batch */
    unsigned int rate;            /* Hz, reported in results */
    size_t       max_frames;      /* slot capacity per stream, frames */
    unsigned int flags;           /* CMHIP_* outputs */
    void        *hip_stream;      /* hipStream_t to launch on, NULL: own stream */
} cmhip_batch_desc_t;

/* ---- process level ------------------------------------------------------- */
int          cmhip_device_count(void);            /* 0 without a usable GPU */
int          cmhip_device_synchronize(int device); /* everything queued on that device has finished */
int          cmhip_device_mem_info(int device, size_t *free_bytes, size_t *total_bytes); /* hipMemGetInfo */
/* plain device memory for a host without HIP headers of its own (e.g. the destination of
 * cmhip_batch_vu_node_partial for a host that brings its own collective); zero-filled */
void        *cmhip_device_alloc(int device, size_t bytes);        /* NULL on failure */
void         cmhip_device_free(int device, void *p);
int          cmhip_device_read(int device, void *dst_host, const void *src_device, size_t bytes); /* synchronises the device */
const char  *cmhip_last_error(void);              /* per-thread text of the last failure */
const char  *cmhip_version(void);

/* ---- life cycle ---------------------------------------------------------- */
cmhip_batch_t *cmhip_batch_new(const cmhip_batch_desc_t *desc);   /* NULL on failure */
void           cmhip_batch_free(cmhip_batch_t *b);

/* ---- placement of the PCM arrays (CMHIP_PLACE_SEARCH) ---------------------- */
/* On MI355X a kernel that streams one large array in and another out runs 3-5 % faster when the two
 * lie in different stretches of the card's memory; nothing but probing shows which.  A batch created
 * with CMHIP_PLACE_SEARCH (two PCM arrays of its own, >= 256 MiB each) allocates up to five more
 * candidate arrays behind spacer allocations, times its own run on every pair, keeps the fastest pair
 * if it beats the first by 2 % and frees the rest before cmhip_batch_new() returns.  It never asks
 * for more than HALF of the memory hipMemGetInfo reports free (spacers and candidates together;
 * fewer candidates on a fuller card) and stops allocating after 0.3 s.  Without the flag nothing of
 * this happens: two hipMalloc calls, no probe launches. */
typedef struct cmhip_placement {
    int      searched;          /* 1 when the probes ran */
    int      candidates;        /* arrays probed, the first two included (2..7) */
    int      chosen_in;         /* candidate kept as the input array (0 = where hipMalloc first put it) */
    int      chosen_out;        /* candidate kept as the output array (1 = where hipMalloc first put it) */
    int      probe_launches;    /* launches of the batch's kernel the search made */
    double   first_pair_ms;     /* the run on the first pair (median of its probes; no gain, no map) */
    double   best_pair_ms;      /* the run on the fastest other pair */
    double   search_ms;         /* wall time of the whole search */
    uint64_t bytes_requested;   /* spacers + extra candidates the search allocated (all freed again) */
    uint64_t bytes_free_before; /* hipMemGetInfo free when it started */
} cmhip_placement_t;
int cmhip_batch_placement(const cmhip_batch_t *b, cmhip_placement_t *out);

/* ---- parameters (take effect at the next run) ---------------------------- */
/* same meaning and return values as coolmic_transform_set_master_gain
 * (ref: src/transform.c:195-222); stream == -1 addresses every stream */
int cmhip_batch_set_gain(cmhip_batch_t *b, long stream, unsigned int channels, uint16_t scale,
                         const uint16_t *gain);
/* out channel c reads input channel map[c]; NULL = identity */
int cmhip_batch_set_chmap(cmhip_batch_t *b, long stream, const uint8_t *map);
/* nsec biquads, 5 floats each {b0,b1,b2,a1,a2} (a0-normalised); nsec 0 = bypass.
 * Every channel of a stream runs the stream's filter with state of its own, kept across
 * runs; cmhip_batch_eq_reset() zeroes it.  The section count is one for the whole batch:
 * stream -1 sets all streams (and may change the count), a stream >= 0 must keep it. */
int cmhip_batch_set_eq(cmhip_batch_t *b, long stream, unsigned int nsec, const float *coef);
int cmhip_batch_eq_reset(cmhip_batch_t *b, long stream);
/* RBJ designs on the host in double, cast to float: kind 0 low shelf, 1 peaking, 2 high
 * shelf (shelf slope 1).  coef receives 5 floats. */
void cmhip_design_biquad(int kind, double rate, double freq, double gain_db, double q,
                         float *coef);

/* ---- geometry and raw device pointers ------------------------------------ */
size_t  cmhip_batch_stride(const cmhip_batch_t *b);       /* samples between stream slots */
size_t  cmhip_batch_max_frames(const cmhip_batch_t *b);
void   *cmhip_batch_dev_in(cmhip_batch_t *b);             /* int16 [S][stride] */
void   *cmhip_batch_dev_out(cmhip_batch_t *b);            /* int16 [S][stride] (== in when INPLACE) */
void   *cmhip_batch_dev_f32(cmhip_batch_t *b);            /* float [S][C][max_frames] or NULL */
void   *cmhip_batch_hip_stream(cmhip_batch_t *b);         /* the hipStream_t launches go to */

/* ---- moving PCM (asynchronous on the batch's stream) ---------------------- */
int cmhip_batch_upload(cmhip_batch_t *b, unsigned int stream, const int16_t *pcm, size_t frames);
int cmhip_batch_download(cmhip_batch_t *b, unsigned int stream, int16_t *pcm, size_t frames);
/* whole-batch forms: `host` mirrors the device layout, int16 [S][cmhip_batch_stride()], and
 * one copy moves every slot; asynchronous on the batch's stream (cmhip_batch_sync() to wait).
 * Pinned memory from cmhip_host_alloc() gives full PCIe speed and real asynchrony. */
int   cmhip_batch_upload_all(cmhip_batch_t *b, const int16_t *host, size_t frames);
int   cmhip_batch_download_all(cmhip_batch_t *b, int16_t *host, size_t frames);
void *cmhip_host_alloc(size_t bytes);             /* NULL on failure */
/* pinned and mapped into the device: the host uses the returned pointer, kernels *device_ptr.
 * (_on: the device whose kernels will use it -- a process that drives several GPUs; the plain form takes
 * whichever device is current in the calling thread) */
void *cmhip_host_alloc_mapped(size_t bytes, void **device_ptr);
void *cmhip_host_alloc_mapped_on(int device, size_t bytes, void **device_ptr);
void  cmhip_host_free(void *p);
/* reads an input slot back (generated or uploaded PCM); synchronises */
int cmhip_batch_download_input(cmhip_batch_t *b, unsigned int stream, int16_t *pcm, size_t frames);
int cmhip_batch_download_f32(cmhip_batch_t *b, unsigned int stream, unsigned int channel,
                             float *dst, size_t frames);
/* fill every stream's input slot on the device; stream s of this batch is global
 * stream first_global + s*global_step (round-robin shards use first=rank, step=N) */
int cmhip_batch_generate(cmhip_batch_t *b, int mode, uint32_t seed, size_t frames,
                         uint64_t first_global, uint64_t global_step, uint64_t frame_offset);

/* ---- the hot path --------------------------------------------------------- */
/* process `frames` frames of every stream (frames_per_stream, if not NULL, gives each
 * stream its own count <= frames; host array of S entries, pageable or pinned, free on return:
 * the batch copies it into a small ring of pinned blocks it owns, so a host loop may refill ONE
 * array for the next run at once.  The fifth of five runs with frames_per_stream queued back to
 * back may wait ON THE HOST until the first one's counts have been copied on the stream).
 * Asynchronous.  cmhip_batch_run_slots takes its counts the same way.
 * A run with the equaliser (CMHIP_EQ with sections set) writes nothing past a stream's count: samples from
 * count * channels on in its PCM slot (in place: the input there) and frames from count on in its float planes
 * keep what they held. */
int cmhip_batch_run(cmhip_batch_t *b, size_t frames, const uint32_t *frames_per_stream);
/* the same pass over PCM arrays named for this run: device-accessible memory laid out like the
 * batch's own, int16 [S][cmhip_batch_stride()] (slots_out NULL exactly when the batch writes no
 * PCM, == slots_in for CMHIP_INPLACE).  With pinned, device-mapped host memory
 * (cmhip_host_alloc_mapped) the kernel moves the block over PCIe itself, and a host can rotate
 * several sets: sources fill one, readers drain another, a third is on the GPU. */
int cmhip_batch_run_slots(cmhip_batch_t *b, size_t frames, const uint32_t *frames_per_stream,
                          const void *slots_in, void *slots_out);
int cmhip_batch_sync(cmhip_batch_t *b);

/* ---- VU windows ------------------------------------------------------------ */
/* result of one stream's current window, then reset of that window -- the contract of
 * coolmic_vumeter_result (ref: src/vumeter.c:189-218), INVAL while it holds no frame */
int cmhip_batch_vu_result(cmhip_batch_t *b, unsigned int stream, coolmic_vumeter_result_t *out);
/* all streams at once: out[S], rc[S] (rc may be NULL); one device round trip */
int cmhip_batch_vu_results(cmhip_batch_t *b, coolmic_vumeter_result_t *out, int *rc);
/* two-phase form that overlaps with the next run: snapshot copies the accumulators of
 * every stream to pinned host memory and opens a new window on the device (async);
 * collect waits for that copy and finishes the dB values on the host */
int cmhip_batch_vu_snapshot(cmhip_batch_t *b);
int cmhip_batch_vu_collect(cmhip_batch_t *b, coolmic_vumeter_result_t *out, int *rc);
/* collect in two halves, for hosts that close a window every block of a few thousand frames: begin waits for
 * the oldest snapshot and hands its windows to the helper threads, end returns when out[] and rc[] (which
 * must stay valid until then) are complete; between the two the caller queues its next run.  One at a time;
 * the snapshot keeps its place among the three that may be pending (cmhip_batch_vu_snapshot returns
 * COOLMIC_ERROR_BUSY for a fourth) until end. */
int cmhip_batch_vu_collect_begin(cmhip_batch_t *b, coolmic_vumeter_result_t *out, int *rc);
int cmhip_batch_vu_collect_end(cmhip_batch_t *b);
int cmhip_batch_vu_reset(cmhip_batch_t *b, long stream);
/* Where the dB values of a snapshot are finished.  CMHIP_VU_FINISH_HOST (how every batch starts): the snapshot
 * carries raw sums and keys, the collect runs the reference's arithmetic on them with the host's libm -- results are
 * bit-equal to coolmic_vumeter_result().  CMHIP_VU_FINISH_DEVICE: the snapshot's kernel runs the same sequence of
 * double operations itself (integer mean, sqrt, / 32768, log10, * 20, capped at 0) and the collect only copies: no
 * libm call on the host, thousands of windows per block cost the host no arithmetic.  The trade: the device's log10
 * is another implementation than the host's, so channel_power / global_power may differ from the host finish in
 * their last bits (measured on MI355X against glibc 2.35: at most 2 units in the last place); -inf for a silent window, 0.0 at full scale, every
 * peak, frames, rate, channels and every rc are exactly the same.
 * The mode governs cmhip_batch_vu_snapshot and what collects it: cmhip_batch_vu_collect, _collect_begin / _end and
 * cmhip_batch_vu_results.  Out of its reach, always finished on the host and bit-equal: cmhip_batch_vu_result (one
 * stream), the per-launch windows of a meter behind a tee, cmhip_node_finish.
 * COOLMIC_ERROR_INVAL for a batch without CMHIP_VU or an unknown value, COOLMIC_ERROR_BUSY while a snapshot is
 * pending or a collect is under way.  The getter returns the mode, or a negative error. */
#define CMHIP_VU_FINISH_HOST   0
#define CMHIP_VU_FINISH_DEVICE 1
int cmhip_batch_vu_set_finish(cmhip_batch_t *b, int where);
int cmhip_batch_vu_get_finish(const cmhip_batch_t *b);
/* raw accumulators of a stream (synchronises): power[16], peak[16], frames */
int cmhip_batch_vu_raw(cmhip_batch_t *b, unsigned int stream, int64_t *power, int16_t *peak,
                       uint64_t *frames);

/* ---- true peak (ITU-R BS.1770 Annex 2 / EBU R128), opt-in ------------------- */
/* The maximum of the 4x oversampled TRANSFORMED stream (after channel map, gain and saturation: the samples the VU
 * window accounts and CMHIP_OUT_PCM writes), by the 48-tap polyphase FIR whose int16 coefficients, in units of
 * 2^-13, cmhip_tp_coefficients() returns: y_p[n] = sum_{k<12} H[p][k] * x[n-k], p = 0..3, in exact int32.  A window's
 * value per channel is max |y_p[n]| over p and the frames accounted since it opened; 268435456 (2^28) is full scale.
 * The filter belongs to the stream, not to the window: its history (the last 11 transformed frames per channel) is
 * zero when true peak is turned on and after cmhip_batch_tp_reset, and is kept across runs AND across window closes;
 * a change of gain or map does not touch it.  A stream that gets 0 frames in a run keeps history and window.
 * The filter runs 4x whatever `rate` says: Annex 2's lower factors for rates of 96 kHz and above are not applied.
 *
 * cmhip_batch_set_true_peak(b, 1), between runs (it waits for the batch's stream), allocates the state on first use
 * and opens empty windows with zero history; from then on every cmhip_batch_run / _run_slots launches the true-peak
 * kernel on the batch's stream AHEAD of the block kernel (it reads the run's input slots and applies map and gain
 * itself).  (b, 0) stops that and discards windows and history.  True peak of the equaliser's result is not
 * measured: COOLMIC_ERROR_INVAL while the batch's equaliser has sections, and cmhip_batch_set_eq with nsec > 0
 * returns COOLMIC_ERROR_INVAL while true peak is on (nsec == 0 stays allowed).
 * The result calls follow their VU counterparts: COOLMIC_ERROR_INVAL with `out` left alone for a window without a
 * frame (per stream in rc[] for _results, rc may be NULL) and for a batch without true peak; the window is closed on
 * success, by these calls only -- the true-peak windows are independent of the VU windows (ask for both between the
 * same two runs for aligned windows).  One device round trip serves all streams; the dBTP doubles are finished on
 * the host with cmhip_tp_dbtp.  cmhip_batch_tp_reset clears window AND history (stream -1: all).
 * cmhip_batch_timing keeps bracketing the block kernel only. */
int    cmhip_batch_set_true_peak(cmhip_batch_t *b, int on);
int    cmhip_batch_get_true_peak(const cmhip_batch_t *b);     /* 0 / 1, negative error */
int    cmhip_batch_tp_result(cmhip_batch_t *b, unsigned int stream, coolmic_truepeak_result_t *out);
int    cmhip_batch_tp_results(cmhip_batch_t *b, coolmic_truepeak_result_t *out, int *rc);
int    cmhip_batch_tp_reset(cmhip_batch_t *b, long stream);
/* the host finish, no device needed: 20. * log10((double)peak / 268435456.) -- not capped at 0, -inf for 0 */
double cmhip_tp_dbtp(uint32_t peak);
/* the filter, no device needed: H[0..3] in order, 12 taps each */
void   cmhip_tp_coefficients(int16_t h[48]);

/* ---- phase correlation / balance, opt-in ------------------------------------- */
/* The needle between -1 and +1 that tells whether a stereo programme survives a mono sum, and the level balance of
 * the two legs, for up to CMHIP_CORR_MAX_PAIRS channel pairs per stream.  Specified, and held, to the bit:
 *
 * Signal.  The TRANSFORMED stream (after channel map, gain and saturation: the samples the VU window accounts and
 *   CMHIP_OUT_PCM writes, exactly as for true peak).  The pass reads the run's input slots and transforms them itself,
 *   so an in-place batch needs nothing special.
 * Pairs.  A batch has 1 to CMHIP_CORR_MAX_PAIRS pairs (a, b) of transformed channels, a != b, both below `channels`,
 *   the same for all streams; the default is the single pair (0, 1).  cmhip_batch_corr_set_pairs replaces them, with
 *   correlation on or off, but only while every window is empty (COOLMIC_ERROR_BUSY otherwise: result or reset first).
 *   COOLMIC_ERROR_INVAL for n == 0, n > 8, a == b or a channel out of range; nothing is changed then.  A mono batch
 *   cannot be metered: cmhip_batch_set_correlation(b, 1) returns COOLMIC_ERROR_INVAL for it.
 * Window sums per stream and pair, over the frames accounted since the window opened, in exact integers:
 *       energy_a = sum x_a^2  (uint64)      energy_b = sum x_b^2  (uint64)      cross = sum x_a * x_b  (int64)
 *   One frame contributes at most 2^30 to each (-32768 squared is exactly 2^30; the cross term lies in
 *   [-2^30 + 2^15, 2^30]), so a window is exact up to 2^33 frames -- 49 hours at 48 kHz.  The bound is not enforced:
 *   close windows more often than that.  Integer sums do not depend on the order they are merged in, nor on how the
 *   stream was cut into runs.  A stream that gets 0 frames in a run keeps its window.
 * Host finish, in double, in this order, no device needed:
 *   cmhip_corr_value(ea, eb, x): 0.0 when ea == 0 || eb == 0; otherwise (double)x / sqrt((double)ea * (double)eb),
 *     clamped to [-1.0, 1.0].  Conversion, product, square root and quotient are each correctly rounded in IEEE 754,
 *     so the value is one fixed double.
 *   cmhip_corr_balance_db(ea, eb): 0.0 when both are 0; otherwise 10.0 * log10((double)ea / (double)eb), which is
 *     -inf for ea == 0 and +inf for eb == 0.  Positive: a is the louder leg.
 *
 * cmhip_batch_set_correlation(b, 1), between runs (it waits for the batch's stream), allocates the [S][8][3] 64-bit
 * sums on first use and opens empty windows; from then on every cmhip_batch_run / _run_slots launches the correlation
 * kernel on the batch's stream AHEAD of the block kernel, beside the true-peak and loudness passes when those are on
 * too.  (b, 0) stops that and discards the windows; the pairs are kept.  Correlation of the equaliser's result is not
 * measured: COOLMIC_ERROR_INVAL while the batch's equaliser has sections, and cmhip_batch_set_eq with nsec > 0
 * returns COOLMIC_ERROR_INVAL while correlation is on (nsec == 0 stays allowed).
 * The result calls follow their true-peak counterparts: COOLMIC_ERROR_INVAL with `out` left alone for a window
 * without a frame (per stream in rc[] for _results, rc may be NULL) and for a batch without correlation; the window
 * is closed on success, by these calls only -- the windows are independent of the VU, true-peak and loudness windows.
 * One device round trip serves all streams, the sums are cleared on the stream behind it.  Entries of a result at
 * and beyond `pairs` are zero.  cmhip_batch_corr_reset clears windows (stream -1: all).
 * cmhip_batch_timing keeps bracketing the block kernel only.  The pass is queued, and its frames are counted, before
 * the block kernel is launched: after a cmhip_batch_run that returns an error, correlation (like true peak) may or
 * may not hold that run's frames -- reset the stream's meters before trying the run again. */
#define CMHIP_CORR_MAX_PAIRS 8
int    cmhip_batch_set_correlation(cmhip_batch_t *b, int on);
int    cmhip_batch_get_correlation(const cmhip_batch_t *b);   /* 0 / 1, negative error */
int    cmhip_batch_corr_set_pairs(cmhip_batch_t *b, unsigned int n, const unsigned char pairs[][2]);
int    cmhip_batch_corr_result(cmhip_batch_t *b, unsigned int stream, coolmic_correlation_result_t *out);
int    cmhip_batch_corr_results(cmhip_batch_t *b, coolmic_correlation_result_t *out, int *rc);
int    cmhip_batch_corr_reset(cmhip_batch_t *b, long stream);
double cmhip_corr_value(uint64_t energy_a, uint64_t energy_b, int64_t cross);
double cmhip_corr_balance_db(uint64_t energy_a, uint64_t energy_b);

/* ---- spectrum, opt-in ---------------------------------------------------------- */
/* Where in frequency the energy lies: band levels from a Hann-windowed FFT in fixed point, for up to
 * CMHIP_SPEC_MAX_CHANNELS channels per stream and up to CMHIP_SPEC_MAX_BANDS bands.  Specified, and held, to the bit:
 *
 * Signal.  The TRANSFORMED stream (after channel map, gain and saturation), exactly as for true peak and correlation.
 *   The pass reads the run's input slots and transforms them itself, so an in-place batch needs nothing special.
 * Geometry.  N = 2^n frames per block, n = fft_log2 in 8..12 (default 10), hop H = N / 2.  Block j of a stream covers
 *   its frames [j H, j H + N), counted from 0 where the meter was turned on or the stream last reset, and is computed
 *   in the run in which its last frame arrives.  Blocks are anchored to the stream's position, so the result does not
 *   depend on how the stream is cut into runs, per-stream counts included.  A stream that gets 0 frames in a run
 *   keeps everything.
 * Channels.  1 to CMHIP_SPEC_MAX_CHANNELS distinct transformed channels, the same for all streams; the default is
 *   channel 0, and channel 1 too where the batch has one.  Mono batches are allowed.
 * Window.  win[i] = min(32767, rint(32768 * 0.5 * (1 - cos(2 pi i / N)))) as int16, the upper half mirrored from the
 *   lower (win[N - i] = win[i]); cmhip_spec_window returns it.  v[i] = x[i] * win[i], exact in int32, |v| < 2^30.
 * Twiddles.  Wr[k] = llround(2^30 cos(2 pi k / N)), Wi[k] = llround(-2^30 sin(2 pi k / N)) for k < N / 2 as int32,
 *   one octant computed and mirrored: k = 0 is exactly (2^30, 0), k = N / 4 exactly (0, -2^30), Wr[N / 4 - k] =
 *   -Wi[k], W[k + N / 4] = (Wi[k], -Wr[k]).  cmhip_spec_twiddles returns them; a model takes them from there.
 * Transform.  Radix-2 decimation in time: z[bitrev(i)] = (v[i], 0), then for stage s = 1..n with m = 2^s, for
 *   a = z[g m + j], b = z[g m + j + m / 2] and W = W[j N / m]:
 *       Pr = br Wr - bi Wi        Pi = br Wi + bi Wr                                  (exact in int64)
 *       a'r = (ar 2^30 + Pr + 2^30) >> 31       b'r = (ar 2^30 - Pr + 2^30) >> 31     (and the imaginary parts likewise)
 *   with an arithmetic shift of the exact int64 sum: one rounding per butterfly output, a factor 1/2 per stage, so X
 *   is the DFT of v divided by N.  |a'| <= (|a| + |b|) / 2 + 1 bounds every component by 2^30 + n (int32 storage
 *   leaves 2^31; measured components stay below 2^29) and every int64 intermediate by 2^63.  An implementation may
 *   fuse stages, skip the trivial twiddles (those entries are exact) or use another radix that reproduces every
 *   stage's rounded values; nothing else may differ.
 * Power and bands.  p[k] = (uint64)(re^2 + im^2) >> 16 for the bins k = 0..N / 2.  A band table has nb in
 *   1..CMHIP_SPEC_MAX_BANDS bands with edges 0 <= e[0] < e[1] < ... < e[nb] <= N / 2 + 1; band b is the sum of p[k]
 *   over e[b] <= k < e[b + 1].  The default table is the bin octaves 1, 2, 4, ..., N / 2, N / 2 + 1: n bands, no DC.
 *   A window's value per stream, channel and band is the uint64 sum over the blocks completed since it opened; a
 *   block that straddles a window's close belongs to the window in which it completes.  One block's total over all
 *   bins is at most 2^42.4 (DC or Nyquist at -32768), so a window is exact for 2^21 blocks -- 6 hours at N = 1024
 *   and 48 kHz.  The bound is not enforced, as with correlation.
 * Band design, no device needed.  cmhip_spec_design_bands(rate, fft_log2, per_octave, edges) gives fractional-octave
 *   bands around 1 kHz, per_octave in 1..3: with f(i) = 1000.0 * pow(2.0, (2 i - 1) / (2.0 * per_octave)) for every
 *   integer i, the bin edge is ceil(f(i) * (double)N / (double)rate) clamped to 1..N / 2 + 1, and the table is the
 *   strictly ascending list of the distinct values (bands narrower than a bin merge upwards, the DC bin is left out;
 *   the table always starts at 1 and ends at N / 2 + 1).  Returns the band count; COOLMIC_ERROR_INVAL for more than
 *   32 bands, rate 0 or an argument out of range.
 * Host finish, no device needed.  cmhip_spec_db(power, blocks) = 10.0 * log10((double)power / ((double)blocks *
 *   1649267441664.0)) -- the constant is 1.5 * 2^40 -- which is -inf for power 0; 0.0 for blocks 0.  0 dB is a
 *   full-scale sine whose three main-lobe bins lie in one band.
 * State.  Per stream and selected channel the last N - 1 transformed samples, in two slots that the runs alternate
 *   between (a run reads one and writes the other, so a run longer than N overwrites nothing a block still reads).
 *   The state belongs to the stream, not to the window: closing a window leaves it alone, and so does a change of
 *   gain or map.  cmhip_batch_spec_reset clears window, state and position (stream -1: all).
 *
 * cmhip_batch_spec_configure(b, fft_log2, nb, edges, nch, channels) sets the geometry, only while the meter is off
 * (COOLMIC_ERROR_BUSY otherwise): nb == 0 takes the default table of that fft_log2 (edges may be NULL then), nch == 0
 * the default channels (channels may be NULL then).  COOLMIC_ERROR_FAULT for NULL otherwise, COOLMIC_ERROR_INVAL for
 * fft_log2 outside 8..12, a bad band table, more than 8 channels, a channel twice or out of range; nothing changes
 * then.  cmhip_batch_set_spectrum(b, 1), between runs (it waits for the batch's stream), allocates windows, state and
 * tables for the geometry in force and opens empty windows at position 0; from then on every cmhip_batch_run /
 * _run_slots launches the spectrum kernel on the batch's stream AHEAD of the block kernel, beside the other meters'
 * passes.  (b, 0) stops that and discards windows and state; the geometry is kept.  The spectrum of the equaliser's
 * result is not measured: COOLMIC_ERROR_INVAL while the batch's equaliser has sections, and cmhip_batch_set_eq with
 * nsec > 0 returns COOLMIC_ERROR_INVAL while the meter is on.
 * The result calls follow correlation's: COOLMIC_ERROR_INVAL with `out` left alone and the window KEPT for a window
 * without a completed block (per stream in rc[] for _results, rc may be NULL), and for a batch without the meter; a
 * window is closed on success, by these calls only.  `frames` of a result counts the frames since the window opened.
 * The pass is queued, and its frames are counted, before the block kernel is launched: see correlation on a run that
 * returns an error. */
#define CMHIP_SPEC_MAX_CHANNELS 8
#define CMHIP_SPEC_MAX_BANDS 32
int    cmhip_batch_set_spectrum(cmhip_batch_t *b, int on);
int    cmhip_batch_get_spectrum(const cmhip_batch_t *b);      /* 0 / 1, negative error */
int    cmhip_batch_spec_configure(cmhip_batch_t *b, unsigned int fft_log2, unsigned int nb, const uint16_t *edges,
                                  unsigned int nch, const unsigned char *channels);
int    cmhip_batch_spec_result(cmhip_batch_t *b, unsigned int stream, coolmic_spectrum_result_t *out);
int    cmhip_batch_spec_results(cmhip_batch_t *b, coolmic_spectrum_result_t *out, int *rc);
int    cmhip_batch_spec_reset(cmhip_batch_t *b, long stream);
int    cmhip_spec_window(unsigned int fft_log2, int16_t *win);                 /* win[N] */
int    cmhip_spec_twiddles(unsigned int fft_log2, int32_t *wr, int32_t *wi);   /* wr[N / 2], wi[N / 2] */
int    cmhip_spec_design_bands(unsigned int rate, unsigned int fft_log2, unsigned int per_octave, uint16_t edges[33]);
double cmhip_spec_db(uint64_t power, uint64_t blocks);

/* ---- signal watch: dead air, clipping, DC offset; opt-in ---------------------- */
/* Which streams are dead and for how long, which are clipped, which carry DC: run-length and sum statistics of the
 * stream, exact in integers and independent of how a stream is cut into runs.  Specified, and held, to the bit:
 *
 * Signal.  The TRANSFORMED stream (after channel map, gain and saturation), exactly as for true peak and correlation.
 *   The pass reads the run's input slots and transforms them itself, so an in-place batch needs nothing special.  All
 *   channels of the stream are covered, C = 1..16; mono is allowed.
 * Parameters, per batch and the same for all streams; cmhip_batch_watch_configure(b, quiet, rail, clip_run) sets them:
 *   quiet in 0..32767 (default 32, -60.2 dBFS): a sample x is QUIET iff -quiet <= x <= quiet.
 *   rail in 1..32767 (default 32767): a sample is AT THE RAIL iff x >= rail || x <= -rail; -32768 is at every rail.
 *   clip_run = K in 1..16 (default 3).
 *   Out of range: COOLMIC_ERROR_INVAL, nothing changes.  Configuring is allowed with the watch on or off, but only
 *   while every window is empty (COOLMIC_ERROR_BUSY otherwise: result or reset first).  A successful configure also
 *   clears every stream's run state (below): the predicates have changed.
 *   cmhip_watch_level(db) = lround(32768 * 10^(db / 20)) clamped to 0..32767, a host helper that needs no device
 *   (-60 dB gives 33, 0 dB and above 32767, -inf 0).
 * Predicates, per frame n -- the stream's absolute frame index since its state was last cleared:
 *   Q(c, n): channel c is quiet.   R(c, n): channel c is at the rail.   D(n): every channel is quiet (dead air).
 *   For each predicate P the run length is l_P(n) = l_P(n - 1) + 1 if P(n), else 0, with l_P(-1) = 0.  l continues
 *   across runs and across windows: it is the STATE, a uint64 per stream and predicate, C + C + 1 of them per stream.
 * Window: the frames accounted since the last result or reset.
 *   dead_frames, quiet_frames[c], clip_samples[c]     the number of window frames with D, Q(c), R(c)
 *   dead_longest, quiet_longest[c], clip_longest[c]   max of l(n) over the window's frames
 *   dead_current, quiet_current[c]                    l at the window's last frame: "silent for this long, now"
 *   clip_events[c]                                    the number of window frames with l_R(c, n) == K
 *   sum[c]                                            sum of x_c as int64; |sum| <= 2^15 * frames
 *   A run that began before the window counts in *_longest with its full length, but only if it continues into the
 *   window: a window whose first frame is not P takes nothing from the state for that predicate.  clip_events counts
 *   each run once, at the frame where it reaches K, wherever cuts and windows fall.
 *   Host finish: dc[c] = (double)sum[c] / (double)frames / 32768.0 -- conversions and both quotients correctly
 *   rounded, one fixed double.
 *   Nothing depends on the order tiles finish in, on the tile size, or on how the stream is cut into runs.  A stream
 *   that gets 0 frames in a run keeps its window and state.
 *
 * cmhip_batch_set_watch(b, 1), between runs (it waits for the batch's stream), allocates the windows and the state on
 * first use and opens empty windows with cleared state; from then on every cmhip_batch_run / _run_slots launches the
 * watch's two kernels on the batch's stream AHEAD of the block kernel, beside the other meters' passes: a tile pass
 * that writes one run-length summary per stream, tile and predicate into a scratch array (grown on need) and adds the
 * channel sums, and a fold that walks every stream's summaries in stream order.  (b, 0) stops that and discards windows
 * and state; the parameters are kept.  The equaliser's result is not measured: COOLMIC_ERROR_INVAL while the batch's
 * equaliser has sections, and cmhip_batch_set_eq with nsec > 0 returns COOLMIC_ERROR_INVAL while the watch is on.
 * cmhip_batch_watch_result / _results close windows and KEEP the state; one device round trip serves all streams.
 * They return COOLMIC_ERROR_INVAL, with `out` left alone, for a window without a frame (per stream in rc[] for
 * _results, rc may be NULL) and for a batch without the watch.  cmhip_batch_watch_reset clears window and state
 * (stream -1: all).  The pass is queued, and its frames are counted, before the block kernel is launched: see
 * correlation on a run that returns an error. */
int    cmhip_batch_set_watch(cmhip_batch_t *b, int on);
int    cmhip_batch_get_watch(const cmhip_batch_t *b);         /* 0 / 1, negative error */
int    cmhip_batch_watch_configure(cmhip_batch_t *b, unsigned int quiet, unsigned int rail, unsigned int clip_run);
int    cmhip_batch_watch_result(cmhip_batch_t *b, unsigned int stream, coolmic_watch_result_t *out);
int    cmhip_batch_watch_results(cmhip_batch_t *b, coolmic_watch_result_t *out, int *rc);
int    cmhip_batch_watch_reset(cmhip_batch_t *b, long stream);
unsigned int cmhip_watch_level(double db);

/* ---- programme loudness (ITU-R BS.1770 / EBU R128), opt-in -------------------- */
/* Momentary, short-term and gated integrated loudness of the TRANSFORMED stream (after channel map, gain and
 * saturation: the samples the VU window accounts, as for true peak).  The arithmetic is specified to the bit:
 *
 * Signal.  u = (double)x / 32768.0 (exact).
 * Filter.  Two biquad sections in double, Direct Form I, history zero at enable and reset; every product and every
 *   sum rounded once (no fused multiply-add), double denormals kept:
 *       f = (b0*u + b1*u1) + b2*u2      y = (f - a2*y2) - a1*y1      (then u2=u1, u1=u, y2=y1, y1=y)
 *   Section 2 takes section 1's y as its u; its numerator is exactly 1, -2, 1.
 * Coefficients.  cmhip_loud_coefficients(rate, c) returns {b0,b1,b2,a1,a2} twice, from libm's tan and pow in exactly
 *   this order:
 *     stage 1: f0=1681.974450955533  G=3.999843853973347  Q=0.7071752369554196
 *              K=tan(M_PI*f0/rate)  Vh=pow(10.0,G/20.0)  Vb=pow(Vh,0.4996667741545416)  a0=1.0+K/Q+K*K
 *              b0=(Vh+Vb*K/Q+K*K)/a0  b1=2.0*(K*K-Vh)/a0  b2=(Vh-Vb*K/Q+K*K)/a0  a1=2.0*(K*K-1.0)/a0
 *              a2=(1.0-K/Q+K*K)/a0
 *     stage 2: f0=38.13547087602444  Q=0.5003270373238773  K=tan(M_PI*f0/rate)  a0=1.0+K/Q+K*K
 *              b = 1.0, -2.0, 1.0   a1=2.0*(K*K-1.0)/a0   a2=(1.0-K/Q+K*K)/a0
 *   At 48000 Hz these are the table values of BS.1770-4 to 9e-16.  Loudness needs 8000 <= rate <= 384000:
 *   cmhip_batch_set_loudness returns COOLMIC_ERROR_INVAL for a batch of any other rate.
 * Sub-blocks.  L = (rate + 5) / 10 frames (100 ms), counted per stream from enable or reset.  Per channel e += y*y,
 *   product and sum each rounded once, sequential in frame order, from 0.0 at each sub-block's start.  A completed
 *   sub-block's e per channel is what the device produces (cmhip_batch_loud_raw).  A stream that gets 0 frames in a
 *   run keeps everything, and the sums do not depend on how the stream was cut into runs.
 * Host finish, all in double, in this order:
 *   z_j = (sum over c ascending of w_c * e_c,j, each product rounded, the sum from 0.0) / (double)L
 *   lufs(v) = -0.691 + 10.0*log10(v), -inf for v == 0                                     (cmhip_loud_lufs)
 *   momentary  = lufs((((z[n-4]+z[n-3])+z[n-2])+z[n-1]) * 0.25), -inf while n < 4
 *   short-term = lufs((z[n-30] + ... + z[n-1], in that order) / 30.0), -inf while n < 30
 *   integrated (cmhip_loud_integrate): blocks B_i = (((z[i-3]+z[i-2])+z[i-1])+z[i]) * 0.25 for i >= 3; keep those
 *     with lufs(B_i) > -70.0; relative threshold = lufs(mean of the kept) - 10.0; the result is lufs(mean of the kept
 *     B_i with lufs(B_i) > threshold), and `gated` counts those.  A mean is the sum in ascending i from 0.0, divided
 *     by (double)count.  With nothing kept by the first gate both values are -inf and gated is 0; with nothing kept
 *     by the second, integrated is -inf.
 *   Default weight w_c is 1.0 for every channel; the library does not know layouts.  A 5.1 host in L R C LFE Ls Rs
 *   order sets {1,1,1,0,1.41,1.41}.
 *
 * cmhip_batch_set_loudness(b, 1), between runs (it waits for the batch's stream), allocates the state on first use
 * (COOLMIC_ERROR_NOMEM when that fails; the batch stays usable) and opens every stream with zero history, no frames
 * and the weights it had (1.0 at first); from then on every cmhip_batch_run / _run_slots launches the loudness
 * kernel on the batch's stream AHEAD of the block kernel, beside the true-peak pass when that is on too.  (b, 0)
 * stops that and discards everything but the weights.  Loudness of the equaliser's result is not measured: the two
 * exclude each other with COOLMIC_ERROR_INVAL both ways round, nsec == 0 stays allowed.
 * The device keeps a ring of completed sub-block sums; the host knows every run's counts and drains the ring (a
 * stream synchronisation and one copy) before a run that could overflow it and at every result call, appending one
 * z_j -- 8 bytes per 100 ms and stream, until reset -- to the stream's array.
 * Results are NOT destructive: loudness integrates until cmhip_batch_loud_reset (stream -1: all), which clears
 * history, the open sub-block and the host's arrays.  A stream without a frame reports zeros and -inf with
 * COOLMIC_ERROR_NONE; rc[] of _results (may be NULL) is COOLMIC_ERROR_NONE for every stream.
 * cmhip_batch_loud_set_weights (stream -1: all): COOLMIC_ERROR_BUSY while a named stream holds completed sub-blocks
 * (reset first), COOLMIC_ERROR_INVAL for a negative or non-finite weight; nothing is changed then.
 * cmhip_batch_loud_raw: the per-channel sums e of the trailing min(cap, 30) complete sub-blocks, oldest first, into
 * sums[i * channels + c]; *returned: how many; *completed: the stream's complete sub-blocks in all (both may be NULL).
 * NULL is COOLMIC_ERROR_FAULT; a stream out of range or a batch without loudness COOLMIC_ERROR_INVAL.
 * cmhip_batch_timing keeps bracketing the block kernel only.  The pass is queued, and its frames are counted, before
 * the block kernel is launched: after a cmhip_batch_run that returns an error, loudness (like true peak) may or may
 * not hold that run's frames -- reset the stream's meters before trying the run again. */
int    cmhip_batch_set_loudness(cmhip_batch_t *b, int on);
int    cmhip_batch_get_loudness(const cmhip_batch_t *b);      /* 0 / 1, negative error */
int    cmhip_batch_loud_set_weights(cmhip_batch_t *b, long stream, const double *w /* [channels] */);
int    cmhip_batch_loud_result(cmhip_batch_t *b, unsigned int stream, coolmic_loudness_result_t *out);
int    cmhip_batch_loud_results(cmhip_batch_t *b, coolmic_loudness_result_t *out, int *rc);
int    cmhip_batch_loud_raw(cmhip_batch_t *b, unsigned int stream, double *sums /* [cap][channels] */, size_t cap,
                            size_t *returned, unsigned long long *completed);
int    cmhip_batch_loud_reset(cmhip_batch_t *b, long stream);
/* host only, no device needed.  _coefficients: c == NULL does nothing; a rate of 0 gives non-finite values.
 * _integrate: any of the three results may be NULL; z == NULL with n > 0 is COOLMIC_ERROR_FAULT. */
void   cmhip_loud_coefficients(unsigned int rate, double c[10]);
double cmhip_loud_lufs(double mean_square);
int    cmhip_loud_integrate(const double *z, size_t n, double *integrated, double *threshold, size_t *gated);

/* ---- sample-rate conversion, an object of its own beside the batch ------------- */
/* A resampler converts rate_in to rate_out for S streams of C interleaved int16 channels by a rational polyphase FIR
 * in exact integers.  The signal is the raw int16 the caller hands in: no gain and no map, the batch does those.
 *
 * Arithmetic.  g = gcd(rate_in, rate_out), L = rate_out / g, M = rate_in / g; a table H[L][T] of int16 coefficients
 *   in units of 2^-14 (unity = 16384).  Output frame m of a stream, counted from creation or reset, reads input frame
 *   n = floor(m*M / L) with phase p = (m*M) mod L, per channel:
 *       acc  = sum_{k<T} H[p][k] * x[n-k]            exact in int32
 *       y[m] = saturate_int16((acc + 8192) >> 14)    arithmetic shift (floor)
 *   x[i] for i < 0 is the stream's history: zero at creation and after cmhip_src_reset.
 * Table validity (designed or supplied): L, M in 1..640 and L != M; T even, in 2..192; every phase has
 *   sum_k |H[p][k]| <= 65535.  Then |acc + 8192| <= 65535*32768 + 8192 < 2^31: int32 never overflows and the result
 *   does not depend on the order of summation.  Anything else is COOLMIC_ERROR_INVAL.
 * Counts.  After N input frames in all a stream has produced K(N) = ceil(N*L / M) output frames (output m exists
 *   once input floor(m*M/L) does); a run of F frames produces K(N+F) - K(N), at most floor(F*L/M) + 1.  Everything is
 *   periodic -- M inputs give exactly L outputs -- so a stream's state is r = N mod M and its last T-1 input frames
 *   per channel, and nothing overflows however long it runs.  A stream that gets 0 frames in a run keeps everything;
 *   the concatenated output does not depend on how the stream was cut into runs.
 *   cmhip_src_out_frames(L, M, r, F) = ceil((r+F)*L / M) - ceil(r*L / M) is that count.
 * The designed table (cmhip_src_design, host only, double precision, in this order): T = 32 when L > M, else
 *   32 * ceil(M/L); N = L*T, fc = 0.92 * 0.5 / max(L, M); for i in 0..N-1 with x = i - (N-1)/2:
 *       w = I0(7.5 * sqrt(max(0, 1 - (x / (N/2))^2))) / I0(7.5)          h[i] = 2*fc * sinc(2*fc*x) * w * L
 *   sinc(t) = sin(pi t) / (pi t), 1 at t = 0; I0 from its power series sum ((x/2)^k / k!)^2, summed until a term no
 *   longer changes the sum.  H[p][k] = h[k*L + p]; every phase is divided by its own sum, multiplied by 16384 and
 *   rounded with rint, and the difference between 16384 and the phase's integer sum is added to the phase's first tap
 *   of largest magnitude: every phase sums to exactly 16384, a constant input comes out as the same constant once the
 *   history is full.  The table's bits are not pinned across libms: whatever table the library returns is the
 *   specification for the kernel.  Equal rates, a zero rate, or L or M above 640 are COOLMIC_ERROR_INVAL.
 *   cmhip_src_design: h == NULL returns the geometry only (L, M, T may each be NULL); with h, cap counts its entries,
 *   and a cap below L*T is COOLMIC_ERROR_INVAL with nothing written.
 *
 * cmhip_src_run: `in` is int16 [S][in_stride], `out` int16 [S][out_stride], strides in samples as in a batch, both
 *   device-accessible; asynchronous on the resampler's stream.  `frames` input frames per stream, or
 *   frames_per_stream[s] <= frames (host array of S entries, may be NULL; free on return: the resampler copies it
 *   into a small ring of pinned blocks it owns, and the fifth of five cmhip_src_run with frames_per_stream queued back
 *   to back may wait ON THE HOST until the first one's counts have been copied on the stream).  COOLMIC_ERROR_INVAL,
 *   with nothing launched and nothing changed, when a base is not 16-byte aligned, a stride is not a multiple of 8 samples
 *   or smaller than
 *   the run needs (frames * C in; the run's largest output count * C out -- cmhip_src_max_out_frames() * C always
 *   suffices), frames > max_in_frames, a per-stream count is above frames, or in == out; COOLMIC_ERROR_FAULT for NULL
 *   arrays.  out_frames[] (host, S entries, may be NULL) receives every stream's output count, computed on the host
 *   from its mirror of r before the call returns, without a device wait -- exactly the frames_per_stream argument of
 *   a cmhip_batch_run on the result.  Outputs past a stream's count are not written.
 * Composition: a batch created with rate = rate_out takes the output straight into its own slots
 *   (out = cmhip_batch_dev_in(b), out_stride = cmhip_batch_stride(b)); a CMHIP_EXTSLOTS batch takes it through
 *   cmhip_batch_run_slots; with hip_stream = cmhip_batch_hip_stream(b) the order is the stream's.
 * cmhip_src_new designs the table for the descriptor's rates; cmhip_src_new_table takes the caller's H[L][T] (the
 *   descriptor's rates are informational then).  max_in_frames * C and the matching output may not pass 2^31 samples.
 *   Both return NULL on failure.  cmhip_src_reset (stream -1: all) zeroes history and r, on the resampler's stream. */
typedef struct cmhip_src cmhip_src_t;
typedef struct cmhip_src_desc {
    int          device;          /* HIP device ordinal */
    unsigned int streams;         /* S >= 1 */
    unsigned int channels;        /* 1..16 */
    unsigned int rate_in;         /* Hz */
    unsigned int rate_out;        /* Hz */
    size_t       max_in_frames;   /* per run and stream */
    void        *hip_stream;      /* hipStream_t to launch on, NULL: own stream */
} cmhip_src_desc_t;
cmhip_src_t *cmhip_src_new(const cmhip_src_desc_t *d);
cmhip_src_t *cmhip_src_new_table(const cmhip_src_desc_t *d, unsigned int L, unsigned int M, unsigned int T,
                                 const int16_t *h /* [L][T] */);
void     cmhip_src_free(cmhip_src_t *r);
int      cmhip_src_geometry(const cmhip_src_t *r, unsigned int *L, unsigned int *M, unsigned int *T);
size_t   cmhip_src_max_out_frames(const cmhip_src_t *r);      /* floor(max_in_frames * L / M) + 1 */
int      cmhip_src_run(cmhip_src_t *r, const void *in, size_t in_stride, size_t frames,
                       const uint32_t *frames_per_stream, void *out, size_t out_stride, uint32_t *out_frames);
int      cmhip_src_reset(cmhip_src_t *r, long stream);
int      cmhip_src_sync(cmhip_src_t *r);
void    *cmhip_src_hip_stream(cmhip_src_t *r);
/* host only, no device needed */
int      cmhip_src_design(unsigned int rate_in, unsigned int rate_out, unsigned int *L, unsigned int *M, unsigned int *T,
                          int16_t *h, size_t cap /* entries */);
uint32_t cmhip_src_out_frames(unsigned int L, unsigned int M, uint32_t r, uint32_t frames);

/* ---- channel mixing, an object of its own beside the batch --------------------- */
/* A mixer turns S streams of channels_in interleaved int16 channels into S streams of channels_out, frame by frame,
 * in exact integers.  The signal is the raw int16 the caller hands in: no gain and no map, the batch does those.
 *
 * Arithmetic.  Every stream has a matrix W[channels_out][channels_in] of its own, int16 in units of 2^-14
 *   (unity = 16384, as the resampler's table); negative weights are allowed.  Output channel o of frame f:
 *       acc     = sum_{c<C_in} W[o][c] * x[f][c]             exact in int32
 *       y[f][o] = saturate_int16((acc + 8192) >> 14)         arithmetic shift (floor): halves round towards +inf
 * Validity.  channels_in and channels_out lie in 1..16 and may be equal (1 -> 1 is a signed gain, 2 -> 2 a balance or
 *   a mid/side matrix); every row has sum_c |W[o][c]| <= 65535.  Then |acc + 8192| <= 65535*32768 + 8192 < 2^31: int32
 *   never overflows and the result does not depend on the order of summation (the resampler's bound and argument).
 *   Anything else is COOLMIC_ERROR_INVAL and changes nothing.
 * Identity.  W = 16384 * I gives acc = 16384 * x, and (16384 * x + 8192) >> 14 = x: the input comes back bit for bit.
 * State.  There is none: no history, nothing carried between runs.  A stream with 0 frames in a run touches nothing,
 *   and the output does not depend on how a stream was cut into runs.
 * The matrix at creation: W[o][o] = 16384 for o < min(C_in, C_out), zero elsewhere -- the leading channels are kept
 *   and extra outputs are silent.
 *
 * cmhip_mix_run: `in` is int16 [S][in_stride], `out` int16 [S][out_stride], strides in samples as in a batch, both
 *   device-accessible; asynchronous on the mixer's stream.  `frames` frames per stream, or frames_per_stream[s] <=
 *   frames (host array of S entries, may be NULL; free on return: the mixer copies it into a small ring of pinned
 *   blocks it owns, and the fifth of five cmhip_mix_run with frames_per_stream queued back to back may wait ON THE HOST
 *   until the first one's counts have been copied on the stream).  COOLMIC_ERROR_INVAL, with nothing launched and
 *   nothing changed,
 *   when a base is not 16-byte aligned, a stride is not a multiple of 8 samples or smaller than frames * C_in (in) or
 *   frames * C_out (out), frames > max_frames, a per-stream count is above frames, the run's grid would reach 2^31
 *   workgroups, or the byte ranges of the input ([in, in + S * in_stride samples)) and of the output overlap at all
 *   -- not only in == out: a narrower output written over the input would race between tiles.  COOLMIC_ERROR_FAULT for
 *   NULL arrays.  Samples past a stream's count are neither read nor written.
 * cmhip_mix_set_matrix (stream -1: all) is ordered with the runs: runs queued before it use the old matrix, runs
 *   queued after it the new one, without the caller synchronising; W may be reused as soon as it returns.  A matrix
 *   that fails the validity rules is refused and the old one stays.  cmhip_mix_get_matrix answers from the host's
 *   mirror: what the last accepted set (or creation) left.
 * Composition: as the resampler -- out = cmhip_batch_dev_in(b), out_stride = cmhip_batch_stride(b) of a batch with
 *   channels = channels_out; with hip_stream = cmhip_batch_hip_stream(b) the order is the stream's.  The chain is
 *   source -> rate (cmhip_src_t) -> width (cmhip_mix_t) -> batch (gain, VU, true peak, loudness).
 * cmhip_mix_new returns NULL on failure; max_frames * max(C_in, C_out) may not pass 2^31 samples.
 *
 * Presets (cmhip_mix_preset; these integers are the specification; 5.1 is in the order L R C LFE Ls Rs):
 *   CMHIP_MIX_MONO_TO_STEREO       1 -> 2   {16384}, {16384}
 *   CMHIP_MIX_STEREO_TO_MONO       2 -> 1   {8192, 8192}
 *   CMHIP_MIX_STEREO_TO_MS         2 -> 2   {8192, 8192}, {8192, -8192}
 *   CMHIP_MIX_51_TO_STEREO         6 -> 2   {16384, 0, 11585, 0, 11585, 0}, {0, 16384, 11585, 0, 0, 11585}
 *                                           ITU-R BS.775: 1, 1/sqrt(2), 1/sqrt(2); may saturate
 *   CMHIP_MIX_51_TO_STEREO_NORM    6 -> 2   {6786, 0, 4799, 0, 4799, 0}, {0, 6786, 4799, 0, 0, 4799}
 *                                           the same divided by 1 + sqrt(2): rows sum to exactly 16384, never saturates
 *   W == NULL returns the geometry only (channels_in, channels_out may each be NULL); with W, cap counts its entries,
 *   and a cap below C_out * C_in is COOLMIC_ERROR_INVAL with nothing written.  An unknown preset is
 *   COOLMIC_ERROR_INVAL.  cmhip_mix_check: 0 for a valid matrix, COOLMIC_ERROR_INVAL for a channel count outside 1..16
 *   or a row above the bound, COOLMIC_ERROR_FAULT for W == NULL. */
#define CMHIP_MIX_MONO_TO_STEREO     0u
#define CMHIP_MIX_STEREO_TO_MONO     1u
#define CMHIP_MIX_STEREO_TO_MS       2u
#define CMHIP_MIX_51_TO_STEREO       3u
#define CMHIP_MIX_51_TO_STEREO_NORM  4u
typedef struct cmhip_mix cmhip_mix_t;
typedef struct cmhip_mix_desc {
    int          device;          /* HIP device ordinal */
    unsigned int streams;         /* S >= 1 */
    unsigned int channels_in;     /* 1..16 */
    unsigned int channels_out;    /* 1..16 */
    size_t       max_frames;      /* per run and stream */
    void        *hip_stream;      /* hipStream_t to launch on, NULL: own stream */
} cmhip_mix_desc_t;
cmhip_mix_t *cmhip_mix_new(const cmhip_mix_desc_t *d);
void     cmhip_mix_free(cmhip_mix_t *m);
int      cmhip_mix_set_matrix(cmhip_mix_t *m, long stream, const int16_t *W /* [C_out][C_in] */);
int      cmhip_mix_get_matrix(const cmhip_mix_t *m, unsigned int stream, int16_t *W);
int      cmhip_mix_run(cmhip_mix_t *m, const void *in, size_t in_stride, size_t frames,
                       const uint32_t *frames_per_stream, void *out, size_t out_stride);
int      cmhip_mix_sync(cmhip_mix_t *m);
void    *cmhip_mix_hip_stream(cmhip_mix_t *m);
/* host only, no device needed */
int      cmhip_mix_check(unsigned int channels_in, unsigned int channels_out, const int16_t *W);
int      cmhip_mix_preset(unsigned int preset, unsigned int *channels_in, unsigned int *channels_out, int16_t *W,
                          size_t cap /* entries */);

/* ---- matrix ramps: a mixer's matrix moves without a click ------------------------ */
/* cmhip_mix_set_matrix is a step between two frames, and a step in a gain is a click.  A ramp takes a stream's matrix
 * from W0, the matrix in force, to W1 over R frames of that stream, every frame with a matrix of its own, still in
 * exact integers.  A fader, a fade in or out, a crossfade between two downmixes are ramps.
 *
 * Arithmetic.  Frames are counted per stream, by the frames the stream is actually given.  Frame n = 1..R of the ramp
 *   uses the weights below, frame R + 1 and every later one W1.  R lies in 2..2^20.
 *       inc   = ceil(2^32 / R)                              uint32 (R >= 2: inc <= 2^31)
 *       p(n)  = min(32768, (n * inc) >> 17)                 64-bit product; the position in units of 2^-15, p(0) = 0
 *       N     = w0 * (32768 - p) + w1 * p                   per matrix entry, exact in int32 (|N| <= 2^30)
 *       w(p)  = N / 32768 truncated TOWARDS ZERO            sgn(N) * (|N| >> 15) -- not an arithmetic shift
 *       acc   = sum_c w(p(n))[o][c] * x[f][c]               y = saturate_int16((acc + 8192) >> 14), the mixer's own tail
 * Properties.
 *   End point: R * inc >= 2^32, so p(R) = 32768 for every R: frame R already uses exactly W1.
 *   Shape: p is non-decreasing and never behind the ideal line: inc exceeds 2^32 / R by less than 1, so
 *     0 <= p(n) - floor(32768 * n / R) <= ceil(n / 2^17) -- at most 1 for R <= 2^17 (2.7 s at 48 kHz), at most 8 at 2^20,
 *     where a ramp whose R is not a power of two arrives up to R / 4096 frames early.
 *   Start: p = 0 gives N = 32768 * w0, so w = w0.       Constant: W0 = W1 gives N = 32768 * w0 at every p.
 *   Monotone: N is linear in p and truncation is monotone, so every entry moves monotonically from w0 to w1.
 *   Row bound: truncation towards zero gives |w(p)| <= |N| / 32768 <= (|w0| (32768 - p) + |w1| p) / 32768.  Summed
 *     over a row this is the convex combination of the two ends' row sums, so sum_c |w(p)[o][c]| <= 65535 at every
 *     position, and the mixer's int32 argument holds for every frame of every ramp.  Neither floor nor
 *     round-to-nearest has this property: either can pass the bound by up to C_in, and 65543 * 32768 overflows.
 * Retargeting.  A ramp requested while one is running starts from the matrix in force, cur = w(p(done)), where done
 *   counts the ramp's frames already produced (W0 when done = 0); n restarts at 1.  cur obeys the row bound, so this
 *   is closed under repetition.
 * Cancelling.  cmhip_mix_set_matrix during a ramp ends it and steps; its contract is otherwise unchanged.
 * Zero frames.  A stream given 0 frames in a run keeps its position.
 * Cuts.  The concatenated output does not depend on how a stream was cut into runs, with ramps and retargets at the
 *   same frames.
 * Read-back.  cmhip_mix_get_matrix keeps answering with the last accepted matrix, which for a ramp is its target.
 *
 * cmhip_mix_ramp_matrix (stream -1: all streams, each from its own matrix in force) is ordered with the runs by the
 *   mixer's stream alone, as cmhip_mix_set_matrix: no host wait and no synchronisation, in it or in cmhip_mix_run; W
 *   may be reused as soon as it returns.  ramp_frames 0 or 1 is exactly cmhip_mix_set_matrix.  COOLMIC_ERROR_INVAL for
 *   ramp_frames above 2^20, a matrix that fails cmhip_mix_check or a stream out of range, COOLMIC_ERROR_FAULT for NULL;
 *   a refused call changes nothing, a running ramp included.  The ramps' state is allocated by the first ramp;
 *   COOLMIC_ERROR_NOMEM then leaves the mixer usable.  A mixer that never ramps runs exactly as before, and so does
 *   every run at which no stream is inside a ramp.
 * cmhip_mix_ramp_state answers from the host's mirror (the host sees every run's counts and advances the positions the
 *   device advances): while the stream ramps 0 <= *done < *ramp_frames and W_now = w(p(done)); otherwise 0, 0 and
 *   the stream's matrix.  W_now may be NULL; COOLMIC_ERROR_FAULT for the other pointers, COOLMIC_ERROR_INVAL for a
 *   stream out of range.
 * cmhip_mix_ramp_position and cmhip_mix_ramp_weight are the specification as code, on the host. */
int      cmhip_mix_ramp_matrix(cmhip_mix_t *m, long stream, const int16_t *W /* [C_out][C_in] */, uint32_t ramp_frames);
int      cmhip_mix_ramp_state(const cmhip_mix_t *m, unsigned int stream, uint32_t *done, uint32_t *ramp_frames,
                              int16_t *W_now /* [C_out][C_in], may be NULL */);
/* host only, no device needed */
uint32_t cmhip_mix_ramp_position(uint32_t n, uint32_t ramp_frames);   /* p(n); n > ramp_frames counts as ramp_frames */
int16_t  cmhip_mix_ramp_weight(int16_t w0, int16_t w1, uint32_t p);   /* p above 32768 counts as 32768 */

/* ---- mix bus, an object of its own beside the batch ------------------------------ */
/* A bus object sums streams: `streams` input slots of channels_in interleaved int16 channels become `buses` output
 * slots of channels_out, by a routing table of n SENDS.  Send j is (bus_j, stream_j, W_j[channels_out][channels_in]),
 * W_j int16 in units of 2^-14 as the mixer's (unity = 16384, negative weights allowed).  A programme of several
 * microphones, a conference room, the "everyone but me" return feed (mix-minus: one bus per participant) are tables.
 *
 * Arithmetic.  For bus b, frame f, output channel o:
 *       p_j        = sum_{c<C_in} W_j[o][c] * x[stream_j][f][c]     exact in int32; 0 where f >= count(stream_j)
 *       acc        = sum over the sends j of bus b of p_j            exact in int64, in any order
 *       y[b][f][o] = saturate_int16((acc + 8192) >> 14)              arithmetic shift (floor); ONE rounding, after the sum
 *   Sends are never rounded or saturated one by one, and their order does not matter.  A stream may feed several buses,
 *   and may appear more than once in one bus: the weights simply add.
 * Validity.  channels_in, channels_out in 1..16; streams, buses >= 1; every row of every send has
 *   sum_c |W_j[o][c]| <= 65535 (the mixer's bound: |p_j| <= 65535 * 32768 < 2^31); bus_j < buses, stream_j < streams;
 *   n <= max_sends, the capacity of the table fixed at creation (>= 1); max_frames * max(C_in, C_out) < 2^31; streams,
 *   buses + 1 and max_sends * C_out * ceil(C_in / 2) each stay below 2^31.  Anything else is COOLMIC_ERROR_INVAL and
 *   changes nothing.  The sum over a bus is not bounded by a rule: 2^31 sends of 2^31 each still fit an int64.
 * Counts.  A bus's output count is the largest count among its sends' streams, 0 for a bus with no sends; such a bus
 *   touches nothing.  Samples past a bus's count are not written.  A send whose stream is shorter than the bus
 *   contributes silence beyond its own count: its slot is not read there.
 * State.  There is none: nothing is carried between runs and the output does not depend on how the streams were cut
 *   into runs.  A bus with one send equals cmhip_mix_run with the same matrix bit for bit.
 *
 * cmhip_bus_run: `in` is int16 [streams][in_stride], `out` int16 [buses][out_stride], strides in samples as in a
 *   batch, both device-accessible; asynchronous on the object's stream.  `frames` frames per stream, or
 *   frames_per_stream[s] <= frames (host array of `streams` entries, may be NULL; free on return).  The contract and
 *   the refusals are cmhip_mix_run's: COOLMIC_ERROR_INVAL, with nothing launched and nothing changed, when a base is
 *   not 16-byte aligned, a stride is not a multiple of 8 samples or smaller than frames * C_in (in) or frames * C_out
 *   (out), frames > max_frames, a per-stream count is above frames, the run's grid would reach 2^31 workgroups, or the
 *   byte ranges [in, in + streams * in_stride samples) and [out, out + buses * out_stride samples) overlap at all;
 *   COOLMIC_ERROR_FAULT for NULL arrays.  out_frames[] (host, `buses` entries, may be NULL) receives every bus's count,
 *   computed on the host from the mirror of the table before the call returns, without a device wait -- exactly the
 *   frames_per_stream argument of a cmhip_batch_run on the result.
 * cmhip_bus_set_routing replaces the whole table (n == 0 empties it; routing at creation: empty).  It is ordered with
 *   the runs by the stream alone: runs queued before it use the old table, runs queued after it the new one, the
 *   caller does not synchronise, and bus[], stream[], W[] are free on return.  The table travels from ONE pinned
 *   staging area the object owns: a second cmhip_bus_set_routing may wait ON THE HOST until the first one's copy has
 *   executed on the stream (likewise the fifth of five cmhip_bus_run with frames_per_stream queued back to back, for
 *   the first one's counts).  A table that fails the validity rules is refused and the old one stays.
 *   cmhip_bus_sends / cmhip_bus_get_routing answer from the host's mirror, in the caller's order; a cap below the
 *   table's sends is COOLMIC_ERROR_INVAL with nothing written.
 * Composition: as the mixer -- out = cmhip_batch_dev_in(b), out_stride = cmhip_batch_stride(b) of a batch with
 *   streams = buses and channels = channels_out, frames_per_stream = out_frames; with hip_stream =
 *   cmhip_batch_hip_stream(b) the order is the stream's.  The chain is source -> rate (cmhip_src_t) -> width
 *   (cmhip_mix_t) -> bus (cmhip_bus_t) -> batch.
 * cmhip_bus_new returns NULL on failure.
 *
 * Host only.  cmhip_bus_check: 0 for a valid table of n sends, else as above (COOLMIC_ERROR_FAULT for a NULL array
 *   with n > 0); sizes are judged before an array is read.  cmhip_bus_mix_minus writes the table of n participants with
 *   C_in == C_out == channels: bus b gets every stream != b with the matrix w * I, bus-major, n * (n - 1) sends; a
 *   cap_sends below that is COOLMIC_ERROR_INVAL with nothing written (n == 1 is the empty table). */
typedef struct cmhip_bus cmhip_bus_t;
typedef struct cmhip_bus_desc {
    int          device;          /* HIP device ordinal */
    unsigned int streams;         /* input slots, >= 1 */
    unsigned int buses;           /* output slots, >= 1 */
    unsigned int channels_in;     /* 1..16 */
    unsigned int channels_out;    /* 1..16 */
    size_t       max_frames;      /* per run and slot */
    size_t       max_sends;       /* capacity of the routing table, >= 1 */
    void        *hip_stream;      /* hipStream_t to launch on, NULL: own stream */
} cmhip_bus_desc_t;
cmhip_bus_t *cmhip_bus_new(const cmhip_bus_desc_t *d);
void     cmhip_bus_free(cmhip_bus_t *m);
int      cmhip_bus_set_routing(cmhip_bus_t *m, size_t n, const uint32_t *bus, const uint32_t *stream,
                               const int16_t *W /* [n][C_out][C_in] */);
size_t   cmhip_bus_sends(const cmhip_bus_t *m);
int      cmhip_bus_get_routing(const cmhip_bus_t *m, size_t cap, uint32_t *bus, uint32_t *stream, int16_t *W);
int      cmhip_bus_run(cmhip_bus_t *m, const void *in, size_t in_stride, size_t frames,
                       const uint32_t *frames_per_stream, void *out, size_t out_stride, uint32_t *out_frames);
int      cmhip_bus_sync(cmhip_bus_t *m);
void    *cmhip_bus_hip_stream(cmhip_bus_t *m);
/* host only, no device needed */
int      cmhip_bus_check(unsigned int buses, unsigned int streams, unsigned int channels_in, unsigned int channels_out,
                         size_t n, const uint32_t *bus, const uint32_t *stream, const int16_t *W);
int      cmhip_bus_mix_minus(unsigned int n, int16_t w, uint32_t *bus, uint32_t *stream, int16_t *W, size_t cap_sends,
                             unsigned int channels);

/* ---- send ramps: a bus's sends move without a click ------------------------------- */
/* cmhip_bus_set_routing replaces the whole table between two frames: every fader move, mute or mix-minus change on a
 * bus is a step in a gain, and a step is a click.  A send of the table in force can instead move from its matrix in
 * force to a target over R frames, every frame with a matrix of its own, still in exact integers.
 *
 * Arithmetic.  The ramp is the mixer's to the bit ("matrix ramps" above): inc = ceil(2^32 / R), p(n) = min(32768,
 *   (n * inc) >> 17), N = w0 * (32768 - p) + w1 * p, w(p) = sgn(N) * (|N| >> 15), R in 2..2^20.  cmhip_mix_ramp_position
 *   and cmhip_mix_ramp_weight remain the specification as code.  Everything else is the bus's own: p_j per send exact
 *   in int32 with the send's matrix of that frame, the sum over a bus's sends exact in int64, ONE rounding
 *   saturate_int16((acc + 8192) >> 14) after the sum.  The row bound of a ramp (every interpolated row stays within the
 *   convex combination of its two ends) is what keeps p_j in int32 at every frame of every ramp.
 * State.  Each send has its own (W0, W1, R, done) and ramps while done < R; different sends of one bus may be at
 *   different positions of different ramps.
 * Clock.  A send's ramp counts the OUTPUT frames of its bus.  In a run, frame f (from 0) of bus b uses
 *   w(p(done_j + f + 1)) for send j while that number is <= R_j, later frames W1_j.  After the run done_j has advanced
 *   by the bus's output count of that run, capped at R_j; a bus that produced 0 frames keeps its sends' positions.  A
 *   send whose stream is shorter than the bus contributes silence beyond its own count, as ever; its ramp moves on all
 *   the same.
 * Retarget.  A ramp requested for a send that is ramping starts from the matrix in force, w(p(done)); n restarts at 1.
 * Step.  ramp_frames 0 or 1 sets the named sends' matrices between two frames and ends their ramps -- one send can be
 *   changed without replacing the table.
 * cmhip_bus_set_routing ends every ramp and steps; its contract is otherwise untouched.  Topology changes only through
 *   it: to fade a send in, put it into the table with a zero matrix and ramp it; to fade it out, ramp it to zero, then
 *   drop it.  A zero-matrix send adds nothing to the sum but does count for its bus's frame count.
 * Read-back.  cmhip_bus_get_routing answers with the last accepted matrices; for a ramping send that is its target.
 * Cuts.  With ramps requested at the same output frames, the concatenated output does not depend on how the run
 *   sequence is cut.
 *
 * cmhip_bus_ramp_sends moves sends first .. first + count - 1, indexed in the caller's order of the last accepted
 *   cmhip_bus_set_routing, to W[0] .. W[count - 1].  It is ordered with the runs by the object's stream alone, as
 *   cmhip_bus_set_routing: W is free on return and there is no host wait for the device's runs, in it or in
 *   cmhip_bus_run; the one host wait it may make is cmhip_bus_set_routing's own, for the object's single pinned staging
 *   area still being the source of the previous table copy.  count == 0 is accepted and does nothing.
 *   COOLMIC_ERROR_INVAL for first + count above cmhip_bus_sends, ramp_frames above 2^20 or a row of a target with
 *   sum |w| > 65535; COOLMIC_ERROR_FAULT for a NULL bus, or NULL W with count > 0.  A refused call changes nothing, a
 *   running ramp included.  Ramp state is allocated by the first ramp; COOLMIC_ERROR_NOMEM there leaves the bus usable.
 *   A bus that never ramps launches exactly what it did before, and so does every run at which no send is inside a
 *   ramp.
 * cmhip_bus_ramp_state answers from the host's mirror, which advances by the counts every cmhip_bus_run sees: while the
 *   send ramps 0 <= *done < *ramp_frames and W_now = w(p(done)); otherwise 0, 0 and the send's matrix.  W_now may be
 *   NULL; COOLMIC_ERROR_FAULT for the other pointers, COOLMIC_ERROR_INVAL for a send out of range. */
int      cmhip_bus_ramp_sends(cmhip_bus_t *m, size_t first, size_t count,
                              const int16_t *W /* [count][C_out][C_in] */, uint32_t ramp_frames);
int      cmhip_bus_ramp_state(const cmhip_bus_t *m, size_t send, uint32_t *done, uint32_t *ramp_frames,
                              int16_t *W_now /* [C_out][C_in], may be NULL */);

/* ---- peak limiter, an object of its own beside the batch -------------------------- */
/* A limiter takes S streams of `channels` interleaved int16 channels in and gives the same out, delayed by a fixed
 * number of frames and held under a ceiling: a brick-wall look-ahead limiter in exact integers.  It is what follows a
 * bus (mix with headroom, drive up, hold a ceiling) and precedes the batch.
 *
 * Geometry, per object: lookahead_log2 = a in 3..9, A = 2^a; the delay is D = A - 1 frames; hold = H >= 0 frames with
 *   W = A + H <= 2048; HIST = A + W - 2 is the number of earlier frames an output depends on.
 * Parameters, per stream, settable between runs: threshold T in 1..32767, in sample units (at creation 32767); drive in
 *   1..65535, in units of 2^-12 (unity 4096, at creation 4096).
 * Arithmetic.  For frame n of a stream, counted over everything it was ever given; frames before the first (or before
 *   a reset) are zero:
 *       p12[n] = drive * max_c |x[n][c]|                   <= 65535 * 32768 < 2^31
 *       pr[n]  = (p12[n] + 4095) >> 12                     peak after drive, rounded up to sample units
 *       g[n]   = 32768                     if pr[n] <= T   (Q15, unity = 32768)
 *                floor(T * 32768 / pr[n])  otherwise       (numerator < 2^30)
 *       m[n]   = min(g[n-W+1 .. n])                        sliding minimum: attack look-ahead + hold
 *       S[n]   = sum(m[n-A+1 .. n])                        <= 2^(15+a) <= 2^24
 *       s[n]   = S[n] >> a                                 linear attack and release over A frames
 *       c[n]   = drive * s[n]                              < 2^31
 *       y[n][ch] = (x[n-D][ch] * c[n] + 2^26) >> 27        64-bit product, arithmetic shift
 *   All channels of a frame share one gain (linked), so the stereo image does not move.
 * Ceiling.  Every m[n-j], j < A, has g[n-D] in its window (0 <= D - j <= W - 1), so s[n] <= g[n-D]; with
 *   |x[n-D][ch]| * drive <= 4096 * pr[n-D] this gives |x * c| <= T * 2^27: |y| <= T always.  Nothing is saturated, so
 *   nothing can hide an error.
 * Transparency.  Where pr <= T over the whole window, s = 32768, c = drive * 2^15 and y = (x * drive + 2^11) >> 12: at
 *   unity drive the output is the input delayed by D frames, bit for bit.
 * Cuts.  A run evaluates every frame it looks at with the parameters in force for that run, the HIST history frames
 *   included: the history holds raw input frames, not gains.  Between parameter changes the concatenated output does
 *   not depend on how a stream was cut into runs; a run that follows a change still holds the ceiling for the new T by
 *   construction.  A stream given 0 frames keeps everything.
 * Gain-reduction meter.  Per stream the minimum s[n] over the frames output since the last reset of the meter, Q15;
 *   32768 when nothing was reduced.
 *
 * cmhip_lim_run has cmhip_mix_run's contract with C_in = C_out = channels: `in` is int16 [S][in_stride], `out` int16
 *   [S][out_stride], strides in samples, both device-accessible; asynchronous on the limiter's stream.  `frames` frames
 *   per stream, or frames_per_stream[s] <= frames (host array of S entries, may be NULL; free on return, with
 *   cmhip_mix_run's possible wait on the host for the fifth run queued back to back).  COOLMIC_ERROR_INVAL, with
 *   nothing launched and nothing changed, when a base is not 16-byte aligned, a stride is not a multiple of 8 samples or
 *   smaller than frames * channels, frames > max_frames, a per-stream count is above frames, the run's grid would reach
 *   2^31 workgroups, or the byte ranges [in, in + S * in_stride samples) and [out, out + S * out_stride samples)
 *   overlap at all.  COOLMIC_ERROR_FAULT for NULL arrays.  Samples past a stream's count are neither read nor written.
 *   A stream produces as many output frames as it is given input frames; the first D after creation or a reset are
 *   zeros from the history, and a caller flushes with D frames of silence.
 * cmhip_lim_set (stream -1: all) is ordered with the runs by the stream alone: runs queued before it use the old
 *   parameters, runs queued after it the new ones, without a host wait.  Invalid values are refused and the old ones
 *   stay.  cmhip_lim_get answers from the host's mirror: what the last accepted set (or creation) left.
 * cmhip_lim_reset (stream -1: all) zeroes the history and re-arms the meter, on the limiter's stream.
 * cmhip_lim_min_gain waits for the stream and writes the S meters to out[]; reset != 0 re-arms them all afterwards.
 * cmhip_lim_delay: D.  cmhip_lim_check (host only): 0 for a valid geometry and parameter pair, else COOLMIC_ERROR_INVAL.
 * Composition: as the mixer -- out = cmhip_batch_dev_in(b), out_stride = cmhip_batch_stride(b) of a batch with the same
 *   channels; with hip_stream = cmhip_batch_hip_stream(b) the order is the stream's.  The chain is source -> rate
 *   (cmhip_src_t) -> width (cmhip_mix_t) -> sum (cmhip_bus_t) -> limit (cmhip_lim_t) -> batch.
 * cmhip_lim_new returns NULL on failure; max_frames * channels may not pass 2^31 samples.
 *
 * True-peak detector.  A limiter has a detector, fixed at creation: CMHIP_LIM_DETECT_SAMPLE (0) is everything above,
 *   CMHIP_LIM_DETECT_TRUE_PEAK (1) derives the gain from the 4x oversampled signal of BS.1770 Annex 2 (the filter of the
 *   batch's true-peak meter, H = cmhip_tp_coefficients(), 4 phases of 12 taps in units of 2^-13), so that the ceiling
 *   also holds between the samples: what EBU R128's -1 dBTP asks for at the end of a programme chain.
 *   Arithmetic.  For frame n of a stream, counted over everything it was ever given, zeros before the first frame or a
 *   reset:
 *       y_p[n][c] = sum_{k<12} H[p][k] * x[n-k][c]         p = 0..3, exact in int32
 *       t[n]   = max_c max(|x[n-8][c]| << 13, max_p |y_p[n-2][c]|)          <= 16571 * 32768 < 2^30
 *       pr[n]  = (drive * t[n] + 2^25 - 1) >> 25           64-bit product; <= 1 060 528 < 2^21
 *       g[n]   = 32768 if pr[n] <= T, else floor(T * 32768 / pr[n])
 *       m[n], S[n], s[n], c[n] exactly as above
 *       y[n][ch] = (x[n-Dtp][ch] * c[n] + 2^26) >> 27,     Dtp = A + 7
 *   Alignment.  Phase 0 peaks at tap 6 and phase 3 at tap 5, so the four values y_p[n-2] lie between x[n-8] and x[n-7]:
 *     t[n] covers sample n - 8 and the interval behind it, in the filter's units of 2^13 per sample unit.
 *   Geometry.  An output depends on HISTtp = A + W - 2 + 13 earlier frames.  The detector requires hold >= 1 and
 *     A + W <= 2549 (HISTtp <= 2560; only a = 9 is affected: hold <= 1525).  Why hold >= 1: the interval between x[m]
 *     and x[m+1] is detector index m + 8, and output frame n carries x[n - Dtp].  For the gain on x[m+1] to be bounded
 *     by that interval's g as well, every window m[n-j], j < A, must contain g-index n - D - 1, which needs
 *     j + W - 1 >= D + 1 at j = 0: W >= A + 1.
 *   Sample ceiling, by construction as above: |x[n-8]| * 2^13 <= t[n] gives |x| * drive <= 4096 * pr, and s[n] <= g of
 *     that frame, so |y| <= T always and nothing is saturated.
 *   True-peak ceiling where the gain is constant: if s is the same over the 12 frames a filter output spans, then
 *     |sum_k H[p][k] * y[n-k]| <= T * 2^13 + 8286: the signal's part is at most T * 2^13 by the definition of g, the
 *     output rounding's at most sum |H[p][k]| / 2.  Where the gain MOVES inside those 12 frames this is NOT a guarantee:
 *     the filtered product is not the product of the filtered signal.  DESIGN 4.10 records the overshoot a model shows
 *     (a longer attack makes it smaller); a caller who needs a proof meters the result (cmhip_batch_set_true_peak).
 *   Unchanged: transparency (below the threshold at unity drive the output is the input delayed by Dtp, bit for bit),
 *     cuts (the history is raw input, HISTtp frames rounded up to 8), a stream given 0 frames keeps everything, the meter
 *     is the minimum of s, the parameter word and the order of cmhip_lim_set with the runs.  A caller flushes with Dtp
 *     frames of silence.
 * cmhip_lim_new_detector: cmhip_lim_new with a detector (0: cmhip_lim_new itself); NULL for a detector above 1 and, for
 *   detector 1, for hold == 0 or A + W > 2549.  cmhip_lim_detector: the object's.  cmhip_lim_delay: D or Dtp.
 *   run, set, get, reset, min_gain, sync and hip_stream serve both.
 * cmhip_lim_check_detector (host only): cmhip_lim_check for a detector.  cmhip_lim_threshold_dbtp (host only): the
 *   threshold for a ceiling in dBTP, floor(32768 * 10^(dbtp / 20)) clamped to 1..32767 (-1.0 gives 29204); 0 for NaN.
 *
 * Release stage.  Without it the gain returns to unity over the A frames of the attack, after the hold: on a bass note
 *   or a dense mix it follows the waveform.  A limiter may have a release of its own, fixed at creation, for either
 *   detector: release_log2 = rho in 0..11, R = 2^rho frames, slope q = 32768 >> rho (Q15 gain units per frame).  Between
 *   m and S of the arithmetic above:
 *       m[n]   = min(g[n-W+1 .. n])                        as above
 *       r[n]   = min over 0 <= k < R of (m[n-k] + k*q)     the release: r <= m, r[n] <= r[n-1] + q
 *       S[n]   = sum(r[n-A+1 .. n]),  s[n] = S[n] >> a     as above, on r instead of m
 *   k*q reaches 32768 at k = R, so the window of R frames is exact: no earlier frame can matter.  rho = 0 gives r = m,
 *   the limiter above.  The gain falls as fast as before and rises by at most q per frame: a full-scale recovery takes R
 *   frames on top of the boxcar's A (2048 frames, 42.7 ms at 48 kHz, at rho = 11).
 *   Ceiling: every r[n-j] <= m[n-j] <= g[n-D], so |y| <= T holds by construction as above and nothing saturates.
 *   Unchanged: the delay (D or Dtp: the stage adds none), transparency (below the threshold the output is the pure
 *     delay), cuts (r is a function of a bounded window of raw input: the history stays raw frames), the meter, the
 *     parameter word and the order of cmhip_lim_set with the runs.
 *   Geometry.  HIST grows by R - 1: HIST = A + W - 2 + (R - 1), plus 13 with the true-peak detector, rounded up to 8
 *     frames for the history slot, and may not pass 4096 (a = 9, rho = 11: hold <= 1027, with the true-peak detector
 *     hold <= 1014).  The bounds above stay as they are.
 * cmhip_lim_new_release: cmhip_lim_new_detector with a release stage (release_log2 0: cmhip_lim_new_detector itself);
 *   NULL also for release_log2 > 11 and for HIST > 4096.  cmhip_lim_release: the object's release_log2.
 *   run, set, get, reset, min_gain, sync, delay and hip_stream serve every form.
 * cmhip_lim_check_release (host only): cmhip_lim_check_detector for a release stage. */
#define CMHIP_LIM_DETECT_SAMPLE    0u
#define CMHIP_LIM_DETECT_TRUE_PEAK 1u
typedef struct cmhip_lim cmhip_lim_t;
typedef struct cmhip_lim_desc {
    int          device;          /* HIP device ordinal */
    unsigned int streams;         /* S >= 1 */
    unsigned int channels;        /* 1..16 */
    unsigned int lookahead_log2;  /* a in 3..9: A = 2^a, delay A - 1 frames */
    unsigned int hold;            /* H frames, A + hold <= 2048 */
    size_t       max_frames;      /* per run and stream */
    void        *hip_stream;      /* hipStream_t to launch on, NULL: own stream */
} cmhip_lim_desc_t;
cmhip_lim_t *cmhip_lim_new(const cmhip_lim_desc_t *d);
cmhip_lim_t *cmhip_lim_new_detector(const cmhip_lim_desc_t *d, unsigned int detector);
cmhip_lim_t *cmhip_lim_new_release(const cmhip_lim_desc_t *d, unsigned int detector, unsigned int release_log2);
unsigned int cmhip_lim_detector(const cmhip_lim_t *m);
unsigned int cmhip_lim_release(const cmhip_lim_t *m);
void     cmhip_lim_free(cmhip_lim_t *m);
unsigned int cmhip_lim_delay(const cmhip_lim_t *m);
int      cmhip_lim_set(cmhip_lim_t *m, long stream, unsigned int threshold, unsigned int drive);
int      cmhip_lim_get(const cmhip_lim_t *m, unsigned int stream, unsigned int *threshold, unsigned int *drive);
int      cmhip_lim_run(cmhip_lim_t *m, const void *in, size_t in_stride, size_t frames,
                       const uint32_t *frames_per_stream, void *out, size_t out_stride);
int      cmhip_lim_reset(cmhip_lim_t *m, long stream);
int      cmhip_lim_min_gain(cmhip_lim_t *m, uint32_t *out /* [S] */, int reset);
int      cmhip_lim_sync(cmhip_lim_t *m);
void    *cmhip_lim_hip_stream(cmhip_lim_t *m);
/* host only, no device needed */
int      cmhip_lim_check(unsigned int lookahead_log2, unsigned int hold, unsigned int threshold, unsigned int drive);
int      cmhip_lim_check_detector(unsigned int detector, unsigned int lookahead_log2, unsigned int hold,
                                  unsigned int threshold, unsigned int drive);
int      cmhip_lim_check_release(unsigned int detector, unsigned int lookahead_log2, unsigned int hold,
                                 unsigned int release_log2, unsigned int threshold, unsigned int drive);
unsigned int cmhip_lim_threshold_dbtp(double dbtp);

/* ---- dynamics: compressor and gate, an object of its own beside the batch ----------- */
/* A dynamics stage takes S streams of `channels` interleaved int16 channels in and gives the same out, delayed by a
 * fixed number of frames and multiplied by a gain that never exceeds unity and follows the level through a per-stream
 * static curve: a compressor (the curve falls above a threshold) and a downward expander / gate (it falls below one) in
 * exact integers.  It stands between a bus and the limiter.  Make-up gain is not here: it is the drive of the limiter
 * that follows, so |y| <= |x| holds by construction, nothing saturates and nothing can hide an error.
 *
 * Geometry, per object: detector_log2 = a in 3..10, A = 2^a, the level window; smooth_log2 = b in 3..9, B = 2^b, the
 *   gain's ramp length; the delay is D = B - 1 frames; hold = H >= 0 frames with W = B + H <= 2048;
 *   HIST = (A - 1) + (W - 1) + (B - 1) <= 3581 is the number of earlier frames an output depends on.
 * Arithmetic.  For frame n of a stream, counted over everything it was ever given; frames before the first (or before
 *   a reset) are zero:
 *       e[n]  = max_c |x[n][c]|                         0..32768
 *       L[n]  = (sum(e[n-A+1 .. n])) >> a               mean magnitude over A frames, 0..32768; the sum is below 2^26
 *       l[n]  = max(L[n-W+1 .. n])                      level with look-ahead and hold
 *       g[n]  = curve(l[n])                             0..32768, Q15, unity = 32768
 *       s[n]  = (sum(g[n-B+1 .. n])) >> b               linear ramps over B frames; the sum is at most 2^24
 *       y[n][ch] = (x[n-D][ch] * s[n] + 2^14) >> 15     arithmetic shift; |y| <= |x|, fits int16 for x = -32768 too
 *   All channels of a frame share one gain (linked).  Taking the maximum of the level, not the minimum of the gain,
 *   lets one stage serve both ends of the curve: a rising level is seen B - 1 frames before it comes out, so the
 *   compressor's reduction and the gate's opening are both in place at the onset; a falling level is held for W
 *   frames, so the compressor releases late and the gate closes late.
 * The curve, per stream, settable between runs: CMHIP_DYN_CURVE = 128 uint16 entries T[]; entries 0..122 are used and
 *   each must be at most 32768, entries 123..127 are ignored.  The knots lie on a pseudo-logarithmic level grid, 8 per
 *   octave, and a lookup interpolates linearly between two knots:
 *       l == 0:            idx = 0, frac = 0, sh = 0
 *       l >= 1, E = floor(log2 l):
 *          E >= 3:         idx = 1 + 8E + ((l >> (E-3)) & 7),  frac = l & ((1 << (E-3)) - 1),  sh = E - 3
 *          E <  3:         idx = 1 + 8E + ((l << (3-E)) & 7),  frac = 0,                       sh = 0
 *       curve(l) = T[idx] + (((int)T[idx+1] - (int)T[idx]) * frac >> sh)      arithmetic shift; |product| < 2^27
 *   Knot k >= 1 stands for level (8 + (k-1) % 8) * 2^((k-1) / 8 - 3); knot 121 is level 32768, the largest index ever
 *   reached, with frac = 0; knot 122 is read but multiplied by 0.  The device takes the table as the specification (as
 *   the resampler its table and the mixer its matrix).  At creation every stream's curve is all 32768: the stage is a
 *   pure delay of D frames, bit for bit.
 * Cuts.  A run evaluates every frame it looks at with the curve in force for that run, the HIST history frames
 *   included: the history holds raw input frames, not levels or gains.  Between curve changes the concatenated output
 *   does not depend on how a stream was cut into runs.  A stream given 0 frames keeps everything.
 * Gain meter.  Per stream the minimum s[n] over the frames output since the last reset of the meter, Q15; 32768 when
 *   nothing was reduced.
 * Side-chain keys.  Per stream s a key k = key[s], another stream of the same object whose level steers the gain of s
 *   (ducking: the music falls when the voice speaks; many streams on one key: linked stems).  Only the first line of
 *   the arithmetic changes:
 *       e[n]  = max_c |x_k[n][c]|                       the key's raw input, never its gain
 *   L, l, g = curve_s(l), s[n] and y[n][ch] = (x_s[n-D][ch] * s[n] + 2^14) >> 15 stay as they are: the curve, the delay,
 *   the history of the delayed samples and the meter are stream s's own, and |y| <= |x| still holds by construction.
 *   Frame n of a run of s is aligned with frame n of the same run of k; the frames before the run come from the history
 *   of each stream, so history frame -j of s is aligned with history frame -j of k.  The detector reads the key's raw
 *   input, so a key may be keyed itself, two streams may key each other, and many streams may share one key.  Every
 *   stream still produces its own output: a key is an ordinary stream.  A run with frames_per_stream is refused with
 *   COOLMIC_ERROR_INVAL -- nothing launched, nothing changed, the message names both streams and both counts -- when a
 *   keyed stream and its key get different counts; equal counts of 0 are fine, both keep everything.  Between changes
 *   of curve or key the concatenated output does not depend on how the streams were cut into runs.  cmhip_dyn_reset(s)
 *   zeroes the history and the meter of s only: resetting a key changes what its followers detect, resetting a
 *   follower leaves its key's history alone.  At creation every stream is its own key, and an object on which no key
 *   is set behaves, and runs, exactly as one without this paragraph.
 * RMS detector.  A dynamics stage has a detector, fixed at creation: CMHIP_DYN_DETECT_MEAN (0) is everything above,
 *   CMHIP_DYN_DETECT_RMS (1) follows the power of the loudest channel, as a broadcast compressor and the loudness meter
 *   beside it do, so that a threshold in dBFS means the same for speech, music and tones.  One line of the arithmetic
 *   changes:
 *       e[n]  = max_c |x[n][c]|                          as above (with a key: the key's raw input), 0..32768
 *       M[n]  = (sum(e[k]^2, k = n-A+1 .. n)) >> a       mean square; the sum is at most 2^40, M <= 2^30
 *       L[n]  = isqrt(M[n])                              the largest r with r*r <= M[n]; 0..32768
 *       l, g, s, y                                       as above
 *   The root is exact: no result depends on how a floating-point operation rounds.  Everything else stays the stream's
 *   own and stays as it is: the geometry (a, b, H, W, HIST, D = B - 1), the curve and its index, the history of raw
 *   frames, cuts, the meter, resets, side-chain keys and every refusal; |y| <= |x| still holds by construction.  The
 *   curve keeps its meaning, gain against level on the amplitude grid, so cmhip_dyn_design and cmhip_dyn_design_duck
 *   serve both detectors unchanged.
 *   For a signal of constant magnitude both detectors give the same level (the mean of A equal squares is the square,
 *   and its root the magnitude).  A full-scale sine reads 23170 (32768 / sqrt 2, -3.01 dBFS) under RMS; under the mean
 *   it reads about 20861 (32768 * 2 / pi, -3.92 dBFS), 0.91 dB lower, while a square wave reads its amplitude under both.
 * cmhip_dyn_new_detector: cmhip_dyn_new with a detector (cmhip_dyn_new(d) is cmhip_dyn_new_detector(d, 0) and runs the
 *   kernels it always ran); NULL for a detector above 1.  cmhip_dyn_detector: the object's (0 for NULL).  Every other
 *   call serves both.  cmhip_dyn_check_detector (host only): cmhip_dyn_check for a detector, COOLMIC_ERROR_INVAL for a
 *   detector above 1.
 *
 * cmhip_dyn_run has cmhip_lim_run's contract: `in` is int16 [S][in_stride], `out` int16 [S][out_stride], strides in
 *   samples, both device-accessible; asynchronous on the stage's stream.  `frames` frames per stream, or
 *   frames_per_stream[s] <= frames (host array of S entries, may be NULL; free on return, with cmhip_mix_run's possible
 *   wait on the host for the fifth run queued back to back).  COOLMIC_ERROR_INVAL, with nothing launched and nothing
 *   changed, when a base is not 16-byte aligned, a stride is not a multiple of 8 samples or smaller than frames *
 *   channels, frames > max_frames, a per-stream count is above frames, the run's grid would reach 2^31 workgroups, or
 *   the byte ranges [in, in + S * in_stride samples) and [out, out + S * out_stride samples) overlap at all.
 *   COOLMIC_ERROR_FAULT for NULL arrays.  Samples past a stream's count are neither read nor written.  A stream
 *   produces as many output frames as it is given input frames; the first D after creation or a reset are zeros from
 *   the history, and a caller flushes with D frames of silence.
 * cmhip_dyn_set_curve (stream -1: all) is ordered with the runs by the stream alone: runs queued before it use the old
 *   curve, runs queued after it the new one, without a host wait; the caller's table is free on return.  A table with a
 *   used entry above 32768 is refused and the old curve stays.  cmhip_dyn_get_curve answers from the host's mirror:
 *   the 128 entries the last accepted set (or creation) left.
 * cmhip_dyn_set_key (stream -1: all; key -1, or key == stream: the stream's own detector) is ordered with the runs by the
 *   stream alone, as cmhip_dyn_set_curve is: runs queued before it use the old key, runs queued after it the new one,
 *   without a host wait and without staging memory.  A NULL stage is COOLMIC_ERROR_FAULT; a stream or a key out of
 *   range is COOLMIC_ERROR_INVAL and the old map stays.  cmhip_dyn_get_key answers from the host's mirror, -1 for a
 *   stream on its own detector (COOLMIC_ERROR_FAULT for NULL, COOLMIC_ERROR_INVAL for a stream out of range).
 * cmhip_dyn_reset (stream -1: all) zeroes the history and re-arms the meter, on the stage's stream.
 * cmhip_dyn_min_gain waits for the stream and writes the S meters to out[]; reset != 0 re-arms them all afterwards.
 * cmhip_dyn_delay: D.  cmhip_dyn_check (host only): 0 for a valid geometry, else COOLMIC_ERROR_INVAL.
 * cmhip_dyn_design (host only, no device needed) fills the 128 entries from a compressor (threshold ct in dBFS, ratio
 *   R >= 1, knee width K >= 0 dB) and a gate (threshold gt in dBFS, expander ratio Re >= 1, range rng >= 0 dB; rng == 0:
 *   no gate).  For a knot of level v > 0: x = 20 log10(v / 32768), d = x - ct;
 *       comp = 0                                   if 2d < -K
 *              (1/R - 1) (d + K/2)^2 / (2K)        if 2|d| <= K and K > 0        (the usual soft knee)
 *              (1/R - 1) d                         otherwise
 *       gate = max(-rng, (x - gt)(Re - 1))         where x < gt and rng > 0, else 0
 *       entry = min(32768, floor(32768 * 10^((comp + gate) / 20) + 0.5))
 *   Knot 0 (silence) gets -rng dB; entries 123..127 are zero.  Non-finite values, R < 1, Re < 1 and negative K or rng
 *   are refused with COOLMIC_ERROR_INVAL, NULL pointers with COOLMIC_ERROR_FAULT.
 * cmhip_dyn_design_duck (host only, in doubles) fills the 128 entries with a curve for a keyed stream: unity below a
 *   threshold of the KEY's level, depth dB down above it.  For a knot of level v > 0: x = 20 log10(v / 32768),
 *   d = x - threshold;
 *       g = -depth * clamp((d + K/2) / K, 0, 1)    with K = knee > 0
 *       g = -depth where d >= 0, else 0            with K = 0
 *       entry = min(32768, floor(32768 * 10^(g / 20) + 0.5))
 *   Knot 0 (silence) is 32768; entries 123..127 are zero.  Non-finite values, depth < 0 or knee < 0 are refused with
 *   COOLMIC_ERROR_INVAL, NULL pointers with COOLMIC_ERROR_FAULT.
 * Composition: as the limiter -- with hip_stream shared the order is the stream's.  The chain is source -> rate
 *   (cmhip_src_t) -> width (cmhip_mix_t) -> sum (cmhip_bus_t) -> dynamics (cmhip_dyn_t) -> limit (cmhip_lim_t) -> batch.
 * cmhip_dyn_new returns NULL on failure; max_frames * channels may not pass 2^31 samples. */
#define CMHIP_DYN_CURVE 128
#define CMHIP_DYN_DETECT_MEAN 0u
#define CMHIP_DYN_DETECT_RMS  1u
typedef struct cmhip_dyn cmhip_dyn_t;
typedef struct cmhip_dyn_desc {
    int          device;          /* HIP device ordinal */
    unsigned int streams;         /* S >= 1 */
    unsigned int channels;        /* 1..16 */
    unsigned int detector_log2;   /* a in 3..10: the level is the mean magnitude (or the RMS) over 2^a frames */
    unsigned int smooth_log2;     /* b in 3..9: B = 2^b, delay B - 1 frames */
    unsigned int hold;            /* H frames, B + hold <= 2048 */
    size_t       max_frames;      /* per run and stream */
    void        *hip_stream;      /* hipStream_t to launch on, NULL: own stream */
} cmhip_dyn_desc_t;
typedef struct cmhip_dyn_curve_desc {
    double comp_threshold_db;     /* ct, dBFS */
    double comp_ratio;            /* R >= 1 */
    double comp_knee_db;          /* K >= 0 */
    double gate_threshold_db;     /* gt, dBFS */
    double gate_ratio;            /* Re >= 1 */
    double gate_range_db;         /* rng >= 0; 0: no gate */
} cmhip_dyn_curve_desc_t;
typedef struct cmhip_dyn_duck_desc { double threshold_db, depth_db, knee_db; } cmhip_dyn_duck_desc_t;
cmhip_dyn_t *cmhip_dyn_new(const cmhip_dyn_desc_t *d);
cmhip_dyn_t *cmhip_dyn_new_detector(const cmhip_dyn_desc_t *d, unsigned int detector);
unsigned int cmhip_dyn_detector(const cmhip_dyn_t *m);
void     cmhip_dyn_free(cmhip_dyn_t *m);
unsigned int cmhip_dyn_delay(const cmhip_dyn_t *m);
int      cmhip_dyn_set_curve(cmhip_dyn_t *m, long stream, const uint16_t *curve /* [CMHIP_DYN_CURVE] */);
int      cmhip_dyn_get_curve(const cmhip_dyn_t *m, unsigned int stream, uint16_t *curve /* [CMHIP_DYN_CURVE] */);
int      cmhip_dyn_set_key(cmhip_dyn_t *m, long stream, long key);   /* stream -1: all; key -1 (or == stream): own detector */
int      cmhip_dyn_get_key(const cmhip_dyn_t *m, unsigned int stream, long *key);   /* -1 for own */
int      cmhip_dyn_run(cmhip_dyn_t *m, const void *in, size_t in_stride, size_t frames,
                       const uint32_t *frames_per_stream, void *out, size_t out_stride);
int      cmhip_dyn_reset(cmhip_dyn_t *m, long stream);
int      cmhip_dyn_min_gain(cmhip_dyn_t *m, uint32_t *out /* [S] */, int reset);
int      cmhip_dyn_sync(cmhip_dyn_t *m);
void    *cmhip_dyn_hip_stream(cmhip_dyn_t *m);
/* host only, no device needed */
int      cmhip_dyn_check(unsigned int detector_log2, unsigned int smooth_log2, unsigned int hold);
int      cmhip_dyn_check_detector(unsigned int detector, unsigned int detector_log2, unsigned int smooth_log2,
                                  unsigned int hold);
int      cmhip_dyn_design(const cmhip_dyn_curve_desc_t *c, uint16_t *curve /* [CMHIP_DYN_CURVE] */);
int      cmhip_dyn_design_duck(const cmhip_dyn_duck_desc_t *c, uint16_t *curve /* [CMHIP_DYN_CURVE] */);

/* ---- band split: a linear-phase FIR crossover, an object of its own beside the batch -- */
/* A band split cuts each of S streams of C interleaved int16 channels (C in 1..16) into B bands (2..8) of the same
 * rate, in exact integers, so that the bands add up to the input delayed by D frames -- to the bit, by construction.
 * The signal is the raw int16 the caller hands in.  T taps per filter, odd, 3..1023; D = (T-1)/2 for every band; a run
 * of F frames gives F frames in every band.
 *
 * Arithmetic, per stream, channel and frame n counted from creation or reset.  The object holds B-1 filters g_b[T],
 *   int16, each with its own scale q_b in 14..20 (units of 2^-q_b); any int16 taps are valid.  For b < B-1:
 *       acc_b = sum_{k<T} g_b[k] * x[n-k]            exact (|acc_b| < 2^41)
 *       r_b   = (acc_b + 2^(q_b-1)) >> q_b           arithmetic shift (floor)
 *       y_b   = saturate_int16(r_b)
 *   and the last band is the residual, from the UNSATURATED r_b:
 *       y_{B-1} = saturate_int16(x[n-D] - sum_{b<B-1} r_b)
 *   x[i] for i < 0 is the stream's history: zero at creation and after cmhip_split_reset.  The state is the last T-1
 *   frames per channel and nothing else; a stream that gets 0 frames in a run keeps it; outputs and clip counters do not
 *   depend on how a stream is cut into runs.  Where no band of a sample saturates, sum_b y_b = x[n-D] exactly.
 *   clips[S][B] (uint32, modulo 2^32, on the device) counts the saturated samples per stream and band: reconstruction
 *   is exact iff they are zero.
 * Output layout: `out` is band-major, int16 [B][S][out_stride]; band b of stream s starts at
 *   out + (b*S + s) * out_stride.  out + b*S*out_stride is an ordinary S-stream input (for a cmhip_dyn_t of that band's
 *   own time constants), the whole array a B*S-stream input (for a cmhip_bus_t that sums the bands: unity sends give
 *   the delayed input back bit for bit while no clip counter moves).  Bands must pass stages of EQUAL delay before
 *   they are summed.
 * cmhip_split_run has cmhip_mix_run's contract with C_in = C_out = channels and B*S output slots: asynchronous on the
 *   object's stream; frames_per_stream (host, S entries, may be NULL) is free on return, with cmhip_mix_run's possible
 *   wait on the host for the fifth run queued back to back; COOLMIC_ERROR_INVAL, with nothing launched and nothing
 *   changed, when a base is not 16-byte aligned, a stride is not a multiple of 8 samples or below frames * C,
 *   frames > max_frames, a count is above frames, either array would end past the address space, or the input and the
 *   B*S output slots share a byte; COOLMIC_ERROR_FAULT for NULL arrays.  Outputs past a stream's count are not written.
 * The designed filters (cmhip_split_design, host only, double precision, in this order).  Crossovers
 *   f_0 < f_1 < ... < f_{B-2} strictly inside (0, rate/2), anything else is COOLMIC_ERROR_INVAL.  For filter j, with
 *   fc = f_j / rate and x = i - D for i in 0..T-1:
 *       w = I0(7.5 * sqrt(max(0, 1 - (x / (D+1))^2))) / I0(7.5)          l_j[i] = 2*fc * sinc(2*fc*x) * w
 *   (sinc and I0 as cmhip_src_design's), l_j divided by its own sum.  h_0 = l_0, h_b = l_b - l_{b-1}.
 *   g_b = rint(h_b * 2^q); the difference to the wanted integer sum (2^q for b = 0, 0 for the others) is added to the
 *   centre tap; q_b is the largest q in 14..20 for which every finished tap lies within +-32767.  Every filter is
 *   symmetric; a constant input c comes out as c in band 0 and 0 in every other band, the residual included, once the
 *   history is full.  The table's bits are not pinned across libms: whatever table the library returns is the
 *   specification for the kernel.  g == NULL checks the arguments only; with g, q may not be NULL, cap counts g's
 *   entries, and a cap below (B-1)*T is COOLMIC_ERROR_INVAL with nothing written.
 * cmhip_split_new designs the filters for `rate` and crossover_hz[B-1]; cmhip_split_new_table takes the caller's
 *   g[B-1][T] and q[B-1] (cmhip_split_check: the geometry and every q_b in 14..20).  max_frames * C may not pass 2^31
 *   samples.  Both return NULL on failure.  cmhip_split_reset (stream -1: all) zeroes history and clip counters, on the
 *   object's stream.  cmhip_split_clips copies the counters to clips[S][B] (host) and, with clear, zeroes them behind
 *   the copy: a synchronous round trip on the object's stream. */
typedef struct cmhip_split cmhip_split_t;
typedef struct cmhip_split_desc {
    int          device;          /* HIP device ordinal */
    unsigned int streams;         /* S >= 1 */
    unsigned int channels;        /* 1..16 */
    unsigned int bands;           /* B in 2..8 */
    unsigned int taps;            /* T odd, in 3..1023 */
    size_t       max_frames;      /* per run and stream */
    void        *hip_stream;      /* hipStream_t to launch on, NULL: own stream */
} cmhip_split_desc_t;
cmhip_split_t *cmhip_split_new(const cmhip_split_desc_t *d, unsigned int rate, const double *crossover_hz /* [B-1] */);
cmhip_split_t *cmhip_split_new_table(const cmhip_split_desc_t *d, const int16_t *g /* [B-1][T] */,
                                     const uint8_t *q /* [B-1] */);
void     cmhip_split_free(cmhip_split_t *m);
unsigned int cmhip_split_delay(const cmhip_split_t *m);               /* D = (T-1)/2 */
int      cmhip_split_get_table(const cmhip_split_t *m, int16_t *g /* [B-1][T] */, uint8_t *q /* [B-1] */);
int      cmhip_split_run(cmhip_split_t *m, const void *in, size_t in_stride, size_t frames,
                         const uint32_t *frames_per_stream, void *out, size_t out_stride);
int      cmhip_split_reset(cmhip_split_t *m, long stream);
int      cmhip_split_clips(cmhip_split_t *m, uint32_t *clips /* [S][B] */, int clear);
int      cmhip_split_sync(cmhip_split_t *m);
void    *cmhip_split_hip_stream(cmhip_split_t *m);
/* host only, no device needed */
int      cmhip_split_design(unsigned int rate, unsigned int bands, const double *crossover_hz /* [B-1] */,
                            unsigned int taps, int16_t *g /* [B-1][T] */, uint8_t *q /* [B-1] */, size_t cap /* entries */);
int      cmhip_split_check(unsigned int bands, unsigned int taps, const int16_t *g, const uint8_t *q);

/* ---- delay: a delay line with click-free moves, an object of its own beside the batch -- */
/* A delay gives each of S streams of C interleaved int16 channels (C in 1..16) back d_s frames later, d_s in
 * 0..max_delay per stream, in exact integers: the consumer of cmhip_split_delay, cmhip_dyn_delay and cmhip_lim_delay
 * (a dry path beside a compressor, bands of unequal latency in front of a bus), and the ordinary delay line of a
 * broadcast chain (time alignment, lip sync, a profanity delay of seconds).
 *
 * Arithmetic, per stream, channel and frame n.  Frames are counted over everything the stream was ever given; x[i] for
 *   i before the first frame, or before the last cmhip_delay_reset, is zero.
 *   Steady state: y[n][c] = x[n - d][c].
 *   History: the state is the stream's last max_delay frames and nothing else.  It does not depend on d: after a move to
 *     a larger delay the output reads real older samples, not zeros.  A stream given 0 frames in a run keeps everything.
 *   Step: cmhip_delay_set(m, stream, d) steps between two frames (stream -1: all streams): from the next frame on,
 *     y[n] = x[n - d].
 *   Crossfade: cmhip_delay_ramp(m, stream, d1, R) moves the delay from d0, the one in force, to d1 without a click, by
 *     a crossfade between the two taps over the stream's next R frames, R in 2..2^20.  Frame k = 1..R of the ramp has
 *     the position p = cmhip_mix_ramp_position(k, R), one per frame for all channels, and
 *         N = x[n-d0][c] * (32768 - p) + x[n-d1][c] * p
 *         y = (N + 16384) >> 15                          arithmetic shift (floor)
 *     Frame R has p = 32768 and is exactly x[n - d1], and so is every later frame.  R of 0 or 1 is exactly
 *     cmhip_delay_set.  cmhip_delay_crossfade(a, b, p) is this formula as code (p above 32768 counts as 32768).
 *   Properties.  |N| <= 2^30, so int32 is exact: |a| (32768 - p) + |b| p <= 32768 * 32768.  The result lies in
 *     -32768..32767 for every p and every pair of int16 samples, so nothing saturates and no clamp can hide an error:
 *     N / 32768 is a convex combination of a and b and lies in [-32768, 32767], so (N + 16384) / 32768 lies in
 *     [-32767.5, 32767.5] and its floor in -32768..32767.  d0 = d1 gives y = x[n - d0] at every p: then
 *     N = 32768 a, and (32768 a + 16384) >> 15 = a.  For the implementer: the weight 32768 does not fit an int16, so
 *     the packed dot product is not the tool; y = a + ((p * (b - a) + 16384) >> 15) is the same integer, as 32768 a is
 *     a multiple of 2^15, and its factors fit 24 bits.
 *   While a ramp runs another cmhip_delay_ramp on that stream is COOLMIC_ERROR_BUSY and changes nothing (for stream -1:
 *     when any stream ramps, and no stream changes) -- a third tap is not built.  cmhip_delay_set ends the ramp and
 *     steps.  Ramp frames are counted by the frames the stream is actually given.
 *   Cuts: the concatenated output does not depend on how a stream is cut into runs, with sets and ramps at the same
 *     frames.
 *   cmhip_delay_reset (stream -1: all) zeroes the history, on the object's stream.  The delay setting and a running
 *     ramp stay.
 * cmhip_delay_new: NULL for C outside 1..16, S = 0, max_frames = 0, (max_delay + max_frames) * C >= 2^31, or a failed
 *   allocation (a stream's history is a ring of max_delay + max_frames frames on the device).  max_delay = 0 is legal
 *   and makes the object a copy.  Every stream starts with d = 0.
 * cmhip_delay_run has cmhip_mix_run's contract with C_in = C_out = channels: asynchronous on the object's stream;
 *   frames_per_stream (host, S entries, may be NULL) is free on return, with cmhip_mix_run's possible wait on the host
 *   for the fifth run queued back to back; COOLMIC_ERROR_INVAL, with nothing launched and nothing changed, when a base
 *   is not 16-byte aligned, a stride is not a multiple of 8 samples or below frames * C, frames > max_frames, a count is
 *   above frames, either array would end past the address space, or the two arrays share a byte; COOLMIC_ERROR_FAULT
 *   for NULL arrays.  Outputs past a stream's count are not written.
 * cmhip_delay_set and cmhip_delay_ramp take effect at the next run queued behind them: the positions, delays and ramps
 *   live in a host mirror that every run hands to the device with its counts, so they are ordered with the runs as the
 *   calls are, need no host wait and touch no device memory.  COOLMIC_ERROR_INVAL for a delay above max_delay,
 *   ramp_frames above 2^20 or a stream out of range; every refused call changes nothing.  cmhip_delay_get answers from
 *   that mirror: *delay is the last accepted target; while the stream ramps *from is d0, *done the ramp frames so far
 *   and *ramp_frames R; otherwise *from = *delay and the other two are 0.  from, done and ramp_frames may be NULL.
 * cmhip_delay_ms (host only): rint(rate * ms / 1000) frames, 0 for a negative or non-finite product. */
typedef struct cmhip_delay cmhip_delay_t;
typedef struct cmhip_delay_desc {
    int          device;          /* HIP device ordinal */
    unsigned int streams;         /* S >= 1 */
    unsigned int channels;        /* 1..16 */
    size_t       max_delay;       /* frames; 0: the object is a copy */
    size_t       max_frames;      /* per run and stream */
    void        *hip_stream;      /* hipStream_t to launch on, NULL: own stream */
} cmhip_delay_desc_t;
cmhip_delay_t *cmhip_delay_new(const cmhip_delay_desc_t *d);
void     cmhip_delay_free(cmhip_delay_t *m);
int      cmhip_delay_set(cmhip_delay_t *m, long stream, uint32_t delay);
int      cmhip_delay_ramp(cmhip_delay_t *m, long stream, uint32_t delay, uint32_t ramp_frames);
int      cmhip_delay_get(const cmhip_delay_t *m, unsigned int stream, uint32_t *delay, uint32_t *from, uint32_t *done,
                         uint32_t *ramp_frames);
int      cmhip_delay_run(cmhip_delay_t *m, const void *in, size_t in_stride, size_t frames,
                         const uint32_t *frames_per_stream, void *out, size_t out_stride);
int      cmhip_delay_reset(cmhip_delay_t *m, long stream);
int      cmhip_delay_sync(cmhip_delay_t *m);
void    *cmhip_delay_hip_stream(cmhip_delay_t *m);
size_t   cmhip_delay_max_delay(const cmhip_delay_t *m);
/* host only, no device needed */
uint32_t cmhip_delay_ms(unsigned int rate, double ms);
int16_t  cmhip_delay_crossfade(int16_t a, int16_t b, uint32_t p);

/* ---- leveller: slow automatic gain control, an object of its own beside the batch ------- */
/* A leveller finds the gain that brings each of S streams of C interleaved int16 channels (C in 1..16) to a target
 * level, in exact integers: the stage that chooses what the limiter's constant drive cannot.  It belongs between the
 * sources (or a bus) and the dynamics and limiter.  The gain moves once per window of W frames and is interpolated
 * in between; the level is the input's own (feed-forward), so nothing can hunt.  The stage adds no delay.
 *
 * Geometry, per object: window_log2 = w in 6..14, W = 2^w.
 * Parameters, per stream, settable between runs (cmhip_agc_set, stream -1: all streams):
 *     target T              1..32767    sample units: the RMS level wanted
 *     gate Q                0..32767    a window whose level is below Q leaves the gain alone: silence is not pumped up
 *     gain_min, gain_max    1 <= gain_min <= gain_max <= 65535, units of 2^-12, unity 4096 (the limiter's drive unit):
 *                           at most +24.08 dB
 *     rise, fall            0..65535    the fraction of the gain in force it may move per window, units of 2^-16;
 *                                       0 freezes that direction
 *     initial               gain_min..gain_max: the gain of a stream's first frames (below)
 *
 * Arithmetic, per stream.  Frames are counted since creation or the last cmhip_agc_reset: n, 64 bits.  Window
 *   k = n >> w, j = n & (W - 1).
 *   Level of a complete window k: E[k] = max over the channels c of the sum over the window's frames of x[n][c]^2;
 *     E <= 2^44, exact in uint64.  L[k] = isqrt(E[k] >> w), the exact integer root, 0 <= L <= 32768.  The loudest
 *     channel is used, as in the dynamics stage's RMS detector: a level means the same in both stages.
 *   Step:
 *     step(A, L): if L == 0 or L < Q: return A
 *                 D = clamp((T << 12) / L, gain_min, gain_max)                integer division, below 2^27
 *                 if D > A and rise: return min(D, A + max(1, (A * rise) >> 16))
 *                 if D < A and fall: return max(D, A - max(1, (A * fall) >> 16))
 *                 return A
 *     A * rise stays below 2^32: uint32 is exact.
 *   Gain nodes: A[0] = A[1] = initial -- the `initial` in force in the run that processes frame 0.  For k >= 1,
 *     A[k+1] = step(A[k], L[k-1]), evaluated when frame n = k W is processed, with the parameters of the last
 *     cmhip_agc_set queued before the run that processes that frame.  The gain of window k depends only on windows
 *     that ended before it began: the stage is causal without a delay.
 *   Per frame: g = A[k] + (((A[k+1] - A[k]) * j) >> w), arithmetic shift (floor); the product stays below 2^30, int32 is
 *     exact.  Every channel of the frame: v = (x * g + 2048) >> 12, arithmetic shift; |x g| + 2048 < 2^31, int32 is
 *     exact.  y = clamp(v, -32768, 32767), and every sample the clamp changes increments the stream's clip counter.
 *     Gain above unity can saturate: the limiter that follows is what holds a ceiling.
 *   Properties.  With gain_min = gain_max = initial = 4096 the output is the input, bit for bit:
 *     (4096 x + 2048) >> 12 = x.  A stream given 0 frames in a run keeps everything.  Cuts: the concatenated output,
 *     the clip counts and the state do not depend on how a stream is cut into runs, with the sets at the same frames
 *     -- every sum is a sum of integers.
 *   cmhip_agc_reset (stream -1: all): the stream's next frame is frame 0 again: the gain is `initial`, the sums of an
 *     open window and the last level are forgotten.  The parameters and the clip counter stay.
 * cmhip_agc_new: NULL for C outside 1..16, S = 0, window_log2 outside 6..14, max_frames = 0, max_frames * C >= 2^31,
 *   or a failed allocation.  Every stream starts with target 3277 (-20 dB re 32768), gate 33 (-60 dB), gain_min =
 *   gain_max = initial = 4096 and rise = fall = 0: a copy, until cmhip_agc_set says otherwise.
 * cmhip_agc_run has cmhip_delay_run's contract: asynchronous on the object's stream; frames_per_stream (host, S entries,
 *   may be NULL) is free on return; COOLMIC_ERROR_INVAL, with nothing launched and nothing changed, when a base is not
 *   16-byte aligned, a stride is not a multiple of 8 samples or below frames * C, frames > max_frames, a count is above
 *   frames, either array would end past the address space, or the two arrays share a byte; COOLMIC_ERROR_FAULT for
 *   NULL arrays.  Outputs past a stream's count are not written.
 * cmhip_agc_set and cmhip_agc_reset are ordered with the runs as the calls are: positions and parameters live in a host
 *   mirror that every run hands to the device with its counts, so they need no host wait and touch no device memory.
 *   COOLMIC_ERROR_INVAL for parameters out of range or a stream out of range; a refused call changes nothing.
 *   cmhip_agc_get answers from that mirror.
 * cmhip_agc_state: synchronous (it waits for the object's stream, like cmhip_lim_min_gain).  Per stream, S entries each:
 *   gain[s] = A[k+1] of the window the stream's last frame lies in (`initial` before its first frame), level[s] = L of
 *   its last complete window (0 before the first), clips[s] = the clip counter; clear_clips != 0 zeroes the counters
 *   after reading them.  Any of the three pointers may be NULL.
 * cmhip_agc_check (host only): 0 for a valid window_log2 and parameter set (params may be NULL: the window alone),
 *   else COOLMIC_ERROR_INVAL.
 * cmhip_agc_design (host only): parameters from a law in dB (levels re 32768, gains re unity) and dB per second:
 *     T = rint(32768 * 10^(target_db / 20)), Q likewise from gate_db; gains rint(4096 * 10^(dB / 20));
 *     rise = rint((10^(rise_db_per_s * W / rate / 20) - 1) * 65536),
 *     fall = rint((1 - 10^(-fall_db_per_s * W / rate / 20)) * 65536),
 *   each clamped to its range, initial into gain_min..gain_max.  COOLMIC_ERROR_INVAL for a non-finite input, a rate
 *   that is not positive, a window_log2 that is no integer in 6..14, negative rates of change, or min_gain_db above
 *   max_gain_db; COOLMIC_ERROR_FAULT for NULL.  3 dB/s and 10 dB/s at w = 12, 48 kHz give 1960 and 6132. */
typedef struct cmhip_agc cmhip_agc_t;
typedef struct cmhip_agc_desc {
    int          device;          /* HIP device ordinal */
    unsigned int streams;         /* S >= 1 */
    unsigned int channels;        /* 1..16 */
    unsigned int window_log2;     /* w in 6..14: the gain moves once per 2^w frames */
    size_t       max_frames;      /* per run and stream */
    void        *hip_stream;      /* hipStream_t to launch on, NULL: own stream */
} cmhip_agc_desc_t;
typedef struct cmhip_agc_params {
    uint16_t target, gate, gain_min, gain_max, rise, fall, initial;
} cmhip_agc_params_t;
typedef struct cmhip_agc_law_desc {
    double rate;                  /* frames per second */
    double window_log2;           /* the object's w */
    double target_db, gate_db;    /* dB re 32768 */
    double max_gain_db, min_gain_db, initial_gain_db;      /* dB re unity */
    double rise_db_per_s, fall_db_per_s;                   /* >= 0 */
} cmhip_agc_law_desc_t;
cmhip_agc_t *cmhip_agc_new(const cmhip_agc_desc_t *d);
void     cmhip_agc_free(cmhip_agc_t *m);
int      cmhip_agc_set(cmhip_agc_t *m, long stream, const cmhip_agc_params_t *p);
int      cmhip_agc_get(const cmhip_agc_t *m, unsigned int stream, cmhip_agc_params_t *p);
int      cmhip_agc_run(cmhip_agc_t *m, const void *in, size_t in_stride, size_t frames,
                       const uint32_t *frames_per_stream, void *out, size_t out_stride);
int      cmhip_agc_reset(cmhip_agc_t *m, long stream);
int      cmhip_agc_state(cmhip_agc_t *m, uint32_t *gain /* [S] */, uint32_t *level /* [S] */, uint64_t *clips /* [S] */,
                         int clear_clips);
int      cmhip_agc_sync(cmhip_agc_t *m);
void    *cmhip_agc_hip_stream(cmhip_agc_t *m);
/* host only, no device needed */
int      cmhip_agc_check(unsigned int window_log2, const cmhip_agc_params_t *p);
int      cmhip_agc_design(const cmhip_agc_law_desc_t *law, cmhip_agc_params_t *p);

/* ---- automixer: gain-sharing groups, an object of its own beside the batch --------------- */
/* An automixer shares one unit of gain among the open microphones of a group, Dugan style, in exact integers: each of S
 * streams of C interleaved int16 channels (C in 1..16) gets the share of its group's gain that its level earns.  One
 * talker passes at unity, two equal talkers at -3 dB each, four at -6 dB; idle microphones sink towards a floor.  The
 * sum keeps the noise and feedback margin of one open microphone however many are plugged in.  It belongs in front of
 * the bus.  It has cmhip_agc_t's shapes: slots, strides, alignment and refusals are cmhip_agc_run's.  The gains move
 * once per window of W frames and are interpolated in between; the stage adds no delay.
 *
 * Geometry, per object: window_log2 = w in 6..14, W = 2^w.
 * Groups.  Each stream has a group id in 0..S-1, or -1 for none; every stream is in no group at creation.  A stream in
 *   no group is copied bit for bit; its gain nodes are 4096 throughout.  A group has ONE clock: all its members have the
 *   same position and must get the same count in every run.
 * Parameters, per stream, settable between runs (cmhip_automix_set, stream -1: all streams):
 *     weight u              0..4096     units of 2^-12 on power: the stream's priority, 4096 is unity
 *     floor                 0..4096     the lowest gain, units of 2^-12 (unity 4096, the leveller's gain unit)
 *     attack, release       0..8        the smoothing shifts of a rising and of a falling power
 *     initial               0..4096     the gain of a stream's first frames (below)
 *   Defaults: weight 4096, floor 0, attack 0, release 0, initial 4096.
 *
 * Arithmetic.  Frames are counted since creation or the last reset: n, 64 bits.  Window k = n >> w, j = n & (W - 1),
 *   as in the leveller.  Per complete window k of stream s:
 *     E = max over the channels c of the sum over the window's frames of x[n][c]^2; m = E >> w, so m <= 2^30: the
 *       leveller's E and shift, to the letter.
 *     v = (m * u) >> 12;  V = v << 8                               V <= 2^38
 *     P[k] = P[k-1] + ((V - P[k-1]) >> sh)                          signed 64-bit, arithmetic shift (floor);
 *       sh = attack when V > P[k-1], else release; P[-1] = 0.  0 <= P <= 2^38: a step never passes V.
 *     Sum[k] = the sum of P_j[k] over the members j of the stream's group: exact in uint64, independent of order.
 *     D[k] = D[k-1] when Sum[k] = 0, else max(floor, isqrt((P[k] << 24) / Sum[k]))
 *       unsigned 64-bit division, integer; the quotient is at most 2^24, the exact integer root at most 4096.
 *       D[-1] = initial.
 *     The parameters used are those in force in the run in which the window completes.
 *   Gain nodes: A[0] = A[1] = initial -- the `initial` in force in the run that processes frame 0.  For k >= 1,
 *     A[k+1] = D[k-1], taken when frame n = k W is processed.  The gain of window k depends only on windows that ended
 *     before it began: the stage is causal without a delay.
 *   Per frame and sample, the leveller's lines: g = A[k] + (((A[k+1] - A[k]) * j) >> w), arithmetic shift;
 *     y = clamp((x * g + 2048) >> 12, -32768, 32767).
 *   Properties.  g <= 4096, so the clamp never acts and |y| <= |x|.  With floors 0 the squares of a group's D[k] sum to
 *     at most 2^24 -- the group never has more than one microphone's gain.  A group of one member with a non-zero level
 *     is a copy from its third window on.  n members with equal input and weights each get isqrt(2^24 / n): 4096,
 *     2896, 2364, 2048 for n = 1..4.  Against members at digital silence one talker gets 4096 and the silent members
 *     their floor.  A stream given 0 frames in a run keeps everything.  Cuts: the concatenated output and the state do
 *     not depend on how the streams are cut into runs, with the sets at the same frames -- every sum is of integers.
 * cmhip_automix_new: NULL for C outside 1..16, S = 0, window_log2 outside 6..14, max_frames = 0,
 *   max_frames * C >= 2^31, or a failed allocation.
 * cmhip_automix_set_group(m, stream, group): the stream joins `group` (0..S-1) or leaves its group (-1).  Every member
 *   of the group left and of the group joined is reset, the stream included: that keeps a group on one clock.
 *   COOLMIC_ERROR_INVAL for a stream outside 0..S-1 or a group outside -1..S-1.  cmhip_automix_get_group answers from
 *   the mirror.
 * cmhip_automix_reset(m, stream): the stream's whole group is reset; a stream in no group alone; stream -1: all.  A reset
 *   stream's next frame is frame 0 again: the gain is `initial`, and P, D, the sums of an open window and the pending
 *   node are forgotten.  Parameters and groups stay.
 * cmhip_automix_run has cmhip_agc_run's signature and contract.  In addition: frames_per_stream that gives two members
 *   of one group different counts is COOLMIC_ERROR_INVAL, nothing is launched and nothing changes; the message names both
 *   streams and both counts.  Equal counts of 0 are fine.
 * cmhip_automix_set, _set_group and _reset touch the host mirror only: they need no host wait and no device memory, and
 *   are ordered with the runs as the calls are.  COOLMIC_ERROR_INVAL for parameters or a stream out of range; a refused
 *   call changes nothing.  cmhip_automix_get answers from the mirror.
 * cmhip_automix_state: synchronous (it waits for the object's stream, like cmhip_agc_state).  Per stream, S entries each:
 *   gain[s] = A[k+1] of the window the stream's last frame lies in (`initial` before its first frame), power[s] = P of
 *   its last complete window (0 before the first), share[s] = D of its last complete window (`initial` before the
 *   first): the node its next window edge brings in.  A stream in no group: 4096, 0, 4096.  Any pointer may be NULL.
 * cmhip_automix_check (host only): 0 for a valid window_log2 and parameter set (params may be NULL: the window alone),
 *   else COOLMIC_ERROR_INVAL.
 * cmhip_automix_design (host only): parameters from a law: weight = rint(4096 * 10^(weight_db / 10)) (weight_db <= 0);
 *   floor and initial = rint(4096 * 10^(dB / 20)), clamped to 0..4096; attack and release =
 *   rint(log2(ms * rate / 1000 / W)) clamped to 0..8 (0 for ms <= 0).  COOLMIC_ERROR_INVAL for a non-finite input, a
 *   rate that is not positive, a window_log2 that is no integer in 6..14 or weight_db above 0; COOLMIC_ERROR_FAULT for
 *   NULL. */
typedef struct cmhip_automix cmhip_automix_t;
typedef struct cmhip_automix_desc {
    int          device;          /* HIP device ordinal */
    unsigned int streams;         /* S >= 1 */
    unsigned int channels;        /* 1..16 */
    unsigned int window_log2;     /* w in 6..14: the gains move once per 2^w frames */
    size_t       max_frames;      /* per run and stream */
    void        *hip_stream;      /* hipStream_t to launch on, NULL: own stream */
} cmhip_automix_desc_t;
typedef struct cmhip_automix_params {
    uint16_t weight, floor, attack, release, initial;
} cmhip_automix_params_t;
typedef struct cmhip_automix_law_desc {
    double rate;                  /* frames per second */
    double window_log2;           /* the object's w */
    double weight_db;             /* <= 0, dB on power */
    double floor_db, initial_db;  /* dB re unity */
    double attack_ms, release_ms;
} cmhip_automix_law_desc_t;
cmhip_automix_t *cmhip_automix_new(const cmhip_automix_desc_t *d);
void     cmhip_automix_free(cmhip_automix_t *m);
int      cmhip_automix_set(cmhip_automix_t *m, long stream, const cmhip_automix_params_t *p);
int      cmhip_automix_get(const cmhip_automix_t *m, unsigned int stream, cmhip_automix_params_t *p);
int      cmhip_automix_set_group(cmhip_automix_t *m, long stream, long group);
int      cmhip_automix_get_group(const cmhip_automix_t *m, unsigned int stream, long *group);
int      cmhip_automix_run(cmhip_automix_t *m, const void *in, size_t in_stride, size_t frames,
                           const uint32_t *frames_per_stream, void *out, size_t out_stride);
int      cmhip_automix_reset(cmhip_automix_t *m, long stream);
int      cmhip_automix_state(cmhip_automix_t *m, uint32_t *gain /* [S] */, uint64_t *power /* [S] */,
                             uint32_t *share /* [S] */);
int      cmhip_automix_sync(cmhip_automix_t *m);
void    *cmhip_automix_hip_stream(cmhip_automix_t *m);
/* host only, no device needed */
int      cmhip_automix_check(unsigned int window_log2, const cmhip_automix_params_t *p);
int      cmhip_automix_design(const cmhip_automix_law_desc_t *law, cmhip_automix_params_t *p);

/* ---- failover switch: silence-triggered source changeover, an object of its own beside the batch */
/* A failover switch gives each of O outputs one of up to four candidate input streams, chosen by the signal: when the
 * source in force has been dead for fail_windows windows the output crossfades to a backup, and when a candidate of
 * higher priority has been live for return_windows windows the output crossfades back.  It is the silence switcher in
 * front of a stream that runs around the clock, in exact integers, decided where the samples are.  It belongs behind a
 * low cut (a DC offset reads as live) and in front of the leveller.  The stage adds no delay.
 *
 * Shapes.  The input is S streams of C interleaved int16 channels (C in 1..16), the output O outputs of C channels in a
 *   second array.  Slots, strides, alignment and overlap refusals are cmhip_agc_run's.  window_log2 = w in 6..14,
 *   W = 2^w.  max_frames is per run and output, max_frames * C < 2^31.
 * Sources.  Each output has an ordered list of K = 1..4 candidate input streams: candidate 0 is the main source, later
 *   candidates are backups.  cmhip_failover_set_sources(m, output, n, streams) sets the list: COOLMIC_ERROR_INVAL for n
 *   outside 1..4, a stream >= S, a stream named twice or an output out of range, COOLMIC_ERROR_FAULT for NULL; it resets
 *   the output (below) and sets its `force` back to -1.  At creation output o has the one candidate min(o, S - 1): a
 *   copy.  An input stream may be a candidate of many outputs; it is measured once per (output, candidate), on that
 *   output's clock, so no two outputs ever have to agree on counts.  cmhip_failover_get_sources answers from the
 *   mirror: *n and the first *n entries of streams[4].
 * Parameters, per output, settable between runs (cmhip_failover_set, output -1: all outputs):
 *     quiet[4]          0..32767, per candidate    a window of candidate i is LIVE iff m_i > quiet[i]^2
 *     fail_windows      1..65535    consecutive non-live windows of the source in force before it is left
 *     return_windows    1..65535    consecutive live windows of a higher-priority candidate before it is taken back
 *     fade_log2 = phi   w..16       a changeover is a crossfade over 2^phi frames, that is 2^(phi - w) whole windows
 *     force             -1..K-1     -1: automatic; i: go to candidate i and stay there
 *   Defaults: quiet 33 (the leveller's gate, -60 dB), fail_windows = return_windows = 1, phi = w, force -1.  A refused
 *   call changes nothing; with output -1 a force that one output's list is too short for refuses the whole call.
 *
 * Arithmetic, per output o.  Frames are counted since creation or the last reset: n, 64 bits.  Window k = n >> w,
 *   j = n & (W - 1).
 *   Level of candidate i in window k: E_i[k] = max over the channels c of the sum over the window's frames of
 *     x_i[n][c]^2; m_i[k] = E_i[k] >> w: the leveller's E and shift, to the letter; m <= 2^30.
 *     LIVE_i[k] iff m_i[k] > quiet[i]^2.
 *     live_run_i[k] = LIVE ? min(live_run_i[k-1] + 1, 65535) : 0
 *     dead_run_i[k] = LIVE ? 0 : min(dead_run_i[k-1] + 1, 65535)           both 0 before window 0
 *   Plan of window k: (from, to, q).  A steady window has from = to and q = 0.  Window q of a fade covers the fade's
 *     frames d = q W + j.
 *     Window 0 is steady on candidate c0 = force if force >= 0, else 0.
 *     When frame n = k W (k >= 1) is processed, first the counters are updated with window k - 1 (with the quiet in
 *     force in that run).  Then:
 *       1. If window k - 1 was fade window q and q + 1 < 2^(phi' - w), window k is fade window q + 1 of the same fade;
 *          phi' is the phi in force when the fade began.  A fade keeps its length, and no decision is taken inside a
 *          fade, `force` included.
 *       2. Otherwise cur = `to` of window k - 1, and want = cmhip_failover_step(K, params, cur, live_run, dead_run):
 *            if force >= 0: want = force
 *            else let b be the smallest i with live_run_i >= return_windows; if b exists and b < cur: want = b
 *            else if dead_run_cur >= fail_windows: want = the smallest i != cur with live_run_i >= 1, or cur if there
 *              is none -- when everything is dead the output stays
 *            else want = cur
 *          If want != cur, window k is fade window 0 of (from = cur, to = want) and the output's `switches` counter
 *          goes up by one; otherwise window k is steady on cur.
 *     The parameters used are those in force in the run that processes frame k W.  The plan of window k depends only on
 *     windows that ended before it began: the stage is causal and adds no delay.
 *   Per frame and channel.  Steady: y = x_to, bit for bit.  Fade: p = (d << 15) >> phi' and
 *     y = cmhip_delay_crossfade(x_from, x_to, p), the delay stage's rule.  d < 2^16, so the shift is exact in uint32 and
 *     p < 32768; nothing saturates.  The fade's first frame is x_from; the window behind the fade's last is steady on
 *     x_to (or the first of another fade from it).
 *   Properties.  K = 1 is a copy.  A steady output is a copy of its source.  An output given 0 frames in a run keeps
 *     everything.  Cuts: the concatenated output and the state do not depend on how an output is cut into runs, with
 *     the sets at the same frames -- every sum is of integers.  Every candidate slot of output o must hold the run's
 *     count[o] frames.
 *   cmhip_failover_reset(m, output) (-1: all): the output's next frame is frame 0 again; the counters, the levels, the
 *     sums of an open window and any fade are forgotten.  `switches`, parameters and lists stay.
 * cmhip_failover_new: NULL for C outside 1..16, S = 0, O = 0 or O >= 2^29, window_log2 outside 6..14, max_frames = 0,
 *   max_frames * C >= 2^31, or a failed allocation.
 * cmhip_failover_run has cmhip_agc_run's contract with S input slots, O output slots and frames_per_output (host, O
 *   entries, may be NULL): asynchronous on the object's stream; the counts are free on return; COOLMIC_ERROR_INVAL, with
 *   nothing launched and nothing changed, when a base is not 16-byte aligned, a stride is not a multiple of 8 samples or
 *   below frames * C, frames > max_frames, a count is above frames, either array would end past the address space, or
 *   the two arrays share a byte; COOLMIC_ERROR_FAULT for NULL arrays.  Outputs past an output's count are not written.
 * cmhip_failover_set, _set_sources and _reset touch the host mirror only: they need no host wait and no device memory,
 *   and are ordered with the runs as the calls are.  cmhip_failover_get answers from the mirror.
 * cmhip_failover_state: synchronous (it waits for the object's stream).  Any pointer may be NULL.  Per output, O entries
 *   each, for the window the output's last frame lies in: from, to, fade_window (before the first frame: c0, c0, 0);
 *   switches (uint64; clear != 0 zeroes the counters after reading them).  Per (output, candidate), [O][4]: live_run
 *   and dead_run as the last window edge processed left them, level = m of the last complete window; 0 before the first
 *   and for candidates the list does not have.
 * cmhip_failover_check (host only): 0 for a valid window_log2, n_sources in 1..4 and parameter set (params may be NULL),
 *   else COOLMIC_ERROR_INVAL.
 * cmhip_failover_design (host only): parameters from a law in dB re 32768 and seconds:
 *     quiet[i] = rint(32768 * 10^(quiet_db[i] / 20)) clamped to 0..32767;
 *     fail_windows = max(1, rint(fail_s * rate / W)), return_windows likewise from return_s, clamped to 65535;
 *     phi = clamp(rint(log2(fade_ms * rate / 1000)), w, 16) (w for fade_ms <= 0); force = -1.
 *   COOLMIC_ERROR_INVAL for a non-finite input, a rate that is not positive, a window_log2 that is no integer in 6..14
 *   or a negative time; COOLMIC_ERROR_FAULT for NULL.
 * cmhip_failover_step (host only): the decision of rule 2 for one edge as a pure function -> want.  n_sources outside
 *   1..4, cur >= n_sources, a force >= n_sources or NULL: cur is returned. */
typedef struct cmhip_failover cmhip_failover_t;
typedef struct cmhip_failover_desc {
    int          device;          /* HIP device ordinal */
    unsigned int streams;         /* S >= 1 input slots */
    unsigned int outputs;         /* O >= 1 output slots */
    unsigned int channels;        /* 1..16 */
    unsigned int window_log2;     /* w in 6..14: a source is judged once per 2^w frames */
    size_t       max_frames;      /* per run and output */
    void        *hip_stream;      /* hipStream_t to launch on, NULL: own stream */
} cmhip_failover_desc_t;
typedef struct cmhip_failover_params {
    uint16_t quiet[4];
    uint16_t fail_windows, return_windows, fade_log2;
    int16_t  force;
} cmhip_failover_params_t;
typedef struct cmhip_failover_law_desc {
    double rate;                  /* frames per second */
    double window_log2;           /* the object's w */
    double quiet_db[4];           /* dB re 32768 */
    double fail_s, return_s;      /* seconds, >= 0 */
    double fade_ms;
} cmhip_failover_law_desc_t;
cmhip_failover_t *cmhip_failover_new(const cmhip_failover_desc_t *d);
void     cmhip_failover_free(cmhip_failover_t *m);
int      cmhip_failover_set_sources(cmhip_failover_t *m, unsigned int output, unsigned int n, const uint32_t *streams);
int      cmhip_failover_get_sources(const cmhip_failover_t *m, unsigned int output, unsigned int *n,
                                    uint32_t *streams /* [4] */);
int      cmhip_failover_set(cmhip_failover_t *m, long output, const cmhip_failover_params_t *p);
int      cmhip_failover_get(const cmhip_failover_t *m, unsigned int output, cmhip_failover_params_t *p);
int      cmhip_failover_run(cmhip_failover_t *m, const void *in, size_t in_stride, size_t frames,
                            const uint32_t *frames_per_output, void *out, size_t out_stride);
int      cmhip_failover_reset(cmhip_failover_t *m, long output);
int      cmhip_failover_state(cmhip_failover_t *m, uint32_t *from /* [O] */, uint32_t *to /* [O] */,
                              uint32_t *fade_window /* [O] */, uint64_t *switches /* [O] */, int clear,
                              uint32_t *live_run /* [O][4] */, uint32_t *dead_run /* [O][4] */,
                              uint32_t *level /* [O][4] */);
int      cmhip_failover_sync(cmhip_failover_t *m);
void    *cmhip_failover_hip_stream(cmhip_failover_t *m);
/* host only, no device needed */
int      cmhip_failover_check(unsigned int window_log2, unsigned int n_sources, const cmhip_failover_params_t *p);
int      cmhip_failover_design(const cmhip_failover_law_desc_t *law, cmhip_failover_params_t *p);
uint32_t cmhip_failover_step(unsigned int n_sources, const cmhip_failover_params_t *p, uint32_t cur,
                             const uint32_t *live_run /* [4] */, const uint32_t *dead_run /* [4] */);

/* ---- clock-drift compensation: a variable-ratio resampler, an object of its own beside the batch -- */
/* A drift stage resamples S streams of C = 1..16 interleaved int16 channels by a ratio close to 1 that the caller
 * moves per stream between runs: what reconciles a source on its own clock (a second sound card, a network
 * contribution, the backup behind a cmhip_failover_t) with the batch's.  Exact integers; the signal is the raw int16.
 *
 * Table.  H[P][T] of int16 coefficients in units of 2^-14, P = 2^phi phases with phi in 5..8, T even in 4..64.  Row p
 *   is the filter for a fractional position of p / P input frames behind frame n.  A table is valid when H[0][0] = 0
 *   and sum_k |H[p][k]| <= 65535 for every row; anything else is COOLMIC_ERROR_INVAL.  The library appends row P
 *   itself: row 0 moved by one tap, H[P][k] = H[0][k+1] for k < T-1 and H[P][T-1] = 0 (a fraction of one whole frame
 *   is the next frame at fraction 0; H[0][0] = 0 is what makes that lose nothing).
 * Position.  Each stream has a position pos, a uint64 in units of 2^-32 input frames, measured from frame 0 of the
 *   NEXT run; 0 at creation and after reset.  Each stream has a step of 2^32 + delta with |delta| <= 2^24
 *   (+-3906 ppm); delta 0 at creation.
 * Arithmetic.  Output m = 0, 1, .. of a run has t = pos + m * step and
 *       n = t >> 32      f = t & (2^32 - 1)      p = f >> (32 - phi)      mu = (f >> (17 - phi)) & 32767
 *   and per channel
 *       a0  = sum_{k<T} H[p][k]   * x[n-k]            exact in int32
 *       a1  = sum_{k<T} H[p+1][k] * x[n-k]            exact in int32
 *       num = a0 * (32768 - mu) + a1 * mu             exact in int64
 *       y   = saturate_int16((num + 2^28) >> 29)      arithmetic shift (floor), one rounding
 *   x[i] for i < 0 is the stream's history, the last T-1 input frames: zero at creation and after reset.  With
 *   sum |H| <= 65535, |a0|, |a1| <= 65535 * 32768 < 2^31 and |num| < 2^46.
 * Counts.  Output m exists once input n exists: a run of F frames produces
 *       K = ceil((F * 2^32 - pos) / step)   outputs,   K = 0 when pos >= F * 2^32
 *   and leaves pos' = pos + K * step - F * 2^32 with 0 <= pos' < step: nothing grows with the stream's age.  With delta
 *   unchanged the concatenated output does not depend on how a stream is cut into runs; a stream that gets 0 frames
 *   keeps everything.  cmhip_drift_out_frames(pos, delta, F) is K on the host (0 for |delta| > 2^24);
 *   cmhip_drift_max_out_frames(m) is K for pos = 0, delta = -2^24 and F = max_in_frames, the most a run can give.
 * Control, each a change of the host's mirror alone (no device work, no wait; the position, the step and the count
 *   travel to the device with each run, so a call takes effect with the first output of the next run queued behind
 *   it):  cmhip_drift_set(m, stream, delta): stream -1 is every stream, |delta| > 2^24 is COOLMIC_ERROR_INVAL.
 *   cmhip_drift_seek(m, stream, frac) sets pos = frac < 2^32 (COOLMIC_ERROR_INVAL otherwise); with delta = 0 and the
 *   designed table the stage is then a fractional delay of T/2 - frac * 2^-32 frames.  cmhip_drift_reset(m, stream)
 *   zeroes the history (that on the object's stream, in order with the runs), pos and the totals, delta stays.
 *   cmhip_drift_get answers from the mirror, which advances by every run's counts: delta, pos, and the total input and
 *   output frames since creation or reset (each pointer may be NULL).
 *   cmhip_drift_ppm(ppm) = rint(ppm * 2^32 / 10^6) clamped to +-2^24 (0 for NaN): +ppm consumes more input per
 *   output; cmhip_drift_to_ppm(delta) = delta * 10^6 / 2^32.
 * cmhip_drift_run has cmhip_src_run's contract and refusals (alignment, strides, counts, in == out, NULL), with
 *   max_in_frames for the input and the run's largest output count for the output stride --
 *   cmhip_drift_max_out_frames() * C always suffices.  out_frames[] (host, S entries, may be NULL) is filled from the
 *   mirror before the call returns.  Outputs past a stream's count are not written.
 * The designed table (cmhip_drift_design(phase_log2, taps, h, cap), host only, double precision, in this order): with
 *   P = 2^phase_log2, T = taps, fc = 0.92 * 0.5, for p < P and k < T with x = k + p/P - T/2:
 *       w = I0(7.5 * sqrt(max(0, 1 - (x / (T/2))^2))) / I0(7.5)          g[p][k] = 2*fc * sinc(2*fc*x) * w
 *   (sinc and I0 as cmhip_src_design's); g[0][0] is set to 0 (its window is 0 there already: x = -T/2) BEFORE row 0 is
 *   normalised; every row is divided by its own sum, multiplied by 16384 and rounded with rint, and the difference
 *   between 16384 and the row's integer sum is added to the row's first tap of largest magnitude.  Every row then
 *   sums to exactly 16384, and so does row P: a constant input comes out as the same constant at every mu once the
 *   history is full.  cap counts the entries of h; below P*T is COOLMIC_ERROR_INVAL with nothing written.
 *   cmhip_drift_new designs phase_log2 = 7, taps = 32; cmhip_drift_new_table takes the caller's H[P][T].
 *   max_in_frames * C and cmhip_drift_max_out_frames() * C may not pass 2^31 samples.  Both return NULL on failure.
 * Where it sits: behind a source's elastic buffer and in front of whatever combines streams (failover switch,
 *   automixer, bus): its out_frames[] are the frames_per_stream of what follows.
 *
 * Servo (host only): a PI controller in integers that turns the fill of the caller's elastic buffer, read once per
 *   block, into the next delta.  State: target, kp_log2, ki_log2 (each 0..24), limit (1..2^24), integ (int64, 0 at
 *   init and reset), delta, clamped.  cmhip_drift_servo_step(servo, fill_frames), with 0 <= fill_frames < 2^31
 *   (anything else returns the last delta and changes nothing):
 *       e    = fill_frames - target
 *       raw  = e * 2^kp_log2 + (integ + e) * 2^ki_log2                     exact in int64
 *       |raw| <= limit:  integ = integ + e,  delta = raw,  clamped = 0
 *       otherwise:       delta = limit with raw's sign,  clamped = 1,  integ stays (the integrator is frozen)
 *   A fill above the target gives a positive delta: more input is consumed per output.  cmhip_drift_servo_init
 *   refuses (COOLMIC_ERROR_INVAL) a target above 2^31 - 1, a shift above 24 or a limit outside 1..2^24. */
typedef struct cmhip_drift cmhip_drift_t;
typedef struct cmhip_drift_desc {
    int          device;          /* HIP device ordinal */
    unsigned int streams;         /* S >= 1 */
    unsigned int channels;        /* 1..16 */
    size_t       max_in_frames;   /* per run and stream */
    void        *hip_stream;      /* hipStream_t to launch on, NULL: own stream */
} cmhip_drift_desc_t;
typedef struct cmhip_drift_servo {
    int64_t      target;          /* frames */
    int64_t      integ;           /* sum of e over the steps that were not clamped */
    uint32_t     kp_log2, ki_log2;
    int32_t      limit;
    int32_t      delta;           /* the last step's answer */
    uint32_t     clamped;
} cmhip_drift_servo_t;
#define CMHIP_DRIFT_DELTA_MAX (1 << 24)
cmhip_drift_t *cmhip_drift_new(const cmhip_drift_desc_t *d);
cmhip_drift_t *cmhip_drift_new_table(const cmhip_drift_desc_t *d, unsigned int phase_log2, unsigned int taps,
                                     const int16_t *h /* [2^phase_log2][taps] */);
void     cmhip_drift_free(cmhip_drift_t *m);
int      cmhip_drift_geometry(const cmhip_drift_t *m, unsigned int *phase_log2, unsigned int *taps);
size_t   cmhip_drift_max_out_frames(const cmhip_drift_t *m);
int      cmhip_drift_set(cmhip_drift_t *m, long stream, int32_t delta);
int      cmhip_drift_seek(cmhip_drift_t *m, long stream, uint64_t frac);
int      cmhip_drift_reset(cmhip_drift_t *m, long stream);
int      cmhip_drift_get(const cmhip_drift_t *m, unsigned int stream, int32_t *delta, uint64_t *pos, uint64_t *in_total,
                         uint64_t *out_total);
int      cmhip_drift_run(cmhip_drift_t *m, const void *in, size_t in_stride, size_t frames,
                         const uint32_t *frames_per_stream, void *out, size_t out_stride, uint32_t *out_frames);
int      cmhip_drift_sync(cmhip_drift_t *m);
void    *cmhip_drift_hip_stream(cmhip_drift_t *m);
/* host only, no device needed */
int      cmhip_drift_design(unsigned int phase_log2, unsigned int taps, int16_t *h, size_t cap /* entries */);
uint32_t cmhip_drift_out_frames(uint64_t pos, int32_t delta, uint32_t frames);
int32_t  cmhip_drift_ppm(double ppm);
double   cmhip_drift_to_ppm(int32_t delta);
int      cmhip_drift_servo_init(cmhip_drift_servo_t *servo, uint32_t target_frames, unsigned int kp_log2,
                                unsigned int ki_log2, int32_t limit);
int32_t  cmhip_drift_servo_step(cmhip_drift_servo_t *servo, int64_t fill_frames);
void     cmhip_drift_servo_reset(cmhip_drift_servo_t *servo);

/* ---- filter: a biquad cascade in exact integers, an object of its own beside the batch -- */
/* A filter runs each of S streams of C interleaved int16 channels (C in 1..16) through a cascade of N second-order
 * sections (N in 1..8), in exact integers: a low cut per microphone in front of a leveller, a gate or a bus, a
 * de-emphasis, a shelf, a notch.  It has cmhip_agc_t's shapes: slots, strides, alignment and refusals are
 * cmhip_agc_run's.  The stage adds no delay (its phase is the sections' own).
 *
 * Geometry, per object: sections = N in 1..8.
 * Coefficients, per stream and section, settable between runs (cmhip_iir_set, stream -1: all streams): five int32
 *   b0, b1, b2, a1, a2 in units of 2^-26 (CMHIP_IIR_ONE = 1 << 26), a0 = 1:
 *     H(z) = (b0 + b1 z^-1 + b2 z^-2) / (1 + a1 z^-1 + a2 z^-2).
 *   Valid (cmhip_iir_check): every |c| <= 2^28, |a2| < 2^26 and |a1| < 2^26 + a2 -- the stability triangle, tested on
 *   the integers.
 *
 * Arithmetic.  A stream's channels are independent.  Every section of every channel keeps u1, u2, v1, v2 (int32) and a
 *   remainder e, 0 <= e < 2^26.  Per frame:
 *     section 0 input:  u = x << 12                    int16 -> 12 fraction bits, |u| <= 2^27
 *     section k input:  u = v of section k - 1
 *     acc = b0 u + b1 u1 + b2 u2 - a1 v1 - a2 v2 + e   int64; |c| <= 2^28 and |state| < 2^31: |acc| < 2^62, exact
 *     e   = acc & (2^26 - 1);   v = acc >> 26          arithmetic shift: floor
 *     v   = clamp(v, -(2^31 - 1), 2^31 - 1)            a changed v increments the stream's `overs`
 *     u2 = u1; u1 = u; v2 = v1; v1 = v
 *     output: y = clamp((v_last + 2048) >> 12, -32768, 32767)      a changed y increments the stream's `clips`
 *   The remainder fed back into the next frame (first-order error feedback) is what keeps a low cut from stalling
 *   in a dead band: with a zero on z = 1 the output and the histories v1, v2 reach exactly zero behind a constant
 *   input and stay there (e rests at whatever value below 2^26 it has reached, where it can move nothing).
 *   Properties.  A unity section (b0 = 2^26, the rest 0) is the identity on u, and the output step gives x back: all
 *     sections are unity until set, so a new object is a copy bit for bit.  A stream given 0 frames in a run keeps
 *     everything.  Cuts: the concatenated output, both counters and the state do not depend on how a stream is cut
 *     into runs, with the sets at the same frames.
 * cmhip_iir_new: NULL for C outside 1..16, N outside 1..8, S = 0, max_frames = 0, max_frames * C >= 2^31, or a failed
 *   allocation.
 * cmhip_iir_run has cmhip_agc_run's contract: asynchronous on the object's stream; frames_per_stream (host, S entries,
 *   may be NULL) is free on return; COOLMIC_ERROR_INVAL, with nothing launched and nothing changed, when a base is not
 *   16-byte aligned, a stride is not a multiple of 8 samples or below frames * C, frames > max_frames, a count is above
 *   frames, either array would end past the address space, or the two arrays share a byte; COOLMIC_ERROR_FAULT for
 *   NULL arrays.  Outputs past a stream's count are not written.
 * cmhip_iir_set takes effect at the stream's next frame and keeps the histories and e.  It is ordered with the runs as
 *   the calls are and does not wait for the host: the coefficients live in a host mirror, and the table goes to the
 *   device on the object's stream with the next run's counts, only when it has changed since the last run.
 *   COOLMIC_ERROR_INVAL for a section cmhip_iir_check refuses, or a stream or section out of range; a refused call
 *   changes nothing.  cmhip_iir_get answers from the mirror.  A move that does not click: cmhip_iir_ramp, below.
 * cmhip_iir_reset (stream -1: all) zeroes the stream's histories and e, ordered with the runs as the calls are.  The
 *   counters, the coefficients and the ramps stay.
 *
 * Coefficient ramps (cmhip_iir_ramp): a section moves to its new coefficients over ramp_frames frames instead of
 *   between two frames, so that a low cut turned from 40 to 80 Hz or a peak pulled down by 6 dB does not click.  Every
 *   (stream, section) has a ramp of its own: two ends c0, c1 (five int32 each), `done` and R; R = 0: at rest on c1.
 *   Position.  A section ramps while done < R.  Frame f (from 0) of its stream's next run uses the section
 *     c(p(done + f + 1)) with p(n) = cmhip_mix_ramp_position(n, R), the mixer's, in units of 2^-15; frames past the
 *     ramp use c1.  After a run of n frames done = min(done + n, R); a section whose ramp is over is at rest
 *     (done = R = 0).  A stream given 0 frames does not advance.  R in 2..2^20 (CMHIP_IIR_RAMP_MAX).
 *   The section at position p, 0 <= p <= 32768.  For a pair of ends (x0, x1) let N(x0, x1) = x0 (32768 - p) + x1 p,
 *     int64, |N| < 2^45.
 *       b0(p), b2(p), a1(p) = sgn(N) (|N| >> 15)         truncated towards zero, as the mixer truncates
 *       a2(p)               = -((-N) >> 15)              rounded up
 *       s(p)                = sgn(N) (|N| >> 15) of the ends s0 = b0 + b1 + b2 of c0 and s1 of c1 (|s| <= 3 * 2^28)
 *       b1(p)               = clamp(s(p) - b0(p) - b2(p), -2^28, 2^28)
 *   Why these roundings.  c(0) = c0 and c(32768) = c1 exactly.  |a1(p)| does not exceed the exact convex combination of
 *     the ends and a2(p) is not below it, so every c(p) passes cmhip_iir_check whenever both ends do: the stability
 *     triangle is convex, and rounding a1 and a2 each to nearest could not promise that on its edge.  Where both ends
 *     have b0 + b1 + b2 = 0 -- every HIGHPASS and HIGHPASS1 of cmhip_iir_design -- s(p) = 0, b1(p) = -(b0(p) + b2(p))
 *     and the clamp does not act: the zero stays on z = 1 exactly through a whole low-cut sweep.  The clamp acts only
 *     in corners of the coefficient range, where the unclamped b1 can pass 2^28 by one.
 *   The arithmetic of a frame does not change: the section runs with that frame's c(p), e and the histories carry on,
 *     and |c| <= 2^28 still gives |acc| < 2^62.  A SECTION VALID AT EVERY FRAME DOES NOT MAKE A TIME-VARYING FILTER
 *     BOUNDED: stability of each frozen c(p) says nothing about the filter that moves through them.  What bounds it is
 *     the inner clamp, and `overs` counts where it acted.
 *   cmhip_iir_ramp (stream -1: all streams) starts from the section IN FORCE, which is c(p(done)) while a ramp runs: a
 *     retarget in the middle of a ramp is allowed and is itself click-free, and a long sweep is a chain of short ramps.
 *     ramp_frames 0 or 1 is exactly cmhip_iir_set.  COOLMIC_ERROR_INVAL for ramp_frames above 2^20, a target that
 *     cmhip_iir_check refuses, or a stream or section out of range; COOLMIC_ERROR_FAULT for NULL; a refused call changes
 *     nothing.  cmhip_iir_set on a ramping section ends that ramp with a step.  cmhip_iir_get returns the section in
 *     force.  cmhip_iir_ramp_state: done and R of a section (0, 0 at rest); either pointer may be NULL.
 *   Ordering.  Like a set, a ramp touches the host mirror only, needs no host wait and is ordered with the runs as the
 *     calls are.  The host sees every run's counts and advances the mirror by them, so cmhip_iir_ramp_state and
 *     cmhip_iir_get ask no device.  While any section ramps, or the table has changed, the table travels behind the
 *     run's counts; in a run at whose start a section ramps it holds both ends, done and R of every section.  A filter
 *     that never ramps launches what it always did.
 *   Cuts.  Output, `clips`, `overs` and every section's state do not depend on how a stream is cut into runs, with the
 *     sets, ramps and resets at the same frames.
 *   cmhip_iir_ramp_section (host only): c(p) between two sections, p above 32768 counting as 32768; an end's coefficient
 *     outside +-2^28, which no valid section has, counts as the bound.  NULL: nothing is written.
 * cmhip_iir_state: synchronous (it waits for the object's stream).  Per stream, S entries each: clips[s] and overs[s];
 *   clear != 0 zeroes both counters after reading them.  Either pointer may be NULL.
 * cmhip_iir_check (host only): 0 for a valid section, else COOLMIC_ERROR_INVAL.
 * cmhip_iir_design (host only): one section from the Audio EQ Cookbook's formulas (R. Bristow-Johnson), w0 = 2 pi f0 /
 *   rate, alpha = sin w0 / (2 q), A = 10^(gain_db / 40); every coefficient is rint(c / a0 * 2^26):
 *     BYPASS      unity
 *     HIGHPASS    b = ((1 + cos) / 2, -(1 + cos), (1 + cos) / 2), a = (1 + alpha, -2 cos, 1 - alpha)
 *     LOWPASS     b = ((1 - cos) / 2, 1 - cos, (1 - cos) / 2), the same a
 *     LOWSHELF, HIGHSHELF, PEAK, NOTCH      the cookbook's, the shelves' slope through q (2 sqrt(A) alpha)
 *     HIGHPASS1   K = tan(w0 / 2): b = (1, -1, 0) / (1 + K), a1 = (K - 1) / (1 + K), b2 = a2 = 0: a DC blocker
 *     LOWPASS1    b = (K, K, 0) / (1 + K), the same a1: a 50 / 75 us de-emphasis is f0 = 3183.1 / 2122.1 Hz
 *   For HIGHPASS b1 := -(b0 + b2) and for HIGHPASS1 b1 := -b0 on the integers, so the zero lies on z = 1 exactly
 *   and the DC gain is 0, not a small number.  gain_db is read by the shelves and PEAK, q by all but the one-pole
 *   kinds and BYPASS; all four values are checked for every kind.  COOLMIC_ERROR_INVAL for non-finite inputs, f0
 *   outside (0, rate / 2), q <= 0, an unknown kind, or a result that cmhip_iir_check refuses; COOLMIC_ERROR_FAULT for
 *   NULL.
 * cmhip_iir_response_db (host only): the magnitude in dB at f Hz of the cascade of the n sections AS THE INTEGERS
 *   REALISE IT; -inf on a zero, NaN for NULL or a rate that is not positive. */
#define CMHIP_IIR_ONE (1 << 26)
#define CMHIP_IIR_RAMP_MAX (1u << 20)
enum {
    CMHIP_IIR_BYPASS = 0, CMHIP_IIR_HIGHPASS = 1, CMHIP_IIR_LOWPASS = 2, CMHIP_IIR_LOWSHELF = 3, CMHIP_IIR_HIGHSHELF = 4,
    CMHIP_IIR_PEAK = 5, CMHIP_IIR_NOTCH = 6, CMHIP_IIR_HIGHPASS1 = 7, CMHIP_IIR_LOWPASS1 = 8
};
typedef struct cmhip_iir cmhip_iir_t;
typedef struct cmhip_iir_desc {
    int          device;          /* HIP device ordinal */
    unsigned int streams;         /* S >= 1 */
    unsigned int channels;        /* 1..16 */
    unsigned int sections;        /* N in 1..8 */
    size_t       max_frames;      /* per run and stream */
    void        *hip_stream;      /* hipStream_t to launch on, NULL: own stream */
} cmhip_iir_desc_t;
typedef struct cmhip_iir_section {
    int32_t b0, b1, b2, a1, a2;   /* units of 2^-26 */
} cmhip_iir_section_t;
typedef struct cmhip_iir_design_desc {
    int    kind;                  /* CMHIP_IIR_... */
    double rate;                  /* frames per second */
    double f0;                    /* Hz, inside (0, rate / 2) */
    double q;                     /* > 0 */
    double gain_db;               /* shelves and PEAK */
} cmhip_iir_design_desc_t;
cmhip_iir_t *cmhip_iir_new(const cmhip_iir_desc_t *d);
void     cmhip_iir_free(cmhip_iir_t *m);
int      cmhip_iir_set(cmhip_iir_t *m, long stream, unsigned int section, const cmhip_iir_section_t *c);
int      cmhip_iir_get(const cmhip_iir_t *m, unsigned int stream, unsigned int section, cmhip_iir_section_t *c);
int      cmhip_iir_ramp(cmhip_iir_t *m, long stream, unsigned int section, const cmhip_iir_section_t *target,
                        uint32_t ramp_frames);
int      cmhip_iir_ramp_state(const cmhip_iir_t *m, unsigned int stream, unsigned int section, uint32_t *done,
                              uint32_t *ramp_frames);                   /* either may be NULL */
int      cmhip_iir_run(cmhip_iir_t *m, const void *in, size_t in_stride, size_t frames,
                       const uint32_t *frames_per_stream, void *out, size_t out_stride);
int      cmhip_iir_reset(cmhip_iir_t *m, long stream);
int      cmhip_iir_state(cmhip_iir_t *m, uint64_t *clips /* [S] */, uint64_t *overs /* [S] */, int clear);
int      cmhip_iir_sync(cmhip_iir_t *m);
void    *cmhip_iir_hip_stream(cmhip_iir_t *m);
/* host only, no device needed */
int      cmhip_iir_check(const cmhip_iir_section_t *c);
int      cmhip_iir_design(const cmhip_iir_design_desc_t *d, cmhip_iir_section_t *c);
double   cmhip_iir_response_db(const cmhip_iir_section_t *sections, unsigned int n, double rate, double f);
void     cmhip_iir_ramp_section(const cmhip_iir_section_t *c0, const cmhip_iir_section_t *c1, uint32_t p,
                                cmhip_iir_section_t *out);              /* c(p) */

/* ---- noise suppressor: a spectral gate in exact integers, an object of its own beside the batch -- */
/* A noise suppressor takes steady background noise -- room tone, fans, hiss -- out of each of S streams of C
 * interleaved int16 channels (C in 1..16), per frequency bin and in exact integers: where a bin's power does not rise
 * above the noise profile learned for it, the bin is turned down towards a floor.  It belongs in front of the leveller,
 * which would otherwise lift the noise of quiet speakers.  It has cmhip_agc_t's shapes: slots, strides, alignment and
 * refusals are cmhip_agc_run's.  Every channel of every stream is a row of its own, with its own profile and gains.
 *
 * Geometry, per object: fft_log2 = n in 8..12, N = 2^n frames per block, hop H = N / 2.  A row's frames are counted
 *   since creation or the last cmhip_denoise_reset; block j covers its frames [j H, j H + N) and is computed in the run
 *   in which its last frame arrives, as the spectrum meter's blocks are.  Frames before frame 0 are zero.
 * Parameters, per stream, settable between runs (cmhip_denoise_set, stream -1: all streams); a block uses the
 *   parameters of the last cmhip_denoise_set queued before the run that completes it:
 *     floor                 0..32768    units of 2^-15: the smallest gain of a bin (32768: nothing is removed)
 *     over (beta)           0..255      units of 2^-4: the profile is multiplied by it before the comparison
 *     rise_shift, fall_shift  0..8      a bin's gain moves by 2^-shift of its distance to the target per block
 *
 * The subtractive form.  The stage computes the REMOVED part r and subtracts it from the delayed input:
 *     y[m + D] = clamp16(x[m] - r[m]),  D = N - 1 (cmhip_denoise_delay),
 *   and every sample the clamp changes increments the stream's `clips`.  With every gain at 32768 the removed spectrum
 *   is zero, the inverse transform of zeros is zero, and the output is the input delayed by D, bit for bit, by
 *   construction: the synthesis window need not sum to one exactly.  Output frames 0 .. D - 1 are 0 (x before frame 0).
 *   Block 0 covers frames [0, N), so frames 0 .. H - 1 are covered by one block only: there the removal fades in with
 *   the window's square.
 *
 * Arithmetic, per row and block j:
 *   Window.  sw[i] = min(32767, rint(32768 sin(pi i / N))) for i <= N / 2, sw[N - i] = sw[i] (cmhip_denoise_window).
 *     v[i] = x[j H + i] * sw[i], exact in int32.
 *   Forward transform.  The spectrum meter's, to the bit (above, "spectrum"): the same twiddles, bit reversal, stages and
 *     roundings, X = DFT(v) / N with every butterfly output (a 2^30 +- P + 2^30) >> 31.  |X| <= 2^30 per component.
 *     p[k] = (uint64)(re^2 + im^2) >> 16, k = 0 .. N / 2.
 *   Target gain.  Np[k]: the row's profile, uint64, at most 2^52.  t = (Np[k] * beta) >> 4 (below 2^60).
 *     If p <= t: target = floor.  Otherwise sh = max(0, bitlength(p) - 34), ps = p >> sh, ts = t >> sh, and
 *       target = max(floor, isqrt(((ps - ts) << 30) / ps))
 *     an unsigned 64-bit division (ps < 2^34, ts <= ps: the numerator fits) and the exact integer root, at most 32768:
 *     the Wiener-like gain sqrt((p - t) / p).  cmhip_denoise_gain(p, np, over, floor) is this rule as code.
 *   Smoothing.  g[k] in 0..32768, 32768 at frame 0.  d = target - g; d > 0: g += max(1, d >> rise_shift); d < 0:
 *     g -= max(1, (-d) >> fall_shift).  No dead band: g reaches every target; a shift of 0 is instant.
 *   Learning (cmhip_denoise_learn, per stream).  A block completed while the stream learns, and while cnt < 65536, does
 *     acc[k] = (cnt ? acc[k] : 0) + p[k], cnt += 1, Np[k] = acc[k] / cnt -- AFTER its own gains: a block's gains use
 *     the profile in force before it.  Turning learning on from off sets cnt = 0 (so the sums start anew); later
 *     learning blocks beyond cnt = 65536 are ignored.  p <= 2^45 (|X| <= 2^30 per component), so acc <= 65536 * 2^45 = 2^61 fits uint64.
 *   Removed spectrum.  Z[k] = (X[k] * (32768 - g[k]) + 2^16) >> 17 on both components, arithmetic shift (int64 product):
 *     two bits of headroom.  Im Z[0] = Im Z[N/2] = 0.  Z[N - k] = conj(Z[k]).
 *   Inverse transform.  The same decimation in time over bit-reversed input, the twiddles conjugated (Wr, -Wi), no
 *     halving: every butterfly output is sat32((a 2^30 +- P + 2^29) >> 30), the exact int64 sum (|a| <= 2^31,
 *     |P| <= 2^61.5) shifted arithmetically and clamped to int32; every clamped component increments the stream's
 *     `sat`.  The imaginary output is discarded; t[i] is the real one.  An implementation may arrange the work as it
 *     likes but reproduces every stage's rounded and clamped values.
 *   Synthesis and overlap-add.  c[i] = (t[i] * sw[i] + 2^14) >> 15, an int64 product, an int32 result.  Frame m sums the
 *     c of the one or two blocks that cover it, in int64: r[m] = (sum + 2^12) >> 13.
 *   Properties.  Cuts: the concatenated output, the counters, g, Np and the state do not depend on how a stream is cut
 *     into runs, per-stream counts and counts of 0 included, with the calls at the same frames.  A row's output never
 *     depends on another row.
 * State per row: the last N - 1 inputs (they serve the next blocks and the delayed dry signal); the overlap-add of
 *   the last completed block's span, N int32 -- its upper half are the not-yet-completed sums, its lower half holds the
 *   finished r that the output, D frames behind, has not reached yet (at most H - 1 of them); g, Np, acc.  Per stream:
 *   cnt, clips, sat.
 * cmhip_denoise_new: NULL for C outside 1..16, S = 0, fft_log2 outside 8..12, max_frames = 0, max_frames * C >= 2^31,
 *   S * C >= 2^31 or a failed allocation.  Every stream starts with floor 32768, over 16, both shifts 0, learning off
 *   and a zero profile: a pure delay, until cmhip_denoise_set says otherwise.
 * cmhip_denoise_run has cmhip_delay_run's contract (asynchronous on the object's stream, frames_per_stream free on
 *   return, the same refusals).  Outputs past a stream's count are not written.
 * cmhip_denoise_set, _learn and _reset are ordered with the runs as the calls are: they touch a host mirror that every
 *   run hands to the device with its counts, need no host wait and touch no device memory.  COOLMIC_ERROR_INVAL for
 *   parameters or a stream out of range; a refused call changes nothing.  cmhip_denoise_get answers from the mirror.
 * cmhip_denoise_set_profile(m, stream, channel, np[N / 2 + 1]): the row's profile, copied from a staged copy in the
 *   object's stream order (np is free on return); acc and cnt stay.  COOLMIC_ERROR_BUSY while the mirror says the stream
 *   learns, COOLMIC_ERROR_INVAL for a value above 2^52 or indices out of range; a refused call changes nothing.
 * cmhip_denoise_get_profile: synchronous.  np[N / 2 + 1] and gain[N / 2 + 1] of the row; either may be NULL.
 * cmhip_denoise_reset (stream -1: all): the stream's next frame is frame 0 again: history and overlap are zero, g is
 *   32768, learning ends.  The profile, the parameters, cnt and the counters stay.
 * cmhip_denoise_state: synchronous.  Per stream, S entries each: clips, sat, learned_blocks = cnt; clear != 0 zeroes
 *   clips and sat after reading them.  Any of the three pointers may be NULL.
 * cmhip_denoise_check (host only): 0 for a valid fft_log2 and parameter set (params may be NULL), else INVAL.
 * cmhip_denoise_design (host only): floor = rint(32768 * 10^(-reduction_db / 20)), over = min(255,
 *   rint(16 * 10^(over_db / 10))), and for each of attack_ms (rise) and release_ms (fall) the nearest shift for the hop:
 *   with h = ms * rate / 1000 / H hops, shift = 0 for h <= 1, else min(8, rint(log2(h))).  COOLMIC_ERROR_INVAL for a
 *   non-finite input, a rate that is not positive, an fft_log2 that is no integer in 8..12, a negative reduction or time.
 * cmhip_denoise_gain (host only): the target rule; 0 for np above 2^52, over above 255 or floor above 32768. */
typedef struct cmhip_denoise cmhip_denoise_t;
typedef struct cmhip_denoise_desc {
    int          device;          /* HIP device ordinal */
    unsigned int streams;         /* S >= 1 */
    unsigned int channels;        /* 1..16 */
    unsigned int fft_log2;        /* n in 8..12: blocks of 2^n frames, hop 2^(n-1) */
    size_t       max_frames;      /* per run and stream */
    void        *hip_stream;      /* hipStream_t to launch on, NULL: own stream */
} cmhip_denoise_desc_t;
typedef struct cmhip_denoise_params {
    uint16_t floor;
    uint8_t  over, rise_shift, fall_shift;
} cmhip_denoise_params_t;
typedef struct cmhip_denoise_law_desc {
    double rate;                  /* frames per second */
    double fft_log2;              /* the object's n */
    double reduction_db;          /* >= 0: the most a bin is turned down */
    double over_db;               /* over-subtraction: dB the profile is raised by before the comparison */
    double attack_ms, release_ms; /* >= 0: how fast a bin's gain rises / falls */
} cmhip_denoise_law_desc_t;
cmhip_denoise_t *cmhip_denoise_new(const cmhip_denoise_desc_t *d);
void     cmhip_denoise_free(cmhip_denoise_t *m);
int      cmhip_denoise_set(cmhip_denoise_t *m, long stream, const cmhip_denoise_params_t *p);
int      cmhip_denoise_get(const cmhip_denoise_t *m, unsigned int stream, cmhip_denoise_params_t *p);
int      cmhip_denoise_learn(cmhip_denoise_t *m, long stream, int on);
int      cmhip_denoise_set_profile(cmhip_denoise_t *m, unsigned int stream, unsigned int channel,
                                   const uint64_t *np /* [N/2 + 1] */);
int      cmhip_denoise_get_profile(cmhip_denoise_t *m, unsigned int stream, unsigned int channel,
                                   uint64_t *np /* [N/2 + 1] */, uint32_t *gain /* [N/2 + 1] */);
int      cmhip_denoise_run(cmhip_denoise_t *m, const void *in, size_t in_stride, size_t frames,
                           const uint32_t *frames_per_stream, void *out, size_t out_stride);
int      cmhip_denoise_reset(cmhip_denoise_t *m, long stream);
int      cmhip_denoise_state(cmhip_denoise_t *m, uint64_t *clips /* [S] */, uint64_t *sat /* [S] */,
                             uint32_t *learned_blocks /* [S] */, int clear);
int      cmhip_denoise_sync(cmhip_denoise_t *m);
void    *cmhip_denoise_hip_stream(cmhip_denoise_t *m);
size_t   cmhip_denoise_delay(const cmhip_denoise_t *m);
/* host only, no device needed */
int      cmhip_denoise_check(unsigned int fft_log2, const cmhip_denoise_params_t *p);
int      cmhip_denoise_window(unsigned int fft_log2, int16_t *win /* [N] */);
int      cmhip_denoise_design(const cmhip_denoise_law_desc_t *law, cmhip_denoise_params_t *p);
uint32_t cmhip_denoise_gain(uint64_t p, uint64_t np, unsigned int over, unsigned int floor);

/* ---- node-global VU ---------------------------------- */
/* Reduces this batch's current windows over its streams into one record of
 * CMHIP_NODE_WORDS int64 words written to device memory `dst` (asynchronous):
 *   [0..15]  sum of squares per channel      -> combine across GPUs with SUM
 *   [16]     frames summed over streams      -> SUM
 *   [17..32] packed peak key per channel     -> combine with MAX
 *   [33]     packed global peak key          -> MAX
 * Keys order by (|peak|, earliest frame, lowest global stream id); decode with
 * cmhip_node_finish().  A host that brings its own collective reduces `dst` itself; one
 * that wants the engine to do it uses cmhip_node_t below. */
#define CMHIP_NODE_WORDS      34
#define CMHIP_NODE_SUM_WORDS  17
int cmhip_batch_vu_node_partial(cmhip_batch_t *b, void *dst_device, uint64_t first_global,
                                uint64_t global_step);
/* the same record straight to host memory, words[CMHIP_NODE_WORDS]; waits for the batch's last run */
int cmhip_batch_vu_node_record(cmhip_batch_t *b, int64_t *words_host, uint64_t first_global,
                               uint64_t global_step);
/* host: turn a combined record into a result (frames = total frames over streams) */
int cmhip_node_finish(const int64_t *words, unsigned int channels, unsigned int rate,
                      coolmic_vumeter_result_t *out);

/* The exchange itself, in C over RCCL (xGMI inside a node) -- no Python, no torch: one
 * cmhip_node_t per GPU (= per rank; one process per GPU, or one thread per GPU of one
 * process).  It owns two sets of `max_records` record slots on its device, so that the
 * records of B blocks travel in ONE pair of collectives (the exchange is latency bound) and
 * a set can be exchanged while the next blocks fill the other.  Per set the sums of all
 * slots are contiguous and so are the keys:
 *     ncclAllReduce(sums, B*17, ncclInt64,  ncclSum)     words 0..16  of every record
 *     ncclAllReduce(keys, B*17, ncclUint64, ncclMax)     words 17..33 of every record
 * issued as one RCCL group on the node's own HIP stream.  librccl is loaded when the first
 * node is created (dlopen of librccl.so.1; a host that never asks for the node-global VU
 * never maps it). */
typedef struct cmhip_node cmhip_node_t;
#define CMHIP_NODE_ID_BYTES 128
/* rank 0 makes the id (ncclGetUniqueId) and hands the 128 bytes to the other ranks by
 * whatever means the host has (a socket, a file, shared memory of one process) */
int           cmhip_node_unique_id(void *id128);
/* collective over all ranks (ncclCommInitRank): every rank calls it with the same id */
cmhip_node_t *cmhip_node_new(int device, int nranks, int rank, const void *id128,
                             unsigned int max_records);
void          cmhip_node_free(cmhip_node_t *n);
int           cmhip_node_ranks(const cmhip_node_t *n);
/* "hip=<path of the HIP runtime the engine is bound to> rccl=<path of the librccl it loaded>": librccl is
 * taken from next to that runtime (a process that also imported a torch wheel holds a second pair) */
const char   *cmhip_node_runtime(void);
/* the batch's current windows -> slot `slot` of set `set` (asynchronous, beside the batch's
 * next run; the batch must live on the node's device).  Waits, on the device, for the last
 * exchange of that set, and clears the set when its first slot after an exchange is filled:
 * fetch a set's results before putting the next block into it. */
int cmhip_node_partial(cmhip_node_t *n, cmhip_batch_t *b, unsigned int set, unsigned int slot,
                       uint64_t first_global, uint64_t global_step);
/* all-reduce slots 0..count-1 of `set` over the ranks, in place, after everything the batch
 * `after` (may be NULL) has queued so far; asynchronous -- the host does not wait */
int cmhip_node_allreduce(cmhip_node_t *n, unsigned int set, unsigned int count, cmhip_batch_t *after);
/* wait for the exchange of `set` and copy its combined records to the host:
 * words[count][CMHIP_NODE_WORDS], ready for cmhip_node_finish() */
int cmhip_node_fetch(cmhip_node_t *n, unsigned int set, unsigned int count, int64_t *words);
/* "replicas only" form of the same combine on the host (no collective): SUM / MAX of `nranks`
 * records into out[CMHIP_NODE_WORDS]; the parity check of the RCCL path */
int cmhip_node_merge_host(const int64_t *records, unsigned int nranks, int64_t *out);

/* ---- measurement ----------------------------------------------------------- */
/* enable = 1: every run is bracketed by hipEvents on the batch's stream (stamped by the kernel's own
 * dispatch); enable = n > 1: every n-th run only -- the events cost a run about 5 us of its stream's time,
 * a sample of the launches leaves the throughput as it is without them; 0: off */
int cmhip_batch_timing(cmhip_batch_t *b, int enable);
/* sums since the last call: milliseconds and launches of the dominant kernel; resets */
int cmhip_batch_timing_read(cmhip_batch_t *b, double *kernel_ms, unsigned int *launches);
/* plain HBM ceilings measured with the same buffers: mode 0 read-only sum, 1 copy.
 * Returns GB/s of algorithmic bytes (read: bytes; copy: 2*bytes) or <0 on error. */
double cmhip_batch_ceiling(cmhip_batch_t *b, int mode, size_t frames, int iters);

#ifdef __cplusplus
}
#endif
#endif
