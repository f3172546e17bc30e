/*
 * vumeter.h -- terminal analyser: per-channel and global peak + power, on the GPU.
 *
 * Drop-in for the reference stage (ref: include/coolmic-dsp/vumeter.h:42-107,
 * src/vumeter.c).  Accumulation (first-max-|x| peak, exact 64-bit sum of squares)
 * runs in HIP kernels; the dB values are finished on the host in double exactly as
 * the reference does (ref: src/vumeter.c:201-212), so results are bit-identical.
 */
#ifndef __COOLMIC_DSP_VUMETER_H__
#define __COOLMIC_DSP_VUMETER_H__

#include <stdint.h>
#include <sys/types.h>
#include "ro-compat.h"
#include "iohandle.h"

#ifdef __cplusplus
extern "C" {
#endif

#define COOLMIC_DSP_VUMETER_MAX_CHANNELS 16

typedef struct coolmic_vumeter coolmic_vumeter_t;

/* Result of one measuring window.  Field order and types are the reference's
 * (ref: vumeter.h:48-83); 192 bytes on LP64.  Peaks are the signed value of the
 * first sample that reached the largest magnitude; powers are in dB relative to
 * full scale, never above 0, -inf for silence. */
typedef struct {
    uint_least32_t rate;
    unsigned int channels;
    size_t frames;
    int16_t global_peak;
    double global_power;
    int16_t channel_peak[COOLMIC_DSP_VUMETER_MAX_CHANNELS];
    double channel_power[COOLMIC_DSP_VUMETER_MAX_CHANNELS];
} coolmic_vumeter_result_t;

coolmic_vumeter_t  *coolmic_vumeter_new(const char *name, igloo_ro_t associated,
                                        uint_least32_t rate, unsigned int channels);
int                 coolmic_vumeter_reset(coolmic_vumeter_t *self);
int                 coolmic_vumeter_attach_iohandle(coolmic_vumeter_t *self,
                                                    coolmic_iohandle_t *handle);
/* pulls at most maxlen bytes (-1: internal default of 1024) and accounts the whole
 * frames; returns the bytes pulled, -1 on error with nothing buffered */
ssize_t             coolmic_vumeter_read(coolmic_vumeter_t *self, ssize_t maxlen);
/* COOLMIC_ERROR_INVAL while the window holds no frame; resets the window on success */
int                 coolmic_vumeter_result(coolmic_vumeter_t *self,
                                           coolmic_vumeter_result_t *result);

/* ---- addition of this implementation (not in the reference) ---- */

/* Which GPU a meter with a launch of its own accounts its frames on (a meter that shares the launch of the
 * transform above it uses that transform's, coolmic_transform_set_device()).  COOLMIC_ERROR_BUSY once the meter
 * has device state of its own, COOLMIC_ERROR_INVAL for a device the process does not see.  Without a call:
 * $COOLMIC_HIP_DEVICE, else 0. */
int                 coolmic_vumeter_set_device(coolmic_vumeter_t *self, int device);

/* Result of one true-peak window (ITU-R BS.1770 Annex 2 / EBU R128: the maximum of the 4x oversampled signal), as
 * the batch engine (cmhip_batch_tp_result, <coolmic_hip.h>) and the group (coolmic_group_true_peak, group.h) report
 * it; the per-stream coolmic_vumeter_t does not measure it.  Peaks are magnitudes of the integer filter's output in
 * units of 2^-28 of full scale (268435456 = 8192 * 32768 is 0 dBTP; the largest possible value is 542986257);
 * the dBTP values are 20 * log10(peak / 268435456.) in double, NOT capped at 0 (true peak may reach +6.12 dBTP),
 * -inf for a silent window.  224 bytes on LP64. */
typedef struct {
    uint_least32_t rate;
    unsigned int channels;
    size_t frames;
    uint32_t global_peak;
    uint32_t channel_peak[COOLMIC_DSP_VUMETER_MAX_CHANNELS];
    double global_dbtp;
    double channel_dbtp[COOLMIC_DSP_VUMETER_MAX_CHANNELS];
} coolmic_truepeak_result_t;

/* Result of one phase-correlation window, as the batch engine (cmhip_batch_corr_result, <coolmic_hip.h>) and the
 * group (coolmic_group_correlation, group.h) report it; the per-stream coolmic_vumeter_t does not measure it.  For
 * each of `pairs` channel pairs (a[i], b[i]) of the transformed stream: the exact integer sums energy_a = sum x_a^2,
 * energy_b = sum x_b^2 and cross = sum x_a * x_b over the window's frames, the correlation cross / sqrt(energy_a *
 * energy_b) in [-1, 1] (0.0 when a leg is silent) and the balance 10 * log10(energy_a / energy_b) in dB (0.0 when
 * both legs are silent, -inf / +inf when one is); the arithmetic is specified to the bit in <coolmic_hip.h>.
 * Entries at and beyond `pairs` are zero.  360 bytes on LP64. */
typedef struct {
    uint_least32_t rate;
    unsigned int channels;
    size_t frames;
    unsigned int pairs;
    unsigned char a[8], b[8];
    uint64_t energy_a[8], energy_b[8];
    int64_t cross[8];
    double correlation[8];
    double balance_db[8];
} coolmic_correlation_result_t;

/* Result of one spectrum window, as the batch engine (cmhip_batch_spec_result, <coolmic_hip.h>) and the group
 * (coolmic_group_spectrum, group.h) report it; the per-stream coolmic_vumeter_t does not measure it.  The window
 * accounted `frames` frames and summed `blocks` blocks of 2^fft_log2 frames that completed in it.  For each of the
 * `selected` transformed channels channel[c] and each of `bands` bands -- band k holds the bins edges[k] <= bin <
 * edges[k + 1] -- power[c][k] is the exact integer sum of the blocks' bin powers and db[c][k] its level,
 * cmhip_spec_db(power, blocks): 0 dB is a full-scale sine whose main lobe lies in the band, -inf an empty band.  The
 * arithmetic is specified to the bit in <coolmic_hip.h>.  Entries beyond what is in use are zero.  4208 bytes on LP64. */
typedef struct {
    uint_least32_t rate;
    unsigned int channels;
    size_t frames;
    size_t blocks;
    unsigned int fft_log2;
    unsigned int bands;
    unsigned int selected;
    uint16_t edges[33];
    unsigned char channel[8];
    uint64_t power[8][32];
    double db[8][32];
} coolmic_spectrum_result_t;

/* Result of one signal-watch window, as the batch engine (cmhip_batch_watch_result, <coolmic_hip.h>) and the group
 * (coolmic_group_watch, group.h) report it; the per-stream coolmic_vumeter_t does not measure it.  Over the window's
 * `frames` frames of the transformed stream, with the batch's thresholds quiet, rail and clip_run (K) as they were:
 * dead air (every channel quiet), per channel the quiet frames, and per channel the samples at the rail -- each as the
 * number of such frames, the longest run of consecutive ones (a run that began before the window counts with its full
 * length if it continues into it) and, for dead air and quiet, the run still going at the window's last frame;
 * clip_events counts the runs at the rail that reached K frames in this window, each once.  sum is the exact sum of
 * the channel's samples and dc = (double)sum / (double)frames / 32768.0.  All integers are exact and independent of
 * how the stream was cut into runs; the arithmetic is specified in <coolmic_hip.h>.  Entries at and beyond `channels`
 * are zero.  1080 bytes on LP64. */
typedef struct {
    uint_least32_t rate;
    unsigned int channels;
    size_t frames;
    unsigned int quiet, rail, clip_run;
    uint64_t dead_frames, dead_longest, dead_current;
    uint64_t quiet_frames[COOLMIC_DSP_VUMETER_MAX_CHANNELS], quiet_longest[COOLMIC_DSP_VUMETER_MAX_CHANNELS],
             quiet_current[COOLMIC_DSP_VUMETER_MAX_CHANNELS];
    uint64_t clip_samples[COOLMIC_DSP_VUMETER_MAX_CHANNELS], clip_events[COOLMIC_DSP_VUMETER_MAX_CHANNELS],
             clip_longest[COOLMIC_DSP_VUMETER_MAX_CHANNELS];
    int64_t sum[COOLMIC_DSP_VUMETER_MAX_CHANNELS];
    double dc[COOLMIC_DSP_VUMETER_MAX_CHANNELS];
} coolmic_watch_result_t;

/* Programme loudness of one stream (ITU-R BS.1770 / EBU R128: K-weighting, 100 ms sub-blocks, 400 ms momentary,
 * 3 s short-term, gated integrated loudness), as the batch engine (cmhip_batch_loud_result, <coolmic_hip.h>) and the
 * group (coolmic_group_loudness, group.h) report it; the per-stream coolmic_vumeter_t does not measure it.  The
 * arithmetic is specified to the bit in <coolmic_hip.h>.  frames: since loudness was turned on or reset; blocks:
 * complete 100 ms sub-blocks among them; gated_blocks: the 400 ms blocks that passed both gates and make up
 * `integrated`.  The four loudness values are LUFS doubles, -inf while there is nothing to report (momentary:
 * fewer than 4 sub-blocks, short_term: fewer than 30, integrated and relative_threshold: no block above -70 LUFS).
 * 64 bytes on LP64. */
typedef struct {
    uint_least32_t rate;
    unsigned int channels;
    size_t frames;
    size_t blocks;
    size_t gated_blocks;
    double momentary;
    double short_term;
    double integrated;
    double relative_threshold;
} coolmic_loudness_result_t;

#ifdef __cplusplus
}
#endif
#endif
