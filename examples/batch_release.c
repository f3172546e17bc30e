/*
 * batch_release.c -- what the limiter's release stage is for, from plain C (include/coolmic_hip.h, "peak limiter",
 * "release stage"): a 50 Hz tone at -1 dBFS is driven 6 dB over a ceiling of -1 dBFS (threshold 29204, drive 8192)
 * through two limiters with a look-ahead of 64 frames and no hold -- one without a release stage (release_log2 0: the
 * gain returns to unity over the 64 frames of the attack, so it follows the waveform, 100 times a second between unity
 * at the zero crossings and one half at the crests) and one with release_log2 11 (the gain rises by at most 16 / 32768
 * per frame, 2048 frames from nothing to unity, so it stays down between two crests 480 frames apart).
 * Prints one line of geometry, then per limiter
 * "release_log2=...: peak=... min_gain=... gain_min=... gain_max=... range=..." -- the meter, and the range of the gain
 * over the last period of the tone, estimated from the output against the delayed input (y * 2^27 / (x * drive), in
 * units of unity, over the frames whose input magnitude is at least 4096) -- and exits non-zero if a sample passes the
 * ceiling or if the range with the release is not smaller than the range without it.
 *
 *   cc -I include examples/batch_release.c -L libcoolmic-dsp_amd/lib -lcoolmic-dsp-hip -lm \
 *      -Wl,-rpath,$PWD/libcoolmic-dsp_amd/lib -o batch_release && ./batch_release
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <coolmic-dsp/coolmic-dsp.h>
#include <coolmic_hip.h>

enum { RATE = 48000, FRAMES = 48000, TONE_HZ = 50, PERIOD = RATE / TONE_HZ, LOOKAHEAD_LOG2 = 6, HOLD = 0, DRIVE = 8192,
       AMPLITUDE = 29204, AUDIBLE = 4096 };

int main(void)
{
    static int16_t x[FRAMES], y[FRAMES];
    static const unsigned release[2] = {0, 11};
    cmhip_batch_desc_t sd = {0};
    cmhip_lim_desc_t ld = {0};
    cmhip_batch_t *src, *dst;
    const unsigned threshold = cmhip_lim_threshold_dbtp(-1.0);
    double range[2] = {0.0, 0.0};
    unsigned i, k;
    int over = 0;

    sd.device = 0; sd.streams = 1; sd.channels = 1; sd.rate = RATE; sd.max_frames = FRAMES; sd.flags = CMHIP_VU;
    src = cmhip_batch_new(&sd);
    dst = cmhip_batch_new(&sd);
    if (!src || !dst) {
        fprintf(stderr, "batch: %s\n", cmhip_last_error());
        return 1;
    }
    for (i = 0; i < FRAMES; i++)
        x[i] = (int16_t)lrint(AMPLITUDE * sin(2.0 * 3.14159265358979323846 * (double)(i % PERIOD) / PERIOD));
    if (cmhip_batch_upload(src, 0, x, FRAMES) != COOLMIC_ERROR_NONE || cmhip_batch_sync(src) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "source: %s\n", cmhip_last_error());
        return 1;
    }
    printf("%d Hz tone at %d (-1 dBFS), drive %d (+6 dB) -> limiter: lookahead %u frames, hold %d, threshold %u "
           "(-1 dBFS); %d frames, the gain read over the last %d\n", (int)TONE_HZ, (int)AMPLITUDE, (int)DRIVE,
           1u << LOOKAHEAD_LOG2, (int)HOLD, threshold, (int)FRAMES, (int)PERIOD);

    ld.device = 0; ld.streams = 1; ld.channels = 1; ld.lookahead_log2 = LOOKAHEAD_LOG2; ld.hold = HOLD;
    ld.max_frames = FRAMES; ld.hip_stream = cmhip_batch_hip_stream(dst);
    for (k = 0; k < 2; k++) {
        cmhip_lim_t *lim = cmhip_lim_new_release(&ld, CMHIP_LIM_DETECT_SAMPLE, release[k]);
        uint32_t min_gain[1];
        double lo = 1e9, hi = -1e9;
        unsigned delay;
        int peak = 0;

        if (!lim || cmhip_lim_release(lim) != release[k] ||
            cmhip_lim_set(lim, -1, threshold, DRIVE) != COOLMIC_ERROR_NONE) {
            fprintf(stderr, "limiter: %s\n", cmhip_last_error());
            return 1;
        }
        delay = cmhip_lim_delay(lim);                             /* the release stage adds none */
        if (cmhip_lim_run(lim, cmhip_batch_dev_in(src), cmhip_batch_stride(src), FRAMES, NULL, cmhip_batch_dev_in(dst),
                          cmhip_batch_stride(dst)) != COOLMIC_ERROR_NONE ||
            cmhip_lim_min_gain(lim, min_gain, 0) != COOLMIC_ERROR_NONE ||         /* (waits for the stream) */
            cmhip_batch_download_input(dst, 0, y, FRAMES) != COOLMIC_ERROR_NONE) {
            fprintf(stderr, "limiter run: %s\n", cmhip_last_error());
            return 1;
        }
        for (i = 0; i < FRAMES; i++) {
            if (abs((int)y[i]) > abs(peak))
                peak = y[i];
            if (abs((int)y[i]) > (int)threshold)
                over = 1;
        }
        for (i = FRAMES - PERIOD; i < FRAMES; i++) {
            const int in = x[i - delay];
            if (abs(in) >= AUDIBLE) {
                const double g = (double)y[i] * 134217728.0 / ((double)in * DRIVE) / 32768.0;
                lo = g < lo ? g : lo;
                hi = g > hi ? g : hi;
            }
        }
        range[k] = hi - lo;
        printf("release_log2=%u: peak=%d min_gain=%u gain_min=%.4f gain_max=%.4f range=%.4f\n", release[k], peak,
               (unsigned)min_gain[0], lo, hi, range[k]);
        cmhip_lim_free(lim);
    }
    cmhip_batch_free(dst);
    cmhip_batch_free(src);
    if (over) {
        fprintf(stderr, "a sample passed the ceiling %u\n", threshold);
        return 2;
    }
    if (!(range[1] < range[0])) {
        fprintf(stderr, "the gain's range with the release, %.4f, is not below the range without it, %.4f\n", range[1],
                range[0]);
        return 3;
    }
    return 0;
}
