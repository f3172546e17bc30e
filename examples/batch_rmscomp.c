/*
 * batch_rmscomp.c -- why a compressor wants an RMS detector, from plain C (include/coolmic_hip.h, "dynamics", "RMS
 * detector"): a 997 Hz sine of amplitude 23170 and a square wave of amplitude 16384 carry the same power, -6.0 dBFS.
 * Both go through one designed compressor (threshold -12 dBFS, ratio 4, hard knee; detector window 1024 frames, ramp 64
 * frames), once with the mean-magnitude detector and once with the RMS detector.  After 43904 frames to settle the gain
 * meter is re-armed, 4096 more frames run, and the meter gives each stream's steady gain.  Under RMS both get the same
 * gain, -4.5 dB (the sine's moves by a fraction of a percent with the window's position over the periods); under the
 * mean detector the sine reads 0.9 dB lower than the square and is compressed 0.7 dB less.  Prints one line of
 * geometry, then per detector "mean: sine_gain=... square_gain=... sine_db=... square_db=..." (gains in Q15: 32768 is
 * unity).
 *
 *   cc -I include examples/batch_rmscomp.c -L libcoolmic-dsp_amd/lib -lcoolmic-dsp-hip -lm \
 *      -Wl,-rpath,$PWD/libcoolmic-dsp_amd/lib -o batch_rmscomp && ./batch_rmscomp
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <coolmic-dsp/coolmic-dsp.h>
#include <coolmic_hip.h>

enum { STREAMS = 2, FRAMES = 48000, STEADY = 4096, SETTLE = FRAMES - STEADY, RATE = 48000, HZ = 997, SINE = 23170,
       SQUARE = 16384, SQUARE_HALF_PERIOD = 24, DETECTOR_LOG2 = 10, SMOOTH_LOG2 = 6 };

int main(void)
{
    static int16_t pcm[FRAMES];
    static const char *const names[2] = {"mean", "rms"};
    const unsigned detectors[2] = {CMHIP_DYN_DETECT_MEAN, CMHIP_DYN_DETECT_RMS};
    const cmhip_dyn_curve_desc_t cd = {-12.0, 4.0, 0.0, -96.0, 1.0, 0.0};
    cmhip_batch_desc_t sd = {0};
    cmhip_dyn_desc_t dd = {0};
    uint16_t curve[CMHIP_DYN_CURVE];
    cmhip_batch_t *src, *dst;
    uint32_t gain[STREAMS];
    unsigned i, n, k;

    /* the two signals and the output: batches used as device memory */
    sd.device = 0; sd.streams = STREAMS; sd.channels = 1; sd.rate = RATE; sd.max_frames = FRAMES; sd.flags = CMHIP_VU;
    src = cmhip_batch_new(&sd);
    dst = cmhip_batch_new(&sd);
    if (!src || !dst) {
        fprintf(stderr, "batch: %s\n", cmhip_last_error());
        return 1;
    }
    for (i = 0; i < STREAMS; i++) {
        for (n = 0; n < FRAMES; n++)
            pcm[n] = i == 0 ? (int16_t)floor(SINE * sin(2.0 * M_PI * HZ * n / RATE) + 0.5)
                            : (int16_t)((n / SQUARE_HALF_PERIOD) % 2 == 0 ? SQUARE : -SQUARE);
        if (cmhip_batch_upload(src, i, pcm, FRAMES) != COOLMIC_ERROR_NONE) {
            fprintf(stderr, "upload: %s\n", cmhip_last_error());
            return 1;
        }
    }
    if (cmhip_batch_sync(src) != COOLMIC_ERROR_NONE || cmhip_dyn_design(&cd, curve) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "setup: %s\n", cmhip_last_error());
        return 1;
    }
    dd.device = 0; dd.streams = STREAMS; dd.channels = 1; dd.detector_log2 = DETECTOR_LOG2; dd.smooth_log2 = SMOOTH_LOG2;
    dd.hold = 0; dd.max_frames = SETTLE;
    for (k = 0; k < 2; k++) {
        const size_t in_stride = cmhip_batch_stride(src), out_stride = cmhip_batch_stride(dst);
        const char *in = (const char *)cmhip_batch_dev_in(src);
        char *out = (char *)cmhip_batch_dev_in(dst);
        cmhip_dyn_t *dyn = cmhip_dyn_new_detector(&dd, detectors[k]);
        if (!dyn || cmhip_dyn_detector(dyn) != detectors[k] || cmhip_dyn_set_curve(dyn, -1, curve) != COOLMIC_ERROR_NONE) {
            fprintf(stderr, "dynamics: %s\n", cmhip_last_error());
            return 1;
        }
        if (k == 0)
            printf("a 997 Hz sine and a square wave of equal power -> compressor: delay %u, detector %d frames, %.0f dBFS "
                   "%.0f:1; %d frames to settle, %d metered\n", cmhip_dyn_delay(dyn), 1 << DETECTOR_LOG2,
                   cd.comp_threshold_db, cd.comp_ratio, (int)SETTLE, (int)STEADY);
        /* the second run continues every stream SETTLE frames into its slot (a multiple of 8 samples: still aligned) */
        if (cmhip_dyn_run(dyn, in, in_stride, SETTLE, NULL, out, out_stride) != COOLMIC_ERROR_NONE ||
            cmhip_dyn_min_gain(dyn, gain, 1) != COOLMIC_ERROR_NONE ||
            cmhip_dyn_run(dyn, in + SETTLE * sizeof(int16_t), in_stride, STEADY, NULL, out + SETTLE * sizeof(int16_t),
                          out_stride) != COOLMIC_ERROR_NONE ||
            cmhip_dyn_min_gain(dyn, gain, 0) != COOLMIC_ERROR_NONE) {
            fprintf(stderr, "dynamics run: %s\n", cmhip_last_error());
            return 1;
        }
        printf("%s: sine_gain=%u square_gain=%u sine_db=%.1f square_db=%.1f\n", names[k], (unsigned)gain[0],
               (unsigned)gain[1], 20.0 * log10(gain[0] / 32768.0), 20.0 * log10(gain[1] / 32768.0));
        cmhip_dyn_free(dyn);
    }
    cmhip_batch_free(dst);
    cmhip_batch_free(src);
    return 0;
}
