/*
 * batch_tplimiter.c -- a programme held under -1 dBTP from plain C (include/coolmic_hip.h, "peak limiter", "true-peak
 * detector"): a full-scale sine at a quarter of the sample rate, 45 degrees off the sample grid -- every sample is
 * +-23170, 3 dB below full scale, while the signal between the samples reaches full scale -- goes through a mix bus at
 * unity into a limiter with the true-peak detector at cmhip_lim_threshold_dbtp(-1.0) = 29204 and on into a mono batch
 * that meters true peak (gain disabled, so the meter sees the limiter's output as it is).  A sample-peak limiter at the
 * same threshold would leave the signal alone and let full scale, +0.04 dBTP, through.  Bus, limiter and batch run on
 * the batch's stream.  The sine is followed by a flush of cmhip_lim_delay() frames of silence; the batch's true-peak
 * window is closed once after the first 2 * HIST frames (the attack has settled) and read again at the sine's last
 * frame.
 * Prints one line of geometry, then
 * "programme: frames=... dbtp=... peak=... bound=... min_gain=..." (peak and bound in units of 2^-13 of a sample unit),
 * and exits non-zero unless peak <= bound = T * 2^13 + 8286.
 *
 *   cc -I include examples/batch_tplimiter.c -L libcoolmic-dsp_amd/lib -lcoolmic-dsp-hip \
 *      -Wl,-rpath,$PWD/libcoolmic-dsp_amd/lib -o batch_tplimiter && ./batch_tplimiter
 */
#include <stdio.h>
#include <stdlib.h>
#include <coolmic-dsp/coolmic-dsp.h>
#include <coolmic_hip.h>

enum { FRAMES = 24000, LOOKAHEAD_LOG2 = 6, HOLD = 1, DRIVE = 4096, UNITY_WEIGHT = 16384, ROUNDING = 8286 };

int main(void)
{
    static int16_t pcm[FRAMES + 1024];
    cmhip_batch_desc_t sd = {0};
    cmhip_bus_desc_t bd = {0};
    cmhip_lim_desc_t ld = {0};
    cmhip_batch_t *src, *mid, *b;
    cmhip_bus_t *bus;
    cmhip_lim_t *lim;
    coolmic_truepeak_result_t settled, tail;
    const unsigned threshold = cmhip_lim_threshold_dbtp(-1.0);
    const unsigned A = 1u << LOOKAHEAD_LOG2, hist = A + (A + HOLD) - 2 + 13;
    const unsigned settle = (2 * hist + 7) / 8 * 8;               /* a multiple of 8 frames: the cut stays 16-byte aligned */
    uint32_t to_bus[1] = {0}, from[1] = {0}, counts[1], part[1], min_gain[1];
    int16_t W[1] = {UNITY_WEIGHT};
    unsigned delay, total, i, cut[4];
    unsigned long bound;

    sd.device = 0; sd.streams = 1; sd.channels = 1; sd.rate = 48000; sd.max_frames = FRAMES + 1024; sd.flags = CMHIP_VU;
    src = cmhip_batch_new(&sd);
    mid = cmhip_batch_new(&sd);
    b = cmhip_batch_new(&sd);
    if (!src || !mid || !b || cmhip_batch_set_true_peak(b, 1) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "batch: %s\n", cmhip_last_error());
        return 1;
    }
    bd.device = 0; bd.streams = 1; bd.buses = 1; bd.channels_in = 1; bd.channels_out = 1;
    bd.max_frames = FRAMES + 1024; bd.max_sends = 1; bd.hip_stream = cmhip_batch_hip_stream(b);
    bus = cmhip_bus_new(&bd);
    if (!bus || cmhip_bus_set_routing(bus, 1, to_bus, from, W) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "bus: %s\n", cmhip_last_error());
        return 1;
    }
    ld.device = 0; ld.streams = 1; ld.channels = 1; ld.lookahead_log2 = LOOKAHEAD_LOG2; ld.hold = HOLD;
    ld.max_frames = FRAMES + 1024; ld.hip_stream = cmhip_batch_hip_stream(b);
    lim = cmhip_lim_new_detector(&ld, CMHIP_LIM_DETECT_TRUE_PEAK);
    if (!lim || cmhip_lim_set(lim, -1, threshold, DRIVE) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "limiter: %s\n", cmhip_last_error());
        return 1;
    }
    delay = cmhip_lim_delay(lim);
    total = FRAMES + delay;
    if (cmhip_lim_detector(lim) != CMHIP_LIM_DETECT_TRUE_PEAK || delay != A + 7 || total > FRAMES + 1024) {
        fprintf(stderr, "limiter: detector %u, delay %u\n", cmhip_lim_detector(lim), delay);
        return 1;
    }
    printf("sine at fs/4, samples +-23170 -> limiter: true-peak detector, lookahead %u frames, hold %d (delay %u), "
           "threshold %u (-1 dBTP), drive %d; %d frames and a flush of %u\n", A, (int)HOLD, delay, threshold, (int)DRIVE,
           (int)FRAMES, delay);

    /* the source: sin(pi/4 + n pi/2) at full scale, then silence; the bus takes it to `mid` in one run */
    for (i = 0; i < FRAMES; i++)
        pcm[i] = (int16_t)((i & 2u) ? -23170 : 23170);
    if (cmhip_batch_upload(src, 0, pcm, total) != COOLMIC_ERROR_NONE || cmhip_batch_sync(src) != COOLMIC_ERROR_NONE ||
        cmhip_bus_run(bus, cmhip_batch_dev_in(src), cmhip_batch_stride(src), total, NULL, cmhip_batch_dev_in(mid),
                      cmhip_batch_stride(mid), counts) != COOLMIC_ERROR_NONE || counts[0] != total) {
        fprintf(stderr, "source / bus run: %s\n", cmhip_last_error());
        return 1;
    }
    /* the limiter and the batch in three runs: the attack, the settled sine, the flush */
    cut[0] = 0; cut[1] = settle; cut[2] = FRAMES; cut[3] = total;
    for (i = 0; i < 3; i++) {
        const int16_t *in = (const int16_t *)cmhip_batch_dev_in(mid) + cut[i];
        coolmic_truepeak_result_t *res = i < 2 ? &settled : &tail;        /* (the attack's window is overwritten) */
        part[0] = cut[i + 1] - cut[i];
        /* (the stride names what is left of the one slot: the run's input range ends where the slot ends) */
        if (cmhip_lim_run(lim, in, cmhip_batch_stride(mid) - cut[i], part[0], part, cmhip_batch_dev_in(b),
                          cmhip_batch_stride(b)) != COOLMIC_ERROR_NONE ||
            cmhip_batch_run(b, part[0], part) != COOLMIC_ERROR_NONE ||
            cmhip_batch_tp_result(b, 0, res) != COOLMIC_ERROR_NONE) {     /* (closes the window; the filter goes on) */
            fprintf(stderr, "limiter / batch run %u: %s\n", i, cmhip_last_error());
            return 1;
        }
    }
    if (cmhip_lim_min_gain(lim, min_gain, 0) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "meter: %s\n", cmhip_last_error());
        return 1;
    }
    bound = (unsigned long)threshold * 8192ul + ROUNDING;
    printf("programme: frames=%zu dbtp=%.4f peak=%u bound=%lu flush_dbtp=%.4f min_gain=%u\n", settled.frames,
           settled.global_dbtp, (unsigned)settled.global_peak, bound, tail.global_dbtp, (unsigned)min_gain[0]);
    cmhip_lim_free(lim);
    cmhip_bus_free(bus);
    cmhip_batch_free(b);
    cmhip_batch_free(mid);
    cmhip_batch_free(src);
    if (settled.global_peak > bound) {
        fprintf(stderr, "the settled programme's true peak %u is above %lu\n", (unsigned)settled.global_peak, bound);
        return 2;
    }
    return 0;
}
