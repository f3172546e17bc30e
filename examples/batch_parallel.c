/*
 * batch_parallel.c -- parallel ("dry/wet", "New York") compression from plain C (include/coolmic_hip.h, "dynamics",
 * "delay", "mix bus" and "peak limiter"): one mono source -- a 220 Hz tone that is quiet, then loud, then quiet, over
 * room noise -- feeds a dynamics object (the wet path) and a delay set to cmhip_dyn_delay() (the dry path, exactly as
 * late); a bus adds the two at half weight each, a limiter holds the sum under -1 dBFS, straight into the slot of a
 * mono batch with VU on.  Everything runs on the batch's stream, with no synchronisation in between.
 *
 * First pass, with the unity curve of creation: the wet path is the delayed input too, so the bus must give the
 * delayed input back bit for bit -- the program checks all frames and prints
 * "unity curve: bus output equals the input delayed by 63 frames: yes".  Then everything is reset, the compressor gets
 * its curve, and the second pass prints
 * "parallel compression: dyn_min_gain=... quiet_peak=... loud_peak=... (dry ... ...)" -- the loud part comes out lower
 * than dry, the quiet part nearly as it went in -- and the "programme:" line of the VU meter.
 *
 *   cc -I include examples/batch_parallel.c -L libcoolmic-dsp_amd/lib -lcoolmic-dsp-hip -lm \
 *      -Wl,-rpath,$PWD/libcoolmic-dsp_amd/lib -o batch_parallel && ./batch_parallel
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <coolmic-dsp/coolmic-dsp.h>
#include <coolmic_hip.h>

enum { FRAMES = 24000, LOUD_FROM = 8000, LOUD_TO = 16000, DETECTOR_LOG2 = 7, SMOOTH_LOG2 = 6, HOLD = 480,
       LOOKAHEAD_LOG2 = 6, THRESHOLD = 29204, DRIVE = 4096 };

static int peak_of(const int16_t *x, unsigned from, unsigned to)
{
    int peak = 0;
    unsigned n;
    for (n = from; n < to; n++)
        if (abs((int)x[n]) > peak)
            peak = abs((int)x[n]);
    return peak;
}

int main(void)
{
    static int16_t pcm[FRAMES], got[FRAMES];
    static const cmhip_dyn_curve_desc_t cd = {-24.0, 8.0, 6.0, -90.0, 1.0, 0.0};     /* a hard compressor, no gate */
    cmhip_batch_desc_t sd = {0};
    cmhip_dyn_desc_t dd = {0};
    cmhip_delay_desc_t yd = {0};
    cmhip_bus_desc_t bd = {0};
    cmhip_lim_desc_t ld = {0};
    uint16_t curve[CMHIP_DYN_CURVE];
    cmhip_batch_t *src, *paths, *sum, *b;
    cmhip_dyn_t *dyn;
    cmhip_delay_t *delay;
    cmhip_bus_t *bus;
    cmhip_lim_t *lim;
    coolmic_vumeter_result_t vu;
    uint32_t to_bus[2] = {0, 0}, from[2] = {0, 1}, counts[1] = {FRAMES}, both[2] = {FRAMES, FRAMES}, out_frames[1];
    uint32_t dyn_gain[1], lim_gain[1], lcg = 12345, d_now, d_from, done, ramp;
    int16_t W[2] = {8192, 8192};
    unsigned n, pass, D, wrong;
    int16_t *wet, *dry;

    /* the source, the two paths side by side, their sum, and the metering batch: batches used as device memory */
    sd.device = 0; sd.streams = 1; sd.channels = 1; sd.rate = 48000; sd.max_frames = FRAMES; sd.flags = CMHIP_VU;
    src = cmhip_batch_new(&sd);
    sum = cmhip_batch_new(&sd);
    b = cmhip_batch_new(&sd);
    sd.streams = 2;
    paths = cmhip_batch_new(&sd);
    if (!src || !sum || !b || !paths) {
        fprintf(stderr, "batch: %s\n", cmhip_last_error());
        return 1;
    }
    for (n = 0; n < FRAMES; n++) {
        const double level = n >= LOUD_FROM && n < LOUD_TO ? 24000.0 : 1500.0;
        lcg = lcg * 1664525u + 1013904223u;
        pcm[n] = (int16_t)(lrint(level * sin(2.0 * M_PI * n * 220.0 / 48000.0)) + (int)(lcg >> 16) % 41 - 20);
    }
    if (cmhip_batch_upload(src, 0, pcm, FRAMES) != COOLMIC_ERROR_NONE || cmhip_batch_sync(src) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "upload: %s\n", cmhip_last_error());
        return 1;
    }
    dd.device = 0; dd.streams = 1; dd.channels = 1; dd.detector_log2 = DETECTOR_LOG2; dd.smooth_log2 = SMOOTH_LOG2;
    dd.hold = HOLD; dd.max_frames = FRAMES; dd.hip_stream = cmhip_batch_hip_stream(b);
    dyn = cmhip_dyn_new(&dd);
    if (!dyn) {
        fprintf(stderr, "dynamics: %s\n", cmhip_last_error());
        return 1;
    }
    D = cmhip_dyn_delay(dyn);
    /* the dry path: as late as the wet one */
    yd.device = 0; yd.streams = 1; yd.channels = 1; yd.max_delay = D; yd.max_frames = FRAMES;
    yd.hip_stream = cmhip_batch_hip_stream(b);
    delay = cmhip_delay_new(&yd);
    if (!delay || cmhip_delay_set(delay, -1, D) != COOLMIC_ERROR_NONE ||
        cmhip_delay_get(delay, 0, &d_now, &d_from, &done, &ramp) != COOLMIC_ERROR_NONE || d_now != D) {
        fprintf(stderr, "delay: %s\n", cmhip_last_error());
        return 1;
    }
    bd.device = 0; bd.streams = 2; bd.buses = 1; bd.channels_in = 1; bd.channels_out = 1; bd.max_frames = FRAMES;
    bd.max_sends = 2; bd.hip_stream = cmhip_batch_hip_stream(b);
    bus = cmhip_bus_new(&bd);
    if (!bus || cmhip_bus_set_routing(bus, 2, to_bus, from, W) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "bus: %s\n", cmhip_last_error());
        return 1;
    }
    ld.device = 0; ld.streams = 1; ld.channels = 1; ld.lookahead_log2 = LOOKAHEAD_LOG2; ld.hold = 0;
    ld.max_frames = FRAMES; ld.hip_stream = cmhip_batch_hip_stream(b);
    lim = cmhip_lim_new(&ld);
    if (!lim || cmhip_lim_set(lim, -1, THRESHOLD, DRIVE) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "limiter: %s\n", cmhip_last_error());
        return 1;
    }
    printf("source -> {dynamics: delay %u, delay line: %u of at most %zu frames} -> bus at 8192 + 8192 -> limiter: delay %u, "
           "threshold %d; %d frames\n", D, (unsigned)d_now, cmhip_delay_max_delay(delay), cmhip_lim_delay(lim),
           (int)THRESHOLD, (int)FRAMES);
    wet = (int16_t *)cmhip_batch_dev_in(paths);
    dry = wet + cmhip_batch_stride(paths);
    for (pass = 0; pass < 2; pass++) {
        if (pass == 1) {
            /* from silence again, now with the compressor's curve */
            if (cmhip_dyn_design(&cd, curve) != COOLMIC_ERROR_NONE || cmhip_dyn_set_curve(dyn, -1, curve) != COOLMIC_ERROR_NONE ||
                cmhip_dyn_reset(dyn, -1) != COOLMIC_ERROR_NONE || cmhip_delay_reset(delay, -1) != COOLMIC_ERROR_NONE ||
                cmhip_lim_reset(lim, -1) != COOLMIC_ERROR_NONE) {
                fprintf(stderr, "reset: %s\n", cmhip_last_error());
                return 1;
            }
        }
        if (cmhip_dyn_run(dyn, cmhip_batch_dev_in(src), cmhip_batch_stride(src), FRAMES, counts, wet,
                          cmhip_batch_stride(paths)) != COOLMIC_ERROR_NONE ||
            cmhip_delay_run(delay, cmhip_batch_dev_in(src), cmhip_batch_stride(src), FRAMES, counts, dry,
                            cmhip_batch_stride(paths)) != COOLMIC_ERROR_NONE ||
            cmhip_bus_run(bus, wet, cmhip_batch_stride(paths), FRAMES, both, cmhip_batch_dev_in(sum),
                          cmhip_batch_stride(sum), out_frames) != COOLMIC_ERROR_NONE ||
            cmhip_lim_run(lim, cmhip_batch_dev_in(sum), cmhip_batch_stride(sum), out_frames[0], out_frames,
                          cmhip_batch_dev_in(b), cmhip_batch_stride(b)) != COOLMIC_ERROR_NONE ||
            cmhip_delay_sync(delay) != COOLMIC_ERROR_NONE ||
            cmhip_batch_download_input(sum, 0, got, FRAMES) != COOLMIC_ERROR_NONE) {
            fprintf(stderr, "run: %s\n", cmhip_last_error());
            return 1;
        }
        if (pass == 0) {
            for (wrong = 0, n = 0; n < FRAMES; n++)
                wrong += got[n] != (n >= D ? pcm[n - D] : 0);
            printf("unity curve: bus output equals the input delayed by %u frames: %s\n", D, wrong ? "NO" : "yes");
            if (wrong)
                return 1;
        }
    }
    if (cmhip_batch_run(b, FRAMES, counts) != COOLMIC_ERROR_NONE || cmhip_batch_vu_result(b, 0, &vu) != COOLMIC_ERROR_NONE ||
        cmhip_dyn_min_gain(dyn, dyn_gain, 0) != COOLMIC_ERROR_NONE || cmhip_lim_min_gain(lim, lim_gain, 0) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "batch run: %s\n", cmhip_last_error());
        return 1;
    }
    printf("parallel compression: dyn_min_gain=%u quiet_peak=%d loud_peak=%d (dry %d %d)\n", (unsigned)dyn_gain[0],
           peak_of(got, 2000, LOUD_FROM), peak_of(got, LOUD_FROM + 2000, LOUD_TO), peak_of(pcm, 2000, LOUD_FROM),
           peak_of(pcm, LOUD_FROM + 2000, LOUD_TO));
    printf("programme: frames=%zu rate=%u channels=%u peak=%d power=%.4f lim_min_gain=%u\n", vu.frames, (unsigned)vu.rate,
           vu.channels, (int)vu.global_peak, vu.global_power, (unsigned)lim_gain[0]);
    cmhip_lim_free(lim);
    cmhip_bus_free(bus);
    cmhip_delay_free(delay);
    cmhip_dyn_free(dyn);
    cmhip_batch_free(b);
    cmhip_batch_free(paths);
    cmhip_batch_free(sum);
    cmhip_batch_free(src);
    return 0;
}
