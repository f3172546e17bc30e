/*
 * batch_dynamics.c -- a small broadcast desk from plain C (include/coolmic_hip.h, "mix bus", "dynamics" and "peak
 * limiter"): four mono microphones go through a mix bus at half weights.  Two of them speak (a 500 Hz tone, 30 degrees
 * apart, from frame 4000 to frame 20000), two are idle and pick up room noise within +-40 the whole time.  The sum is
 * gated (below -45 dBFS, expander ratio 3, range 40 dB: the room disappears while nobody speaks) and compressed (above
 * -18 dBFS, ratio 4, knee 6 dB) by a dynamics stage, then driven up by 8 (drive 32768: the make-up gain) and held under
 * -1 dBFS (threshold 29204) by the limiter, straight into the slot of a mono batch with VU on.  Bus, dynamics, limiter
 * and batch run on the batch's stream, with no synchronisation between them.  Prints one line of geometry, then
 * "programme: frames=24000 rate=48000 channels=1 peak=... power=... dyn_min_gain=... lim_min_gain=..." (gains in Q15:
 * 32768 is unity).
 *
 *   cc -I include examples/batch_dynamics.c -L libcoolmic-dsp_amd/lib -lcoolmic-dsp-hip -lm \
 *      -Wl,-rpath,$PWD/libcoolmic-dsp_amd/lib -o batch_dynamics && ./batch_dynamics
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <coolmic-dsp/coolmic-dsp.h>
#include <coolmic_hip.h>

enum { MICS = 4, FRAMES = 24000, SPEECH_FROM = 4000, SPEECH_TO = 20000, DETECTOR_LOG2 = 7, SMOOTH_LOG2 = 6, HOLD = 960,
       LOOKAHEAD_LOG2 = 6, THRESHOLD = 29204, DRIVE = 32768 };

int main(void)
{
    static int16_t pcm[FRAMES];
    cmhip_batch_desc_t sd = {0}, md = {0};
    cmhip_bus_desc_t bd = {0};
    cmhip_dyn_desc_t dd = {0};
    cmhip_lim_desc_t ld = {0};
    const cmhip_dyn_curve_desc_t cd = {-18.0, 4.0, 6.0, -45.0, 3.0, 40.0};
    uint16_t curve[CMHIP_DYN_CURVE];
    cmhip_batch_t *src, *sum, *mid, *b;
    cmhip_bus_t *bus;
    cmhip_dyn_t *dyn;
    cmhip_lim_t *lim;
    coolmic_vumeter_result_t vu;
    uint32_t to_bus[MICS], from[MICS], counts[1], dyn_gain[1], lim_gain[1], lcg = 12345;
    int16_t W[MICS];
    unsigned i, n;

    /* the microphones: a batch used as device memory */
    sd.device = 0; sd.streams = MICS; sd.channels = 1; sd.rate = 48000; sd.max_frames = FRAMES; sd.flags = CMHIP_VU;
    src = cmhip_batch_new(&sd);
    if (!src) {
        fprintf(stderr, "sources: %s\n", cmhip_last_error());
        return 1;
    }
    for (i = 0; i < MICS; i++) {
        for (n = 0; n < FRAMES; n++) {
            if (i < 2) {
                pcm[n] = n >= SPEECH_FROM && n < SPEECH_TO ? (int16_t)lrint(12000.0 * sin(2.0 * M_PI * (n + 8 * i) / 96.0)) : 0;
            } else {
                lcg = lcg * 1664525u + 1013904223u;
                pcm[n] = (int16_t)((int)(lcg >> 16) % 81 - 40);
            }
        }
        if (cmhip_batch_upload(src, i, pcm, FRAMES) != COOLMIC_ERROR_NONE) {
            fprintf(stderr, "upload: %s\n", cmhip_last_error());
            return 1;
        }
    }
    /* one slot each for the bus's sum and the dynamics stage's output, and the batch that meters the programme */
    md = sd;
    md.streams = 1;
    sum = cmhip_batch_new(&md);
    mid = cmhip_batch_new(&md);
    b = cmhip_batch_new(&md);
    if (!sum || !mid || !b) {
        fprintf(stderr, "batch: %s\n", cmhip_last_error());
        return 1;
    }
    /* bus, dynamics and limiter in front of it, on the batch's stream */
    bd.device = 0; bd.streams = MICS; bd.buses = 1; bd.channels_in = 1; bd.channels_out = 1;
    bd.max_frames = FRAMES; bd.max_sends = MICS; bd.hip_stream = cmhip_batch_hip_stream(b);
    bus = cmhip_bus_new(&bd);
    for (i = 0; i < MICS; i++) {
        to_bus[i] = 0;
        from[i] = i;
        W[i] = 8192;
    }
    if (!bus || cmhip_bus_set_routing(bus, MICS, to_bus, from, W) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "bus: %s\n", cmhip_last_error());
        return 1;
    }
    dd.device = 0; dd.streams = 1; dd.channels = 1; dd.detector_log2 = DETECTOR_LOG2; dd.smooth_log2 = SMOOTH_LOG2;
    dd.hold = HOLD; dd.max_frames = FRAMES; dd.hip_stream = cmhip_batch_hip_stream(b);
    dyn = cmhip_dyn_new(&dd);
    if (!dyn || cmhip_dyn_design(&cd, curve) != COOLMIC_ERROR_NONE ||
        cmhip_dyn_set_curve(dyn, -1, curve) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "dynamics: %s\n", cmhip_last_error());
        return 1;
    }
    ld.device = 0; ld.streams = 1; ld.channels = 1; ld.lookahead_log2 = LOOKAHEAD_LOG2; ld.hold = 0;
    ld.max_frames = FRAMES; ld.hip_stream = cmhip_batch_hip_stream(b);
    lim = cmhip_lim_new(&ld);
    if (!lim || cmhip_lim_set(lim, -1, THRESHOLD, DRIVE) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "limiter: %s\n", cmhip_last_error());
        return 1;
    }
    printf("%d microphones (2 idle) -> bus -> dynamics: delay %u, detector %d frames, hold %d; gate %.0f dBFS 1:%.0f range "
           "%.0f dB, compressor %.0f dBFS %.0f:1 -> limiter: delay %u, threshold %d, drive %d; %d frames\n", (int)MICS,
           cmhip_dyn_delay(dyn), 1 << DETECTOR_LOG2, (int)HOLD, cd.gate_threshold_db, cd.gate_ratio, cd.gate_range_db,
           cd.comp_threshold_db, cd.comp_ratio, cmhip_lim_delay(lim), (int)THRESHOLD, (int)DRIVE, (int)FRAMES);
    if (cmhip_batch_sync(src) != COOLMIC_ERROR_NONE ||
        cmhip_bus_run(bus, cmhip_batch_dev_in(src), cmhip_batch_stride(src), FRAMES, NULL, cmhip_batch_dev_in(sum),
                      cmhip_batch_stride(sum), counts) != COOLMIC_ERROR_NONE ||
        cmhip_dyn_run(dyn, cmhip_batch_dev_in(sum), cmhip_batch_stride(sum), counts[0], counts, cmhip_batch_dev_in(mid),
                      cmhip_batch_stride(mid)) != COOLMIC_ERROR_NONE ||
        cmhip_lim_run(lim, cmhip_batch_dev_in(mid), cmhip_batch_stride(mid), counts[0], counts, cmhip_batch_dev_in(b),
                      cmhip_batch_stride(b)) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "bus / dynamics / limiter run: %s\n", cmhip_last_error());
        return 1;
    }
    if (cmhip_batch_run(b, counts[0], counts) != COOLMIC_ERROR_NONE ||
        cmhip_batch_vu_result(b, 0, &vu) != COOLMIC_ERROR_NONE ||
        cmhip_dyn_min_gain(dyn, dyn_gain, 0) != COOLMIC_ERROR_NONE ||
        cmhip_lim_min_gain(lim, lim_gain, 0) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "batch run: %s\n", cmhip_last_error());
        return 1;
    }
    printf("programme: frames=%zu rate=%u channels=%u peak=%d power=%.4f dyn_min_gain=%u lim_min_gain=%u\n", vu.frames,
           (unsigned)vu.rate, vu.channels, (int)vu.global_peak, vu.global_power, (unsigned)dyn_gain[0],
           (unsigned)lim_gain[0]);
    cmhip_lim_free(lim);
    cmhip_dyn_free(dyn);
    cmhip_bus_free(bus);
    cmhip_batch_free(b);
    cmhip_batch_free(mid);
    cmhip_batch_free(sum);
    cmhip_batch_free(src);
    return 0;
}
