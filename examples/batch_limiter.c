/*
 * batch_limiter.c -- a programme on air from plain C (include/coolmic_hip.h, "mix bus" and "peak limiter"): four mono
 * microphones, the device-side sine 60 degrees apart, are summed by a mix bus at half weights (headroom: the sum stays
 * at 0.87 of full scale), driven up by 2 (drive 8192) and held under -1 dBFS (threshold 29204) by a look-ahead limiter
 * of 64 frames, straight into the slot of a mono batch with VU on.  Bus, limiter and batch run on the batch's stream,
 * with no synchronisation between them.  Prints one line of geometry, then
 * "programme: frames=24000 rate=48000 channels=1 peak=... power=... min_gain=..." (min_gain in Q15: 32768 is unity).
 *
 *   cc -I include examples/batch_limiter.c -L libcoolmic-dsp_amd/lib -lcoolmic-dsp-hip \
 *      -Wl,-rpath,$PWD/libcoolmic-dsp_amd/lib -o batch_limiter && ./batch_limiter
 */
#include <stdio.h>
#include <stdlib.h>
#include <coolmic-dsp/coolmic-dsp.h>
#include <coolmic_hip.h>

enum { MICS = 4, FRAMES = 24000, LOOKAHEAD_LOG2 = 6, THRESHOLD = 29204, DRIVE = 8192 };

int main(void)
{
    cmhip_batch_desc_t sd = {0}, md = {0};
    cmhip_bus_desc_t bd = {0};
    cmhip_lim_desc_t ld = {0};
    cmhip_batch_t *src, *mid, *b;
    cmhip_bus_t *bus;
    cmhip_lim_t *lim;
    coolmic_vumeter_result_t vu;
    uint32_t to_bus[MICS], from[MICS], counts[1], min_gain[1];
    int16_t W[MICS];
    unsigned i;

    /* the microphones: a batch used as device memory, filled with the engine's sine.  The sine's phase is 7 samples of
     * its 48 per global stream: a global step of 8 puts the microphones 8 samples, 60 degrees, apart */
    sd.device = 0; sd.streams = MICS; sd.channels = 1; sd.rate = 48000; sd.max_frames = FRAMES; sd.flags = CMHIP_VU;
    src = cmhip_batch_new(&sd);
    if (!src || cmhip_batch_generate(src, CMHIP_GEN_SINE, 0, FRAMES, 0, 8, 0) != COOLMIC_ERROR_NONE ||
        cmhip_batch_sync(src) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "sources: %s\n", cmhip_last_error());
        return 1;
    }
    /* one slot for the bus's sum, and the batch that meters the programme */
    md = sd;
    md.streams = 1;
    mid = cmhip_batch_new(&md);
    b = cmhip_batch_new(&md);
    if (!mid || !b) {
        fprintf(stderr, "batch: %s\n", cmhip_last_error());
        return 1;
    }
    /* bus and limiter in front of it, on the batch's stream */
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
    ld.device = 0; ld.streams = 1; ld.channels = 1; ld.lookahead_log2 = LOOKAHEAD_LOG2; ld.hold = 0;
    ld.max_frames = FRAMES; ld.hip_stream = cmhip_batch_hip_stream(b);
    lim = cmhip_lim_new(&ld);
    if (!lim || cmhip_lim_set(lim, -1, THRESHOLD, DRIVE) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "limiter: %s\n", cmhip_last_error());
        return 1;
    }
    printf("%d microphones at %d -> limiter: lookahead %d frames (delay %u), threshold %d, drive %d; %d frames\n",
           (int)MICS, (int)W[0], 1 << LOOKAHEAD_LOG2, cmhip_lim_delay(lim), (int)THRESHOLD, (int)DRIVE, (int)FRAMES);
    if (cmhip_bus_run(bus, cmhip_batch_dev_in(src), cmhip_batch_stride(src), FRAMES, NULL, cmhip_batch_dev_in(mid),
                      cmhip_batch_stride(mid), counts) != COOLMIC_ERROR_NONE ||
        cmhip_lim_run(lim, cmhip_batch_dev_in(mid), cmhip_batch_stride(mid), counts[0], counts, cmhip_batch_dev_in(b),
                      cmhip_batch_stride(b)) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "bus / limiter run: %s\n", cmhip_last_error());
        return 1;
    }
    if (cmhip_batch_run(b, counts[0], counts) != COOLMIC_ERROR_NONE ||
        cmhip_batch_vu_result(b, 0, &vu) != COOLMIC_ERROR_NONE ||
        cmhip_lim_min_gain(lim, min_gain, 0) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "batch run: %s\n", cmhip_last_error());
        return 1;
    }
    printf("programme: frames=%zu rate=%u channels=%u peak=%d power=%.4f min_gain=%u\n", vu.frames, (unsigned)vu.rate,
           vu.channels, (int)vu.global_peak, vu.global_power, (unsigned)min_gain[0]);
    cmhip_lim_free(lim);
    cmhip_bus_free(bus);
    cmhip_batch_free(b);
    cmhip_batch_free(mid);
    cmhip_batch_free(src);
    return 0;
}
