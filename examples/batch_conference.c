/*
 * batch_conference.c -- a conference's return feeds from plain C (include/coolmic_hip.h, "mix bus"): 8 mono
 * participants, each the device-side sine in the same phase, go through a mix bus with the mix-minus table -- bus b
 * carries everyone but participant b, each at 1/7 -- straight into the slots of a mono batch with VU on.  The bus and
 * the batch run on the batch's stream, with no synchronisation between them.  Prints one line of geometry, then one VU
 * line per participant: "participant N: frames=24000 rate=48000 channels=1 peak=... power=..." (power in dB; seven
 * sines in phase at 1/7 each are the sine again: about -3).
 *
 *   cc -I include examples/batch_conference.c -L libcoolmic-dsp_amd/lib -lcoolmic-dsp-hip \
 *      -Wl,-rpath,$PWD/libcoolmic-dsp_amd/lib -o batch_conference && ./batch_conference
 */
#include <stdio.h>
#include <stdlib.h>
#include <coolmic-dsp/coolmic-dsp.h>
#include <coolmic_hip.h>

enum { PEOPLE = 8, SENDS = PEOPLE * (PEOPLE - 1), FRAMES = 24000 };

int main(void)
{
    cmhip_batch_desc_t sd = {0}, bd = {0};
    cmhip_bus_desc_t md = {0};
    cmhip_batch_t *src, *b;
    cmhip_bus_t *m;
    coolmic_vumeter_result_t vu[PEOPLE];
    uint32_t bus[SENDS], stream[SENDS], counts[PEOPLE];
    int16_t W[SENDS];
    const int16_t w = 16384 / (PEOPLE - 1);
    unsigned p;

    /* the participants: a batch used as device memory, filled with the engine's sine.  A global step of 0 makes every
     * slot global stream 0: the sine's phase depends on the global stream, and here all participants are in phase */
    sd.device = 0; sd.streams = PEOPLE; sd.channels = 1; sd.rate = 48000; sd.max_frames = FRAMES; sd.flags = CMHIP_VU;
    src = cmhip_batch_new(&sd);
    if (!src || cmhip_batch_generate(src, CMHIP_GEN_SINE, 0, FRAMES, 0, 0, 0) != COOLMIC_ERROR_NONE ||
        cmhip_batch_sync(src) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "sources: %s\n", cmhip_last_error());
        return 1;
    }
    /* the batch that meters what every participant hears */
    bd = sd;
    b = cmhip_batch_new(&bd);
    if (!b) {
        fprintf(stderr, "batch: %s\n", cmhip_last_error());
        return 1;
    }
    /* the bus in front of it, on the batch's stream */
    md.device = 0; md.streams = PEOPLE; md.buses = PEOPLE; md.channels_in = 1; md.channels_out = 1;
    md.max_frames = FRAMES; md.max_sends = SENDS; md.hip_stream = cmhip_batch_hip_stream(b);
    m = cmhip_bus_new(&md);
    if (!m || cmhip_bus_mix_minus(PEOPLE, w, bus, stream, W, SENDS, 1) != COOLMIC_ERROR_NONE ||
        cmhip_bus_set_routing(m, SENDS, bus, stream, W) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "bus: %s\n", cmhip_last_error());
        return 1;
    }
    printf("mix-minus: %d participants, %zu sends, w = %d; %d frames\n", (int)PEOPLE, cmhip_bus_sends(m), (int)w,
           (int)FRAMES);
    if (cmhip_bus_run(m, cmhip_batch_dev_in(src), cmhip_batch_stride(src), FRAMES, NULL, cmhip_batch_dev_in(b),
                      cmhip_batch_stride(b), counts) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "bus_run: %s\n", cmhip_last_error());
        return 1;
    }
    if (cmhip_batch_run(b, FRAMES, counts) != COOLMIC_ERROR_NONE ||
        cmhip_batch_vu_results(b, vu, NULL) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "batch run: %s\n", cmhip_last_error());
        return 1;
    }
    for (p = 0; p < PEOPLE; p++)
        printf("participant %u: frames=%zu rate=%u channels=%u peak=%d power=%.4f\n", p, vu[p].frames,
               (unsigned)vu[p].rate, vu[p].channels, (int)vu[p].global_peak, vu[p].global_power);
    cmhip_bus_free(m);
    cmhip_batch_free(b);
    cmhip_batch_free(src);
    return 0;
}
