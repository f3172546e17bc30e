/*
 * batch_automix.c -- an automixer in front of a bus from plain C (include/coolmic_hip.h, "automixer" and "mix bus"):
 * four mono microphones in one gain-sharing group, windows of 256 frames and smoothing shifts 0, summed by a mix bus at
 * unity weights into the slot of a mono batch with VU on.  Automixer, bus and batch run on the batch's stream, with no
 * synchronisation between them.  Three phases of 1024 frames each:
 *   1: a square wave of magnitude 8000 on microphone 0, digital silence on the others
 *   2: the same square wave on microphones 0 and 1
 *   3: the same square wave on all four
 * After each phase it prints the four gains (cmhip_automix_state; 4096 is unity) and the bus output's peak:
 *   "phase 1: gains 4096 0 0 0, programme peak 8000"       one talker passes at unity
 *   "phase 2: gains 2896 2896 0 0, programme peak 11312"   two equal talkers at -3 dB each
 *   "phase 3: gains 2048 2048 2048 2048, programme peak 16000"   four at -6 dB each
 * The gains' squares sum to one microphone's, however many talk.
 *
 *   cc -I include examples/batch_automix.c -L libcoolmic-dsp_amd/lib -lcoolmic-dsp-hip \
 *      -Wl,-rpath,$PWD/libcoolmic-dsp_amd/lib -o batch_automix && ./batch_automix
 */
#include <stdio.h>
#include <stdlib.h>
#include <coolmic-dsp/coolmic-dsp.h>
#include <coolmic_hip.h>

enum { MICS = 4, FRAMES = 1024, WINDOW_LOG2 = 8, MAGNITUDE = 8000, PHASES = 3 };

int main(void)
{
    static const unsigned talkers[PHASES] = {1, 2, 4};
    cmhip_batch_desc_t sd = {0}, md = {0};
    cmhip_automix_desc_t ad = {0};
    cmhip_bus_desc_t bd = {0};
    cmhip_batch_t *src, *mid, *b;
    cmhip_automix_t *amx;
    cmhip_bus_t *bus;
    coolmic_vumeter_result_t vu;
    static int16_t pcm[FRAMES];
    uint32_t to_bus[MICS], from[MICS], counts[1], gain[MICS];
    int16_t W[MICS];
    unsigned i, n, phase;

    /* the microphones and the automixer's output: batches used as device memory */
    sd.device = 0; sd.streams = MICS; sd.channels = 1; sd.rate = 48000; sd.max_frames = FRAMES; sd.flags = CMHIP_VU;
    src = cmhip_batch_new(&sd);
    mid = cmhip_batch_new(&sd);
    /* the batch that meters the programme */
    md = sd;
    md.streams = 1;
    b = cmhip_batch_new(&md);
    if (!src || !mid || !b) {
        fprintf(stderr, "batch: %s\n", cmhip_last_error());
        return 1;
    }
    /* automixer and bus in front of it, on the batch's stream; all four microphones in group 0 */
    ad.device = 0; ad.streams = MICS; ad.channels = 1; ad.window_log2 = WINDOW_LOG2; ad.max_frames = FRAMES;
    ad.hip_stream = cmhip_batch_hip_stream(b);
    amx = cmhip_automix_new(&ad);
    for (i = 0; amx && i < MICS; i++) {
        if (cmhip_automix_set_group(amx, (long)i, 0) != COOLMIC_ERROR_NONE) {
            fprintf(stderr, "automixer: %s\n", cmhip_last_error());
            return 1;
        }
    }
    bd.device = 0; bd.streams = MICS; bd.buses = 1; bd.channels_in = 1; bd.channels_out = 1;
    bd.max_frames = FRAMES; bd.max_sends = MICS; bd.hip_stream = cmhip_batch_hip_stream(b);
    bus = cmhip_bus_new(&bd);
    for (i = 0; i < MICS; i++) {
        to_bus[i] = 0;
        from[i] = i;
        W[i] = 16384;
    }
    if (!amx || !bus || cmhip_bus_set_routing(bus, MICS, to_bus, from, W) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "automixer / bus: %s\n", cmhip_last_error());
        return 1;
    }
    printf("%d microphones in one group -> automixer: window %d frames -> bus at unity; %d frames a phase\n", (int)MICS,
           1 << WINDOW_LOG2, (int)FRAMES);
    for (phase = 0; phase < PHASES; phase++) {
        for (i = 0; i < MICS; i++) {
            for (n = 0; n < FRAMES; n++)
                pcm[n] = (int16_t)(i < talkers[phase] ? ((n / 8) % 2 ? -MAGNITUDE : MAGNITUDE) : 0);
            if (cmhip_batch_upload(src, i, pcm, FRAMES) != COOLMIC_ERROR_NONE) {
                fprintf(stderr, "upload: %s\n", cmhip_last_error());
                return 1;
            }
        }
        if (cmhip_batch_sync(src) != COOLMIC_ERROR_NONE ||
            cmhip_automix_run(amx, cmhip_batch_dev_in(src), cmhip_batch_stride(src), FRAMES, NULL, cmhip_batch_dev_in(mid),
                              cmhip_batch_stride(mid)) != COOLMIC_ERROR_NONE ||
            cmhip_bus_run(bus, cmhip_batch_dev_in(mid), cmhip_batch_stride(mid), FRAMES, NULL, cmhip_batch_dev_in(b),
                          cmhip_batch_stride(b), counts) != COOLMIC_ERROR_NONE ||
            cmhip_batch_run(b, counts[0], counts) != COOLMIC_ERROR_NONE ||
            cmhip_batch_vu_result(b, 0, &vu) != COOLMIC_ERROR_NONE ||
            cmhip_automix_state(amx, gain, NULL, NULL) != COOLMIC_ERROR_NONE) {
            fprintf(stderr, "run: %s\n", cmhip_last_error());
            return 1;
        }
        printf("phase %u: gains %u %u %u %u, programme peak %d\n", phase + 1, (unsigned)gain[0], (unsigned)gain[1],
               (unsigned)gain[2], (unsigned)gain[3], abs((int)vu.global_peak));
    }
    cmhip_bus_free(bus);
    cmhip_automix_free(amx);
    cmhip_batch_free(b);
    cmhip_batch_free(mid);
    cmhip_batch_free(src);
    return 0;
}
