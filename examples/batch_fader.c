/*
 * batch_fader.c -- a fader move on a mix bus from plain C (include/coolmic_hip.h, "send ramps"): four mono
 * microphones, each the device-side sine, on one stereo bus -- microphone 0 on the left, microphone 1 on the right (in
 * the table from the start, with a zero matrix), 2 and 3 in the centre -- straight into a stereo batch with PCM out and
 * VU on.  At frame 1208, with microphone 0's sine near its crest, microphone 0 goes out and microphone 1 comes in:
 * once as a ramp over 480 frames, once as a step (ramp_frames 0).  The programme runs in blocks; bus and batch share
 * the batch's stream.  Prints cmhip_bus_ramp_state of both sends after every block of the faded programme, one VU line
 * per programme, and the largest sample-to-sample jump of the left channel of each: the step clicks, the ramp does not.
 *
 *   cc -I include examples/batch_fader.c -L libcoolmic-dsp_amd/lib -lcoolmic-dsp-hip \
 *      -Wl,-rpath,$PWD/libcoolmic-dsp_amd/lib -o batch_fader && ./batch_fader
 */
#include <stdio.h>
#include <stdlib.h>
#include <coolmic-dsp/coolmic-dsp.h>
#include <coolmic_hip.h>

enum { MICS = 4, FRAMES = 2400, CUT = 1208, FADE = 480, BLOCKS = 4 };
static const size_t BLOCK[BLOCKS] = {CUT, FADE / 2, FADE / 2, FRAMES - CUT - FADE};

/* one programme: -> the largest jump between two successive samples of the left channel, or -1 */
static int programme(cmhip_batch_t *src, uint32_t ramp_frames, int talk)
{
    static int16_t pcm[FRAMES * 2];
    /* [send][C_out = 2][C_in = 1]: left, right, centre, centre; microphone 1 is in the table with a zero matrix */
    const int16_t W[MICS * 2] = {8192, 0, 0, 0, 4096, 4096, 4096, 4096};
    const int16_t W_out[2] = {0, 0}, W_in[2] = {0, 8192};
    const uint32_t bus[MICS] = {0, 0, 0, 0}, stream[MICS] = {0, 1, 2, 3};
    cmhip_batch_desc_t bd = {0};
    cmhip_bus_desc_t md = {0};
    coolmic_vumeter_result_t vu;
    cmhip_batch_t *b;
    cmhip_bus_t *m;
    size_t at = 0;
    int jump = 0;
    unsigned i;

    bd.device = 0; bd.streams = 1; bd.channels = 2; bd.rate = 48000; bd.max_frames = FRAMES;
    bd.flags = CMHIP_OUT_PCM | CMHIP_VU;
    b = cmhip_batch_new(&bd);
    if (!b) {
        fprintf(stderr, "batch: %s\n", cmhip_last_error());
        return -1;
    }
    md.device = 0; md.streams = MICS; md.buses = 1; md.channels_in = 1; md.channels_out = 2;
    md.max_frames = FRAMES; md.max_sends = MICS; md.hip_stream = cmhip_batch_hip_stream(b);
    m = cmhip_bus_new(&md);
    if (!m || cmhip_bus_set_routing(m, MICS, bus, stream, W) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "bus: %s\n", cmhip_last_error());
        return -1;
    }
    for (i = 0; i < BLOCKS; i++) {
        const int16_t *in = (const int16_t *)cmhip_batch_dev_in(src) + at;       /* (mono: a frame is a sample) */
        uint32_t count, done[2], of[2];
        if (at == CUT && (cmhip_bus_ramp_sends(m, 0, 1, W_out, ramp_frames) != COOLMIC_ERROR_NONE ||
                          cmhip_bus_ramp_sends(m, 1, 1, W_in, ramp_frames) != COOLMIC_ERROR_NONE)) {
            fprintf(stderr, "bus_ramp_sends: %s\n", cmhip_last_error());
            return -1;
        }
        if (cmhip_bus_run(m, in, cmhip_batch_stride(src), BLOCK[i], NULL, cmhip_batch_dev_in(b), cmhip_batch_stride(b),
                          &count) != COOLMIC_ERROR_NONE ||
            cmhip_batch_run(b, BLOCK[i], &count) != COOLMIC_ERROR_NONE ||
            cmhip_batch_download(b, 0, pcm + at * 2, count) != COOLMIC_ERROR_NONE ||
            cmhip_batch_sync(b) != COOLMIC_ERROR_NONE) {
            fprintf(stderr, "block %u: %s\n", i, cmhip_last_error());
            return -1;
        }
        if (cmhip_bus_ramp_state(m, 0, &done[0], &of[0], NULL) != COOLMIC_ERROR_NONE ||
            cmhip_bus_ramp_state(m, 1, &done[1], &of[1], NULL) != COOLMIC_ERROR_NONE)
            return -1;
        at += count;
        if (talk)
            printf("block %u: frames=%u at=%zu send0=%u/%u send1=%u/%u\n", i, (unsigned)count, at, (unsigned)done[0],
                   (unsigned)of[0], (unsigned)done[1], (unsigned)of[1]);
    }
    if (cmhip_batch_vu_results(b, &vu, NULL) != COOLMIC_ERROR_NONE)
        return -1;
    printf("%s: frames=%zu channels=%u peak=%d power=%.4f\n", ramp_frames ? "faded" : "stepped", vu.frames, vu.channels,
           (int)vu.global_peak, vu.global_power);
    for (at = 1; at < FRAMES; at++) {
        const int d = abs((int)pcm[at * 2] - (int)pcm[at * 2 - 2]);
        jump = d > jump ? d : jump;
    }
    cmhip_bus_free(m);
    cmhip_batch_free(b);
    return jump;
}

int main(void)
{
    cmhip_batch_desc_t sd = {0};
    cmhip_batch_t *src;
    int faded, stepped;

    /* the microphones: a batch used as device memory, filled with the engine's sine (stream s starts at phase 7 s); one
     * slot more than there are microphones, so that MICS slots from a block's first frame on stay inside the array */
    sd.device = 0; sd.streams = MICS + 1; sd.channels = 1; sd.rate = 48000; sd.max_frames = FRAMES; sd.flags = CMHIP_VU;
    src = cmhip_batch_new(&sd);
    if (!src || cmhip_batch_generate(src, CMHIP_GEN_SINE, 0, FRAMES, 0, 1, 0) != COOLMIC_ERROR_NONE ||
        cmhip_batch_sync(src) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "sources: %s\n", cmhip_last_error());
        return 1;
    }
    faded = programme(src, FADE, 1);
    stepped = programme(src, 0, 0);
    if (faded < 0 || stepped < 0)
        return 1;
    printf("largest jump, left channel: faded=%d stepped=%d click-free=%s\n", faded, stepped,
           faded < stepped ? "yes" : "no");
    cmhip_batch_free(src);
    return faded < stepped ? 0 : 1;
}
