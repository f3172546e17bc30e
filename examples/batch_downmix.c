/*
 * batch_downmix.c -- the chain source -> rate -> width -> batch (include/coolmic_hip.h) from plain C: 8 stereo streams
 * of the device-side sine at 44 100 Hz go through a resampler to 48 000 Hz and through a mixer with the preset
 * CMHIP_MIX_STEREO_TO_MONO straight into the slots of a mono 48 000 Hz batch with VU and loudness on.  All three run
 * on the batch's stream, with no synchronisation between them.  Prints one line of geometry, then one line per
 * stream: "stream N: frames=24000 rate=48000 channels=1 peak=... power=... momentary=..." (power in dB, momentary
 * loudness in LUFS; half a second of a full-scale sine gives about -3 for both).
 *
 *   cc -I include examples/batch_downmix.c -L libcoolmic-dsp_amd/lib -lcoolmic-dsp-hip \
 *      -Wl,-rpath,$PWD/libcoolmic-dsp_amd/lib -o batch_downmix && ./batch_downmix
 */
#include <stdio.h>
#include <stdlib.h>
#include <coolmic-dsp/coolmic-dsp.h>
#include <coolmic_hip.h>

enum { STREAMS = 8, FRAMES_IN = 22050 };          /* 500 ms: five sub-blocks of loudness */

static void *dev_alloc(cmhip_batch_t **keep, unsigned channels, unsigned rate, size_t frames)
{
    /* a batch used as device memory: STREAMS slots of `frames` frames */
    cmhip_batch_desc_t d = {0};
    d.device = 0; d.streams = STREAMS; d.channels = channels; d.rate = rate; d.max_frames = frames;
    d.flags = CMHIP_VU;
    *keep = cmhip_batch_new(&d);
    return *keep ? cmhip_batch_dev_in(*keep) : NULL;
}

int main(void)
{
    cmhip_batch_desc_t bd = {0};
    cmhip_src_desc_t rd = {0};
    cmhip_mix_desc_t md = {0};
    cmhip_batch_t *src, *mid, *b;
    cmhip_src_t *r;
    cmhip_mix_t *m;
    coolmic_vumeter_result_t vu[STREAMS];
    coolmic_loudness_result_t loud[STREAMS];
    uint32_t counts[STREAMS], most = 0;
    int16_t W[2];
    unsigned L, M, T, ci, co, s;
    size_t max_out;

    if (cmhip_src_design(44100, 48000, &L, &M, &T, NULL, 0) != COOLMIC_ERROR_NONE ||
        cmhip_mix_preset(CMHIP_MIX_STEREO_TO_MONO, &ci, &co, W, 2) != COOLMIC_ERROR_NONE)
        return 1;
    max_out = (size_t)FRAMES_IN * L / M + 1;
    /* the sources at 44.1 kHz, filled with the engine's sine, and the stereo 48 kHz signal between rate and width */
    if (!dev_alloc(&src, 2, 44100, FRAMES_IN) || !dev_alloc(&mid, 2, 48000, max_out) ||
        cmhip_batch_generate(src, CMHIP_GEN_SINE, 0, FRAMES_IN, 0, 1, 0) != COOLMIC_ERROR_NONE ||
        cmhip_batch_sync(src) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "sources: %s\n", cmhip_last_error());
        return 1;
    }
    /* the mono 48 kHz batch that meters what is sent */
    bd.device = 0; bd.streams = STREAMS; bd.channels = co; bd.rate = 48000; bd.max_frames = max_out;
    bd.flags = CMHIP_VU;
    b = cmhip_batch_new(&bd);
    if (!b || cmhip_batch_set_loudness(b, 1) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "batch: %s\n", cmhip_last_error());
        return 1;
    }
    /* rate and width in front of it, on the batch's stream: each one's output is the next one's input, in order */
    rd.device = 0; rd.streams = STREAMS; rd.channels = ci; rd.rate_in = 44100; rd.rate_out = 48000;
    rd.max_in_frames = FRAMES_IN; rd.hip_stream = cmhip_batch_hip_stream(b);
    md.device = 0; md.streams = STREAMS; md.channels_in = ci; md.channels_out = co; md.max_frames = max_out;
    md.hip_stream = cmhip_batch_hip_stream(b);
    r = cmhip_src_new(&rd);
    m = cmhip_mix_new(&md);
    if (!r || !m || cmhip_mix_set_matrix(m, -1, W) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "resampler, mixer: %s\n", cmhip_last_error());
        return 1;
    }
    printf("44100 -> 48000: L %u M %u T %u; %u -> %u channels: W = {%d, %d}; %d frames in, at most %zu out\n", L, M, T,
           ci, co, (int)W[0], (int)W[1], (int)FRAMES_IN, max_out);
    if (cmhip_src_run(r, cmhip_batch_dev_in(src), cmhip_batch_stride(src), FRAMES_IN, NULL, cmhip_batch_dev_in(mid),
                      cmhip_batch_stride(mid), counts) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "src_run: %s\n", cmhip_last_error());
        return 1;
    }
    for (s = 0; s < STREAMS; s++)
        if (counts[s] > most)
            most = counts[s];
    if (cmhip_mix_run(m, cmhip_batch_dev_in(mid), cmhip_batch_stride(mid), most, counts, cmhip_batch_dev_in(b),
                      cmhip_batch_stride(b)) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "mix_run: %s\n", cmhip_last_error());
        return 1;
    }
    if (cmhip_batch_run(b, most, counts) != COOLMIC_ERROR_NONE ||
        cmhip_batch_vu_results(b, vu, NULL) != COOLMIC_ERROR_NONE ||
        cmhip_batch_loud_results(b, loud, NULL) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "batch run: %s\n", cmhip_last_error());
        return 1;
    }
    for (s = 0; s < STREAMS; s++)
        printf("stream %u: frames=%zu rate=%u channels=%u peak=%d power=%.4f momentary=%.4f\n", s, vu[s].frames,
               (unsigned)vu[s].rate, vu[s].channels, (int)vu[s].global_peak, vu[s].global_power, loud[s].momentary);
    cmhip_mix_free(m);
    cmhip_src_free(r);
    cmhip_batch_free(b);
    cmhip_batch_free(mid);
    cmhip_batch_free(src);
    return 0;
}
