/*
 * batch_resample.c -- sample-rate conversion in front of a batch (include/coolmic_hip.h) from plain C: 8 stereo
 * streams of the device-side sine at 44 100 Hz, resampled straight into the slots of a 48 000 Hz batch on the
 * batch's stream, then VU and true peak of the 48 kHz signal per stream.
 *
 *   cc -I include examples/batch_resample.c -L libcoolmic-dsp_amd/lib -lcoolmic-dsp-hip \
 *      -Wl,-rpath,$PWD/libcoolmic-dsp_amd/lib -o batch_resample && ./batch_resample
 */
#include <stdio.h>
#include <stdlib.h>
#include <coolmic-dsp/coolmic-dsp.h>
#include <coolmic_hip.h>

enum { STREAMS = 8, FRAMES_IN = 4410 };           /* 100 ms */

int main(void)
{
    cmhip_batch_desc_t sd = {0}, bd = {0};
    cmhip_src_desc_t rd = {0};
    cmhip_batch_t *src, *b;
    cmhip_src_t *r;
    coolmic_vumeter_result_t vu[STREAMS];
    coolmic_truepeak_result_t tp[STREAMS];
    uint32_t counts[STREAMS], most = 0;
    unsigned L, M, T, s;

    /* the sources: a batch used as 44.1 kHz device memory that the engine fills with its sine */
    sd.device = 0; sd.streams = STREAMS; sd.channels = 2; sd.rate = 44100; sd.max_frames = FRAMES_IN;
    sd.flags = CMHIP_VU;
    src = cmhip_batch_new(&sd);
    if (!src || cmhip_batch_generate(src, CMHIP_GEN_SINE, 0, FRAMES_IN, 0, 1, 0) != COOLMIC_ERROR_NONE ||
        cmhip_batch_sync(src) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "sources: %s\n", cmhip_last_error());
        return 1;
    }
    /* the 48 kHz batch, sized by the geometry of the conversion: floor(max_in * L / M) + 1 frames */
    if (cmhip_src_design(44100, 48000, &L, &M, &T, NULL, 0) != COOLMIC_ERROR_NONE)
        return 1;
    bd.device = 0; bd.streams = STREAMS; bd.channels = 2; bd.rate = 48000;
    bd.max_frames = (size_t)FRAMES_IN * L / M + 1;
    bd.flags = CMHIP_VU;
    b = cmhip_batch_new(&bd);
    if (!b || cmhip_batch_set_true_peak(b, 1) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "batch: %s\n", cmhip_last_error());
        return 1;
    }
    /* the resampler between them, on the batch's stream: its output is the batch's input, in order */
    rd.device = 0; rd.streams = STREAMS; rd.channels = 2; rd.rate_in = 44100; rd.rate_out = 48000;
    rd.max_in_frames = FRAMES_IN; rd.hip_stream = cmhip_batch_hip_stream(b);
    r = cmhip_src_new(&rd);
    if (!r || cmhip_src_max_out_frames(r) != bd.max_frames) {
        fprintf(stderr, "resampler: %s\n", cmhip_last_error());
        return 1;
    }
    printf("44100 -> 48000: L %u M %u T %u, %d frames in, at most %zu out\n", L, M, T, (int)FRAMES_IN,
           cmhip_src_max_out_frames(r));
    if (cmhip_src_run(r, cmhip_batch_dev_in(src), cmhip_batch_stride(src), FRAMES_IN, NULL, cmhip_batch_dev_in(b),
                      cmhip_batch_stride(b), counts) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "src_run: %s\n", cmhip_last_error());
        return 1;
    }
    for (s = 0; s < STREAMS; s++)
        if (counts[s] > most)
            most = counts[s];
    if (cmhip_batch_run(b, most, counts) != COOLMIC_ERROR_NONE ||
        cmhip_batch_vu_results(b, vu, NULL) != COOLMIC_ERROR_NONE ||
        cmhip_batch_tp_results(b, tp, NULL) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "batch run: %s\n", cmhip_last_error());
        return 1;
    }
    for (s = 0; s < STREAMS; s++)
        printf("stream %u: frames=%zu rate=%u peak=%d power=%.4f dbtp=%.4f\n", s, vu[s].frames, (unsigned)vu[s].rate,
               (int)vu[s].global_peak, vu[s].global_power, tp[s].global_dbtp);
    cmhip_src_free(r);
    cmhip_batch_free(b);
    cmhip_batch_free(src);
    return 0;
}
