/*
 * batch_lowcut.c -- a low cut in front of a gate, from plain C (include/coolmic_hip.h, "filter" and "dynamics"): a
 * microphone with a DC offset of 1500 and a quiet voice on top of it (a 500 Hz tone of amplitude 1200, a quarter of a
 * second on, a quarter off), twice: stream 0 reaches the gate as it is, stream 1 behind a 40 Hz HIGHPASS from
 * cmhip_iir_design.  Both streams go through ONE filter object -- stream 0's section is left at unity, a copy bit for
 * bit -- then through one gate (below -45 dBFS, expander ratio 3, range 40 dB) into a batch with VU on, in eight blocks
 * on the batch's stream with no synchronisation between the stages.
 *
 * The gate's detector reads the offset as level: without the filter it stays open through the pauses, behind the
 * filter it closes.  The program prints the section, what the integers realise at DC and at the voice, and the gate's
 * lowest gain (Q15: 32768 is open) over a block of voice and over a block of pause, for both streams:
 *   "voice: gate gain without the filter 32768, behind the low cut 32768"
 *   "pause: gate gain without the filter 32768, behind the low cut 328"
 *
 *   cc -I include examples/batch_lowcut.c -L libcoolmic-dsp_amd/lib -lcoolmic-dsp-hip -lm \
 *      -Wl,-rpath,$PWD/libcoolmic-dsp_amd/lib -o batch_lowcut && ./batch_lowcut
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <coolmic-dsp/coolmic-dsp.h>
#include <coolmic_hip.h>

enum { STREAMS = 2, RATE = 48000, BLOCK = 12000, BLOCKS = 8, OFFSET = 1500, VOICE = 1200, DETECTOR_LOG2 = 7,
       SMOOTH_LOG2 = 6, HOLD = 960 };

int main(void)
{
    static int16_t pcm[BLOCK];
    static const cmhip_iir_design_desc_t cut = {CMHIP_IIR_HIGHPASS, RATE, 40.0, 0.70710678118654752, 0.0};
    static const cmhip_dyn_curve_desc_t gate = {0.0, 1.0, 0.0, -45.0, 3.0, 40.0};
    cmhip_batch_desc_t sd = {0};
    cmhip_iir_desc_t fd = {0};
    cmhip_dyn_desc_t dd = {0};
    cmhip_iir_section_t sec;
    uint16_t curve[CMHIP_DYN_CURVE];
    cmhip_batch_t *src, *mid, *b;
    cmhip_iir_t *iir;
    cmhip_dyn_t *dyn;
    coolmic_vumeter_result_t vu;
    uint32_t counts[STREAMS] = {BLOCK, BLOCK}, gain[STREAMS], voice[STREAMS] = {0, 0}, pause[STREAMS] = {0, 0};
    uint64_t clips[STREAMS], overs[STREAMS];
    unsigned n, s, k;

    sd.device = 0; sd.streams = STREAMS; sd.channels = 1; sd.rate = RATE; sd.max_frames = BLOCK; sd.flags = CMHIP_VU;
    src = cmhip_batch_new(&sd);                      /* (batches used as device memory) */
    mid = cmhip_batch_new(&sd);
    b = cmhip_batch_new(&sd);
    if (!src || !mid || !b) {
        fprintf(stderr, "batch: %s\n", cmhip_last_error());
        return 1;
    }
    fd.device = 0; fd.streams = STREAMS; fd.channels = 1; fd.sections = 1; fd.max_frames = BLOCK;
    fd.hip_stream = cmhip_batch_hip_stream(b);
    iir = cmhip_iir_new(&fd);
    if (!iir || cmhip_iir_design(&cut, &sec) != COOLMIC_ERROR_NONE || cmhip_iir_set(iir, 1, 0, &sec) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "filter: %s\n", cmhip_last_error());
        return 1;
    }
    dd.device = 0; dd.streams = STREAMS; dd.channels = 1; dd.detector_log2 = DETECTOR_LOG2; dd.smooth_log2 = SMOOTH_LOG2;
    dd.hold = HOLD; dd.max_frames = BLOCK; dd.hip_stream = cmhip_batch_hip_stream(b);
    dyn = cmhip_dyn_new(&dd);
    if (!dyn || cmhip_dyn_design(&gate, curve) != COOLMIC_ERROR_NONE ||
        cmhip_dyn_set_curve(dyn, -1, curve) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "gate: %s\n", cmhip_last_error());
        return 1;
    }
    printf("low cut: HIGHPASS %.0f Hz at %d: b %d %d %d a %d %d (units of 2^-26), b0 + b1 + b2 = %d; %.1f dB at 0 Hz, "
           "%.2f dB at 500 Hz\n", cut.f0, (int)RATE, (int)sec.b0, (int)sec.b1, (int)sec.b2, (int)sec.a1, (int)sec.a2,
           (int)(sec.b0 + sec.b1 + sec.b2), cmhip_iir_response_db(&sec, 1, RATE, 0.0),
           cmhip_iir_response_db(&sec, 1, RATE, 500.0));
    for (k = 0; k < BLOCKS; k++) {
        const int speaking = (k & 2u) == 0;              /* blocks 0, 1, 4, 5: voice; 2, 3, 6, 7: pause */
        for (n = 0; n < BLOCK; n++)
            pcm[n] = (int16_t)(OFFSET + (speaking ? lrint(VOICE * sin(2.0 * M_PI * (k * BLOCK + n) / 96.0)) : 0));
        for (s = 0; s < STREAMS; s++) {
            if (cmhip_batch_upload(src, s, pcm, BLOCK) != COOLMIC_ERROR_NONE) {
                fprintf(stderr, "upload: %s\n", cmhip_last_error());
                return 1;
            }
        }
        if (cmhip_batch_sync(src) != COOLMIC_ERROR_NONE ||
            cmhip_iir_run(iir, cmhip_batch_dev_in(src), cmhip_batch_stride(src), BLOCK, counts, cmhip_batch_dev_in(mid),
                          cmhip_batch_stride(mid)) != COOLMIC_ERROR_NONE ||
            cmhip_dyn_run(dyn, cmhip_batch_dev_in(mid), cmhip_batch_stride(mid), BLOCK, counts, cmhip_batch_dev_in(b),
                          cmhip_batch_stride(b)) != COOLMIC_ERROR_NONE ||
            cmhip_batch_run(b, BLOCK, counts) != COOLMIC_ERROR_NONE ||
            cmhip_dyn_min_gain(dyn, gain, 1) != COOLMIC_ERROR_NONE) {        /* this block's lowest gain; re-armed */
            fprintf(stderr, "run: %s\n", cmhip_last_error());
            return 1;
        }
        for (s = 0; s < STREAMS; s++) {
            if (k == 5)                                  /* the second block of a stretch: the gate has settled */
                voice[s] = gain[s];
            if (k == 7)
                pause[s] = gain[s];
        }
    }
    if (cmhip_iir_state(iir, clips, overs, 0) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "state: %s\n", cmhip_last_error());
        return 1;
    }
    printf("voice: gate gain without the filter %u, behind the low cut %u\n", (unsigned)voice[0], (unsigned)voice[1]);
    printf("pause: gate gain without the filter %u, behind the low cut %u\n", (unsigned)pause[0], (unsigned)pause[1]);
    for (s = 0; s < STREAMS; s++) {
        if (cmhip_batch_vu_result(b, s, &vu) != COOLMIC_ERROR_NONE) {
            fprintf(stderr, "vu: %s\n", cmhip_last_error());
            return 1;
        }
        printf("programme %u: frames=%zu rate=%u channels=%u peak=%d power=%.4f filter clips=%llu overs=%llu\n", s, vu.frames,
               (unsigned)vu.rate, vu.channels, (int)vu.global_peak, vu.global_power, (unsigned long long)clips[s],
               (unsigned long long)overs[s]);
    }
    cmhip_dyn_free(dyn);
    cmhip_iir_free(iir);
    cmhip_batch_free(b);
    cmhip_batch_free(mid);
    cmhip_batch_free(src);
    return pause[0] == 32768 && pause[1] < 1000 && voice[0] == 32768 && voice[1] == 32768 ? 0 : 1;
}
