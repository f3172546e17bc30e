/*
 * batch_sweep.c -- a low cut that is moved while the signal runs, from plain C (include/coolmic_hip.h, "filter",
 * coefficient ramps): a 100 Hz tone of amplitude 8000 on a DC offset of 3000 through a HIGHPASS from cmhip_iir_design,
 * twice, in thirty blocks of 20 ms.  In front of the sixteenth block the low cut goes from 40 to 160 Hz: on stream 0 with
 * cmhip_iir_set, between two frames; on stream 1 with cmhip_iir_ramp over 50 ms, every frame with a section of its own
 * between the two, all of them with their zero on z = 1 exactly.
 *
 * The program prints both sections, where stream 1's ramp stands after every block from then on (cmhip_iir_ramp_state
 * and cmhip_iir_get ask the host mirror, no device), and for each stream around the move -- 10 ms in front of it to
 * 60 ms behind it -- the largest sample-to-sample jump and the largest second difference of the output, beside the
 * second difference of the undisturbed tone in front of the move; then the last 100 ms' mean, the residual DC, and
 * their peak: both streams have arrived at the same 160 Hz filter.
 *   "stream 0 (step): largest jump 104, largest second difference 5 (4 before the move)"
 *   "stream 1 (ramp over 2400 frames): largest jump 104, largest second difference 4 (4 before the move)"
 * The sections are direct form I and a low cut's b0 + b1 + b2 is 0 at both ends, so the offset moves nothing and even
 * the step bends the tone by no more than an LSB or so; a peak filter pulled down by 12 dB is where a step is heard
 * (tests/test_iir_ramp_host.py has that case on the model).
 *
 *   cc -I include examples/batch_sweep.c -L libcoolmic-dsp_amd/lib -lcoolmic-dsp-hip -lm \
 *      -Wl,-rpath,$PWD/libcoolmic-dsp_amd/lib -o batch_sweep && ./batch_sweep
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <coolmic-dsp/coolmic-dsp.h>
#include <coolmic_hip.h>

enum { STREAMS = 2, RATE = 48000, BLOCK = 960, BLOCKS = 30, MOVE = 15, RAMP = 2400, TAIL = 4800, OFFSET = 3000, TONE = 8000 };

static long largest_difference(const int16_t *y, long lo, long hi, int order)
{
    long worst = 0, n;
    for (n = lo + order; n < hi; n++) {
        const long d = order == 1 ? (long)y[n] - y[n - 1] : (long)y[n] - 2L * y[n - 1] + y[n - 2];
        worst = labs(d) > worst ? labs(d) : worst;
    }
    return worst;
}

int main(void)
{
    static int16_t pcm[BLOCK], y[STREAMS][BLOCKS * BLOCK];
    static const cmhip_iir_design_desc_t low = {CMHIP_IIR_HIGHPASS, RATE, 40.0, 0.70710678118654752, 0.0};
    static const cmhip_iir_design_desc_t high = {CMHIP_IIR_HIGHPASS, RATE, 160.0, 0.70710678118654752, 0.0};
    cmhip_batch_desc_t sd = {0};
    cmhip_iir_desc_t fd = {0};
    cmhip_iir_section_t from, to, now;
    cmhip_batch_t *src, *dst;
    cmhip_iir_t *iir;
    uint32_t counts[STREAMS] = {BLOCK, BLOCK}, done, frames;
    uint64_t clips[STREAMS], overs[STREAMS];
    const long at = (long)MOVE * BLOCK;
    long jump[STREAMS], bend[STREAMS];
    unsigned n, s, k;

    sd.device = 0; sd.streams = STREAMS; sd.channels = 1; sd.rate = RATE; sd.max_frames = BLOCK; sd.flags = CMHIP_VU;
    src = cmhip_batch_new(&sd);                      /* (batches used as device memory) */
    dst = cmhip_batch_new(&sd);
    if (!src || !dst) {
        fprintf(stderr, "batch: %s\n", cmhip_last_error());
        return 1;
    }
    fd.device = 0; fd.streams = STREAMS; fd.channels = 1; fd.sections = 1; fd.max_frames = BLOCK;
    iir = cmhip_iir_new(&fd);
    if (!iir || cmhip_iir_design(&low, &from) != COOLMIC_ERROR_NONE || cmhip_iir_design(&high, &to) != COOLMIC_ERROR_NONE ||
        cmhip_iir_set(iir, -1, 0, &from) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "filter: %s\n", cmhip_last_error());
        return 1;
    }
    printf("low cut: HIGHPASS %.0f Hz: b %d %d %d a %d %d -> %.0f Hz: b %d %d %d a %d %d (units of 2^-26)\n", low.f0,
           (int)from.b0, (int)from.b1, (int)from.b2, (int)from.a1, (int)from.a2, high.f0, (int)to.b0, (int)to.b1, (int)to.b2,
           (int)to.a1, (int)to.a2);
    for (k = 0; k < BLOCKS; k++) {
        if (k == MOVE && (cmhip_iir_set(iir, 0, 0, &to) != COOLMIC_ERROR_NONE ||
                          cmhip_iir_ramp(iir, 1, 0, &to, RAMP) != COOLMIC_ERROR_NONE)) {
            fprintf(stderr, "move: %s\n", cmhip_last_error());
            return 1;
        }
        for (n = 0; n < BLOCK; n++)
            pcm[n] = (int16_t)(OFFSET + lrint(TONE * sin(2.0 * M_PI * (k * BLOCK + n) / 480.0)));
        for (s = 0; s < STREAMS; s++) {
            if (cmhip_batch_upload(src, s, pcm, BLOCK) != COOLMIC_ERROR_NONE) {
                fprintf(stderr, "upload: %s\n", cmhip_last_error());
                return 1;
            }
        }
        if (cmhip_batch_sync(src) != COOLMIC_ERROR_NONE ||
            cmhip_iir_run(iir, cmhip_batch_dev_in(src), cmhip_batch_stride(src), BLOCK, counts, cmhip_batch_dev_in(dst),
                          cmhip_batch_stride(dst)) != COOLMIC_ERROR_NONE ||
            cmhip_iir_sync(iir) != COOLMIC_ERROR_NONE) {
            fprintf(stderr, "run: %s\n", cmhip_last_error());
            return 1;
        }
        for (s = 0; s < STREAMS; s++) {
            if (cmhip_batch_download_input(dst, s, y[s] + (size_t)k * BLOCK, BLOCK) != COOLMIC_ERROR_NONE) {
                fprintf(stderr, "download: %s\n", cmhip_last_error());
                return 1;
            }
        }
        if (k >= MOVE && k <= MOVE + 2) {
            if (cmhip_iir_ramp_state(iir, 1, 0, &done, &frames) != COOLMIC_ERROR_NONE ||
                cmhip_iir_get(iir, 1, 0, &now) != COOLMIC_ERROR_NONE) {
                fprintf(stderr, "state: %s\n", cmhip_last_error());
                return 1;
            }
            printf("after block %u: stream 1's ramp at %u of %u, in force b %d %d %d a %d %d, b0 + b1 + b2 = %d\n", k,
                   (unsigned)done, (unsigned)frames, (int)now.b0, (int)now.b1, (int)now.b2, (int)now.a1, (int)now.a2,
                   (int)(now.b0 + now.b1 + now.b2));
        }
    }
    if (cmhip_iir_state(iir, clips, overs, 0) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "state: %s\n", cmhip_last_error());
        return 1;
    }
    for (s = 0; s < STREAMS; s++) {
        jump[s] = largest_difference(y[s], at - 480, at + 2880, 1);
        bend[s] = largest_difference(y[s], at - 480, at + 2880, 2);
        if (s == 0)
            printf("stream 0 (step): ");
        else
            printf("stream 1 (ramp over %d frames): ", (int)RAMP);
        printf("largest jump %ld, largest second difference %ld (%ld before the move)\n", jump[s], bend[s],
               largest_difference(y[s], at - 960, at - 480, 2));
    }
    for (s = 0; s < STREAMS; s++) {
        long sum = 0, peak = 0;
        for (n = 0; n < TAIL; n++) {                     /* ten whole periods of the tone */
            const long v = y[s][(size_t)BLOCKS * BLOCK - TAIL + n];
            sum += v;
            peak = labs(v) > peak ? labs(v) : peak;
        }
        printf("stream %u: last 100 ms mean %.3f peak %ld, filter clips=%llu overs=%llu\n", s, (double)sum / TAIL, peak,
               (unsigned long long)clips[s], (unsigned long long)overs[s]);
    }
    cmhip_iir_free(iir);
    cmhip_batch_free(dst);
    cmhip_batch_free(src);
    return bend[1] <= bend[0] && jump[1] <= jump[0] ? 0 : 1;
}
