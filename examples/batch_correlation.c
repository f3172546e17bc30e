/*
 * batch_correlation.c -- the phase-correlation / balance meter from plain C (include/coolmic_hip.h, "phase
 * correlation"): what a stereo programme will do in a mono sum, before it is summed.  Three stereo streams of one
 * batch: L = R (mono compatible: +1), L = -R (cancels in the sum: -1) and a sine at fs/8 against its quarter-period
 * shift (quadrature: 0).  The sums are exact integers, so the first two values are exactly +1.0 and -1.0; the
 * programme exits non-zero unless they are, and unless the third is below 0.01 in magnitude.
 *
 *   cc -I include examples/batch_correlation.c -L libcoolmic-dsp_amd/lib -lcoolmic-dsp-hip -lm \
 *      -Wl,-rpath,$PWD/libcoolmic-dsp_amd/lib -o batch_correlation && ./batch_correlation
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <coolmic-dsp/coolmic-dsp.h>
#include <coolmic_hip.h>

enum { STREAMS = 3, FRAMES = 4800 };

/* 30000 * sin(2 pi k / 8), rounded */
static const int16_t sine8[8] = {0, 21213, 30000, 21213, 0, -21213, -30000, -21213};

int main(void)
{
    static const char *const name[STREAMS] = {"L = R", "L = -R", "sine against its quarter period"};
    cmhip_batch_desc_t d = {0};
    coolmic_correlation_result_t res[STREAMS];
    int rcs[STREAMS];
    int16_t *pcm = malloc(sizeof(int16_t) * 2 * FRAMES);
    cmhip_batch_t *b;
    uint32_t st = 12345u;
    unsigned s;
    int i, ok;

    d.device = 0; d.streams = STREAMS; d.channels = 2; d.rate = 48000; d.max_frames = FRAMES;
    d.flags = CMHIP_VU;
    b = cmhip_batch_new(&d);
    if (!b || !pcm) {
        fprintf(stderr, "cmhip_batch_new: %s\n", cmhip_last_error());
        return 1;
    }
    if (cmhip_batch_set_correlation(b, 1) != COOLMIC_ERROR_NONE) {      /* the default pair: channels (0, 1) */
        fprintf(stderr, "cmhip_batch_set_correlation: %s\n", cmhip_last_error());
        return 1;
    }
    for (s = 0; s < STREAMS; s++) {
        for (i = 0; i < FRAMES; i++) {
            int l, r;
            if (s < 2) {                            /* noise, kept off -32768 so that -L is a sample */
                st = st * 1664525u + 1013904223u;
                l = (int16_t)(st >> 16);
                if (l < -32767)
                    l = -32767;
                r = s == 0 ? l : -l;
            } else {
                l = sine8[i % 8];
                r = sine8[(i + 2) % 8];
            }
            pcm[2 * i] = (int16_t)l;
            pcm[2 * i + 1] = (int16_t)r;
        }
        if (cmhip_batch_upload(b, s, pcm, FRAMES) != COOLMIC_ERROR_NONE)
            return 1;
    }
    if (cmhip_batch_run(b, FRAMES, NULL) != COOLMIC_ERROR_NONE ||
        cmhip_batch_corr_results(b, res, rcs) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "batch failed: %s\n", cmhip_last_error());
        return 1;
    }
    for (s = 0; s < STREAMS; s++) {
        if (rcs[s] != COOLMIC_ERROR_NONE)
            return 1;
        printf("%s: correlation %+.6f, balance %+.2f dB (%lu frames: energy %llu / %llu, cross %lld)\n", name[s],
               res[s].correlation[0], res[s].balance_db[0], (unsigned long)res[s].frames,
               (unsigned long long)res[s].energy_a[0], (unsigned long long)res[s].energy_b[0],
               (long long)res[s].cross[0]);
    }
    ok = res[0].correlation[0] == 1.0 && res[1].correlation[0] == -1.0 && fabs(res[2].correlation[0]) < 0.01;
    cmhip_batch_free(b);
    free(pcm);
    return ok ? 0 : 1;
}
