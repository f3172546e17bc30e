/*
 * batch_watch.c -- the signal watch from plain C (include/coolmic_hip.h, "signal watch"): which streams are dead, which
 * are clipped, which carry DC.  Four mono streams of ten seconds at 8 kHz go through one batch in blocks of one second:
 * programme (a 440 Hz tone at -12 dBFS); the same programme with two seconds of digital silence in the middle; a sine at
 * -3 dBFS that the batch's gain drives 6 dB up, so that it saturates; and a sine at -20 dBFS on a DC offset of 1000.
 * The programme prints per stream the longest dead air in seconds, the clip events and the DC.  The dead air is found
 * although it straddles three blocks and a VU window over the ten seconds would show a mean of programme; the clipped
 * sine touches the rail for runs of 3 or more samples at every crest; the DC reads 1000 / 32768 = +0.0305.  It exits
 * non-zero unless the four streams read as described.
 *
 *   cc -I include examples/batch_watch.c -L libcoolmic-dsp_amd/lib -lcoolmic-dsp-hip -lm \
 *      -Wl,-rpath,$PWD/libcoolmic-dsp_amd/lib -o batch_watch && ./batch_watch
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <coolmic-dsp/coolmic-dsp.h>
#include <coolmic_hip.h>

enum { RATE = 8000, SECONDS = 10, STREAMS = 4 };

static double level(double db) { return 32768.0 * pow(10.0, db / 20.0); }

int main(void)
{
    static const char *name[STREAMS] = {"programme", "programme with a gap", "sine 6 dB over", "sine on DC"};
    const double pi = 3.14159265358979323846;
    const uint16_t unity = 1000, twice = 1995;       /* +6 dB over a scale of 1000 */
    cmhip_batch_desc_t d = {0};
    coolmic_watch_result_t res[STREAMS];
    int rc[STREAMS];
    int16_t *pcm = malloc(sizeof(int16_t) * RATE);
    cmhip_batch_t *b;
    int s, sec, i, ok;

    d.device = 0; d.streams = STREAMS; d.channels = 1; d.rate = RATE; d.max_frames = RATE;
    d.flags = CMHIP_VU;
    b = cmhip_batch_new(&d);
    if (!b || !pcm) {
        fprintf(stderr, "cmhip_batch_new: %s\n", cmhip_last_error());
        return 1;
    }
    if (cmhip_batch_set_gain(b, -1, 1, 1000, &unity) != COOLMIC_ERROR_NONE ||
        cmhip_batch_set_gain(b, 2, 1, 1000, &twice) != COOLMIC_ERROR_NONE ||
        cmhip_batch_watch_configure(b, cmhip_watch_level(-60.2), 32767, 3) != COOLMIC_ERROR_NONE ||
        cmhip_batch_set_watch(b, 1) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "watch: %s\n", cmhip_last_error());
        return 1;
    }
    for (sec = 0; sec < SECONDS; sec++) {
        for (s = 0; s < STREAMS; s++) {
            for (i = 0; i < RATE; i++) {
                const double t = (double)(sec * RATE + i) / RATE;
                double v;
                switch (s) {
                case 0: v = level(-12.0) * sin(2.0 * pi * 440.0 * t); break;
                case 1: v = t >= 3.5 && t < 5.5 ? 0.0 : level(-12.0) * sin(2.0 * pi * 440.0 * t); break;
                case 2: v = level(-3.0) * sin(2.0 * pi * 100.0 * t); break;
                default: v = 1000.0 + level(-20.0) * sin(2.0 * pi * 250.0 * t); break;
                }
                pcm[i] = (int16_t)lrint(v);
            }
            if (cmhip_batch_upload(b, (unsigned)s, pcm, RATE) != COOLMIC_ERROR_NONE) {
                fprintf(stderr, "upload: %s\n", cmhip_last_error());
                return 1;
            }
        }
        if (cmhip_batch_run(b, RATE, NULL) != COOLMIC_ERROR_NONE) {
            fprintf(stderr, "run: %s\n", cmhip_last_error());
            return 1;
        }
    }
    if (cmhip_batch_watch_results(b, res, rc) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "results: %s\n", cmhip_last_error());
        return 1;
    }
    for (s = 0; s < STREAMS; s++) {
        if (rc[s] != COOLMIC_ERROR_NONE)
            return 1;
        printf("%s: longest dead air %.3f s, clip events %llu, DC %+.4f\n", name[s],
               (double)res[s].dead_longest / RATE, (unsigned long long)res[s].clip_events[0], res[s].dc[0]);
    }
    ok = res[0].dead_longest < 8 && res[0].clip_events[0] == 0 && fabs(res[0].dc[0]) < 1e-3;
    ok = ok && res[1].dead_longest >= 2 * RATE && res[1].dead_longest < 2 * RATE + 8 && res[1].clip_events[0] == 0;
    ok = ok && res[2].clip_events[0] == 2 * 100 * SECONDS && res[2].dead_longest < 8;
    ok = ok && res[3].clip_events[0] == 0 && fabs(res[3].dc[0] - 1000.0 / 32768.0) < 1e-4;
    cmhip_batch_free(b);
    free(pcm);
    return ok ? 0 : 1;
}
