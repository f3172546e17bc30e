/*
 * batch_spectrum.c -- the spectrum meter from plain C (include/coolmic_hip.h, "spectrum"): where in frequency the
 * energy lies.  One mono stream at 8 kHz carries a 1 kHz tone at -20 dBFS and 50 Hz mains hum at -60 dBFS; the meter
 * runs blocks of 4096 frames (1.95 Hz per bin) over third-octave bands around 1 kHz, designed by the library, and the
 * programme prints every band that holds anything.  The tone's band (bins 457..574) reads -20.00 dB and the hum's
 * (bins 23..28, 44.9 to 56.6 Hz) -60.01 dB; everything else together -- the rounding of the samples to integers and
 * of the transform -- lies at -97 dB in the model of the specification, the loudest other band at -102 dB.  The
 * programme exits non-zero unless both bands are within 0.1 dB of their levels and every other band below -90 dB.
 *
 * (At 48 kHz a 4096-point bin is 11.7 Hz wide, the 50 Hz third octave is the single bin 4 and holds a part of the
 * hum's main lobe only: it reads -62.2 dB there.  A band reads a tone's level when it holds the lobe's four bins.)
 *
 *   cc -I include examples/batch_spectrum.c -L libcoolmic-dsp_amd/lib -lcoolmic-dsp-hip -lm \
 *      -Wl,-rpath,$PWD/libcoolmic-dsp_amd/lib -o batch_spectrum && ./batch_spectrum
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <coolmic-dsp/coolmic-dsp.h>
#include <coolmic_hip.h>

enum { RATE = 8000, LOG2 = 12, FRAMES = 8 << LOG2 };

int main(void)
{
    const double pi = 3.14159265358979323846;
    const double tone = 32768.0 * pow(10.0, -20.0 / 20.0), hum = 32768.0 * pow(10.0, -60.0 / 20.0);
    cmhip_batch_desc_t d = {0};
    coolmic_spectrum_result_t res;
    uint16_t edges[CMHIP_SPEC_MAX_BANDS + 1];
    int16_t *pcm = malloc(sizeof(int16_t) * FRAMES);
    cmhip_batch_t *b;
    int nb, i, k, ok = 1, seen = 0;

    d.device = 0; d.streams = 1; d.channels = 1; d.rate = RATE; d.max_frames = FRAMES;
    d.flags = CMHIP_VU;
    b = cmhip_batch_new(&d);
    if (!b || !pcm) {
        fprintf(stderr, "cmhip_batch_new: %s\n", cmhip_last_error());
        return 1;
    }
    nb = cmhip_spec_design_bands(RATE, LOG2, 3, edges);
    if (nb < 1 || cmhip_batch_spec_configure(b, LOG2, (unsigned)nb, edges, 0, NULL) != COOLMIC_ERROR_NONE ||
        cmhip_batch_set_spectrum(b, 1) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "spectrum: %s\n", cmhip_last_error());
        return 1;
    }
    for (i = 0; i < FRAMES; i++)
        pcm[i] = (int16_t)lrint(tone * sin(2.0 * pi * 1000.0 * i / RATE) + hum * sin(2.0 * pi * 50.0 * i / RATE));
    if (cmhip_batch_upload(b, 0, pcm, FRAMES) != COOLMIC_ERROR_NONE ||
        cmhip_batch_run(b, FRAMES, NULL) != COOLMIC_ERROR_NONE ||
        cmhip_batch_spec_result(b, 0, &res) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "batch failed: %s\n", cmhip_last_error());
        return 1;
    }
    printf("%lu blocks of %u frames, %u bands\n", (unsigned long)res.blocks, 1u << res.fft_log2, res.bands);
    for (k = 0; k < (int)res.bands; k++) {
        const double lo = (double)res.edges[k] * RATE / (1 << LOG2), hi = (double)res.edges[k + 1] * RATE / (1 << LOG2);
        const int is_tone = lo <= 1000.0 && 1000.0 < hi, is_hum = lo <= 50.0 && 50.0 < hi;
        const double level = res.db[0][k];
        if (is_tone || is_hum) {
            printf("%s (%.1f to %.1f Hz): %.2f dB\n", is_tone ? "1 kHz band" : "50 Hz band", lo, hi, level);
            ok = ok && fabs(level - (is_tone ? -20.0 : -60.0)) < 0.1;
            seen++;
        } else {
            if (res.power[0][k])
                printf("band %d (%.1f to %.1f Hz): %.2f dB\n", k, lo, hi, level);
            ok = ok && level < -90.0;
        }
    }
    cmhip_batch_free(b);
    free(pcm);
    return ok && seen == 2 ? 0 : 1;
}
