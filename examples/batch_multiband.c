/*
 * batch_multiband.c -- a multiband compressor from plain C (include/coolmic_hip.h, "mix bus", "band split", "dynamics"
 * and "peak limiter"): four mono microphones go through a mix bus at half weights -- a 100 Hz hum, a 1 kHz voice, a
 * 6 kHz sibilant (each from frame 4000 to frame 20000) and room noise within +-40.  The sum is cut into three bands at
 * 300 Hz and 3 kHz by a band split of 255 taps; every band has a dynamics object of its own -- its own curve, level
 * window and hold, and ONE smoothing length, so the three delays are equal -- and a second bus adds the bands again at
 * unity.  A limiter holds the result under -1 dBFS, straight into the slot of a mono batch with VU on.  Everything runs
 * on the batch's stream, with no synchronisation in between.  Prints one line of geometry, one line per band
 * ("band 0: ... min_gain=... clips=...", gains in Q15: 32768 is unity) and
 * "programme: frames=24000 rate=48000 channels=1 peak=... power=... lim_min_gain=...".
 *
 *   cc -I include examples/batch_multiband.c -L libcoolmic-dsp_amd/lib -lcoolmic-dsp-hip -lm \
 *      -Wl,-rpath,$PWD/libcoolmic-dsp_amd/lib -o batch_multiband && ./batch_multiband
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <coolmic-dsp/coolmic-dsp.h>
#include <coolmic_hip.h>

enum { MICS = 4, BANDS = 3, TAPS = 255, FRAMES = 24000, SPEECH_FROM = 4000, SPEECH_TO = 20000, SMOOTH_LOG2 = 6,
       LOOKAHEAD_LOG2 = 6, THRESHOLD = 29204, DRIVE = 4096 };

int main(void)
{
    static int16_t pcm[FRAMES];
    static const double period[3] = {480.0, 48.0, 8.0}, level[3] = {16000.0, 9000.0, 6000.0};
    static const double crossover_hz[BANDS - 1] = {300.0, 3000.0};
    /* per band: compressor threshold, ratio, knee; no gate.  The top band works as a de-esser */
    static const cmhip_dyn_curve_desc_t cd[BANDS] = {
        {-24.0, 4.0, 6.0, -90.0, 1.0, 0.0}, {-18.0, 3.0, 6.0, -90.0, 1.0, 0.0}, {-30.0, 6.0, 3.0, -90.0, 1.0, 0.0}};
    static const unsigned detector_log2[BANDS] = {9, 7, 5}, hold[BANDS] = {960, 480, 96};
    cmhip_batch_desc_t sd = {0}, md = {0};
    cmhip_bus_desc_t bd = {0};
    cmhip_split_desc_t pd = {0};
    cmhip_dyn_desc_t dd = {0};
    cmhip_lim_desc_t ld = {0};
    uint16_t curve[CMHIP_DYN_CURVE];
    cmhip_batch_t *src, *sum, *bands, *comp, *mix, *b;
    cmhip_bus_t *bus, *back;
    cmhip_split_t *split;
    cmhip_dyn_t *dyn[BANDS];
    cmhip_lim_t *lim;
    coolmic_vumeter_result_t vu;
    uint32_t to_bus[MICS], from[MICS], counts[1], band_counts[BANDS], dyn_gain[BANDS][1], lim_gain[1], clips[BANDS];
    uint32_t lcg = 12345;
    int16_t W[MICS];
    unsigned i, n;

    /* the microphones: a batch used as device memory */
    sd.device = 0; sd.streams = MICS; sd.channels = 1; sd.rate = 48000; sd.max_frames = FRAMES; sd.flags = CMHIP_VU;
    src = cmhip_batch_new(&sd);
    if (!src) {
        fprintf(stderr, "sources: %s\n", cmhip_last_error());
        return 1;
    }
    for (i = 0; i < MICS; i++) {
        for (n = 0; n < FRAMES; n++) {
            if (i < 3) {
                pcm[n] = n >= SPEECH_FROM && n < SPEECH_TO ? (int16_t)lrint(level[i] * sin(2.0 * M_PI * n / period[i])) : 0;
            } else {
                lcg = lcg * 1664525u + 1013904223u;
                pcm[n] = (int16_t)((int)(lcg >> 16) % 81 - 40);
            }
        }
        if (cmhip_batch_upload(src, i, pcm, FRAMES) != COOLMIC_ERROR_NONE) {
            fprintf(stderr, "upload: %s\n", cmhip_last_error());
            return 1;
        }
    }
    /* device memory for the sum, the bands before and behind their dynamics, their sum, and the metering batch */
    md = sd;
    md.streams = 1;
    sum = cmhip_batch_new(&md);
    mix = cmhip_batch_new(&md);
    b = cmhip_batch_new(&md);
    md.streams = BANDS;
    bands = cmhip_batch_new(&md);
    comp = cmhip_batch_new(&md);
    if (!sum || !mix || !b || !bands || !comp) {
        fprintf(stderr, "batch: %s\n", cmhip_last_error());
        return 1;
    }
    /* the microphones' bus */
    bd.device = 0; bd.streams = MICS; bd.buses = 1; bd.channels_in = 1; bd.channels_out = 1;
    bd.max_frames = FRAMES; bd.max_sends = MICS; bd.hip_stream = cmhip_batch_hip_stream(b);
    bus = cmhip_bus_new(&bd);
    for (i = 0; i < MICS; i++) {
        to_bus[i] = 0;
        from[i] = i;
        W[i] = 8192;
    }
    if (!bus || cmhip_bus_set_routing(bus, MICS, to_bus, from, W) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "bus: %s\n", cmhip_last_error());
        return 1;
    }
    /* the split: one stream in, BANDS slots out, band-major */
    pd.device = 0; pd.streams = 1; pd.channels = 1; pd.bands = BANDS; pd.taps = TAPS; pd.max_frames = FRAMES;
    pd.hip_stream = cmhip_batch_hip_stream(b);
    split = cmhip_split_new(&pd, 48000, crossover_hz);
    if (!split) {
        fprintf(stderr, "split: %s\n", cmhip_last_error());
        return 1;
    }
    /* a dynamics object per band: equal smoothing, so equal delay */
    for (i = 0; i < BANDS; i++) {
        dd.device = 0; dd.streams = 1; dd.channels = 1; dd.detector_log2 = detector_log2[i]; dd.smooth_log2 = SMOOTH_LOG2;
        dd.hold = hold[i]; dd.max_frames = FRAMES; dd.hip_stream = cmhip_batch_hip_stream(b);
        dyn[i] = cmhip_dyn_new(&dd);
        if (!dyn[i] || cmhip_dyn_design(&cd[i], curve) != COOLMIC_ERROR_NONE ||
            cmhip_dyn_set_curve(dyn[i], -1, curve) != COOLMIC_ERROR_NONE ||
            cmhip_dyn_delay(dyn[i]) != cmhip_dyn_delay(dyn[0])) {
            fprintf(stderr, "dynamics of band %u: %s\n", i, cmhip_last_error());
            return 1;
        }
    }
    /* the bands' bus: unity sends */
    bd.streams = BANDS; bd.max_sends = BANDS;
    back = cmhip_bus_new(&bd);
    for (i = 0; i < BANDS; i++) {
        to_bus[i] = 0;
        from[i] = i;
        W[i] = 16384;
    }
    if (!back || cmhip_bus_set_routing(back, BANDS, to_bus, from, W) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "bands' bus: %s\n", cmhip_last_error());
        return 1;
    }
    ld.device = 0; ld.streams = 1; ld.channels = 1; ld.lookahead_log2 = LOOKAHEAD_LOG2; ld.hold = 0;
    ld.max_frames = FRAMES; ld.hip_stream = cmhip_batch_hip_stream(b);
    lim = cmhip_lim_new(&ld);
    if (!lim || cmhip_lim_set(lim, -1, THRESHOLD, DRIVE) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "limiter: %s\n", cmhip_last_error());
        return 1;
    }
    printf("%d microphones -> bus -> split: %d bands at %.0f and %.0f Hz, %d taps, delay %u -> dynamics per band: delay %u "
           "-> bus -> limiter: delay %u, threshold %d; %d frames\n", (int)MICS, (int)BANDS, crossover_hz[0], crossover_hz[1],
           (int)TAPS, cmhip_split_delay(split), cmhip_dyn_delay(dyn[0]), cmhip_lim_delay(lim), (int)THRESHOLD, (int)FRAMES);
    if (cmhip_batch_sync(src) != COOLMIC_ERROR_NONE ||
        cmhip_bus_run(bus, cmhip_batch_dev_in(src), cmhip_batch_stride(src), FRAMES, NULL, cmhip_batch_dev_in(sum),
                      cmhip_batch_stride(sum), counts) != COOLMIC_ERROR_NONE ||
        cmhip_split_run(split, cmhip_batch_dev_in(sum), cmhip_batch_stride(sum), counts[0], counts,
                        cmhip_batch_dev_in(bands), cmhip_batch_stride(bands)) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "bus / split run: %s\n", cmhip_last_error());
        return 1;
    }
    for (i = 0; i < BANDS; i++) {
        /* band i of the one stream is slot i of the band-major array */
        const int16_t *in = (const int16_t *)cmhip_batch_dev_in(bands) + (size_t)i * cmhip_batch_stride(bands);
        int16_t *out = (int16_t *)cmhip_batch_dev_in(comp) + (size_t)i * cmhip_batch_stride(comp);
        band_counts[i] = counts[0];
        if (cmhip_dyn_run(dyn[i], in, cmhip_batch_stride(bands), counts[0], counts, out, cmhip_batch_stride(comp)) !=
            COOLMIC_ERROR_NONE) {
            fprintf(stderr, "dynamics run of band %u: %s\n", i, cmhip_last_error());
            return 1;
        }
    }
    if (cmhip_bus_run(back, cmhip_batch_dev_in(comp), cmhip_batch_stride(comp), counts[0], band_counts,
                      cmhip_batch_dev_in(mix), cmhip_batch_stride(mix), counts) != COOLMIC_ERROR_NONE ||
        cmhip_lim_run(lim, cmhip_batch_dev_in(mix), cmhip_batch_stride(mix), counts[0], counts, cmhip_batch_dev_in(b),
                      cmhip_batch_stride(b)) != COOLMIC_ERROR_NONE ||
        cmhip_batch_run(b, counts[0], counts) != COOLMIC_ERROR_NONE ||
        cmhip_batch_vu_result(b, 0, &vu) != COOLMIC_ERROR_NONE ||
        cmhip_split_clips(split, clips, 0) != COOLMIC_ERROR_NONE ||
        cmhip_lim_min_gain(lim, lim_gain, 0) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "bus / limiter / batch run: %s\n", cmhip_last_error());
        return 1;
    }
    for (i = 0; i < BANDS; i++) {
        if (cmhip_dyn_min_gain(dyn[i], dyn_gain[i], 0) != COOLMIC_ERROR_NONE) {
            fprintf(stderr, "dynamics of band %u: %s\n", i, cmhip_last_error());
            return 1;
        }
        printf("band %u: threshold=%.0f dBFS ratio=%.0f:1 detector=%u frames min_gain=%u clips=%u\n", i,
               cd[i].comp_threshold_db, cd[i].comp_ratio, 1u << detector_log2[i], (unsigned)dyn_gain[i][0],
               (unsigned)clips[i]);
    }
    printf("programme: frames=%zu rate=%u channels=%u peak=%d power=%.4f lim_min_gain=%u\n", vu.frames, (unsigned)vu.rate,
           vu.channels, (int)vu.global_peak, vu.global_power, (unsigned)lim_gain[0]);
    cmhip_lim_free(lim);
    cmhip_bus_free(back);
    for (i = 0; i < BANDS; i++)
        cmhip_dyn_free(dyn[i]);
    cmhip_split_free(split);
    cmhip_bus_free(bus);
    cmhip_batch_free(b);
    cmhip_batch_free(mix);
    cmhip_batch_free(comp);
    cmhip_batch_free(bands);
    cmhip_batch_free(sum);
    cmhip_batch_free(src);
    return 0;
}
