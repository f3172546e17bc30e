/*
 * batch_ducking.c -- a music bed that falls when the presenter speaks, from plain C (include/coolmic_hip.h, "mix bus",
 * "dynamics" with its side-chain keys, and "peak limiter").  Four stereo sources: two of music (tones, all the time) and
 * two voices (a 500 Hz tone from frame 8000 to frame 24000).  A first bus makes two stereo sums, music (slot 0) and
 * voice (slot 1).  The dynamics stage takes both: the music is keyed on the voice (cmhip_dyn_set_key(dyn, 0, 1)) with a
 * duck curve from cmhip_dyn_design_duck (12 dB down once the voice passes -36 dBFS, a knee of 8 dB), the voice keeps a
 * compressor of its own (-18 dBFS, 3:1).  A second bus adds the two, the limiter holds the sum under -1 dBFS, and a
 * stereo batch meters the programme.  The stages run on the batch's stream in two blocks, frames 0..31999 (with the
 * speech) and 32000..47999 (after it), with no synchronisation between the stages.  Prints one line of geometry,
 * "speech: music_min_gain=... duck_floor=..." and "after: music_min_gain=..." (the music stream's gain meter, re-armed
 * between the blocks; Q15, 32768 is unity), and "programme: frames=48000 rate=48000 channels=2 peak=... power=...".
 *
 *   cc -I include examples/batch_ducking.c -L libcoolmic-dsp_amd/lib -lcoolmic-dsp-hip -lm \
 *      -Wl,-rpath,$PWD/libcoolmic-dsp_amd/lib -o batch_ducking && ./batch_ducking
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <coolmic-dsp/coolmic-dsp.h>
#include <coolmic_hip.h>

enum { SOURCES = 4, CH = 2, FRAMES = 48000, BLOCK0 = 32000, SPEECH_FROM = 8000, SPEECH_TO = 24000, DETECTOR_LOG2 = 7,
       SMOOTH_LOG2 = 6, HOLD = 960, LOOKAHEAD_LOG2 = 6, THRESHOLD = 29204, DRIVE = 4096, MUSIC = 0, VOICE = 1 };

int main(void)
{
    static int16_t pcm[SOURCES][FRAMES * CH];
    cmhip_batch_desc_t sd = {0}, md = {0};
    cmhip_bus_desc_t bd = {0};
    cmhip_dyn_desc_t dd = {0};
    cmhip_lim_desc_t ld = {0};
    const cmhip_dyn_duck_desc_t duck = {-36.0, 12.0, 8.0};
    const cmhip_dyn_curve_desc_t comp = {-18.0, 3.0, 6.0, -96.0, 1.0, 0.0};
    uint16_t curve[CMHIP_DYN_CURVE];
    cmhip_batch_t *src, *sums, *ducked, *mix, *b;
    cmhip_bus_t *bus, *add;
    cmhip_dyn_t *dyn;
    cmhip_lim_t *lim;
    coolmic_vumeter_result_t vu;
    uint32_t to_bus[SOURCES], from[SOURCES], counts[2], total[1], gain[2], floor_q15;
    int16_t W[SOURCES * CH * CH];
    long key = 0;
    unsigned i, n, block;

    /* the sources: a batch used as device memory */
    sd.device = 0; sd.streams = SOURCES; sd.channels = CH; sd.rate = 48000; sd.max_frames = FRAMES; sd.flags = CMHIP_VU;
    src = cmhip_batch_new(&sd);
    if (!src) {
        fprintf(stderr, "sources: %s\n", cmhip_last_error());
        return 1;
    }
    for (i = 0; i < SOURCES; i++) {
        for (n = 0; n < FRAMES; n++) {
            double v;
            if (i < 2)                                /* music: 220 Hz and 330 Hz */
                v = 9000.0 * sin(2.0 * M_PI * n * (220.0 + 110.0 * i) / 48000.0);
            else                                      /* voices */
                v = n >= SPEECH_FROM && n < SPEECH_TO ? 12000.0 * sin(2.0 * M_PI * (n + 8 * i) / 96.0) : 0.0;
            pcm[i][CH * n] = (int16_t)lrint(v);
            pcm[i][CH * n + 1] = (int16_t)lrint(0.8 * v);
        }
    }
    /* two slots each for the sums and the dynamics stage's output, one for their sum, and the batch that meters */
    md = sd;
    md.streams = 2;
    sums = cmhip_batch_new(&md);
    ducked = cmhip_batch_new(&md);
    md.streams = 1;
    mix = cmhip_batch_new(&md);
    b = cmhip_batch_new(&md);
    if (!sums || !ducked || !mix || !b) {
        fprintf(stderr, "batch: %s\n", cmhip_last_error());
        return 1;
    }
    /* the first bus: sources 0, 1 -> music, 2, 3 -> voice, left to left and right to right at half weight */
    bd.device = 0; bd.streams = SOURCES; bd.buses = 2; bd.channels_in = CH; bd.channels_out = CH;
    bd.max_frames = FRAMES; bd.max_sends = SOURCES; bd.hip_stream = cmhip_batch_hip_stream(b);
    bus = cmhip_bus_new(&bd);
    for (i = 0; i < SOURCES; i++) {
        to_bus[i] = i < 2 ? MUSIC : VOICE;
        from[i] = i;
        W[4 * i] = W[4 * i + 3] = 8192;
        W[4 * i + 1] = W[4 * i + 2] = 0;
    }
    if (!bus || cmhip_bus_set_routing(bus, SOURCES, to_bus, from, W) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "bus: %s\n", cmhip_last_error());
        return 1;
    }
    /* the dynamics stage: the music ducks under the voice, the voice is compressed on its own level */
    dd.device = 0; dd.streams = 2; dd.channels = CH; dd.detector_log2 = DETECTOR_LOG2; dd.smooth_log2 = SMOOTH_LOG2;
    dd.hold = HOLD; dd.max_frames = FRAMES; dd.hip_stream = cmhip_batch_hip_stream(b);
    dyn = cmhip_dyn_new(&dd);
    if (!dyn || cmhip_dyn_design_duck(&duck, curve) != COOLMIC_ERROR_NONE ||
        cmhip_dyn_set_curve(dyn, MUSIC, curve) != COOLMIC_ERROR_NONE ||
        cmhip_dyn_set_key(dyn, MUSIC, VOICE) != COOLMIC_ERROR_NONE ||
        cmhip_dyn_get_key(dyn, MUSIC, &key) != COOLMIC_ERROR_NONE || key != VOICE) {
        fprintf(stderr, "dynamics: %s\n", cmhip_last_error());
        return 1;
    }
    floor_q15 = curve[121];                          /* the gain at full scale: all the way down */
    if (cmhip_dyn_design(&comp, curve) != COOLMIC_ERROR_NONE ||
        cmhip_dyn_set_curve(dyn, VOICE, curve) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "dynamics: %s\n", cmhip_last_error());
        return 1;
    }
    /* the second bus adds the two at unity, the limiter follows */
    bd.streams = 2; bd.buses = 1; bd.max_sends = 2;
    add = cmhip_bus_new(&bd);
    for (i = 0; i < 2; i++) {
        to_bus[i] = 0;
        from[i] = i;
        W[4 * i] = W[4 * i + 3] = 16384;
    }
    if (!add || cmhip_bus_set_routing(add, 2, to_bus, from, W) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "second bus: %s\n", cmhip_last_error());
        return 1;
    }
    ld.device = 0; ld.streams = 1; ld.channels = CH; ld.lookahead_log2 = LOOKAHEAD_LOG2; ld.hold = 0;
    ld.max_frames = FRAMES; ld.hip_stream = cmhip_batch_hip_stream(b);
    lim = cmhip_lim_new(&ld);
    if (!lim || cmhip_lim_set(lim, -1, THRESHOLD, DRIVE) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "limiter: %s\n", cmhip_last_error());
        return 1;
    }
    printf("music + voice -> bus -> dynamics (music keyed on voice): delay %u, detector %d frames, hold %d; duck %.0f dB "
           "above %.0f dBFS, knee %.0f dB; voice compressor %.0f dBFS %.0f:1 -> bus -> limiter: delay %u, threshold %d; "
           "%d frames in blocks of %d and %d\n", cmhip_dyn_delay(dyn), 1 << DETECTOR_LOG2, (int)HOLD, duck.depth_db,
           duck.threshold_db, duck.knee_db, comp.comp_threshold_db, comp.comp_ratio, cmhip_lim_delay(lim), (int)THRESHOLD,
           (int)FRAMES, (int)BLOCK0, (int)(FRAMES - BLOCK0));
    for (block = 0; block < 2; block++) {
        const size_t first = block ? BLOCK0 : 0, frames = block ? FRAMES - BLOCK0 : BLOCK0;
        /* the block into the sources' slots (the meter read below waited for the stream: the last block is through) */
        for (i = 0; i < SOURCES; i++)
            if (cmhip_batch_upload(src, i, pcm[i] + first * CH, frames) != COOLMIC_ERROR_NONE) {
                fprintf(stderr, "upload: %s\n", cmhip_last_error());
                return 1;
            }
        if (cmhip_batch_sync(src) != COOLMIC_ERROR_NONE ||
            cmhip_bus_run(bus, cmhip_batch_dev_in(src), cmhip_batch_stride(src), frames, NULL, cmhip_batch_dev_in(sums),
                          cmhip_batch_stride(sums), counts) != COOLMIC_ERROR_NONE ||
            /* (music and voice get the same count: a keyed stream and its key advance together) */
            cmhip_dyn_run(dyn, cmhip_batch_dev_in(sums), cmhip_batch_stride(sums), frames, counts,
                          cmhip_batch_dev_in(ducked), cmhip_batch_stride(ducked)) != COOLMIC_ERROR_NONE ||
            cmhip_bus_run(add, cmhip_batch_dev_in(ducked), cmhip_batch_stride(ducked), frames, counts,
                          cmhip_batch_dev_in(mix), cmhip_batch_stride(mix), total) != COOLMIC_ERROR_NONE ||
            cmhip_lim_run(lim, cmhip_batch_dev_in(mix), cmhip_batch_stride(mix), total[0], total, cmhip_batch_dev_in(b),
                          cmhip_batch_stride(b)) != COOLMIC_ERROR_NONE ||
            cmhip_batch_run(b, total[0], total) != COOLMIC_ERROR_NONE ||
            cmhip_dyn_min_gain(dyn, gain, 1) != COOLMIC_ERROR_NONE) {
            fprintf(stderr, "block %u: %s\n", block, cmhip_last_error());
            return 1;
        }
        if (block == 0)
            printf("speech: music_min_gain=%u duck_floor=%u voice_min_gain=%u\n", (unsigned)gain[MUSIC], (unsigned)floor_q15,
                   (unsigned)gain[VOICE]);
        else
            printf("after: music_min_gain=%u voice_min_gain=%u\n", (unsigned)gain[MUSIC], (unsigned)gain[VOICE]);
    }
    if (cmhip_batch_vu_result(b, 0, &vu) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "vu: %s\n", cmhip_last_error());
        return 1;
    }
    printf("programme: frames=%zu rate=%u channels=%u peak=%d power=%.4f\n", vu.frames, (unsigned)vu.rate, vu.channels,
           (int)vu.global_peak, vu.global_power);
    cmhip_lim_free(lim);
    cmhip_bus_free(add);
    cmhip_dyn_free(dyn);
    cmhip_bus_free(bus);
    cmhip_batch_free(b);
    cmhip_batch_free(mix);
    cmhip_batch_free(ducked);
    cmhip_batch_free(sums);
    cmhip_batch_free(src);
    return 0;
}
