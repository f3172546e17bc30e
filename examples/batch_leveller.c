/*
 * batch_leveller.c -- two microphones nobody rides by hand, from plain C (include/coolmic_hip.h, "leveller" and "peak
 * limiter"): one talker at -40 dBFS and one at -6 dBFS (RMS re full scale; tones of five cycles per window, so a
 * window's level is steady) are levelled towards -20 dBFS by a leveller whose parameters cmhip_agc_design makes from a
 * law in dB -- at most +-24 dB, up 6 dB/s, down 20 dB/s, a gate at -60 dBFS -- then a limiter holds -1 dBFS, straight
 * into the slots of a batch with VU on.  Four seconds in, the quiet talker coughs: twenty milliseconds ten times as
 * loud, which the gain of +20 dB drives into the leveller's clamp and the limiter brings under its ceiling.
 * Five seconds run in ten blocks on the batch's stream, with no synchronisation between the stages.
 *
 * The program prints the two gains before and after with the gain (T << 12) / L each level asks for, whether each
 * gain lies within one rise / fall step of it, and the meters:
 *   "mic 0: gain 4096 -> 41047 (wanted 41047 at level 327), within a step: yes, clips ..."
 *   "programme 0: frames=240000 peak=... lim_min_gain=..."
 *
 *   cc -I include examples/batch_leveller.c -L libcoolmic-dsp_amd/lib -lcoolmic-dsp-hip -lm \
 *      -Wl,-rpath,$PWD/libcoolmic-dsp_amd/lib -o batch_leveller && ./batch_leveller
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <coolmic-dsp/coolmic-dsp.h>
#include <coolmic_hip.h>

enum { MICS = 2, RATE = 48000, BLOCK = 24000, BLOCKS = 10, WINDOW_LOG2 = 10, COUGH_AT = 4 * RATE, COUGH_FRAMES = 960,
       LOOKAHEAD_LOG2 = 6, THRESHOLD = 29204, DRIVE = 4096 };

int main(void)
{
    static int16_t pcm[MICS][BLOCK];
    static const double level_db[MICS] = {-40.0, -6.0};
    static const cmhip_agc_law_desc_t law = {RATE, WINDOW_LOG2, -20.0, -60.0, 24.0, -24.0, 0.0, 6.0, 20.0};
    cmhip_batch_desc_t sd = {0};
    cmhip_agc_desc_t ad = {0};
    cmhip_lim_desc_t ld = {0};
    cmhip_agc_params_t par;
    cmhip_batch_t *src, *mid, *b;
    cmhip_agc_t *agc;
    cmhip_lim_t *lim;
    coolmic_vumeter_result_t vu;
    uint32_t counts[MICS] = {BLOCK, BLOCK}, before[MICS], gain[MICS], level[MICS], lim_gain[MICS];
    uint64_t clips[MICS];
    unsigned n, s, k, bad = 0;

    sd.device = 0; sd.streams = MICS; sd.channels = 1; sd.rate = RATE; sd.max_frames = BLOCK; sd.flags = CMHIP_VU;
    src = cmhip_batch_new(&sd);                      /* (batches used as device memory) */
    mid = cmhip_batch_new(&sd);
    b = cmhip_batch_new(&sd);
    if (!src || !mid || !b) {
        fprintf(stderr, "batch: %s\n", cmhip_last_error());
        return 1;
    }
    ad.device = 0; ad.streams = MICS; ad.channels = 1; ad.window_log2 = WINDOW_LOG2; ad.max_frames = BLOCK;
    ad.hip_stream = cmhip_batch_hip_stream(b);
    agc = cmhip_agc_new(&ad);
    if (!agc || cmhip_agc_design(&law, &par) != COOLMIC_ERROR_NONE || cmhip_agc_set(agc, -1, &par) != COOLMIC_ERROR_NONE ||
        cmhip_agc_state(agc, before, NULL, NULL, 0) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "leveller: %s\n", cmhip_last_error());
        return 1;
    }
    ld.device = 0; ld.streams = MICS; ld.channels = 1; ld.lookahead_log2 = LOOKAHEAD_LOG2; ld.hold = 0;
    ld.max_frames = BLOCK; ld.hip_stream = cmhip_batch_hip_stream(b);
    lim = cmhip_lim_new(&ld);
    if (!lim || cmhip_lim_set(lim, -1, THRESHOLD, DRIVE) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "limiter: %s\n", cmhip_last_error());
        return 1;
    }
    printf("%d microphones -> leveller: window %d frames, target %u, gate %u, gain %u..%u, rise %u, fall %u -> limiter: "
           "threshold %d\n", (int)MICS, 1 << WINDOW_LOG2, (unsigned)par.target, (unsigned)par.gate, (unsigned)par.gain_min,
           (unsigned)par.gain_max, (unsigned)par.rise, (unsigned)par.fall, (int)THRESHOLD);
    for (k = 0; k < BLOCKS; k++) {
        for (s = 0; s < MICS; s++) {
            const double amp = 32768.0 * pow(10.0, level_db[s] / 20.0) * sqrt(2.0);
            for (n = 0; n < BLOCK; n++) {
                const unsigned at = k * BLOCK + n;
                const double cough = s == 0 && at >= COUGH_AT && at < COUGH_AT + COUGH_FRAMES ? 10.0 : 1.0;
                pcm[s][n] = (int16_t)lrint(cough * amp * sin(2.0 * M_PI * 5.0 * at / (double)(1 << WINDOW_LOG2)));
            }
            if (cmhip_batch_upload(src, s, pcm[s], BLOCK) != COOLMIC_ERROR_NONE) {
                fprintf(stderr, "upload: %s\n", cmhip_last_error());
                return 1;
            }
        }
        if (cmhip_batch_sync(src) != COOLMIC_ERROR_NONE ||
            cmhip_agc_run(agc, cmhip_batch_dev_in(src), cmhip_batch_stride(src), BLOCK, counts, cmhip_batch_dev_in(mid),
                          cmhip_batch_stride(mid)) != COOLMIC_ERROR_NONE ||
            cmhip_lim_run(lim, cmhip_batch_dev_in(mid), cmhip_batch_stride(mid), BLOCK, counts, cmhip_batch_dev_in(b),
                          cmhip_batch_stride(b)) != COOLMIC_ERROR_NONE ||
            cmhip_batch_run(b, BLOCK, counts) != COOLMIC_ERROR_NONE || cmhip_batch_sync(b) != COOLMIC_ERROR_NONE) {
            fprintf(stderr, "run: %s\n", cmhip_last_error());
            return 1;
        }
    }
    if (cmhip_agc_state(agc, gain, level, clips, 0) != COOLMIC_ERROR_NONE ||
        cmhip_lim_min_gain(lim, lim_gain, 0) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "state: %s\n", cmhip_last_error());
        return 1;
    }
    for (s = 0; s < MICS; s++) {
        /* the gain the last level asks for, and one step of the gain in force towards it */
        uint32_t wanted = level[s] ? ((uint32_t)par.target << 12) / level[s] : gain[s];
        uint32_t rate, step, apart;
        wanted = wanted < par.gain_min ? par.gain_min : wanted > par.gain_max ? par.gain_max : wanted;
        rate = wanted > gain[s] ? par.rise : par.fall;
        step = (gain[s] * rate) >> 16;
        step = step ? step : 1;
        apart = wanted > gain[s] ? wanted - gain[s] : gain[s] - wanted;
        bad += apart > step;
        printf("mic %u: gain %u -> %u (wanted %u at level %u), within a step: %s, clips %llu\n", s, (unsigned)before[s],
               (unsigned)gain[s], (unsigned)wanted, (unsigned)level[s], apart > step ? "NO" : "yes",
               (unsigned long long)clips[s]);
    }
    for (s = 0; s < MICS; s++) {
        if (cmhip_batch_vu_result(b, s, &vu) != COOLMIC_ERROR_NONE) {
            fprintf(stderr, "vu: %s\n", cmhip_last_error());
            return 1;
        }
        printf("programme %u: frames=%zu rate=%u channels=%u peak=%d power=%.4f lim_min_gain=%u\n", s, vu.frames,
               (unsigned)vu.rate, vu.channels, (int)vu.global_peak, vu.global_power, (unsigned)lim_gain[s]);
    }
    cmhip_lim_free(lim);
    cmhip_agc_free(agc);
    cmhip_batch_free(b);
    cmhip_batch_free(mid);
    cmhip_batch_free(src);
    return bad ? 1 : 0;
}
