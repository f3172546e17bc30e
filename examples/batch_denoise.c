/*
 * batch_denoise.c -- a quiet talker in a noisy room, from plain C (include/coolmic_hip.h, "noise suppressor", "leveller"
 * and "peak limiter"): a 1 kHz tone at -32 dBFS over steady noise at -56 dBFS (RMS re full scale) goes through
 * noise suppressor -> leveller -> limiter straight into the slots of a batch with VU on.  The leveller brings the talker
 * to -20 dBFS, 12 dB up -- and with the talker the noise, which is what a leveller does to a quiet speaker's room.  Microphone 0
 * has the suppressor at work (18 dB of reduction, 6 dB of over-subtraction, designed by cmhip_denoise_design; the profile
 * learned during the first half second, before anybody speaks), microphone 1 has it at its defaults, a pure delay.
 * Four seconds run in eight blocks on the batch's stream, with no synchronisation between the stages; the last half
 * second is a pause between words, the leveller's gate holds the gain, and the programme there is the noise floor.
 *
 * The program prints the noise floor at the microphone and in the two programmes, the reduction, and whether the
 * leveller still lifts the noise above what the microphone heard:
 *   "noise floor: microphone -56.0 dBFS, programme without suppression <about 12 dB above> dBFS, with <below the microphone's> dBFS"
 *   "reduction <about 16> dB, leveller gains <about 16300, +12 dB> and ..., learned blocks 92, clips 0, sat 0, noise lifted: no"
 *
 *   cc -I include examples/batch_denoise.c -L libcoolmic-dsp_amd/lib -lcoolmic-dsp-hip -lm \
 *      -Wl,-rpath,$PWD/libcoolmic-dsp_amd/lib -o batch_denoise && ./batch_denoise
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <coolmic-dsp/coolmic-dsp.h>
#include <coolmic_hip.h>

enum { MICS = 2, RATE = 48000, BLOCK = 24000, BLOCKS = 8, FFT_LOG2 = 9, WINDOW_LOG2 = 10, LOOKAHEAD_LOG2 = 6,
       THRESHOLD = 29204, DRIVE = 4096, MEASURE = 12000 };

/* steady noise: the sum of twelve uniform numbers, about Gaussian, from a linear congruential generator */
static uint32_t lcg = 12345;
static double noise(void)
{
    double v = -6.0;
    int i;
    for (i = 0; i < 12; i++) {
        lcg = lcg * 1664525u + 1013904223u;
        v += (double)(lcg >> 8) / 16777216.0;
    }
    return v;
}

static double dbfs(const int16_t *x, unsigned n)
{
    double e = 0.0;
    unsigned i;
    for (i = 0; i < n; i++)
        e += (double)x[i] * x[i];
    return 10.0 * log10(e / n / (32768.0 * 32768.0) + 1e-30);
}

int main(void)
{
    static int16_t pcm[BLOCK], prog[MICS][BLOCK];
    static const cmhip_denoise_law_desc_t dlaw = {RATE, FFT_LOG2, 18.0, 6.0206, 10.7, 21.4};
    static const cmhip_agc_law_desc_t alaw = {RATE, WINDOW_LOG2, -20.0, -46.0, 24.0, -24.0, 0.0, 12.0, 20.0};
    cmhip_batch_desc_t sd = {0};
    cmhip_denoise_desc_t nd = {0};
    cmhip_agc_desc_t ad = {0};
    cmhip_lim_desc_t ld = {0};
    cmhip_denoise_params_t npar;
    cmhip_agc_params_t apar;
    cmhip_batch_t *src, *clean, *mid, *b;
    cmhip_denoise_t *dn;
    cmhip_agc_t *agc;
    cmhip_lim_t *lim;
    uint32_t counts[MICS] = {BLOCK, BLOCK}, gain[MICS], learned[MICS];
    uint64_t clips[MICS], sat[MICS];
    const double tone = 32768.0 * pow(10.0, -32.0 / 20.0) * sqrt(2.0), sigma = 32768.0 * pow(10.0, -56.0 / 20.0);
    double mic_db = 0.0, prog_db[MICS], reduction;
    unsigned n, s, k;
    int lifted;

    sd.device = 0; sd.streams = MICS; sd.channels = 1; sd.rate = RATE; sd.max_frames = BLOCK; sd.flags = CMHIP_VU;
    src = cmhip_batch_new(&sd);                      /* (batches used as device memory) */
    clean = cmhip_batch_new(&sd);
    mid = cmhip_batch_new(&sd);
    b = cmhip_batch_new(&sd);
    if (!src || !clean || !mid || !b) {
        fprintf(stderr, "batch: %s\n", cmhip_last_error());
        return 1;
    }
    nd.device = 0; nd.streams = MICS; nd.channels = 1; nd.fft_log2 = FFT_LOG2; nd.max_frames = BLOCK;
    nd.hip_stream = cmhip_batch_hip_stream(b);
    dn = cmhip_denoise_new(&nd);
    if (!dn || cmhip_denoise_design(&dlaw, &npar) != COOLMIC_ERROR_NONE || cmhip_denoise_set(dn, 0, &npar) != COOLMIC_ERROR_NONE ||
        cmhip_denoise_learn(dn, 0, 1) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "noise suppressor: %s\n", cmhip_last_error());
        return 1;
    }
    ad.device = 0; ad.streams = MICS; ad.channels = 1; ad.window_log2 = WINDOW_LOG2; ad.max_frames = BLOCK;
    ad.hip_stream = cmhip_batch_hip_stream(b);
    agc = cmhip_agc_new(&ad);
    if (!agc || cmhip_agc_design(&alaw, &apar) != COOLMIC_ERROR_NONE || cmhip_agc_set(agc, -1, &apar) != COOLMIC_ERROR_NONE) {
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
    printf("%d microphones -> noise suppressor: blocks of %d frames, delay %zu, floor %u, over %u, shifts %u and %u -> "
           "leveller: target %u, gate %u -> limiter: threshold %d\n", (int)MICS, 1 << FFT_LOG2, cmhip_denoise_delay(dn),
           (unsigned)npar.floor, (unsigned)npar.over, (unsigned)npar.rise_shift, (unsigned)npar.fall_shift,
           (unsigned)apar.target, (unsigned)apar.gate, (int)THRESHOLD);
    for (k = 0; k < BLOCKS; k++) {
        const int speaks = k >= 1 && k + 1 < BLOCKS;     /* nobody in the first half second, a pause in the last */
        for (n = 0; n < BLOCK; n++)
            pcm[n] = (int16_t)lrint(sigma * noise() + (speaks ? tone * sin(2.0 * M_PI * 1000.0 * (k * BLOCK + n) / RATE) : 0.0));
        if (k + 1 == BLOCKS)
            mic_db = dbfs(pcm + BLOCK - MEASURE, MEASURE);
        for (s = 0; s < MICS; s++)                       /* both microphones hear the same room */
            if (cmhip_batch_upload(src, s, pcm, BLOCK) != COOLMIC_ERROR_NONE) {
                fprintf(stderr, "upload: %s\n", cmhip_last_error());
                return 1;
            }
        if (k == 1 && cmhip_denoise_learn(dn, 0, 0) != COOLMIC_ERROR_NONE) {      /* the profile stands: somebody speaks */
            fprintf(stderr, "learn: %s\n", cmhip_last_error());
            return 1;
        }
        if (cmhip_batch_sync(src) != COOLMIC_ERROR_NONE ||
            cmhip_denoise_run(dn, cmhip_batch_dev_in(src), cmhip_batch_stride(src), BLOCK, counts, cmhip_batch_dev_in(clean),
                              cmhip_batch_stride(clean)) != COOLMIC_ERROR_NONE ||
            cmhip_agc_run(agc, cmhip_batch_dev_in(clean), cmhip_batch_stride(clean), BLOCK, counts, cmhip_batch_dev_in(mid),
                          cmhip_batch_stride(mid)) != COOLMIC_ERROR_NONE ||
            cmhip_lim_run(lim, cmhip_batch_dev_in(mid), cmhip_batch_stride(mid), BLOCK, counts, cmhip_batch_dev_in(b),
                          cmhip_batch_stride(b)) != COOLMIC_ERROR_NONE ||
            cmhip_batch_run(b, BLOCK, counts) != COOLMIC_ERROR_NONE || cmhip_batch_sync(b) != COOLMIC_ERROR_NONE) {
            fprintf(stderr, "run: %s\n", cmhip_last_error());
            return 1;
        }
    }
    /* the programme of the last block: its second half lies well inside the pause, the stages' delays included */
    for (s = 0; s < MICS; s++) {
        if (cmhip_batch_download_input(b, s, prog[s], BLOCK) != COOLMIC_ERROR_NONE) {
            fprintf(stderr, "download: %s\n", cmhip_last_error());
            return 1;
        }
        prog_db[s] = dbfs(prog[s] + BLOCK - MEASURE, MEASURE);
    }
    if (cmhip_agc_state(agc, gain, NULL, NULL, 0) != COOLMIC_ERROR_NONE ||
        cmhip_denoise_state(dn, clips, sat, learned, 0) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "state: %s\n", cmhip_last_error());
        return 1;
    }
    reduction = prog_db[1] - prog_db[0];
    lifted = prog_db[0] > mic_db;
    printf("noise floor: microphone %.1f dBFS, programme without suppression %.1f dBFS, with %.1f dBFS\n", mic_db, prog_db[1],
           prog_db[0]);
    printf("reduction %.2f dB, leveller gains %u and %u, learned blocks %u, clips %llu, sat %llu, noise lifted: %s\n", reduction,
           (unsigned)gain[0], (unsigned)gain[1], (unsigned)learned[0], (unsigned long long)clips[0],
           (unsigned long long)sat[0], lifted ? "YES" : "no");
    cmhip_lim_free(lim);
    cmhip_agc_free(agc);
    cmhip_denoise_free(dn);
    cmhip_batch_free(b);
    cmhip_batch_free(mid);
    cmhip_batch_free(clean);
    cmhip_batch_free(src);
    return lifted || prog_db[1] < mic_db + 8.0 ? 1 : 0;
}
