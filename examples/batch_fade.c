/*
 * batch_fade.c -- click-free matrix ramps (include/coolmic_hip.h, "matrix ramps") from plain C: a stereo programme, the
 * device-side sine, goes block by block through a mixer into the slots of a stereo batch with VU on.  The mixer starts
 * on the zero matrix and fades in to unity over 480 frames, plays, crossfades to the channel-swapped matrix over 4800
 * frames, plays, and fades out to zero over 480 frames.  Nothing waits between the ramp calls and the runs: the order
 * is the batch's stream's.  Prints one VU window per block of 96 frames:
 * "block N: phase=fade-in frames=96 power=... done=... of=..." (power in dB; done / of: the ramp's position after
 * the block, 0 0 when none runs).
 *
 *   cc -I include examples/batch_fade.c -L libcoolmic-dsp_amd/lib -lcoolmic-dsp-hip \
 *      -Wl,-rpath,$PWD/libcoolmic-dsp_amd/lib -o batch_fade && ./batch_fade
 */
#include <stdio.h>
#include <stdlib.h>
#include <coolmic-dsp/coolmic-dsp.h>
#include <coolmic_hip.h>

enum { BLOCK = 96, FADE = 480, CROSS = 4800, HOLD = 3 };       /* a block is two periods of the sine */

static const int16_t W_ZERO[4] = {0, 0, 0, 0}, W_UNITY[4] = {16384, 0, 0, 16384}, W_SWAP[4] = {0, 16384, 16384, 0};

int main(void)
{
    static const struct {
        const char *name;
        const int16_t *target;       /* NULL: no call, the matrix stays */
        unsigned ramp, blocks;
    } phases[] = {
        {"fade-in", W_UNITY, FADE, FADE / BLOCK}, {"steady", NULL, 0, HOLD}, {"crossfade", W_SWAP, CROSS, CROSS / BLOCK},
        {"swapped", NULL, 0, HOLD}, {"fade-out", W_ZERO, FADE, FADE / BLOCK},
    };
    cmhip_batch_desc_t sd = {0}, bd = {0};
    cmhip_mix_desc_t md = {0};
    cmhip_batch_t *src, *b;
    cmhip_mix_t *m;
    coolmic_vumeter_result_t vu;
    uint32_t done, of;
    unsigned ph, i, block = 0;

    /* the source: a batch used as device memory, filled with the engine's sine block by block */
    sd.device = 0; sd.streams = 1; sd.channels = 2; sd.rate = 48000; sd.max_frames = BLOCK; sd.flags = CMHIP_VU;
    bd = sd;
    src = cmhip_batch_new(&sd);
    b = cmhip_batch_new(&bd);
    if (!src || !b) {
        fprintf(stderr, "batches: %s\n", cmhip_last_error());
        return 1;
    }
    md.device = 0; md.streams = 1; md.channels_in = 2; md.channels_out = 2; md.max_frames = BLOCK;
    md.hip_stream = cmhip_batch_hip_stream(b);
    m = cmhip_mix_new(&md);
    if (!m || cmhip_mix_set_matrix(m, -1, W_ZERO) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "mixer: %s\n", cmhip_last_error());
        return 1;
    }
    for (ph = 0; ph < sizeof(phases) / sizeof(phases[0]); ph++) {
        if (phases[ph].target &&
            cmhip_mix_ramp_matrix(m, -1, phases[ph].target, phases[ph].ramp) != COOLMIC_ERROR_NONE) {
            fprintf(stderr, "mix_ramp_matrix: %s\n", cmhip_last_error());
            return 1;
        }
        for (i = 0; i < phases[ph].blocks; i++, block++) {
            /* the source's own stream is waited for; the mixer and the batch share one and need no wait */
            if (cmhip_batch_generate(src, CMHIP_GEN_SINE, 0, BLOCK, 0, 1, (uint64_t)block * BLOCK) != COOLMIC_ERROR_NONE ||
                cmhip_batch_sync(src) != COOLMIC_ERROR_NONE ||
                cmhip_mix_run(m, cmhip_batch_dev_in(src), cmhip_batch_stride(src), BLOCK, NULL, cmhip_batch_dev_in(b),
                              cmhip_batch_stride(b)) != COOLMIC_ERROR_NONE ||
                cmhip_batch_run(b, BLOCK, NULL) != COOLMIC_ERROR_NONE ||
                cmhip_batch_vu_results(b, &vu, NULL) != COOLMIC_ERROR_NONE ||
                cmhip_mix_ramp_state(m, 0, &done, &of, NULL) != COOLMIC_ERROR_NONE) {
                fprintf(stderr, "block %u: %s\n", block, cmhip_last_error());
                return 1;
            }
            printf("block %u: phase=%s frames=%zu power=%.4f done=%u of=%u\n", block, phases[ph].name, vu.frames,
                   vu.global_power, (unsigned)done, (unsigned)of);
        }
    }
    cmhip_mix_free(m);
    cmhip_batch_free(b);
    cmhip_batch_free(src);
    return 0;
}
