/*
 * batch_failover.c -- a failover switch in front of a metered programme from plain C (include/coolmic_hip.h, "failover
 * switch" and "signal watch"): a mono programme of six seconds at 48 kHz -- a square wave of magnitude 6000 -- with two
 * seconds of digital silence in it, and a backup tone -- a square wave of magnitude 8000 -- go through a switch with
 * windows of 1024 frames, designed from a law: leave a source after half a second of silence, take it back after half a
 * second of signal, crossfade over 20 ms.  The switch writes into slot 1 of a batch with the signal watch on; slot 0 of
 * that batch gets the programme as it came in.  Switch and batch run on the batch's stream, with no synchronisation
 * between them, in blocks of 4800 frames.  It prints
 *   "input: longest dead air 96000 frames (2000.0 ms)"
 *   "output: longest dead air 23813 frames (496.1 ms)"     23 dead windows, up to the next window edge, 5 frames of fade
 *   "output went to the backup in block 24 and came back in block 44; switches 2"
 *
 *   cc -I include examples/batch_failover.c -L libcoolmic-dsp_amd/lib -lcoolmic-dsp-hip \
 *      -Wl,-rpath,$PWD/libcoolmic-dsp_amd/lib -o batch_failover && ./batch_failover
 */
#include <stdio.h>
#include <stdlib.h>
#include <coolmic-dsp/coolmic-dsp.h>
#include <coolmic_hip.h>

enum { RATE = 48000, BLOCK = 4800, BLOCKS = 60, WINDOW_LOG2 = 10, GAP_FROM = 2 * RATE, GAP_TO = 4 * RATE };

int main(void)
{
    static const uint32_t list[2] = {0, 1};          /* the programme, then the backup */
    cmhip_batch_desc_t sd = {0}, md = {0};
    cmhip_failover_desc_t fd = {0};
    cmhip_failover_law_desc_t law = {0};
    cmhip_failover_params_t par;
    cmhip_batch_t *src, *b;
    cmhip_failover_t *sw;
    coolmic_watch_result_t res[2];
    static int16_t programme[BLOCK], backup[BLOCK];
    uint32_t to = 0, was = 0;
    uint64_t switches = 0;
    int rc[2], went = -1, came = -1;
    unsigned i, n, block;

    /* the two sources: a batch used as device memory */
    sd.device = 0; sd.streams = 2; sd.channels = 1; sd.rate = RATE; sd.max_frames = BLOCK; sd.flags = CMHIP_VU;
    src = cmhip_batch_new(&sd);
    /* the batch that watches the programme as it came in (slot 0) and as it goes out (slot 1) */
    md = sd;
    b = cmhip_batch_new(&md);
    if (!src || !b || cmhip_batch_set_watch(b, 1) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "batch: %s\n", cmhip_last_error());
        return 1;
    }
    /* the switch, on the batch's stream: one output with the list programme, backup */
    fd.device = 0; fd.streams = 2; fd.outputs = 1; fd.channels = 1; fd.window_log2 = WINDOW_LOG2; fd.max_frames = BLOCK;
    fd.hip_stream = cmhip_batch_hip_stream(b);
    sw = cmhip_failover_new(&fd);
    law.rate = RATE; law.window_log2 = WINDOW_LOG2; law.fail_s = 0.5; law.return_s = 0.5; law.fade_ms = 20.0;
    for (i = 0; i < 4; i++)
        law.quiet_db[i] = -60.0;
    if (!sw || cmhip_failover_design(&law, &par) != COOLMIC_ERROR_NONE ||
        cmhip_failover_set_sources(sw, 0, 2, list) != COOLMIC_ERROR_NONE ||
        cmhip_failover_set(sw, 0, &par) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "switch: %s\n", cmhip_last_error());
        return 1;
    }
    printf("programme of %d frames, silent from %d to %d; switch: windows of %d frames, leave after %u, return after %u, "
           "fade %d frames\n", BLOCKS * BLOCK, (int)GAP_FROM, (int)GAP_TO, 1 << WINDOW_LOG2, (unsigned)par.fail_windows,
           (unsigned)par.return_windows, 1 << par.fade_log2);
    for (block = 0; block < BLOCKS; block++) {
        for (n = 0; n < BLOCK; n++) {
            const unsigned f = block * BLOCK + n;
            programme[n] = (int16_t)(f >= GAP_FROM && f < GAP_TO ? 0 : ((f / 50) % 2 ? -6000 : 6000));
            backup[n] = (int16_t)((f / 24) % 2 ? -8000 : 8000);
        }
        if (cmhip_batch_upload(src, 0, programme, BLOCK) != COOLMIC_ERROR_NONE ||
            cmhip_batch_upload(src, 1, backup, BLOCK) != COOLMIC_ERROR_NONE ||
            cmhip_batch_upload(b, 0, programme, BLOCK) != COOLMIC_ERROR_NONE ||
            cmhip_batch_sync(src) != COOLMIC_ERROR_NONE ||
            cmhip_failover_run(sw, cmhip_batch_dev_in(src), cmhip_batch_stride(src), BLOCK, NULL,
                               (int16_t *)cmhip_batch_dev_in(b) + cmhip_batch_stride(b), cmhip_batch_stride(b)) !=
                COOLMIC_ERROR_NONE ||
            cmhip_batch_run(b, BLOCK, NULL) != COOLMIC_ERROR_NONE ||
            cmhip_failover_state(sw, NULL, &to, NULL, &switches, 0, NULL, NULL, NULL) != COOLMIC_ERROR_NONE) {
            fprintf(stderr, "run: %s\n", cmhip_last_error());
            return 1;
        }
        if (to != was) {
            if (to == 1 && went < 0)
                went = (int)block;
            if (to == 0 && came < 0)
                came = (int)block;
            was = to;
        }
    }
    if (cmhip_batch_watch_results(b, res, rc) != COOLMIC_ERROR_NONE || rc[0] != COOLMIC_ERROR_NONE ||
        rc[1] != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "results: %s\n", cmhip_last_error());
        return 1;
    }
    printf("input: longest dead air %llu frames (%.1f ms)\n", (unsigned long long)res[0].dead_longest,
           1000.0 * (double)res[0].dead_longest / RATE);
    printf("output: longest dead air %llu frames (%.1f ms)\n", (unsigned long long)res[1].dead_longest,
           1000.0 * (double)res[1].dead_longest / RATE);
    printf("output went to the backup in block %d and came back in block %d; switches %llu\n", went, came,
           (unsigned long long)switches);
    cmhip_failover_free(sw);
    cmhip_batch_free(b);
    cmhip_batch_free(src);
    return 0;
}
