/*
 * group_meters.c -- a server that draws a meter per stream per block: N "sine" sound devices behind
 * coolmic_group_t, and per block the loop pumps, reads every stream's transformed PCM through its
 * coolmic_iohandle_t and takes EVERY stream's VU result in one call (coolmic_group_vumeter_results: one
 * snapshot and one collect of the group's engine instead of a copy and a wait per stream).
 *
 * The fourth argument says where the dB values are finished: "host" (the default: the reference's arithmetic
 * with the host's libm, bit-equal to coolmic_vumeter_result) or "device" (the snapshot's kernel does it; the
 * host only copies -- the last bits of the power doubles may differ, everything else is the same).
 *
 *   cc -I include examples/group_meters.c -L libcoolmic-dsp_amd/lib -lcoolmic-dsp-hip -lpthread \
 *      -Wl,-rpath,$PWD/libcoolmic-dsp_amd/lib -o group_meters
 *   ./group_meters [streams] [block] [rounds] [host|device] [r128]
 *
 * Prints the time per block, how many meters were taken, and the last block's meter of stream 0 and of the
 * last stream.  With "r128" as the fifth argument the group also measures true peak and programme loudness
 * (ITU-R BS.1770 / EBU R128: coolmic_group_set_true_peak, coolmic_group_set_loudness) and two more lines give the
 * same two streams' true peak over the whole run beside their momentary, short-term and integrated loudness.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <coolmic-dsp/coolmic-dsp.h>
#include <coolmic-dsp/snddev.h>
#include <coolmic-dsp/group.h>
#include <coolmic_hip.h>

static double now_ms(void)
{
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec * 1e3 + t.tv_nsec * 1e-6;
}

int main(int argc, char **argv)
{
    const unsigned streams = argc > 1 ? (unsigned)atoi(argv[1]) : 1024;
    const size_t block = argc > 2 ? (size_t)atoi(argv[2]) : 512;
    const unsigned rounds = argc > 3 ? (unsigned)atoi(argv[3]) : 64;
    const char *where = argc > 4 ? argv[4] : "host";
    const int r128 = argc > 5 && !strcmp(argv[5], "r128");
    static const uint16_t unity[1] = {1000};
    const size_t nbytes = block * 2;                      /* mono int16 */
    coolmic_group_t *grp;
    coolmic_iohandle_t **out;
    coolmic_vumeter_result_t *meters;
    int *rcs, rc = 1;
    int16_t *buf;
    unsigned long long taken = 0;
    double t0 = 0;
    unsigned s, r;

    if (!streams || !block || !rounds || (strcmp(where, "host") && strcmp(where, "device"))) {
        fprintf(stderr, "usage: group_meters [streams] [block] [rounds] [host|device] [r128]\n");
        return 1;
    }
    grp = coolmic_group_new(NULL, igloo_RO_NULL, 48000, 1, streams, block, 2);
    out = calloc(streams, sizeof(*out));
    meters = calloc(streams, sizeof(*meters));
    rcs = calloc(streams, sizeof(*rcs));
    buf = malloc(nbytes);
    if (!grp || !out || !meters || !rcs || !buf) {
        fprintf(stderr, "no group (no GPU?)\n");
        return 1;
    }
    if (coolmic_group_set_vu_finish(grp, strcmp(where, "device") ? CMHIP_VU_FINISH_HOST : CMHIP_VU_FINISH_DEVICE) !=
        COOLMIC_ERROR_NONE)
        goto done;
    if (r128 && (coolmic_group_set_true_peak(grp, 1) != COOLMIC_ERROR_NONE ||
                 coolmic_group_set_loudness(grp, 1) != COOLMIC_ERROR_NONE)) {
        fprintf(stderr, "r128: %s\n", cmhip_last_error());
        goto done;
    }
    for (s = 0; s < streams; s++) {
        coolmic_snddev_t *dev = coolmic_snddev_new(NULL, igloo_RO_NULL, "sine", NULL, 48000, 1,
                                                   COOLMIC_DSP_SNDDEV_RX, -1);
        coolmic_iohandle_t *h = coolmic_snddev_get_iohandle(dev);
        const int slot = coolmic_group_add_stream(grp, h);
        igloo_ro_unref(h);
        igloo_ro_unref(dev);
        if (slot != (int)s || coolmic_group_set_master_gain(grp, s, 1, 1000, unity) != COOLMIC_ERROR_NONE)
            goto done;
        out[s] = coolmic_group_get_iohandle(grp, s);
    }
    for (r = 0; r < rounds; r++) {
        if (r == 2 || (r == 0 && rounds < 3))             /* two warm-up rounds where there are enough */
            t0 = now_ms();
        if (coolmic_group_pump(grp) < 0)                  /* block r goes to the GPU ... */
            goto done;
        for (s = 0; r > 0 && s < streams; s++)            /* ... while block r-1 is read */
            if (coolmic_iohandle_read(out[s], buf, nbytes) != (ssize_t)nbytes)
                goto done;
        /* every stream's window since the last call -- block r, the block in flight -- in one call */
        if (coolmic_group_vumeter_results(grp, meters, rcs) != COOLMIC_ERROR_NONE) {
            fprintf(stderr, "meters: %s\n", cmhip_last_error());
            goto done;
        }
        for (s = 0; s < streams; s++)
            taken += rcs[s] == COOLMIC_ERROR_NONE;
    }
    t0 = (now_ms() - t0) / (rounds < 3 ? rounds : rounds - 2);
    for (s = 0; s < streams; s++)                         /* the last block */
        if (coolmic_iohandle_read(out[s], buf, nbytes) != (ssize_t)nbytes)
            goto done;
    printf("streams %u block %zu rounds %u finish %s: %.3f ms per block, meters %llu\n", streams, block, rounds, where,
           t0, taken);
    for (s = 0; s < streams; s += streams > 1 ? streams - 1 : 1)
        printf("stream %u: frames %zu peak %d power %.17g\n", s, meters[s].frames, (int)meters[s].global_peak,
               meters[s].global_power);
    for (s = 0; r128 && s < streams; s += streams > 1 ? streams - 1 : 1) {
        coolmic_truepeak_result_t tp;
        coolmic_loudness_result_t loud;
        if (coolmic_group_true_peak(grp, s, &tp) != COOLMIC_ERROR_NONE ||
            coolmic_group_loudness(grp, s, &loud) != COOLMIC_ERROR_NONE)
            goto done;
        printf("stream %u: true peak %.2f dBTP over %zu frames; loudness M %.2f S %.2f I %.2f LUFS (%zu sub-blocks)\n", s,
               tp.global_dbtp, tp.frames, loud.momentary, loud.short_term, loud.integrated, loud.blocks);
    }
    rc = 0;
done:
    for (s = 0; s < streams; s++)
        igloo_ro_unref(out[s]);
    igloo_ro_unref(grp);
    free(out); free(meters); free(rcs); free(buf);
    return rc;
}
