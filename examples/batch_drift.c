/*
 * batch_drift.c -- clock-drift compensation in front of a mix bus from plain C (include/coolmic_hip.h, "clock-drift
 * compensation", "mix bus" and "signal watch").  Two mono sources feed a conference bus that a batch meters in blocks of
 * 512 frames at 48 kHz.  Source A runs on a clock of its own and delivers 1000 ppm more frames than the batch consumes;
 * it lands in an elastic buffer of 2048 frames that starts half full.  Source B is on the batch's clock.  Both go through
 * one cmhip_drift_t (A with the delta a cmhip_drift_servo_t makes of the buffer's fill, B with delta 0), then through a
 * cmhip_bus_t into the batch, all on the batch's stream.  Each source is a tone riding on an offset, so that no frame of
 * the undamaged sum is quiet: any dead frame the signal watch finds is a dropout, any sample at the rail a click.
 * Every 250 blocks it prints the fill, delta in ppm and the totals; at the end
 *   "fill stayed in LO..HI of 2048; settled at PPM ppm"
 *   "dead air 0 frames, clipped samples 0"
 *
 *   cc -I include examples/batch_drift.c -L libcoolmic-dsp_amd/lib -lcoolmic-dsp-hip -lm \
 *      -Wl,-rpath,$PWD/libcoolmic-dsp_amd/lib -o batch_drift && ./batch_drift
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <coolmic-dsp/coolmic-dsp.h>
#include <coolmic_hip.h>

enum { RATE = 48000, BLOCK = 512, BLOCKS = 3000, TARGET = 1024, CAPACITY = 2 * TARGET, MAX_IN = BLOCK + 8, EVERY = 250 };
static const double PPM = 1000.0, PI2 = 6.283185307179586;

static int16_t tone(double hz, uint64_t n) { return (int16_t)lrint(9000.0 + 6000.0 * sin(PI2 * hz * (double)n / RATE)); }

int main(void)
{
    static const uint32_t bus_of[2] = {0, 0}, stream_of[2] = {0, 1};
    static const int16_t half[2] = {8192, 8192};     /* each source at -6 dB */
    cmhip_batch_desc_t sd = {0}, md = {0};
    cmhip_drift_desc_t dd = {0};
    cmhip_bus_desc_t bd = {0};
    cmhip_batch_t *src, *mid, *b;
    cmhip_drift_t *drift;
    cmhip_bus_t *bus;
    cmhip_drift_servo_t servo;
    coolmic_watch_result_t res;
    static int16_t ring[CAPACITY], a[MAX_IN], bb[MAX_IN];
    uint64_t made_a = 0, made_b = 0, pos, in_total = 0, out_total = 0;
    double owed = 0.0, settled = 0.0;
    int32_t delta = 0;
    unsigned fill = TARGET, lo = TARGET, hi = TARGET, block, i;

    for (i = 0; i < TARGET; i++)                     /* the buffer starts half full */
        ring[i] = tone(1000.0, made_a++);
    /* device memory for the sources and for what the drift stage gives: batches used as slots */
    sd.device = 0; sd.streams = 2; sd.channels = 1; sd.rate = RATE; sd.max_frames = MAX_IN; sd.flags = CMHIP_VU;
    src = cmhip_batch_new(&sd);
    mid = cmhip_batch_new(&sd);
    md = sd; md.streams = 1;
    b = cmhip_batch_new(&md);
    if (!src || !mid || !b) {
        fprintf(stderr, "batch: %s\n", cmhip_last_error());
        return 1;
    }
    dd.device = 0; dd.streams = 2; dd.channels = 1; dd.max_in_frames = MAX_IN; dd.hip_stream = cmhip_batch_hip_stream(b);
    drift = cmhip_drift_new(&dd);
    bd.device = 0; bd.streams = 2; bd.buses = 1; bd.channels_in = bd.channels_out = 1; bd.max_frames = MAX_IN;
    bd.max_sends = 2; bd.hip_stream = cmhip_batch_hip_stream(b);
    bus = cmhip_bus_new(&bd);
    if (!drift || !bus || cmhip_bus_set_routing(bus, 2, bus_of, stream_of, half) != COOLMIC_ERROR_NONE ||
        cmhip_drift_servo_init(&servo, TARGET, 15, 6, CMHIP_DRIFT_DELTA_MAX) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "stages: %s\n", cmhip_last_error());
        return 1;
    }
    for (block = 0; block < BLOCKS; block++) {
        uint32_t counts[2], got[2], mixed, arrive, need;
        /* source A delivers on its own clock, into the elastic buffer */
        owed += BLOCK * (1.0 + PPM * 1e-6);
        arrive = (uint32_t)owed;
        owed -= arrive;
        if (fill + arrive > CAPACITY) {
            fprintf(stderr, "block %u: the buffer overflows\n", block);
            return 1;
        }
        for (i = 0; i < arrive; i++)
            ring[fill + i] = tone(1000.0, made_a++);
        fill += arrive;
        if (fill > hi)
            hi = fill;
        /* the servo turns the fill into this block's delta; the frames that BLOCK outputs read follow from the position */
        delta = cmhip_drift_servo_step(&servo, fill);
        if (cmhip_drift_set(drift, 0, delta) != COOLMIC_ERROR_NONE ||
            cmhip_drift_get(drift, 0, NULL, &pos, NULL, NULL) != COOLMIC_ERROR_NONE) {
            fprintf(stderr, "set: %s\n", cmhip_last_error());
            return 1;
        }
        need = (uint32_t)((pos + (uint64_t)(BLOCK - 1) * (uint64_t)(4294967296ll + delta)) >> 32) + 1u;
        if (need > fill || need > MAX_IN) {
            fprintf(stderr, "block %u: the buffer underruns (%u of %u frames)\n", block, fill, need);
            return 1;
        }
        memcpy(a, ring, need * sizeof(int16_t));
        memmove(ring, ring + need, (fill - need) * sizeof(int16_t));
        fill -= need;
        if (fill < lo)
            lo = fill;
        for (i = 0; i < BLOCK; i++)                  /* source B: the batch's clock */
            bb[i] = tone(440.0, made_b++);
        counts[0] = need;
        counts[1] = BLOCK;
        if (cmhip_batch_upload(src, 0, a, need) != COOLMIC_ERROR_NONE ||
            cmhip_batch_upload(src, 1, bb, BLOCK) != COOLMIC_ERROR_NONE || cmhip_batch_sync(src) != COOLMIC_ERROR_NONE ||
            cmhip_drift_run(drift, cmhip_batch_dev_in(src), cmhip_batch_stride(src), need > BLOCK ? need : BLOCK, counts,
                            cmhip_batch_dev_in(mid), cmhip_batch_stride(mid), got) != COOLMIC_ERROR_NONE) {
            fprintf(stderr, "drift: %s\n", cmhip_last_error());
            return 1;
        }
        if (got[0] != BLOCK || got[1] != BLOCK) {    /* (a delta below 0 can give one more: not with this source) */
            fprintf(stderr, "block %u: %u and %u outputs\n", block, got[0], got[1]);
            return 1;
        }
        /* the drift stage's counts are the frames_per_stream of what follows */
        if (cmhip_bus_run(bus, cmhip_batch_dev_in(mid), cmhip_batch_stride(mid), BLOCK, got, cmhip_batch_dev_in(b),
                          cmhip_batch_stride(b), &mixed) != COOLMIC_ERROR_NONE ||
            cmhip_batch_run(b, BLOCK, &mixed) != COOLMIC_ERROR_NONE ||
            cmhip_batch_sync(b) != COOLMIC_ERROR_NONE) {         /* (the next block's upload overwrites the sources) */
            fprintf(stderr, "run: %s\n", cmhip_last_error());
            return 1;
        }
        /* the first block carries the filter's way in from an empty history: the watch begins behind it */
        if (block == 0 && cmhip_batch_set_watch(b, 1) != COOLMIC_ERROR_NONE) {
            fprintf(stderr, "watch: %s\n", cmhip_last_error());
            return 1;
        }
        if (block >= BLOCKS - 500)
            settled += cmhip_drift_to_ppm(delta) / 500.0;
        if ((block + 1) % EVERY == 0) {
            (void)cmhip_drift_get(drift, 0, NULL, NULL, &in_total, &out_total);
            printf("block %4u: fill %4u, delta %+8.1f ppm, %llu frames in, %llu out\n", block + 1, fill,
                   cmhip_drift_to_ppm(delta), (unsigned long long)in_total, (unsigned long long)out_total);
        }
    }
    if (cmhip_batch_watch_result(b, 0, &res) != COOLMIC_ERROR_NONE) {
        fprintf(stderr, "results: %s\n", cmhip_last_error());
        return 1;
    }
    printf("fill stayed in %u..%u of %d; settled at %.1f ppm\n", lo, hi, (int)CAPACITY, settled);
    printf("dead air %llu frames, clipped samples %llu\n", (unsigned long long)res.dead_frames,
           (unsigned long long)res.clip_samples[0]);
    cmhip_bus_free(bus);
    cmhip_drift_free(drift);
    cmhip_batch_free(b);
    cmhip_batch_free(mid);
    cmhip_batch_free(src);
    return res.dead_frames || res.clip_samples[0];
}
