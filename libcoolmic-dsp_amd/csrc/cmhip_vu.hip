// cmhip_vu.hip -- VU windows of a batch on the host side: per-stream results, packed snapshots and their collect
// (the dB finish in double, as ref: src/vumeter.c:189-218), per-launch window records for the meters behind a
// tee, node records for the node-global VU.
#include "cmhip_engine.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <thread>

// ---------------------------------------------------------------------------
// VU windows

// keys hold |peak| from bit `shift` up and the sign in bit 0: KEY_ABS_SHIFT (a window), NODE_KEY_ABS_SHIFT (a node record)
static int16_t key_peak(unsigned long long key, int shift)
{
    const int mag = (int)(key >> shift);
    return (int16_t)((key & 1ull) ? -mag : mag);
}

// ref: src/vumeter.c:203-205 -- integer mean first, then dB in double, capped at 0
static double power_db(unsigned long long sum, unsigned long long count)
{
    double p = (double)(sum / count);
    p = 20. * log10(sqrt(p) / 32768.);
    return fmin(p, 0.);
}

// The window's result (ref: src/vumeter.c:189-218): `frames` frames of C channels, the sums and peak keys of channel c
// at sum[c * stride] / key[c * stride] -- in one of the three spellings of a 64-bit word the windows come in -- and
// the key of the global peak.  Out is left alone while the window holds no frame.
template <typename Word>
static int finish(unsigned long long frames, unsigned C, unsigned rate, const Word *sum, const Word *key, size_t stride,
                  unsigned long long global_key, int shift, coolmic_vumeter_result_t *out)
{
    if (frames == 0)
        return COOLMIC_ERROR_INVAL;                      // ref: src/vumeter.c:198-199
    memset(out, 0, sizeof(*out));
    out->rate = rate;
    out->channels = C;
    out->frames = (size_t)frames;
    unsigned long long all = 0;
    for (unsigned c = 0; c < C; c++) {
        all += (unsigned long long)sum[c * stride];
        out->channel_power[c] = power_db((unsigned long long)sum[c * stride], frames);
        out->channel_peak[c] = key_peak((unsigned long long)key[c * stride], shift);
    }
    // (mono: the same arguments as channel 0, hence the same bits)
    out->global_power = C == 1 ? out->channel_power[0] : power_db(all, frames * C);
    out->global_peak = key_peak(global_key, shift);
    return COOLMIC_ERROR_NONE;
}

// a batch window's global peak: the largest key over its channels, the first max-|x| over all of them
template <typename Word>
static unsigned long long max_key(const Word *key, size_t stride, unsigned C)
{
    unsigned long long best = 0;
    for (unsigned c = 0; c < C; c++)
        if (key[c * stride] > best)
            best = key[c * stride];
    return best;
}

// one stream's window to the host, behind what the main stream has queued
static int read_window(cmhip_batch_t *b, unsigned int stream, VuState *v)
{
    if (use(b) || cmhip_engine_settle_node(b))
        return COOLMIC_ERROR_GENERIC;
    HIP_TRY(hipMemcpyAsync(v, b->d_vu + stream, sizeof(*v), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_batch_vu_result(cmhip_batch_t *b, unsigned int stream,
                                     coolmic_vumeter_result_t *out)
{
    if (!b || !out)
        return fail(COOLMIC_ERROR_FAULT, "vu_result: NULL argument");
    if (stream >= b->d.streams || !(b->d.flags & CMHIP_VU))
        return fail(COOLMIC_ERROR_INVAL, "vu_result: stream out of range or batch without VU");
    b->last_done = nullptr;                  // main-stream work on the windows follows the last run
    VuState v;
    if (read_window(b, stream, &v))
        return COOLMIC_ERROR_GENERIC;
    const unsigned C = b->d.channels;
    const int rc = finish(v.samples[b->parity] / C, C, b->d.rate, v.power, v.key, 1, max_key(v.key, 1, C),
                          KEY_ABS_SHIFT, out);
    if (rc == COOLMIC_ERROR_NONE)
        HIP_TRY(hipMemsetAsync(b->d_vu + stream, 0, sizeof(VuState), b->stream));
    return rc;
}

extern "C" int cmhip_batch_vu_snapshot(cmhip_batch_t *b)
{
    if (!b)
        return fail(COOLMIC_ERROR_FAULT, "vu_snapshot: batch is NULL");
    if (!(b->d.flags & CMHIP_VU))
        return fail(COOLMIC_ERROR_INVAL, "vu_snapshot: batch without VU");
    if (b->snap_count == 3)
        return fail(COOLMIC_ERROR_BUSY, "vu_snapshot: three snapshots are waiting to be collected");
    if (use(b))
        return COOLMIC_ERROR_GENERIC;
    // The closed windows travel to the host on the copy stream and are cleared there, while
    // the main stream goes straight on with the next block into the next set.  Three sets
    // rotate so that the set a launch switches to was cleared a whole launch earlier: with
    // two, every launch waited for the copy + clear that ran beside its predecessor.
    // One kernel does both (k_vu_pack): it writes what the host needs of every window -- 1 + 2C words,
    // 40 bytes for stereo instead of the 264 of a VuState -- straight into pinned host memory and
    // clears the set; its own dispatch stamps the set's event.
    const unsigned i = b->cur;
    const unsigned slot = (b->snap_head + b->snap_count) % 3u;
    if (b->last_done) {
        HIP_TRY(hipStreamWaitEvent(b->copy_stream, b->last_done, 0));
        b->last_done = nullptr;
    } else {
        HIP_TRY(hipEventRecord(b->ev_main, b->stream));
        HIP_TRY(hipStreamWaitEvent(b->copy_stream, b->ev_main, 0));
    }
    // (CMHIP_VU_FINISH_DEVICE: k_vu_finish in its place -- same stream, same event, same clear; the record
    // holds finished dB doubles and peaks)
    if (b->vu_finish == CMHIP_VU_FINISH_DEVICE)
        HIP_TRY(launch_vu_finish(b->d_vu2[i], b->d.streams, b->d.channels, b->parity, b->d_pack[slot],
                                 b->copy_stream, b->ev_reset[i]));
    else
        HIP_TRY(launch_vu_pack(b->d_vu2[i], b->d.streams, b->d.channels, b->parity, b->d_pack[slot],
                               b->copy_stream, b->ev_reset[i]));
    b->snap_set2[slot] = i;
    b->reset_pending[i] = true;
    b->cur = (i + 1u) % 3u;
    b->d_vu = b->d_vu2[b->cur];
    b->node_reading = false;                 // (a node partial of the closed set runs ahead of this copy, same stream)
    if (b->reset_pending[b->cur]) {          // the set we switch to must have been cleared
        // (it was, a launch ago, in the steady state: then the main stream needs no packet for it)
        if (hipEventQuery(b->ev_reset[b->cur]) != hipSuccess)
            HIP_TRY(hipStreamWaitEvent(b->stream, b->ev_reset[b->cur], 0));
        b->reset_pending[b->cur] = false;
    }
    b->snap_count++;
    return COOLMIC_ERROR_NONE;
}

// Helpers beside the calling thread: half the hardware threads, at most 12 -- and, inside a container, no more
// than its CPU-time quota leaves beside the launching thread and the runtime's own (measured under a quota of
// 16 CPUs with 256 hardware threads visible: 12 helpers finish 4096 windows in 25 us, 14 take the CPU from the
// thread that launches and the step gets longer, NOTES_r03).  $CMHIP_POOL_THREADS overrides.
static unsigned pool_threads()
{
    if (const char *e = getenv("CMHIP_POOL_THREADS"))
        if (atoi(e) > 0)
            return (unsigned)atoi(e);
    unsigned n = std::thread::hardware_concurrency() / 2;
    n = n < 1 ? 1 : (n > 12 ? 12 : n);
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {          // cgroup v2: "<quota> <period>" or "max <period>"
        char q[32] = "";
        long period = 0;
        if (fscanf(f, "%31s %ld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0) {
            const long cpus = atol(q) / period;
            if (cpus >= 1 && (unsigned)cpus < n + 4u)
                n = cpus > 4 ? (unsigned)(cpus - 4) : 1u;
        }
        fclose(f);
    }
    return n;
}

// A record k_vu_finish wrote (the layout is stated there), [word][stream] over S streams, into a result: copies
// only -- no libm call.  Out is left alone while the window holds no frame.
static int unpack_finished(const unsigned long long *words, size_t S, size_t s, unsigned C, unsigned rate,
                           coolmic_vumeter_result_t *out)
{
    const unsigned long long frames = words[s] / C;
    if (frames == 0)
        return COOLMIC_ERROR_INVAL;                      // ref: src/vumeter.c:198-199
    memset(out, 0, sizeof(*out));
    out->rate = rate;
    out->channels = C;
    out->frames = (size_t)frames;
    const unsigned P = C == 1 ? 1u : C + 1u;             // power words: mono has no global word of its own
    for (unsigned c = 0; c < C; c++) {
        memcpy(&out->channel_power[c], &words[(1u + c) * S + s], sizeof(double));
        out->channel_peak[c] = (int16_t)(words[(1u + P + c / 4u) * S + s] >> (16u * (c % 4u)));
    }
    if (C == 1)
        out->global_power = out->channel_power[0];
    else
        memcpy(&out->global_power, &words[(1u + C) * S + s], sizeof(double));
    out->global_peak = (int16_t)(words[(1u + P + C / 4u) * S + s] >> (16u * (C % 4u)));
    return COOLMIC_ERROR_NONE;
}

// a packed snapshot is [word][stream]: samples, C sums, C keys -- or, finished on the device, what unpack_finished reads
static void collect_body(void *p, unsigned lo, unsigned hi)
{
    cmhip_batch_t *b = (cmhip_batch_t *)p;
    const unsigned C = b->d.channels;
    const size_t S = b->d.streams;
    const unsigned long long *pack = b->h_pack[b->job_slot];
    if (b->vu_finish == CMHIP_VU_FINISH_DEVICE) {
        for (unsigned s = lo; s < hi; s++) {
            const int r = unpack_finished(pack, S, s, C, b->d.rate, &b->job_out[s]);
            if (b->job_rc)
                b->job_rc[s] = r;
        }
        return;
    }
    for (unsigned s = lo; s < hi; s++) {
        const unsigned long long *sum = pack + S + s, *key = sum + C * S;
        const int r = finish(pack[s] / C, C, b->d.rate, sum, key, S, max_key(key, S, C), KEY_ABS_SHIFT, &b->job_out[s]);
        if (b->job_rc)
            b->job_rc[s] = r;
    }
}

// The dB finish of the oldest snapshot, in two halves: begin() waits for the snapshot's data and hands the
// windows to the helper pool, end() takes what is left itself and returns when out[] / rc[] are complete.
// Between the two the caller queues the next block -- with a window per block of a few thousand frames the
// host's finish (thousands of log10 per step) is as long as the kernel, and only beside the next launch does
// it stop counting.  cmhip_batch_vu_collect() is the two in one.
extern "C" int cmhip_batch_vu_collect_begin(cmhip_batch_t *b, coolmic_vumeter_result_t *out, int *rc)
{
    if (!b || !out)
        return fail(COOLMIC_ERROR_FAULT, "vu_collect: NULL argument");
    if (b->collecting)
        return fail(COOLMIC_ERROR_BUSY, "vu_collect_begin: the collect before has not been ended");
    if (b->snap_count == 0)
        return fail(COOLMIC_ERROR_INVAL, "vu_collect: no snapshot pending");
    if (use(b))
        return COOLMIC_ERROR_GENERIC;
    const unsigned slot = b->snap_head;
    HIP_TRY(hipEventSynchronize(b->ev_reset[b->snap_set2[slot]]));
    b->job_out = out;
    b->job_rc = rc;
    b->job_slot = slot;
    b->collecting = true;                    // (the snapshot keeps its place in the ring until end())
    if (b->d.streams >= 512) {
        if (!b->pool) {
            // (helpers beside the calling thread; $CMHIP_POOL_THREADS for hosts with a CPU quota below their
            // core count)
            b->pool = new WorkPool(pool_threads());
        }
        b->pool->start(collect_body, b, b->d.streams);
    }
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_batch_vu_collect_end(cmhip_batch_t *b)
{
    if (!b)
        return fail(COOLMIC_ERROR_FAULT, "vu_collect_end: batch is NULL");
    if (!b->collecting)
        return fail(COOLMIC_ERROR_INVAL, "vu_collect_end: no collect under way");
    if (b->d.streams >= 512)
        b->pool->finish();
    else
        collect_body(b, 0, b->d.streams);
    b->collecting = false;
    b->snap_head = (b->snap_head + 1u) % 3u;
    b->snap_count--;
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_batch_vu_collect(cmhip_batch_t *b, coolmic_vumeter_result_t *out, int *rc)
{
    const int r = cmhip_batch_vu_collect_begin(b, out, rc);
    return r != COOLMIC_ERROR_NONE ? r : cmhip_batch_vu_collect_end(b);
}

extern "C" int cmhip_batch_vu_set_finish(cmhip_batch_t *b, int where)
{
    if (!b)
        return fail(COOLMIC_ERROR_FAULT, "vu_set_finish: batch is NULL");
    if (!(b->d.flags & CMHIP_VU) || (where != CMHIP_VU_FINISH_HOST && where != CMHIP_VU_FINISH_DEVICE))
        return fail(COOLMIC_ERROR_INVAL, "vu_set_finish: batch without VU, or unknown place %d", where);
    if (b->snap_count || b->collecting)      // a pending snapshot is read the way it was written
        return fail(COOLMIC_ERROR_BUSY, "vu_set_finish: %u snapshot(s) wait to be collected", b->snap_count);
    b->vu_finish = where;
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_batch_vu_get_finish(const cmhip_batch_t *b)
{
    if (!b)
        return fail(COOLMIC_ERROR_FAULT, "vu_get_finish: batch is NULL");
    if (!(b->d.flags & CMHIP_VU))
        return fail(COOLMIC_ERROR_INVAL, "vu_get_finish: batch without VU");
    return b->vu_finish;
}

extern "C" int cmhip_batch_vu_results(cmhip_batch_t *b, coolmic_vumeter_result_t *out, int *rc)
{
    const int r = cmhip_batch_vu_snapshot(b);
    if (r != COOLMIC_ERROR_NONE)
        return r;
    // NB: unlike the per-stream call this resets every window, also those with no frames
    return cmhip_batch_vu_collect(b, out, rc);
}

extern "C" int cmhip_batch_vu_reset(cmhip_batch_t *b, long stream)
{
    if (!b)
        return fail(COOLMIC_ERROR_FAULT, "vu_reset: batch is NULL");
    const StreamRange sr = stream_range(stream, b->d.streams);
    if (!sr.ok)
        return fail(COOLMIC_ERROR_INVAL, "vu_reset: stream %ld out of range", stream);
    if (use(b))
        return COOLMIC_ERROR_GENERIC;
    b->last_done = nullptr;                  // main-stream work on the windows follows the last run
    if (cmhip_engine_settle_node(b))
        return COOLMIC_ERROR_GENERIC;
    HIP_TRY(hipMemsetAsync(b->d_vu + sr.lo, 0, sr.n * sizeof(VuState), b->stream));
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_batch_vu_raw(cmhip_batch_t *b, unsigned int stream, int64_t *power,
                                  int16_t *peak, uint64_t *frames)
{
    if (!b)
        return fail(COOLMIC_ERROR_FAULT, "vu_raw: batch is NULL");
    if (stream >= b->d.streams)
        return fail(COOLMIC_ERROR_INVAL, "vu_raw: stream out of range");
    VuState v;
    if (read_window(b, stream, &v))
        return COOLMIC_ERROR_GENERIC;
    for (unsigned c = 0; c < MAX_CH; c++) {
        if (power)
            power[c] = (int64_t)v.power[c];
        if (peak)
            peak[c] = key_peak(v.key[c], KEY_ABS_SHIFT);
    }
    if (frames)
        *frames = v.samples[b->parity] / b->d.channels;
    return COOLMIC_ERROR_NONE;
}

// ---------------------------------------------------------------------------
// per-launch window records (engine internal, host_internal.h): transform.c / vumeter.c

static void raw_from_state(const VuState &v, unsigned parity, cmhip_vu_raw_t *out)
{
    static_assert(MAX_CH == 16, "cmhip_vu_raw_t holds sixteen channels");
    for (unsigned c = 0; c < MAX_CH; c++) {
        out->power[c] = v.power[c];
        out->key[c] = v.key[c];
    }
    out->samples = v.samples[parity];
}

extern "C" CMHIP_INTERNAL int cmhip_batch_vu_ring(cmhip_batch_t *b, unsigned int slots)
{
    if (!b)
        return fail(COOLMIC_ERROR_FAULT, "vu_ring: batch is NULL");
    if (!(b->d.flags & CMHIP_VU) || slots > 65536)
        return fail(COOLMIC_ERROR_INVAL, "vu_ring: batch without VU, or too many slots");
    if (use(b))
        return COOLMIC_ERROR_GENERIC;
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (slots != b->ring_slots) {
        (void)hipFree(b->d_ring);
        if (b->h_ring)
            (void)hipHostFree(b->h_ring);
        b->d_ring = b->h_ring = nullptr;
        b->ring_slots = 0;
        if (slots) {
            const size_t bytes = (size_t)slots * b->d.streams * sizeof(VuState);
            HIP_TRY(hipMalloc((void **)&b->d_ring, bytes));
            HIP_TRY(hipHostMalloc((void **)&b->h_ring, bytes, hipHostMallocDefault));
            b->ring_slots = slots;
        }
    }
    if (b->ring_slots)
        HIP_TRY(hipMemsetAsync(b->d_ring, 0, (size_t)b->ring_slots * b->d.streams * sizeof(VuState), b->stream));
    b->ring_fetched = b->ring_seq;           // every slot is clear
    return COOLMIC_ERROR_NONE;
}

extern "C" CMHIP_INTERNAL uint64_t cmhip_batch_vu_ring_seq(const cmhip_batch_t *b) { return b ? b->ring_seq : 0; }

extern "C" CMHIP_INTERNAL int cmhip_batch_vu_ring_fetch(cmhip_batch_t *b, uint64_t first_seq, unsigned int count,
                                                        cmhip_vu_raw_t *out)
{
    if (!b || !out)
        return fail(COOLMIC_ERROR_FAULT, "vu_ring_fetch: NULL argument");
    if (!b->ring_slots || count == 0 || count > b->ring_slots || first_seq + count > b->ring_seq ||
        b->ring_seq - first_seq > b->ring_slots || first_seq != b->ring_fetched)
        return fail(COOLMIC_ERROR_INVAL, "vu_ring_fetch: runs %llu..+%u are not the oldest unfetched ones of the ring (%llu)",
                    (unsigned long long)first_seq, count, (unsigned long long)b->ring_fetched);
    if (use(b))
        return COOLMIC_ERROR_GENERIC;
    const size_t S = b->d.streams;
    const unsigned first = (unsigned)(first_seq % b->ring_slots);
    const unsigned n1 = count < b->ring_slots - first ? count : b->ring_slots - first;     // up to the wrap
    HIP_TRY(hipMemcpyAsync(b->h_ring + (size_t)first * S, b->d_ring + (size_t)first * S, n1 * S * sizeof(VuState),
                           hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipMemsetAsync(b->d_ring + (size_t)first * S, 0, n1 * S * sizeof(VuState), b->stream));
    if (n1 < count) {
        HIP_TRY(hipMemcpyAsync(b->h_ring, b->d_ring, (count - n1) * S * sizeof(VuState), hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipMemsetAsync(b->d_ring, 0, (count - n1) * S * sizeof(VuState), b->stream));
    }
    HIP_TRY(hipStreamSynchronize(b->stream));
    for (unsigned i = 0; i < count; i++)
        raw_from_state(b->h_ring[(size_t)((first + i) % b->ring_slots) * S], 1u, &out[i]);
    b->ring_fetched = first_seq + count;
    return COOLMIC_ERROR_NONE;
}

extern "C" CMHIP_INTERNAL int cmhip_batch_vu_raw_state(cmhip_batch_t *b, unsigned int stream, cmhip_vu_raw_t *out)
{
    if (!b || !out)
        return fail(COOLMIC_ERROR_FAULT, "vu_raw_state: NULL argument");
    if (stream >= b->d.streams || !(b->d.flags & CMHIP_VU))
        return fail(COOLMIC_ERROR_INVAL, "vu_raw_state: stream out of range or batch without VU");
    VuState v;
    if (read_window(b, stream, &v))
        return COOLMIC_ERROR_GENERIC;
    raw_from_state(v, b->parity, out);
    return COOLMIC_ERROR_NONE;
}

extern "C" CMHIP_INTERNAL void cmhip_vu_raw_merge(cmhip_vu_raw_t *acc, const cmhip_vu_raw_t *piece, unsigned int channels)
{
    for (unsigned c = 0; c < channels && c < MAX_CH; c++) {
        acc->power[c] += piece->power[c];
        uint64_t k = piece->key[c];
        if (k) {                             // the piece's sample indices continue the window's
            const uint64_t idx = (~(k >> 1) & KEY_IDX_MASK) + acc->samples;
            k = (k & ~(KEY_IDX_MASK << 1)) | ((~idx & KEY_IDX_MASK) << 1);
            if (k > acc->key[c])
                acc->key[c] = k;
        }
    }
    acc->samples += piece->samples;
}

extern "C" CMHIP_INTERNAL int cmhip_vu_raw_finish(const cmhip_vu_raw_t *w, unsigned int channels, unsigned int rate,
                                                  coolmic_vumeter_result_t *out)
{
    if (!w || !out || channels == 0 || channels > MAX_CH)
        return COOLMIC_ERROR_FAULT;
    return finish(w->samples / channels, channels, rate, w->power, w->key, 1, max_key(w->key, 1, channels),
                  KEY_ABS_SHIFT, out);
}

// test hook (host logic, needs no GPU): `count` raw windows of 33 words each (16 sums, 16 keys, samples), one after
// the other in stream order, merged as a meter behind a tee merges the records of the launches it has consumed
// (csrc/vumeter.c), and finished
extern "C" int cmhip_test_merge_windows(const uint64_t *windows, unsigned int count, unsigned int channels,
                                        unsigned int rate, coolmic_vumeter_result_t *out)
{
    if (!windows || !out)
        return COOLMIC_ERROR_FAULT;
    cmhip_vu_raw_t acc;
    memset(&acc, 0, sizeof(acc));
    for (unsigned int i = 0; i < count; i++) {
        cmhip_vu_raw_t w;
        memcpy(&w, windows + (size_t)i * 33u, sizeof(w));
        cmhip_vu_raw_merge(&acc, &w, channels);
    }
    return cmhip_vu_raw_finish(&acc, channels, rate, out);
}

// test hook (host logic, needs no GPU): the unpack of a device-finished record the caller made up, [word][stream]
// over `streams` streams of `channels` channels
extern "C" int cmhip_test_unpack_finished(const uint64_t *words, unsigned int streams, unsigned int channels,
                                          unsigned int rate, coolmic_vumeter_result_t *out, int *rc)
{
    if (!words || !out)
        return COOLMIC_ERROR_FAULT;
    if (channels == 0 || channels > MAX_CH)
        return COOLMIC_ERROR_INVAL;
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "a record's word");
    for (unsigned int s = 0; s < streams; s++) {
        const int r = unpack_finished((const unsigned long long *)words, streams, s, channels, rate, &out[s]);
        if (rc)
            rc[s] = r;
    }
    return COOLMIC_ERROR_NONE;
}

// test hook: the kernels' own __device__ finish (vu_power_db, k_misc.hip) over n (sum, count) pairs on the default
// device; out_log (may be NULL) takes log10(...) before the * 20, so that a deviation can be put to a stage
extern "C" int cmhip_test_power_db_device(const uint64_t *sum, const uint64_t *count, unsigned int n, double *out_db,
                                          double *out_log)
{
    if (!sum || !count || !out_db)
        return fail(COOLMIC_ERROR_FAULT, "test_power_db_device: NULL argument");
    if (n == 0)
        return COOLMIC_ERROR_NONE;
    HIP_TRY(hipSetDevice(coolmic_hip_default_device()));
    const size_t bytes = (size_t)n * 8u;
    unsigned long long *d = nullptr;                     // sums, counts, dB values, logarithms
    HIP_TRY(hipMalloc((void **)&d, 4u * bytes));
    hipError_t e = hipMemcpy(d, sum, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = hipMemcpy(d + n, count, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = launch_test_power_db(d, d + n, n, (double *)(d + 2u * (size_t)n), (double *)(d + 3u * (size_t)n), nullptr);
    if (e == hipSuccess)
        e = hipMemcpy(out_db, d + 2u * (size_t)n, bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess && out_log)
        e = hipMemcpy(out_log, d + 3u * (size_t)n, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    HIP_TRY(e);
    return COOLMIC_ERROR_NONE;
}

// ---------------------------------------------------------------------------
// node-global VU

// the node record of the batch's windows, its sums and its keys in two places, on the main stream (after use())
static int node_partial_split(cmhip_batch_t *b, long long *dst_sum, long long *dst_key,
                              uint64_t first_global, uint64_t global_step)
{
    // This kernel reads the windows after the last run, on the same stream: its own end, stamped by
    // its dispatch, is what the next snapshot has to wait for -- no event packet on the main stream.
    if (cmhip_engine_settle_node(b))
        return COOLMIC_ERROR_GENERIC;
    hipEvent_t done = b->ev_done[b->done_next];
    b->done_next = (b->done_next + 1u) & 3u;
    b->last_done = nullptr;
    HIP_TRY(launch_node_partial(b->d_vu, b->d.streams, b->d.channels, b->parity, first_global, global_step,
                                dst_sum, dst_key, true, b->stream, done));
    b->last_done = done;
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_batch_vu_node_partial(cmhip_batch_t *b, void *dst_device,
                                           uint64_t first_global, uint64_t global_step)
{
    if (!b || !dst_device)
        return fail(COOLMIC_ERROR_FAULT, "vu_node_partial: NULL argument");
    if (!(b->d.flags & CMHIP_VU))
        return fail(COOLMIC_ERROR_INVAL, "vu_node_partial: batch without VU");
    if (use(b))
        return COOLMIC_ERROR_GENERIC;
    long long *dst = (long long *)dst_device;
    return node_partial_split(b, dst, dst + CMHIP_NODE_SUM_WORDS, first_global, global_step);
}

extern "C" int cmhip_batch_vu_node_record(cmhip_batch_t *b, int64_t *words_host, uint64_t first_global,
                                          uint64_t global_step)
{
    if (!b || !words_host)
        return fail(COOLMIC_ERROR_FAULT, "vu_node_record: NULL argument");
    if (!(b->d.flags & CMHIP_VU))
        return fail(COOLMIC_ERROR_INVAL, "vu_node_record: batch without VU");
    if (use(b))
        return COOLMIC_ERROR_GENERIC;
    if (!b->d_node_scratch)
        HIP_TRY(hipMalloc((void **)&b->d_node_scratch, CMHIP_NODE_WORDS * sizeof(long long)));
    const int rc = node_partial_split(b, b->d_node_scratch, b->d_node_scratch + CMHIP_NODE_SUM_WORDS,
                                      first_global, global_step);
    if (rc != COOLMIC_ERROR_NONE)
        return rc;
    HIP_TRY(hipMemcpyAsync(words_host, b->d_node_scratch, CMHIP_NODE_WORDS * sizeof(long long),
                           hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return COOLMIC_ERROR_NONE;
}

// internal (node.hip): the record of a cmhip_node_t set, built on the COPY stream -- beside the batch's
// next run instead of between two runs (the main stream carries nothing for it: 8 us per block of
// config 5).  The copy stream waits for the last run's own end; a snapshot that follows is behind the
// kernel on the same stream; anything else that touches the windows goes through settle_node().
int cmhip_batch_node_partial_side(cmhip_batch_t *b, long long *dst_sum, long long *dst_key,
                                  uint64_t first_global, uint64_t global_step)
{
    if (use(b))
        return COOLMIC_ERROR_GENERIC;
    if (b->last_done) {
        HIP_TRY(hipStreamWaitEvent(b->copy_stream, b->last_done, 0));
    } else {
        HIP_TRY(hipEventRecord(b->ev_main, b->stream));
        HIP_TRY(hipStreamWaitEvent(b->copy_stream, b->ev_main, 0));
    }
    HIP_TRY(launch_node_partial(b->d_vu, b->d.streams, b->d.channels, b->parity, first_global, global_step,
                                dst_sum, dst_key, false, b->copy_stream, nullptr));
    b->node_reading = true;
    return COOLMIC_ERROR_NONE;
}

// internal (transform.c): a batch with windows runs without touching them while paused -- the
// transform accumulates only the blocks its fused meter has asked for
extern "C" __attribute__((visibility("hidden"))) void cmhip_batch_vu_pause(cmhip_batch_t *b, int paused)
{
    if (b)
        b->vu_off = paused != 0;
}

extern "C" int cmhip_node_finish(const int64_t *w, unsigned int channels, unsigned int rate,
                                 coolmic_vumeter_result_t *out)
{
    if (!w || !out)
        return fail(COOLMIC_ERROR_FAULT, "node_finish: NULL argument");
    if (channels == 0 || channels > MAX_CH)
        return fail(COOLMIC_ERROR_INVAL, "node_finish: channels out of range");
    // [0, 16): sums, [16]: frames, [17, 33): keys, [33]: the key of the global peak
    return finish((unsigned long long)w[MAX_CH], channels, rate, w, w + MAX_CH + 1, 1,
                  (unsigned long long)w[2 * MAX_CH + 1], NODE_KEY_ABS_SHIFT, out);
}

