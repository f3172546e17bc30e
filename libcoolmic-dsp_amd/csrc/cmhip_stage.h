// cmhip_stage.h -- a stage object beside the batch, on the HIP side: what the thirteen stages (resampler, mixer, bus, limiter,
// dynamics, band split, delay, leveller, filter, automixer, failover switch, drift stage, noise suppressor) do alike, once.  Not part of the C ABI; cmhip_engine.h includes it
// once fail and HIP_TRY exist.
//   CountsRing        the pinned ring a run's counts travel through
//   StageBase         the device, the stream (the caller's or its own), the counts, and every device array of the object
//   stage_guard       std::bad_alloc kept on this side of the C ABI
//   stage_new, _free  the two ends of an object
//   HistoryPair       a history in two slots that change places with every run
//   stage_run_begin   how every run begins: the refusals of csrc/stage_io.h's checks as the caller reads them in
//                     cmhip_last_error(), "nothing to do", or the device made current; stage_launched, a launch's verdict
//   stage_streams     how reset, set and friends begin: the object and the streams the call names
//   stage_sync, stage_read   the body of cmhip_*_sync, and one synchronous readback
#pragma once

#include <string.h>

#include <new>
#include <vector>

#include "stage_io.h"

namespace cmhip {

// A run's per-stream counts on their way to the device (cmhip_batch_run, cmhip_src_run, cmhip_mix_run, cmhip_bus_run,
// cmhip_lim_run): hipMemcpyAsync from pinned memory reads the host array when the stream reaches the copy, not when it
// is queued, so the copy never starts at memory the caller owns.  The object owns a small ring of pinned blocks with an
// event each; a run takes the next block (waiting on the host only when run COUNTS_RING + 1 finds run 1's copy not yet
// executed), fills it, and sends it.  The caller's array is free when the call returns.  The blocks are made with
// the object, not by its first ragged run: nothing on the hot path allocates.
constexpr unsigned COUNTS_RING = 4;                  // runs whose counts may be on their way at once
struct CountsRing {
    uint32_t  *h = nullptr;                          // pinned [COUNTS_RING][words]
    size_t     words = 0;
    hipEvent_t ev[COUNTS_RING] = {};
    bool       busy[COUNTS_RING] = {};
    unsigned   next = 0;

    hipError_t init(size_t words_per_run)            // (on the object's device, which the caller has made current)
    {
        words = words_per_run;
        hipError_t e = hipHostMalloc((void **)&h, COUNTS_RING * words * sizeof(uint32_t), hipHostMallocDefault);
        for (unsigned i = 0; i < COUNTS_RING && e == hipSuccess; i++)
            e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming);
        return e;
    }
    void destroy()
    {
        if (h)
            (void)hipHostFree(h);
        h = nullptr;
        for (unsigned i = 0; i < COUNTS_RING; i++) {
            if (ev[i])
                (void)hipEventDestroy(ev[i]);
            ev[i] = nullptr;
        }
    }
    // the block of the next run, free to be written
    hipError_t take(uint32_t **block)
    {
        if (busy[next]) {                            // COUNTS_RING runs back: its counts have long been copied
            const hipError_t e = hipEventSynchronize(ev[next]);
            if (e != hipSuccess)
                return e;
            busy[next] = false;
        }
        *block = h + (size_t)next * words;
        return hipSuccess;
    }
    // the block take() gave, filled: `n` words of it to dst, in stream order
    hipError_t send(uint32_t *dst, size_t n, hipStream_t st)
    {
        hipError_t e = hipMemcpyAsync(dst, h + (size_t)next * words, n * sizeof(uint32_t), hipMemcpyHostToDevice, st);
        if (e != hipSuccess)
            return e;
        busy[next] = true;                           // (whatever follows: the block may be in use)
        e = hipEventRecord(ev[next], st);
        next = (next + 1) % COUNTS_RING;
        return e;
    }
    // counts[n] as they are: take, fill, send
    hipError_t upload(uint32_t *dst, const uint32_t *counts, size_t n, hipStream_t st)
    {
        uint32_t *block;
        const hipError_t e = take(&block);
        if (e != hipSuccess)
            return e;
        for (size_t i = 0; i < n; i++)
            block[i] = counts[i];
        return send(dst, n, st);
    }
};

// std::bad_alloc stays on this side of the C ABI: f() -> its error number, or COOLMIC_ERROR_NOMEM in the caller's name
template <typename F>
static inline int stage_guard(const char *who, F &&f)
{
    try {
        return f();
    } catch (const std::bad_alloc &) {
        return fail(COOLMIC_ERROR_NOMEM, "%s: out of memory", who);
    }
}

// What a stage owns beside its host mirror: its device, the stream its runs are ordered on (the caller's, or one of
// its own), a run's counts on the device with the ring they arrive through, and every device array made by array().
// An object that was never opened (the cmhip_test_*_new_dry hooks) has its mirror and its checks and no device.
struct CMHIP_INTERNAL StageBase {
    int         device = 0;
    hipStream_t stream = nullptr;
    bool        own_stream = false;
    bool        opened = false;                      // open() was called: there is a device behind the object
    uint32_t   *d_counts = nullptr;                  // [count_words] a run's counts, per stream
    CountsRing  counts;                              // ... on their way there
    std::vector<void *> arrays;                      // what close() frees

    // n elements on the object's device, which the object owns until close(); not filled (for a table that a
    // synchronous copy fills at once).  (May throw std::bad_alloc: creation runs under stage_guard.)
    template <typename T>
    int alloc(const char *who, T **p, size_t n)
    {
        arrays.reserve(arrays.size() + 1);
        if (hipMalloc((void **)p, n * sizeof(T)) != hipSuccess) {
            (void)hipGetLastError();                 // (the error is reported here: it does not stay behind)
            *p = nullptr;
            return fail(COOLMIC_ERROR_NOMEM, "%s: no device memory for %zu bytes", who, n * sizeof(T));
        }
        arrays.push_back(*p);
        return COOLMIC_ERROR_NONE;
    }
    // ... filled in stream order with zeros, or with `pattern` in every 32 bits
    template <typename T>
    int array(const char *who, T **p, size_t n, uint32_t pattern = 0)
    {
        const size_t bytes = n * sizeof(T);
        if (alloc(who, p, n))
            return COOLMIC_ERROR_NOMEM;
        if (pattern)
            HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)*p, (int)pattern, bytes / sizeof(uint32_t), stream));
        else
            HIP_TRY(hipMemsetAsync(*p, 0, bytes, stream));
        return COOLMIC_ERROR_NONE;
    }

    // what a kernel's argument takes for a run's counts: d_counts, or nullptr for a run without counts
    const uint32_t *counts_arg(const uint32_t *frames_per_stream) const { return frames_per_stream ? d_counts : nullptr; }
    // ... with the caller's n counts on their way there (the array is free on return)
    hipError_t send_counts(const uint32_t *frames_per_stream, size_t n, const uint32_t **arg)
    {
        *arg = counts_arg(frames_per_stream);
        return frames_per_stream ? counts.upload(d_counts, frames_per_stream, n, stream) : hipSuccess;
    }

    int open(const char *who, int dev, void *hip_stream, size_t count_words)
    {
        device = dev;
        opened = true;
        HIP_TRY(hipSetDevice(device));
        if (hip_stream) {
            stream = (hipStream_t)hip_stream;
        } else {
            HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
            own_stream = true;
        }
        if (array(who, &d_counts, count_words))
            return COOLMIC_ERROR_NOMEM;
        HIP_TRY(counts.init(count_words));
        return COOLMIC_ERROR_NONE;
    }
    // (also of an object whose creation failed half way, or that was never opened.)  The stream is synchronised before
    // anything is freed; the device stays current for what the stage's destructor ends itself.
    void close()
    {
        if (!opened)
            return;
        (void)hipSetDevice(device);
        if (stream)
            (void)hipStreamSynchronize(stream);
        for (void *p : arrays)
            (void)hipFree(p);
        arrays.clear();
        counts.destroy();
        if (own_stream)
            (void)hipStreamDestroy(stream);
        opened = false;
    }
};

// the body of every cmhip_*_free (m may be NULL)
template <typename M>
static inline void stage_free(M *m)
{
    if (!m)
        return;
    m->close();
    delete m;
}

// The end of every cmhip_*_new, once the arguments are checked: the object, then init(m) -- the fields, open() and the
// device state; it may throw std::bad_alloc -- and on failure the end of whatever was made.
template <typename M, typename Init>
static inline M *stage_new(const char *who, Init &&init)
{
    M *m = new (std::nothrow) M();
    if (!m) {
        fail(COOLMIC_ERROR_NOMEM, "%s: out of memory", who);
        return nullptr;
    }
    if (stage_guard(who, [&] { return init(m); })) {
        stage_free(m);
        return nullptr;
    }
    return m;
}

// A history in two slots, int16 [2][S][per] (the resampler, the limiter, the dynamics stage, the band split, the drift
// stage, whose drift_history is src_history's twin): a run
// reads slot `parity` and writes the other one, flip() after a successful launch makes that the slot the next run reads.
// reset() zeroes the streams' part of the slot the next run reads and nothing else.  That is sufficient: k_src.hip's
// src_history, k_split.hip's split_history, k_lim.h's lim_write_hist and k_dyn.h's dyn_write_hist each write every
// element of the stream's part of the other slot in every run, for a stream without frames too (it copies its slot
// over), so nothing a later run reads is older than the reset.
struct HistoryPair {
    int16_t     *d = nullptr;
    size_t       per = 0;                            // samples per stream and slot
    HistorySlots slots;

    int init(StageBase &b, const char *who, size_t streams, size_t per_stream)
    {
        slots.streams = streams;
        per = per_stream;
        return b.array(who, &d, 2 * streams * per);
    }
    unsigned parity() const { return slots.parity; }
    void flip() { slots.flip(); }
    hipError_t reset(uint32_t lo, uint32_t n, hipStream_t st)
    {
        return hipMemsetAsync(d + slots.at(lo, per), 0, (size_t)n * per * sizeof(int16_t), st);
    }
};

// the body of cmhip_*_sync (m may be NULL)
static inline int stage_sync(StageBase *m, const char *who)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "%s: NULL argument", who);
    if (!m->opened)
        return COOLMIC_ERROR_NONE;
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipStreamSynchronize(m->stream));
    return COOLMIC_ERROR_NONE;
}

// How reset, set and friends begin (m may be NULL; M has d.streams): the streams the call names, -1 for all of them
template <typename M>
static inline int stage_streams(const M *m, const char *who, long stream, StreamRange *sr)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "%s: NULL argument", who);
    *sr = stream_range(stream, m->d.streams);
    if (!sr->ok)
        return fail(COOLMIC_ERROR_INVAL, "%s: stream %ld out of range", who, stream);
    return COOLMIC_ERROR_NONE;
}

// a launch's verdict as an error number
static inline int stage_launched(const char *who, hipError_t e)
{
    return e == hipSuccess ? COOLMIC_ERROR_NONE : fail(COOLMIC_ERROR_GENERIC, "%s: %s", who, hipGetErrorString(e));
}

// One synchronous readback: everything queued before the call has executed, `bytes` of the device array `src` are in
// dst (may be NULL: nothing is copied), and with `refill` the array holds zeros again, or `pattern` in every 32 bits,
// before the call returns.  An object without a device yields zeros.
static inline int stage_read(StageBase *m, void *dst, void *src, size_t bytes, bool refill, uint32_t pattern = 0)
{
    if (!m->opened) {
        if (dst)
            memset(dst, 0, bytes);
        return COOLMIC_ERROR_NONE;
    }
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipStreamSynchronize(m->stream));
    if (dst)
        HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    if (!refill)
        return COOLMIC_ERROR_NONE;
    if (pattern)
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)src, (int)pattern, bytes / sizeof(uint32_t), m->stream));
    else
        HIP_TRY(hipMemsetAsync(src, 0, bytes, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    return COOLMIC_ERROR_NONE;
}

// stage_run_check's verdict on a run as an error number, said in the caller's name
static inline int stage_run_refusal(const char *who, const StageRun &r)
{
    size_t where = 0;
    switch (stage_run_check(r, &where)) {
    case STAGE_RUN_OK: return COOLMIC_ERROR_NONE;
    case STAGE_RUN_NULL: return fail(COOLMIC_ERROR_FAULT, "%s: NULL argument", who);
    case STAGE_RUN_ALIGN: return fail(COOLMIC_ERROR_INVAL, "%s: in and out must be 16-byte aligned", who);
    case STAGE_RUN_STRIDE8: return fail(COOLMIC_ERROR_INVAL, "%s: strides must be multiples of 8 samples", who);
    case STAGE_RUN_FRAMES:
        return fail(COOLMIC_ERROR_INVAL, "%s: %zu frames above the object's %zu", who, r.frames, r.max_frames);
    case STAGE_RUN_COUNT: return fail(COOLMIC_ERROR_INVAL, "%s: frames_per_stream[%zu] above frames", who, where);
    case STAGE_RUN_IN_STRIDE:
        return fail(COOLMIC_ERROR_INVAL, "%s: in_stride %zu below %zu frames of %zu channels", who, r.in_stride, r.frames,
                    r.in_channels);
    case STAGE_RUN_OUT_STRIDE:
        return fail(COOLMIC_ERROR_INVAL, "%s: out_stride %zu below the run's %zu frames of %zu channels", who,
                    r.out_stride, r.out_frames, r.out_channels);
    case STAGE_RUN_SPAN: return fail(COOLMIC_ERROR_INVAL, "%s: slots of these strides would end past the address space", who);
    case STAGE_RUN_OVERLAP:
        return fail(COOLMIC_ERROR_INVAL, r.overlap == STAGE_APART ? "%s: the input and the output overlap" : "%s: in == out",
                    who);
    }
    return fail(COOLMIC_ERROR_GENERIC, "%s: unknown error", who);
}

// How every cmhip_*_run begins, behind its NULL check (the run is built from the object): true -- go, the object's
// device is current; false with *rc an error -- refused, nothing was touched; false with *rc COOLMIC_ERROR_NONE -- a run
// of no frames, nothing to do.  A stage's own refusals (its plan's grid limit, the dynamics stage's keys) follow.
static inline bool stage_run_begin(StageBase *m, const char *who, const StageRun &r, int *rc)
{
    *rc = stage_run_refusal(who, r);
    if (*rc || r.frames == 0)
        return false;
    if (!m->opened) {
        *rc = fail(COOLMIC_ERROR_INVAL, "%s: the object has no device", who);
        return false;
    }
    const hipError_t e = hipSetDevice(m->device);
    *rc = stage_launched(who, e);
    return e == hipSuccess;
}

}  // namespace cmhip
